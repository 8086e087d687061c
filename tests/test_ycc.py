"""The raw-video contract without a device (include/maray_hip.h, "raw video"): tests/ycc_model.py's numpy restatement against
the contract written as a double loop, the facts the header pins (ranges, greys, hand-computed pixels, plane sizes), and the
container round-tripped through the parser -- with the mutants the parser must reject."""
import numpy as np
import pytest

import maray_amd as M
import ycc_model as Y

SHAPES = [(5, 7), (1, 1), (4, 1), (1, 4), (3, 2)]              # (h, w): 7 x 5, 1 x 1, 1 x 4, 4 x 1 and 2 x 3 as w x h


def random_raster(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


@pytest.mark.parametrize('matrix', Y.MATRICES)
@pytest.mark.parametrize('sampling', Y.SAMPLINGS)
@pytest.mark.parametrize('h,w', SHAPES)
def test_the_numpy_model_is_the_contracts_double_loop(h, w, sampling, matrix):
    for seed in range(3):
        rgb = random_raster(100 * seed + 10 * h + w, h, w)
        got = Y.planes(rgb, sampling, matrix)
        want = Y.contract(rgb.tolist(), sampling, matrix)
        for g, c in zip(got, want):
            assert g.tolist() == c
    edge = np.array([0, 1, 127, 128, 254, 255], np.uint8)[random_raster(h + w, h, w) % 6]
    for g, c in zip(Y.planes(edge, sampling, matrix), Y.contract(edge.tolist(), sampling, matrix)):
        assert g.tolist() == c


def test_the_coefficient_rows_sum_as_the_header_says():
    for m in Y.MATRICES:
        ky, kb, kr = Y.COEFF[m]
        assert sum(ky) == 220 and sum(kb) == 0 and sum(kr) == 0
    assert Y.COEFF[Y.BT601] == ((66, 129, 25), (-38, -74, 112), (112, -94, -18))
    assert Y.COEFF[Y.BT709] == ((47, 157, 16), (-26, -86, 112), (112, -102, -10))


@pytest.mark.parametrize('matrix', Y.MATRICES)
@pytest.mark.parametrize('sampling', Y.SAMPLINGS)
def test_greys_and_cube_corners_stay_in_range(sampling, matrix):
    greys = np.repeat(np.arange(256, dtype=np.uint8), 3).reshape(16, 16, 3)
    y, cb, cr = Y.planes(greys, sampling, matrix)
    assert y.min() == 16 and y.max() == 235 and y[0, 0] == 16 and y[15, 15] == 235
    assert np.all(cb == 128) and np.all(cr == 128)
    corners = np.array([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)], np.uint8)
    for c in corners:                   # a constant raster: at 4:2:0 the four-pixel sums of one colour
        y, cb, cr = Y.planes(np.broadcast_to(c, (3, 3, 3)), sampling, matrix)
        assert 16 <= y.min() and y.max() <= 235
        assert 16 <= min(cb.min(), cr.min()) and max(cb.max(), cr.max()) <= 240
    # the extremes are reached: blue's Cb and red's Cr are 240, their complements' 16
    y, cb, cr = Y.planes(corners.reshape(1, 8, 3), Y.YCC_444, matrix)
    assert cb.max() == 240 and cr.max() == 240 and cb.min() == 16 and cr.min() == 16


def test_hand_computed_pixels():
    def one(rgb, matrix=Y.BT601):
        y, cb, cr = Y.planes(np.array([[rgb]], np.uint8), Y.YCC_444, matrix)
        return int(y[0, 0]), int(cb[0, 0]), int(cr[0, 0])
    assert one((255, 0, 0)) == (82, 90, 240)            # (66 * 255 + 128) >> 8 = 66; (-9690 + 128) >> 8 = -38; (28560 + 128) >> 8 = 112
    assert one((0, 255, 0)) == (144, 54, 34)            # 128 + 16; -74 + 128; -94 + 128
    assert one((0, 0, 255)) == (41, 240, 110)           # 25 + 16; 112 + 128; -18 + 128
    assert one((255, 255, 255)) == (235, 128, 128) and one((0, 0, 0)) == (16, 128, 128)
    assert one((255, 0, 0), Y.BT709) == (63, 102, 240)  # 47 + 16; (-6630 + 128) >> 8 = -26
    # 4:2:0: red, green, blue and white sum to a grey; a 2 x 1 image's only block counts both pixels twice (the row is clamped)
    block = np.array([[(255, 0, 0), (0, 255, 0)], [(0, 0, 255), (255, 255, 255)]], np.uint8)
    y, cb, cr = Y.planes(block)
    assert y.tolist() == [[82, 144], [41, 235]] and cb.tolist() == [[128]] and cr.tolist() == [[128]]
    y, cb, cr = Y.planes(np.array([[(255, 0, 0), (0, 0, 0)]], np.uint8))
    assert cb.tolist() == [[109]] and cr.tolist() == [[184]]        # (-38 * 510 + 512) >> 10 = -19; (112 * 510 + 512) >> 10 = 56
    # an odd width's last column pairs with itself
    y, cb, cr = Y.planes(np.array([[(0, 0, 0), (0, 0, 0), (0, 0, 255)]], np.uint8))
    assert cb.tolist() == [[128, 240]]


def test_frame_bytes_for_odd_and_even_sizes():
    for w, h, n420 in ((1, 1, 3), (2, 2, 6), (3, 3, 17), (7, 5, 35 + 2 * 12), (4, 1, 4 + 2 * 2), (1, 4, 4 + 2 * 2), (640, 480, 460800), (67, 41, 2747 + 2 * 34 * 21)):
        assert Y.frame_bytes(w, h, Y.YCC_420) == n420 == M.ycc_frame_bytes(w, h) == M.ycc_frame_bytes(w, h, M.YCC_420)
        assert Y.frame_bytes(w, h, Y.YCC_444) == 3 * w * h == M.ycc_frame_bytes(w, h, M.YCC_444)
        assert len(Y.frame(np.zeros((h, w, 3), np.uint8))) == n420
    assert M.ycc_frame_bytes(1 << 20, 1 << 20, M.YCC_444) == 3 << 40          # no device, no limit: arithmetic in size_t
    with pytest.raises(M.MarayError) as e:
        M.ycc_frame_bytes(4, 4, 2)
    assert e.value.code == -1


@pytest.mark.parametrize('sampling', Y.SAMPLINGS)
def test_the_container_round_trips(sampling):
    for (h, w), n, fps in (((5, 7), 3, (25, 1)), ((1, 1), 1, (30000, 1001)), ((2, 3), 2, (100, 4))):
        rasters = [random_raster(7 * i + h, h, w) for i in range(n)]
        data = Y.build(rasters, fps, sampling, Y.BT709)
        first = data[:data.index(b'\n') + 1]
        assert first == b'YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 %s XCOLORRANGE=LIMITED\n' % (w, h, fps[0], fps[1], b'C444' if sampling else b'C420jpeg')
        assert len(data) == len(first) + n * (6 + Y.frame_bytes(w, h, sampling))
        d = Y.parse(data)
        assert (d.w, d.h, d.fps, d.sampling) == (w, h, fps, sampling)
        assert Y.frames_equal(d, rasters, Y.BT709)
        with pytest.raises(AssertionError):
            Y.frames_equal(d, rasters[::-1] if n > 1 else [255 - rasters[0]], Y.BT709)


def test_the_parser_rejects():
    rasters = [random_raster(i, 4, 6) for i in range(2)]
    good = Y.build(rasters)
    Y.parse(good)
    nl = good.index(b'\n')
    for bad in (good[:-1], good + b'\0', good[:nl + 1], good.replace(b'FRAME\n', b'FRAME \n', 1), good.replace(b' Ip', b' It', 1),
                good.replace(b'W6', b'W7', 1), good.replace(b'F25:1', b'F25:0', 1), good.replace(b'C420jpeg', b'C420', 1),
                good.replace(b' XCOLORRANGE=LIMITED', b'', 1), good[:nl] + b' \n' + good[nl + 1:], b'FRAME\n' + good):
        with pytest.raises(AssertionError):
            Y.parse(bad)

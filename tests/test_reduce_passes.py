"""The shapes of tests/reduce_passes.py without a device: that they are what tests/test_gpu_reduce_passes.py needs them to be.

  - every filter case makes block row 0 of its pass take at least three trips round its loop and ends on a ragged tile that a
    block reaches after a full one; the shutter's frames take every lane round at least twice, by at least 1024 vectors, with a
    head at one of the two destination misalignments and a tail at both;
  - no sample raster is larger than 16 MiB;
  - the numpy contracts do not depend on where the raster is cut (the tent with its halo, the box and the mean plainly), as
    include/maray_hip.h promises of the kernels: the expected pictures of the tall rasters are the contracts' in one piece;
  - the shutter's frame lists tell the mean from a group of 8 left out and from a group counted twice.
"""
import numpy as np
import pytest

import byte_rasters as BR
import linear_light as LL
import reduce_passes as RP

CASES = RP.filter_cases()


# ---- the constants and the worked examples ---------------------------------------------------------------------------------
def test_constants_are_read_from_the_sources_and_the_worked_examples_hold():
    c = RP.constants()
    assert set(c) == {'LIN_MAX_BLOCKS', 'LIN_BLOCK', 'TH', 'FILTER_TILE_W', 'FILTER_TILE_H', 'SH_BLOCK', 'SH_MAX_BLOCKS'}
    # with today's constants (a change of them moves the shapes; these lines then say how far)
    assert (c['LIN_MAX_BLOCKS'], c['LIN_BLOCK'], c['FILTER_TILE_W'], c['TH']) == (2048, 256, 64, {2: 8, 4: 8, 8: 4})
    assert (c['SH_BLOCK'], c['SH_MAX_BLOCKS']) == (256, 2048)
    case = RP.case_by_name('tall k=2 w=3')
    assert case.h == 8 * 4097 + 3 == 32779 and case.sample_shape == (65558, 6, 3)
    gx, gy, tiles = case.grid('tent')
    assert (gx, gy, tiles) == (1, 2048, 4098)
    assert RP.trips(0, gy, tiles) == [0, 2048, 4096] and RP.trips(1, gy, tiles) == [1, 2049, 4097]
    assert (case.k * case.w * 3) % 4 == 2            # every dword misalignment from row to row
    wide = RP.one_block_row_cases()[0]
    assert (wide.w, wide.h) == (64 * 1024 + 1, 19)
    assert wide.grid('tent') == (1025, 1, 3) and wide.grid('box') == (1025, 1, 5)
    two = RP.two_column_tile_cases()[0]
    assert two.w == 65 and two.grid('tent')[:2] == (2, 1024) and two.grid('box')[:2] == (2, 1024)


def test_a_constant_that_no_longer_matches_is_an_assertion_failure():
    with pytest.raises(AssertionError):
        RP._one('constexpr uint32_t LIN_MAX_BLOCKS = kBlocks;', r'constexpr uint32_t LIN_MAX_BLOCKS = (\d+);', 'LIN_MAX_BLOCKS')
    with pytest.raises(AssertionError):
        RP._one('constexpr int X = 1;\nconstexpr int X = 2;', r'constexpr int X = (\d+);', 'X')
    with pytest.raises(AssertionError):
        RP._has('const uint32_t by_budget = LIN_MAX_BLOCKS / gx;', 'const uint32_t by_budget = std::max(1u, LIN_MAX_BLOCKS / gx);', 'launch_filter_k')


def test_the_cases_the_gpu_tests_cover():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    assert sorted((c.k, c.w) for c in RP.narrow_tall_cases()) == [(k, w) for k in (2, 4, 8) for w in (1, 3)]
    assert all(c.grid(kernel)[0] == 1 for c in RP.narrow_tall_cases() for kernel in RP.KERNELS)
    assert all(c.grid(kernel)[0] == 2 and c.w % RP.constants()['FILTER_TILE_W'] == 1 for c in RP.two_column_tile_cases() for kernel in RP.KERNELS)
    assert all(c.grid(kernel)[1] == 1 for c in RP.one_block_row_cases() for kernel in RP.KERNELS)


# ---- trips, ragged tails, bytes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES, ids=repr)
@pytest.mark.parametrize('kernel', RP.KERNELS)
def test_block_row_0_takes_three_trips_and_the_last_tile_is_ragged(kernel, case):
    u = RP.unit_rows(kernel, case.k)
    assert case.h >= RP.min_height(kernel, case.k, case.w)
    assert case.h == RP.min_height('tent', case.k, case.w)          # (the larger of the two: one raster for both kernels)
    assert case.sample_bytes <= RP.MAX_SAMPLE_BYTES and case.sample_bytes == int(np.prod(case.sample_shape))
    for n_out in (case.h, case.h - 5, case.y1_inside_the_last_full_tile(kernel)):      # the whole image, rows [5, h), rows [0, y1)
        gx, gy, tiles = case.grid(kernel, n_out)
        assert gx * gy <= RP.constants()['LIN_MAX_BLOCKS'] or gy == 1
        assert len(RP.trips(0, gy, tiles)) >= (3 if n_out == case.h or gy > 1 else 2)       # (one block row, rows [5, 19): 8 + 6 rows of the tent)
        last_rows = n_out - (tiles - 1) * u
        assert 0 < last_rows < u                                                    # ragged
        assert (tiles - 1) >= gy                                                    # ... and not its block's first tile
    # the whole image: what min_height() promises
    gx, gy, tiles = case.grid(kernel)
    assert case.h - (tiles - 1) * u == RP.RAGGED
    if gy > 1 and kernel == 'tent':
        assert RP.trips(0, gy, tiles) == [0, gy, 2 * gy] and RP.trips(1, gy, tiles)[-1] == tiles - 1
    if gy == 1:
        assert RP.trips(0, gy, tiles) == list(range(tiles))
    # one band by the default budget of 128 MiB of samples, so one filter launch (filter_backend.cpp: band_rows)
    by_budget = (128 << 20) // (case.w * 3 * case.k * case.k) // RP.constants()['FILTER_TILE_H'] * RP.constants()['FILTER_TILE_H']
    assert case.h <= min(max(RP.constants()['FILTER_TILE_H'], by_budget), 65535 * RP.constants()['FILTER_TILE_H'])
    # the range that ends inside the last full tile does
    y1 = case.y1_inside_the_last_full_tile(kernel)
    assert (case.h // u - 1) * u < y1 < (case.h // u) * u


def test_the_byte_tent_control_is_a_4098_tile_grid():
    """maray_filter_tent<K> takes one tile of FILTER_TILE_H rows per block and does not loop."""
    th = RP.constants()['FILTER_TILE_H']
    assert [(c.h + th - 1) // th for c in RP.narrow_tall_cases() if c.k in (2, 8)] == [4098, 4098, 2049, 2049]


# ---- the contracts do not depend on the cut -------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES, ids=repr)
@pytest.mark.parametrize('kernel', RP.KERNELS)
def test_the_contract_of_the_whole_raster_is_the_contract_of_its_tiles(kernel, case):
    s8 = case.raster()
    assert s8.shape == case.sample_shape and s8.nbytes <= RP.MAX_SAMPLE_BYTES
    contract = RP.CONTRACTS[kernel]
    whole = contract(s8, case.k)
    assert whole.shape == (case.h, case.w, 3)
    u = RP.unit_rows(kernel, case.k)
    gx, gy, tiles = case.grid(kernel)
    for t in RP.cut_tiles(gy, tiles):
        y0, y1 = t * u, min(case.h, (t + 1) * u)
        assert np.array_equal(cut_contract_rows(contract, s8, case.k, y0, y1, kernel == 'tent'), whole[y0:y1]), t
    if kernel == 'tent':
        # the halo is needed: a tile cut plainly clamps where the whole raster reads its neighbours
        y0 = gy * u if gy * u < case.h - u else u
        assert not np.array_equal(RP.cut_contract(contract, s8, case.k, y0, y0 + u, False), whole[y0:y0 + u])


def cut_contract_rows(contract, s8, k, y0, y1, halo):
    got = RP.cut_contract(contract, s8, k, y0, y1, halo)
    assert got.shape[0] == y1 - y0
    return got


@pytest.mark.parametrize('k', [2, 8])
def test_the_byte_tent_contract_of_the_tall_raster_is_the_contract_of_its_tiles(k):
    case = RP.case_by_name('tall k=%d w=3' % k)
    s8 = case.raster()
    whole = BR.tent_general(s8, k)
    th = RP.constants()['FILTER_TILE_H']
    tiles = (case.h + th - 1) // th
    for t in (0, 1, tiles // 2, tiles - 2, tiles - 1):
        y0, y1 = t * th, min(case.h, (t + 1) * th)
        assert np.array_equal(RP.cut_contract(BR.tent_general, s8, k, y0, y1, True), whole[y0:y1]), t


# ---- the shutter ---------------------------------------------------------------------------------------------------------
def test_shutter_frames_exceed_one_pass_with_a_tail_at_both_misalignments():
    c = RP.constants()
    h = RP.shutter_height()
    nbytes = 3 * RP.SHUTTER_W * h
    assert RP.SHUTTER_W == BR.PITCH - 1 and nbytes <= RP.MAX_SAMPLE_BYTES
    assert (3 * BR.PITCH * h) % 16 == 0         # why the frames are not as wide as the pitch: no tail at an aligned destination
    assert RP.shutter_blocks(nbytes) == c['SH_MAX_BLOCKS']
    for mis in RP.SHUTTER_MIS:
        head, n_vec, tail, stride = RP.shutter_split(nbytes, mis)
        assert head == (16 - mis) % 16 and head + 16 * n_vec + tail == nbytes
        assert stride == c['SH_MAX_BLOCKS'] * c['SH_BLOCK'] and n_vec >= stride + RP.SHUTTER_PAST
        assert -(-n_vec // stride) >= 2             # lane 0's trips
        assert 1 <= tail <= 15
    assert RP.SHUTTER_MIS == (0, 9)
    assert RP.shutter_height_ok(h) and not any(RP.shutter_height_ok(lower) for lower in range(h - 64, h))      # the smallest such height


def test_shutter_orders_are_uneven_and_the_mean_is_the_contract_whatever_the_cut():
    assert sorted(RP.SHUTTER_ORDER) == [2, 16]
    o = RP.SHUTTER_ORDER[16]
    assert len(o) == 16 and set(o) == set(range(RP.SHUTTER_SLICES))
    assert sorted(o[:8]) != sorted(o[8:]) and len({o.count(t) for t in range(RP.SHUTTER_SLICES)}) > 1
    assert len(set(RP.SHUTTER_ORDER[2])) == 2
    h = RP.shutter_height()
    # rows around the byte at which lane 0 starts its second trip (the contracts are bytewise: a cut of rows is a cut of bytes)
    y = (RP.constants()['SH_MAX_BLOCKS'] * RP.constants()['SH_BLOCK'] * 16) // (3 * RP.SHUTTER_W)
    slices = RP.shutter_slices()
    assert slices[0].shape == (h, RP.SHUTTER_W, 3) and len(slices) == RP.SHUTTER_SLICES
    assert all(not np.array_equal(slices[i], slices[j]) for i in range(4) for j in range(i))
    for n in (2, 16):
        frames = RP.shutter_frames(slices, n)
        for lin, contract in ((True, LL.mean_lin), (False, BR.mean_general)):
            whole = contract(frames)
            assert whole.shape == (h, RP.SHUTTER_W, 3)
            for y0, y1 in ((0, 3), (y - 2, y + 3), (h - 3, h)):
                cut = [f[y0:y1] for f in frames]
                assert np.array_equal(contract(cut), whole[y0:y1]), (n, lin, y0)
                assert np.array_equal(RP.mean_groups(cut, lin), whole[y0:y1]), (n, lin, y0)


@pytest.mark.parametrize('lin', [False, True])
def test_shutter_frame_lists_tell_the_mean_from_a_group_left_out_or_counted_twice(lin):
    h = 64
    slices = RP.shutter_slices(h)
    frames = RP.shutter_frames(slices, 16)
    want = RP.mean_groups(frames, lin)
    assert np.array_equal(want, (LL.mean_lin if lin else BR.mean_general)(frames))
    mutants = RP.group_mutants(16)
    assert [m[1] for m in mutants] == [(0, 1), (2, 1), (1, 0), (1, 2)]
    for name, weights in mutants:
        got = RP.mean_groups(frames, lin, weights)
        assert (got != want).mean() > 0.9, name           # (nearly every byte: a strip of skipped vectors shows wherever it lies)
    assert RP.group_mutants(2) == []
    # a frame list that takes its groups from the same slices could not tell: the order must be uneven
    even = [slices[t] for t in (0, 1, 2, 3) * 4]
    assert np.array_equal(RP.mean_groups(even, lin, (2, 0)), RP.mean_groups(even, lin))

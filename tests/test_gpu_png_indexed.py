"""The indexed-colour form of the device PNG encoder on the device (include/maray_hip.h, "Indexed colour"): every file is
compared byte for byte with tests/png_indexed.py's model_file, decoded by its strict decoder and by the library's own reader.

Most rasters go through Context.render_png(..., png_color=...) on the texture-identity scene of tests/byte_rasters.py.  The
png_encode_device and png_palette cases need a raster in device memory: torch tensors, in child processes that import torch
before the library, as tests/test_gpu_png_device.py's do."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import byte_rasters as BR
import maray_amd as M
import png_indexed as X
import png_stream as P
from test_gpu_png_device import band_rows, chess_scene, identity_tape, on_device
from test_gpu_supersample import BACKENDS, scene_case, supersampled

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INDEXED, AUTO = M.PNG_COLOR_INDEXED, M.PNG_COLOR_AUTO
E_LIMIT = -7

# The launch constants of maray_png_colors (maray_amd/csrc/png_indexed.hpp), restated: blocks of 256 lanes, four pixels a lane
# and pass, at most 512 blocks.  A block's pass is 1,024 pixels, the grid's 524,288.
COLORS_BLOCK, COLORS_LANE_PIXELS, COLORS_MAX_BLOCKS = 256, 4, 512
BLOCK_PIXELS = COLORS_BLOCK * COLORS_LANE_PIXELS
PASS_PIXELS = BLOCK_PIXELS * COLORS_MAX_BLOCKS


def test_the_launch_constants_are_the_headers():
    text = open(os.path.join(ROOT, 'maray_amd', 'csrc', 'png_indexed.hpp')).read()
    m = re.findall(r'PNG_COLORS_BLOCK = (\d+), PNG_COLORS_LANE_PIXELS = (\d+), PNG_COLORS_MAX_BLOCKS = (\d+);', text)
    assert m == [(str(COLORS_BLOCK), str(COLORS_LANE_PIXELS), str(COLORS_MAX_BLOCKS))]
    assert re.findall(r'PNG_IDX_SEG = (\d+);', text) == [str(X.SEG)]


# ---- helpers -----------------------------------------------------------------------------------------------------------------
def render_png_of(img, color=INDEXED, backend=M.BACKEND_TAPE_SMEM):
    ctx = M.Context(identity_tape(), textures=[img], backend=backend)
    try:
        return ctx.render_png(img.shape[1], img.shape[0], png_color=color)
    finally:
        ctx.close()


def encode_tensor(img, color=INDEXED, offset=0, stream=0):
    buf, ptr = on_device(img, offset)
    return M.png_encode_device(ptr, img.shape[1], img.shape[0], stream=stream, png_color=color)


def palette_of_tensor(img, offset=0):
    buf, ptr = on_device(img, offset)
    return M.png_palette(ptr, img.shape[1], img.shape[0])


def check(png, img, tmp_path, name=''):
    """The file is the model's, byte for byte; and both decoders give the raster back."""
    assert png == X.model_file(img), name
    got, pal = X.decode_indexed(png)
    assert np.array_equal(got, img), name
    path = str(tmp_path / 'check.png')
    with open(path, 'wb') as f:
        f.write(png)
    assert np.array_equal(M.png_read(path), img), name
    return pal


_CHILD = r"""
import sys
sys.path[:0] = [%(root)r, %(tests)r]
import torch
import test_gpu_png_indexed as T
T.%(call)s
print('child ok')
"""


def _run(call, timeout=240):
    code = _CHILD % dict(root=ROOT, tests=HERE, call=call)
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0 and out.stdout.strip().endswith('child ok'), (out.stdout[-2000:], out.stderr[-4000:])
    return out.stdout


def _tmp():
    import pathlib
    import tempfile
    return pathlib.Path(tempfile.mkdtemp(prefix='png_indexed_'))


# ---- colour counts -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,d', [(1, 1), (2, 1), (3, 2), (4, 2), (5, 4), (16, 4), (17, 8), (255, 8), (256, 8)])
def test_colour_counts_and_depths(n, d, tmp_path):
    img = X.of_colours(X.n_colours(n, n), 23, 37, seed=n)
    for color in (INDEXED, AUTO):
        png = render_png_of(img, color)
        pal = check(png, img, tmp_path)
        assert len(pal) == n and P.chunks(png)[0][1][8:10] == bytes([d, 3])


@pytest.mark.parametrize('n', [257, 4096])
def test_more_than_256_colours(n, tmp_path):
    img = X.of_colours(X.n_colours(n, n), 70, 67, seed=n)
    ctx = M.Context(identity_tape(), textures=[img], backend=M.BACKEND_TAPE_SMEM)
    with pytest.raises(M.MarayError) as e:
        ctx.render_png(67, 70, png_color=INDEXED)
    assert e.value.code == E_LIMIT and 'more than 256 colours' in str(e.value)
    plain = ctx.render_png(67, 70)                                  # the next call on the same process succeeds
    assert np.array_equal(P.decode(plain), img)
    assert ctx.render_png(67, 70, png_color=AUTO) == plain
    assert ctx.render_png(67, 70, png_color=M.PNG_COLOR_RGB) == plain
    few = X.of_colours(X.n_colours(5), 70, 67)
    ctx2 = M.Context(identity_tape(), textures=[few], backend=M.BACKEND_TAPE_SMEM)
    check(ctx2.render_png(67, 70, png_color=INDEXED), few, tmp_path)
    ctx.close()
    ctx2.close()


# ---- colour sets that stress the set in LDS ------------------------------------------------------------------------------
@pytest.mark.parametrize('name,keys', X.colour_sets(), ids=[n for n, _ in X.colour_sets()])
def test_colour_sets(name, keys, tmp_path):
    img = X.of_colours(keys, 40, 131, seed=len(name))               # 5,240 pixels: six blocks of the collecting kernel
    pal = check(render_png_of(img), img, tmp_path)
    assert np.array_equal(pal, X.palette(img))


# ---- union across blocks and passes (png_palette and png_encode_device: a child process) -----------------------------------------
def union_rasters():
    """[(name, raster, colours)]: rasters of at least two blocks of the collecting kernel whose colours no single block sees."""
    w, h = 64, 4 * BLOCK_PIXELS // 64                               # four blocks, one pass
    a, b = X.n_colours(456, 1)[:256], X.n_colours(456, 1)[256:]
    out = []
    img = np.concatenate([X.of_colours(a[:128], h // 2, w, 1), X.of_colours(a[128:], h // 2, w, 2)])
    out.append(('128 colours above, 128 others below', img, 256))
    img = np.concatenate([X.of_colours(b, h // 2, w, 3), X.of_colours(a[:100], h // 2, w, 4)])
    out.append(('200 colours above, 100 others below', img, 300))
    base = X.of_colours(a, h, w, 5)
    img = base.copy()
    img[-1, -1] = (b[0] >> 16, (b[0] >> 8) & 255, b[0] & 255)
    out.append(('the 257th colour in the last pixel', img, 257))
    img = base.copy()
    img[0, 0] = (b[1] >> 16, (b[1] >> 8) & 255, b[1] & 255)
    out.append(('the 257th colour in the first pixel', img, 257))
    return out


def passes_raster():
    """More than two passes of the capped grid (1,025 x 1,024 pixels): row y is one colour, a[y % 128] above the first pass'
    end and a[128 + y % 128] below it, so that the second half of the palette is seen in later passes only."""
    w, h = 1024, 2 * PASS_PIXELS // 1024 + 1
    a = X.n_colours(256, 2)
    keys = np.where(np.arange(h) < PASS_PIXELS // w, a[np.arange(h) % 128], a[128 + np.arange(h) % 128])
    img = np.zeros((h, w, 3), np.uint8)
    img[:] = np.stack([keys >> 16, (keys >> 8) & 255, keys & 255], axis=1).astype(np.uint8)[:, None, :]
    return img


def child_union():
    tmp = _tmp()
    for name, img, n in union_rasters():
        assert img.shape[0] * img.shape[1] >= 2 * BLOCK_PIXELS
        want = X.palette(img)
        assert len(want) == n, name
        got_n, got = palette_of_tensor(img)
        if n <= 256:
            assert got_n == n and np.array_equal(got, want), name
            check(encode_tensor(img), img, tmp, name)
            assert encode_tensor(img, AUTO) == X.model_file(img), name
        else:
            assert got_n == 257 and len(got) == 0, name
            try:
                encode_tensor(img)
                raise SystemExit('%s: INDEXED gave a file' % name)
            except M.MarayError as e:
                assert e.code == E_LIMIT and 'more than 256 colours' in str(e), name
            plain = encode_tensor(img, M.PNG_COLOR_RGB)
            assert plain == M.png_encode_device(on_device(img)[1], img.shape[1], img.shape[0]) and np.array_equal(P.decode(plain), img), name
            assert encode_tensor(img, AUTO) == plain, name
    img = passes_raster()
    assert img.shape[0] * img.shape[1] > 2 * PASS_PIXELS
    got_n, got = palette_of_tensor(img)
    assert got_n == 256 and np.array_equal(got, X.palette(img))
    check(encode_tensor(img), img, tmp, 'passes')
    img[-1, -1] = 255 - img[-1, -1]                                   # and a 257th colour in the last pixel of the last pass
    assert len(X.palette(img)) == 257
    assert palette_of_tensor(img)[0] == 257
    for name, keys in X.colour_sets():                                # the palettes of the hashed set's hard cases, as png_palette gives them
        img = X.of_colours(keys, 40, 131, seed=len(name))
        got_n, got = palette_of_tensor(img, offset=1)
        assert got_n == len(keys) and np.array_equal(got, X.palette(img)), name


def test_union_across_blocks_and_passes():
    _run('child_union()')


# ---- geometry ------------------------------------------------------------------------------------------------------------------
RB_EDGES = (63, 64, 65, 767, 768, 769, 1537)          # packed row lengths at the step's and the segment's boundaries


def child_geometry():
    tmp = _tmp()
    for n in (2, 4, 16, 256):                          # depths 1, 2, 4, 8: a last byte that holds 1 .. 8 / d pixels
        for w in range(1, 18):
            for h in (1, 2, 19):
                if w * h < n:
                    continue
                img = X.of_colours(X.n_colours(n, w), h, w, seed=100 * w + h)
                check(encode_tensor(img), img, tmp, (n, w, h))
    for rb in RB_EDGES:
        for h in (1, 2, 19):
            for k in (0, 3, 7):                        # one bit a pixel: w = 8 rb - k
                w = 8 * rb - k
                img = X.of_colours(np.array([0x102030, 0xF0E0D0]), h, w, seed=rb + k)
                img[h // 2, w // 3:w // 3 + 2000] = (0x10, 0x20, 0x30)          # (runs too)
                check(encode_tensor(img), img, tmp, (rb, h, k))
        img = X.of_colours(X.n_colours(256, rb), 2, rb, seed=rb)               # and a byte a pixel
        img[1, rb // 4:rb // 4 + 200] = img[0, 0]
        check(encode_tensor(img), img, tmp, rb)


def test_geometry():
    """For each depth a last byte holding 1 .. 8 / d pixels (w = 1 .. 17); packed rows of 63 .. 1,537 bytes, the step's and the
    segment's boundaries, at one bit (w = 8 rb - k) and at eight; heights 1, 2, 19."""
    _run('child_geometry()')


# ---- runs --------------------------------------------------------------------------------------------------------------------
def child_runs():
    tmp = _tmp()
    for name, img in X.byte_runs() + X.small_rasters():
        check(encode_tensor(img), img, tmp, name)


def test_runs_on_tensors():
    """At depth 8, where pixel runs are byte runs: every length 1 .. 130, every start and end modulo 64, over a segment
    boundary, over a row end, lengths 1 and 2 next to 3; constants, checkers, and png_stream's rasters of at most 256 colours."""
    _run('child_runs()')


@pytest.mark.parametrize('name,img', [(n, i) for n, i in X.byte_runs() + X.small_rasters() if i.shape[1] <= 600],
                         ids=[n for n, i in X.byte_runs() + X.small_rasters() if i.shape[1] <= 600])
def test_runs_rendered(name, img, tmp_path):
    check(render_png_of(img), img, tmp_path, name)


# ---- alignment, cuts, streams, scratch ------------------------------------------------------------------------------------------
def child_alignment():
    tmp = _tmp()
    for n, w in ((2, 1), (2, 77), (16, 5), (256, 65), (200, 301)):
        img = X.of_colours(X.n_colours(n, w), 7, w, seed=w)
        files = [encode_tensor(img, offset=o) for o in range(16)]
        check(files[0], img, tmp, (n, w))
        assert all(f == files[0] for f in files), (n, w)
        assert all(np.array_equal(palette_of_tensor(img, offset=o)[1], X.palette(img)) for o in range(16)), (n, w)


def test_source_at_every_byte_offset():
    _run('child_alignment()')


def child_band_cuts():
    tmp = _tmp()
    for n, w, h in ((2, 8 * 769 - 3, 19), (16, 131, 19), (256, 300, 19), (256, 2 * X.SEG + 1, 2), (3, 5, 1)):
        img = X.of_colours(X.n_colours(n, w), h, w, seed=h)
        img[h // 2, w // 3:w // 3 + 300] = img[0, 0]
        files = []
        for rows in P.BAND_ROWS:
            with band_rows(rows):
                files.append(encode_tensor(img))
                files.append(render_png_of(img))                      # (bands of 1 and 3 rows: every band is rendered twice)
                files.append(render_png_of(img, AUTO))
        check(files[0], img, tmp, (n, w, h))
        assert all(f == files[0] for f in files), (n, w, h)
    many = X.of_colours(X.n_colours(300, 1), 19, 131)                  # AUTO on more than 256 colours in bands that are rendered twice
    with band_rows(None):
        plain = render_png_of(many, M.PNG_COLOR_RGB)
    for rows in P.BAND_ROWS:
        with band_rows(rows):
            assert render_png_of(many, AUTO) == plain and encode_tensor(many, AUTO) == plain, rows


def test_band_cuts_give_one_file():
    """MARAY_PNG_BAND_ROWS = 1, 3, 1000 through both entry points, the case where render_png renders twice included."""
    _run('child_band_cuts()')


def child_streams():
    import torch
    tmp = _tmp()
    a, b = X.of_colours(X.n_colours(7, 1), 30, 100, 1), X.of_colours(X.n_colours(200, 2), 30, 100, 2)
    big, small = X.of_colours(X.n_colours(256, 3), 90, 1700, 3), X.of_colours(X.n_colours(2, 4), 3, 9, 4)
    big[10:20, 100:1600] = big[0, 0]
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ta, pa = on_device(a)
        tb, pb = on_device(b)
        fa = M.png_encode_device(pa, 100, 30, stream=st.cuda_stream, png_color=INDEXED)
        fb = M.png_encode_device(pb, 100, 30, stream=st.cuda_stream, png_color=AUTO)
        na, pal_a = M.png_palette(pa, 100, 30, stream=st.cuda_stream)
    check(fa, a, tmp)
    check(fb, b, tmp)
    assert na == 7 and np.array_equal(pal_a, X.palette(a))
    before = M.png_bytes_to_host()
    fbig = encode_tensor(big)                                         # scratch that grows,
    assert M.png_bytes_to_host() - before == 1028 + 24 + len(P.idat_stream(fbig)) - 11      # (the palette, the totals, the band's bytes)
    check(fbig, big, tmp)
    check(encode_tensor(small), small, tmp)                           # shrinks,
    check(encode_tensor(big), big, tmp)                               # and grows again; and a truecolour call in between
    plain = M.png_encode_device(on_device(big)[1], 1700, 90)
    assert np.array_equal(P.decode(plain), big)
    check(encode_tensor(a), a, tmp)
    ms, nb = M.time_png_encode(on_device(big)[1], 1700, 90, reps=2, png_color=INDEXED)
    assert ms > 0 and nb == len(P.idat_stream(fbig)) - 11
    ms, nb = M.time_png_encode(on_device(big)[1], 1700, 90, reps=2, png_color=M.PNG_COLOR_RGB)
    assert ms > 0 and nb == len(P.idat_stream(plain)) - 11


def test_two_streams_and_scratch_that_grows_shrinks_and_grows():
    _run('child_streams()')


# ---- rendered scenes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_chess_is_two_colours_at_one_bit(chess_bytes, backend, tmp_path):
    s = chess_scene(chess_bytes)
    want = M.gen_to_image(s, backend=M.BACKEND_TAPE_SMEM)
    ctx = M.Context(s.lower(), backend=backend)
    png = ctx.render_png(1024, 1024, png_color=AUTO)
    plain = ctx.render_png(1024, 1024)
    ctx.close()
    pal = check(png, want, tmp_path)
    assert len(pal) == 2 and P.chunks(png)[0][1][8:10] == bytes([1, 3])
    print('chess 1024 x 1024: indexed %d bytes, truecolour %d' % (len(png), len(plain)))
    assert len(png) < len(plain)


def test_chess_supersampled(chess_bytes, tmp_path):
    want = M.gen_to_image(chess_scene(chess_bytes), backend=M.BACKEND_TAPE_SMEM, samples=4)
    assert len(X.palette(want)) <= 17
    ctx = M.Context(supersampled(chess_bytes, 4).lower(), backend=M.BACKEND_TAPE_SMEM, samples=4)
    with band_rows(300):                                              # (four bands: each rendered twice)
        ctx2 = M.Context(supersampled(chess_bytes, 4).lower(), backend=M.BACKEND_TAPE_SMEM, samples=4)
        cut = ctx2.render_png(1024, 1024, png_color=INDEXED)
        ctx2.close()
    png = ctx.render_png(1024, 1024, png_color=INDEXED)
    ctx.close()
    check(png, want, tmp_path)
    assert cut == png


@pytest.mark.parametrize('backend', BACKENDS)
def test_a_shutter_call(backend, tmp_path):
    """Four frames of black and white on the atlas scene (a parameterised scene): their mean holds at most five greys."""
    rng = np.random.default_rng(5)
    frames = [np.repeat((rng.integers(0, 2, (23, 50, 1)) * 255).astype(np.uint8), 3, axis=2) for _ in range(4)]
    ctx = M.Context(BR.atlas_scene().lower(), textures=[BR.atlas(frames)], backend=backend)
    values = np.arange(4, dtype=np.float64)[:, None]
    want = ctx.render_rows_shutter(50, 23, 0, 23, values)
    assert np.array_equal(want, BR.mean_general(frames)) and 2 < len(X.palette(want)) <= 5
    png = ctx.render_png(50, 23, frames=values, png_color=INDEXED)
    with band_rows(3):
        ctx2 = M.Context(BR.atlas_scene().lower(), textures=[BR.atlas(frames)], backend=backend)
        assert ctx2.render_png(50, 23, frames=values, png_color=INDEXED) == png
        ctx2.close()
    ctx.close()
    check(png, want, tmp_path)


@pytest.mark.parametrize('backend', BACKENDS)
def test_auto_on_a_textured_scene_is_the_truecolour_file(backend):
    data, w, h, tex = scene_case('textured')
    ctx = M.Context(M.Scene(data).lower(), textures=tex, backend=backend)
    want, _ = ctx.render_rows(w, h, 0, h, want_f64=False)
    assert len(X.palette(want)) > 256
    plain = ctx.render_png(w, h)
    assert np.array_equal(P.decode(plain), want)
    assert ctx.render_png(w, h, png_color=AUTO) == plain
    with pytest.raises(M.MarayError) as e:
        ctx.render_png(w, h, png_color=INDEXED)
    assert e.value.code == E_LIMIT
    ctx.close()

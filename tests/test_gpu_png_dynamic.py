"""The device PNG encoder with dynamic-Huffman codes on the device (include/maray_hip.h, "device PNG encoder":
MARAY_PNG_CODES_DYNAMIC): every file is decoded by tests/png_stream.py -- signature, CRCs, IHDR, zlib.decompress with its
Adler-32, length, unfilter -- and by the library's own reader, and the decoded raster is compared with the input by
np.array_equal; sizes are held against tests/png_dynamic_model.py's derived bound.

Device rasters for png_encode_device are torch tensors: those tests run in child processes that import torch before the
library, as tests/test_gpu_png_device.py's do."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import apng_stream as A
import byte_rasters as BR
import maray_amd as M
import png_dynamic_model as D
import png_stream as P
from test_gpu_png_device import band_rows, check, chess_scene, on_device
from test_gpu_supersample import BACKENDS, scene_case, supersampled

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DYN = M.CODES_DYNAMIC

_CHILD = r"""
import sys
sys.path[:0] = [%(root)r, %(tests)r]
import torch
import test_gpu_png_dynamic as T
T.%(call)s
print('child ok')
"""


def _run(call, timeout=300):
    code = _CHILD % dict(root=ROOT, tests=HERE, call=call)
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0 and out.stdout.strip().endswith('child ok'), (out.stdout[-2000:], out.stderr[-4000:])
    return out.stdout


def _tmp():
    import pathlib
    import tempfile
    return pathlib.Path(tempfile.mkdtemp(prefix='png_dynamic_'))


def encode(img, offset=0, stream=0, codes=DYN):
    buf, ptr = on_device(img, offset)
    return M.png_encode_device(ptr, img.shape[1], img.shape[0], stream=stream, codes=codes)


def pieces_bytes(png):
    """The bytes of a file's pieces: its zlib stream without 78 01 in front and the final stored block and the Adler-32 behind."""
    z = P.idat_stream(png)
    assert z[:2] == b'\x78\x01' and z[-9:-4] == b'\x01\x00\x00\xff\xff'
    return z[2:-9]


def launch_constants():
    """PNG_HIST_WAVES, PNG_HIST_MAX_BLOCKS as png_device.hpp exports them."""
    text = open(os.path.join(ROOT, 'maray_amd', 'csrc', 'png_device.hpp')).read()
    m = re.search(r'PNG_HIST_WAVES = (\d+), PNG_HIST_MAX_BLOCKS = (\d+)', text)
    return int(m.group(1)), int(m.group(2))


# ---- random bytes ------------------------------------------------------------------------------------------------------
def child_random_bytes():
    tmp = _tmp()
    for w in P.GEOMETRY_WS:
        for h in P.GEOMETRY_HS:
            img = P.random_bytes(100 * w + h, h, w)
            img[h // 2, w // 3:w // 3 + 70] = 77          # (a run too, where the row is long enough)
            for rows in P.BAND_ROWS:
                with band_rows(rows):
                    try:
                        check(encode(img), img, tmp)
                    except AssertionError:
                        raise AssertionError((w, h, rows))


def test_random_bytes_at_every_geometry_and_band_cut():
    """Widths 1 .. 2 SEG + 1 around the step and the segment, heights 1, 2 and 19, bands of 1, 3 and 1000 rows."""
    _run('child_random_bytes()')


# ---- runs, alignment ---------------------------------------------------------------------------------------------------
def child_runs():
    tmp = _tmp()
    for name, img in P.run_rasters():
        try:
            check(encode(img), img, tmp)
            with band_rows(2):
                check(encode(img), img, tmp)
        except AssertionError:
            raise AssertionError(name)


def test_runs():
    """The rasters of tests/png_stream.py on which the bit packing and the run logic can go wrong, as one band and in bands of 2."""
    _run('child_runs()')


def child_alignment():
    tmp = _tmp()
    for w in P.ALIGN_WS:
        img = P.random_bytes(300 + w, 7, w)
        img[3, w // 2:] = 9
        files = [encode(img, offset=o) for o in range(16)]
        check(files[0], img, tmp)
        assert all(f == files[0] for f in files), w


def test_source_at_every_byte_offset():
    _run('child_alignment()')


# ---- histograms that break a code builder or an emitter ----------------------------------------------------------------
def fibonacci_raster():
    """509 x 1426: the byte values 100 .. 129 with counts 1, 1, 2, 3, 5, ... (the last cut to what the raster holds), shuffled."""
    fib = [1, 1]
    while len(fib) < 30:
        fib.append(fib[-1] + fib[-2])
    n = 509 * 1426 * 3
    fib[-1] -= sum(fib) - n
    assert fib[-1] > fib[-2]
    flat = np.repeat(np.arange(100, 130, dtype=np.uint8), fib)
    np.random.default_rng(5).shuffle(flat)
    return flat.reshape(1426, 509, 3)


def child_histograms():
    tmp = _tmp()
    check(encode(np.zeros((9, 300, 3), np.uint8)), np.zeros((9, 300, 3), np.uint8), tmp)         # only symbols 0, 256 and lengths
    for h in (1, 2, 700):                                       # w = 1: no match in any band, a distance code of zero bits
        img = P.random_bytes(h, h, 1)
        check(encode(img), img, tmp)
        lit, dist, _ = D.token_counts(img)
        assert dist.sum() == 0
    one = np.array([[[0, 0, 0]]], np.uint8)                     # 1 x 1, and of the byte 0 alone: two symbols
    check(encode(one), one, tmp)
    check(encode(one + 200), one + 200, tmp)
    every = np.arange(256 * 3, dtype=np.uint32).reshape(1, 256, 3).astype(np.uint8)      # all 256 byte values
    assert len(np.unique(every)) == 256
    check(encode(every), every, tmp)
    every2 = np.concatenate([every, every[:, ::-1]], axis=1)
    check(encode(every2), every2, tmp)


def test_histograms_that_break_a_code_builder_or_an_emitter():
    _run('child_histograms()')


def child_fibonacci():
    img = fibonacci_raster()
    bits, depth = D.token_bits(img)
    print('fibonacci raster: the unrestricted tree is %d deep' % depth)
    assert depth > 15
    png = encode(img)
    assert np.array_equal(P.decode(png), img)
    lit, dist, extra = D.token_counts(img)
    assert len(pieces_bytes(png)) * 8 < D.fixed_cost(lit) + extra + 5 * int(dist[2])      # and still below the fixed codes


def test_a_histogram_whose_tree_is_deeper_than_15():
    """Thirty values with Fibonacci counts: the helper's tree is 18 deep or so, the code must be cut to 15 bits."""
    print(_run('child_fibonacci()'))


# ---- many segments, several passes -------------------------------------------------------------------------------------
def child_many_segments():
    for h, w in ((70000, 2), (140000, 1)):
        img = P.random_bytes(h, h, w)
        img[1000:1200] = 5
        png = encode(img)
        assert np.array_equal(P.decode(png), img), h
        with band_rows(60000):
            assert np.array_equal(P.decode(encode(img)), img), h


def test_more_segments_in_a_band_than_the_scan_has_single_groups_for():
    """70,000 and 140,000 segments in one band (groups of 128 and 192 segments in the scan), and cut at 60,000."""
    _run('child_many_segments()')


def passes_shape():
    """(w, h) whose one band gives the histogram's blocks three passes, the last ragged: 2 1/2 times the segments a full grid
    takes at once, and three more."""
    waves, blocks = launch_constants()
    per_pass = waves * blocks
    return 3, 2 * per_pass + per_pass // 2 + 3


def test_the_multi_pass_shape_is_what_it_is_for():
    waves, blocks = launch_constants()
    w, h = passes_shape()
    n_segs = h * -(-w // P.SEG)
    assert n_segs > 2 * waves * blocks and n_segs % (waves * blocks) and n_segs % waves
    assert (3 * w + 1) * h < 64 << 20                      # one band by the default budget


def child_passes():
    w, h = passes_shape()
    img = P.random_bytes(7, h, w) & 3                       # few values: runs and literals in every pass
    img[-5:] = 250                                          # values only the last, ragged pass sees
    png = encode(img)
    assert np.array_equal(P.decode(png), img)
    bound = D.piece_bound(img)
    assert len(pieces_bytes(png)) <= bound, (len(pieces_bytes(png)), bound)       # (a lost or doubled count would cost bits, or the decode)


def test_a_band_whose_histogram_blocks_take_several_passes():
    _run('child_passes()')


# ---- size ------------------------------------------------------------------------------------------------------------------
def child_sizes(chess_path):
    chess = np.load(chess_path)
    for name, img in (('chess', chess), ('constant', np.full((64, 256, 3), 7, np.uint8)), ('checker', P.checker(40, 300))):
        for rows in (None, 1000, 17):
            step = rows or img.shape[0]
            parts = []
            for r0 in range(0, img.shape[0], step):     # every band on its own: one piece
                band = np.ascontiguousarray(img[r0:r0 + step])
                piece = pieces_bytes(encode(band))
                bound = D.piece_bound(band)
                assert len(piece) <= bound, (name, rows, r0, len(piece), bound)
                parts.append(piece)
            with band_rows(rows):
                whole = encode(img)
            assert np.array_equal(P.decode(whole), img)
            assert pieces_bytes(whole) == b''.join(parts), (name, rows)      # the same cut, the same bytes
    rnd = P.random_bytes(0, 512, 512)
    fixed, dyn = encode(rnd, codes=M.CODES_FIXED), encode(rnd)
    print('random 512 x 512: fixed %d bytes, dynamic %d' % (len(fixed), len(dyn)))
    assert len(dyn) <= len(fixed)
    fixed, dyn = encode(chess, codes=M.CODES_FIXED), encode(chess)
    print('chess 1024 x 1024: fixed %d bytes, dynamic %d, ratio %.3f' % (len(fixed), len(dyn), len(dyn) / len(fixed)))
    assert np.array_equal(P.decode(dyn), chess) and np.array_equal(P.decode(fixed), chess)
    assert len(dyn) <= 0.35 * len(fixed)


def test_every_piece_is_within_the_derived_bound_and_chess_shrinks(chess_bytes, tmp_path):
    """Chess (from the scalar-cache interpreter), a constant raster and the checker, as one band and cut at 1000 and 17 rows:
    every band's piece is at most ceil((2286 + T) / 8) + 5 bytes, T the optimal cost of its tokens; dynamic <= fixed on random
    bytes; the dynamic chess file is at most 0.35 of the fixed coder's (the model gives 0.28)."""
    chess = M.gen_to_image(chess_scene(chess_bytes), backend=M.BACKEND_TAPE_SMEM)
    path = str(tmp_path / 'chess.npy')
    np.save(path, chess)
    print(_run('child_sizes(%r)' % path))


# ---- determinism -----------------------------------------------------------------------------------------------------------
def child_determinism():
    import torch
    tmp = _tmp()
    img = P.random_bytes(31, 90, 700)
    img[10:20, 100:600] = 3
    a = encode(img)
    assert encode(img) == a
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        buf, ptr = on_device(img)
        assert M.png_encode_device(ptr, 700, 90, stream=st.cuda_stream, codes=DYN) == a
    check(a, img, tmp)
    for rows in (1, 7, 89):                                  # other cuts: other bytes maybe, the same pixels
        with band_rows(rows):
            b = encode(img)
            assert encode(img) == b
        check(b, img, tmp)
    # MARAY_PNG_CODES_FIXED through _ex is the plain call's file
    buf, ptr = on_device(img)
    p, sz = C.c_void_p(), C.c_size_t()
    assert M.lib().maray_hip_png_encode_device(0, ptr, 700, 90, None, C.byref(p), C.byref(sz)) == 0
    plain = C.string_at(p, sz.value)
    M.lib().maray_free(p)
    assert M.png_encode_device(ptr, 700, 90, codes=M.CODES_FIXED) == plain
    check(plain, img, tmp)
    ms, nb = M.time_png_encode(ptr, 700, 90, reps=2, codes=DYN)
    assert nb == len(pieces_bytes(a)) and ms > 0
    ms, nb = M.time_png_encode(ptr, 700, 90, reps=2)
    assert nb == len(pieces_bytes(plain))


def test_the_same_bytes_twice_on_any_stream_and_the_same_pixels_for_every_cut():
    _run('child_determinism()')


# ---- through contexts --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', BACKENDS)
def test_render_png_with_dynamic_codes_equals_render_rows(backend, tmp_path):
    data, w, h, tex = scene_case('all_ops')
    ctx = M.Context(M.Scene(data).lower(), textures=tex, backend=backend)
    want, _ = ctx.render_rows(w, h, 0, h, want_f64=False)
    with band_rows(16):
        ctx2 = M.Context(M.Scene(data).lower(), textures=tex, backend=backend)
        check(ctx2.render_png(w, h, codes=DYN), want, tmp_path)
        ctx2.close()
    png = ctx.render_png(w, h, codes=DYN)
    check(png, want, tmp_path)
    assert len(png) < len(ctx.render_png(w, h))
    ctx.close()


@pytest.mark.parametrize('backend', BACKENDS)
def test_render_png_with_dynamic_codes_supersampled_with_tent_and_srgb(backend, tmp_path):
    data, w, h, tex = scene_case('all_ops')
    ctx = M.Context(supersampled(data, 2).lower(), textures=tex, backend=backend, samples=2, filter=M.FILTER_TENT, transfer=M.TRANSFER_SRGB)
    want, _ = ctx.render_rows(w, h, 0, h, want_f64=False)
    check(ctx.render_png(w, h, codes=DYN), want, tmp_path)
    ctx.close()


@pytest.mark.parametrize('backend', BACKENDS)
def test_render_png_with_dynamic_codes_of_a_shutter_call(backend, tmp_path):
    frames = BR.random_frames(77, 4, 23, 50)
    ctx = M.Context(BR.atlas_scene().lower(), textures=[BR.atlas(frames)], backend=backend)
    values = np.arange(4, dtype=np.float64)[:, None]
    want = ctx.render_rows_shutter(50, 23, 0, 23, values)
    check(ctx.render_png(50, 23, frames=values, codes=DYN), want, tmp_path)
    ctx.close()


# ---- through gen, the CLI and gen_animation --------------------------------------------------------------------------------
@pytest.mark.parametrize('report', [False, True])
def test_gen_with_the_dynamic_flag(chess_bytes, report, tmp_path):
    s = chess_scene(chess_bytes)
    want = M.gen_to_image(s, backend=M.BACKEND_TAPE_SMEM)
    out, fixed = str(tmp_path / 'gen.png'), str(tmp_path / 'fixed.png')
    assert M.ENCODER_DEVICE | M.ENCODER_DYNAMIC == 0x101
    M.gen(s, out, backend=M.BACKEND_TAPE_SMEM, encoder=0x101, **(dict(report_kind=M.api.REPORT_ROW, report_value=10) if report else {}))
    check(open(out, 'rb').read(), want, tmp_path)
    M.gen(s, fixed, backend=M.BACKEND_TAPE_SMEM, encoder=M.ENCODER_DEVICE)
    assert os.path.getsize(out) <= 0.35 * os.path.getsize(fixed)


def test_gen_with_two_workers_and_the_dynamic_flag(chess_bytes, tmp_path, monkeypatch):
    monkeypatch.setenv('MARAY_GEN_WRAP_DEVICES', '1')
    s = chess_scene(chess_bytes)
    out = str(tmp_path / 'two.png')
    M.gen(s, out, backend=M.BACKEND_TAPE_SMEM, n_devices=2, encoder=0x101)
    check(open(out, 'rb').read(), M.gen_to_image(s, backend=M.BACKEND_TAPE_SMEM, n_devices=1), tmp_path)


def test_cli_with_dynamic_codes(chess_bytes, tmp_path):
    scene = str(tmp_path / 'chess.maray')
    s = chess_scene(chess_bytes)
    s.save(scene)
    want = M.gen_to_image(s, backend=M.BACKEND_TAPE_SMEM)
    exe = os.path.join(os.path.dirname(M.lib_path()), 'maray')
    out, fixed = str(tmp_path / 'cli.png'), str(tmp_path / 'fixed.png')
    r = subprocess.run([exe, '-i', scene, '-o', out, '--backend', 'tape-smem', '--encoder', 'device', '--png-codes', 'dynamic'], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    check(open(out, 'rb').read(), want, tmp_path)
    r = subprocess.run([exe, '-i', scene, '-o', fixed, '--backend', 'tape-smem', '--encoder', 'device', '--png-codes', 'fixed'], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    plain = str(tmp_path / 'plain.png')
    M.gen(s, plain, backend=M.BACKEND_TAPE_SMEM, encoder=M.ENCODER_DEVICE)
    assert open(fixed, 'rb').read() == open(plain, 'rb').read()
    assert os.path.getsize(out) < os.path.getsize(fixed)


def test_gen_animation_with_dynamic_codes(tmp_path):
    from test_gpu_apng import ATLAS_N, atlas_case
    M.gen_cache_clear()
    scene, tex, frames = atlas_case()
    plain, dyn = str(tmp_path / 'a.png'), str(tmp_path / 'b.png')
    M.gen_animation(scene, plain, {'t': range(ATLAS_N)}, fps=(10, 1), loops=3, textures=tex, backend=M.BACKEND_TAPE_SMEM)
    M.gen_animation(scene, dyn, {'t': range(ATLAS_N)}, fps=(10, 1), loops=3, textures=tex, backend=M.BACKEND_TAPE_SMEM, codes=DYN)
    a, b = A.decode(open(plain, 'rb').read()), A.decode(open(dyn, 'rb').read())
    assert b.delay == a.delay and b.plays == a.plays and b.rects == a.rects and len(b.frames) == ATLAS_N
    for i in range(ATLAS_N):
        assert np.array_equal(b.frames[i], frames[i]) and np.array_equal(a.frames[i], frames[i]), i
    assert os.path.getsize(dyn) <= os.path.getsize(plain)
    # the flag is all the animation reads of the word
    go_word = str(tmp_path / 'c.png')
    go = M.GenOpts()
    go.backend, go.encoder = M.BACKEND_TAPE_SMEM, M.ENCODER_DYNAMIC | 7
    arr, n, keep = M.api._textures(tex)
    values = np.arange(ATLAS_N, dtype=np.float64)
    assert M.lib().maray_gen_animation(scene._h, arr, n, C.byref(go), values.ctypes.data, ATLAS_N, 1, 10, 3, os.fsencode(go_word)) == 0
    assert open(go_word, 'rb').read() == open(dyn, 'rb').read()
    M.gen_cache_clear()

"""The row filters of the device PNG encoder on the device (include/maray_hip.h, "Row filters").  Every file is decoded by
tests/png_stream.py -- signature, CRCs, IHDR, zlib.decompress with its Adler-32, length, unfilter -- and by the library's own
reader, and the decoded raster is compared with the input by np.array_equal; the filter bytes read from the decompressed
stream must be the forced type, or tests/png_filter_model.py's choice row by row; with fixed codes the file's length is the
model's, exactly.

Device rasters for png_encode_device are torch tensors: those tests run in child processes that import torch before the
library, as tests/test_gpu_png_device.py's do."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import maray_amd as M
import png_filter_model as F
import png_stream as P
from test_gpu_png_device import band_rows, check, on_device
from test_gpu_supersample import scene_case, supersampled

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXED, DYN = M.CODES_FIXED, M.CODES_DYNAMIC
OPTIONS = list(range(6))                                 # MARAY_PNG_FILTER_*
NAMES = ('none', 'adaptive', 'sub', 'up', 'average', 'paeth')
# no left neighbour; lane 0 across a step; a segment's first pixel with its left and upper-left in the previous segment
WIDTHS = (1, 2, 3, 63, 64, 65, 255, 256, 257, 513)
HEIGHTS = (1, 2, 19)                                     # no row above; a carry across bands of 1 and 3 rows

_CHILD = r"""
import sys
sys.path[:0] = [%(root)r, %(tests)r]
import torch
import test_gpu_png_filter as T
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
    return pathlib.Path(tempfile.mkdtemp(prefix='png_filter_'))


def encode(img, option, codes=FIXED, offset=0, stream=0):
    buf, ptr = on_device(img, offset)
    return M.png_encode_device(ptr, img.shape[1], img.shape[0], stream=stream, codes=codes, png_filter=option)


def held(png, img, types, tmp):
    """What every file is held against: both decoders return the raster, and the rows' filter bytes are `types`."""
    check(png, img, tmp)
    got = F.filter_bytes(png)
    assert np.array_equal(got, types), (list(got), list(types))


def mixed_raster(seed, h, w):
    """Random bytes in which rows repeat the row above (y % 4 = 1: Up makes them constant), are ramps along x (y % 4 = 2: Sub
    does) or repeat the row above shifted by a constant (y % 4 = 3), and one row holds a run: every type has rows to win."""
    img = P.random_bytes(seed, h, w)
    x = np.arange(w)
    for y in range(1, h):
        if y % 4 == 1:
            img[y] = img[y - 1]
        elif y % 4 == 2:
            img[y] = np.stack([(3 * x + y) & 255, (250 + x) & 255, (7 * x) & 255], axis=1)
        elif y % 4 == 3:
            img[y] = img[y - 1] + np.array([1, 255, 128], np.uint8)
    img[h // 2, w // 3:w // 3 + 70] = 77
    return img


# ---- geometry ----------------------------------------------------------------------------------------------------------
def child_geometry(option):
    tmp = _tmp()
    picked = np.zeros(5, np.int64)
    for w in WIDTHS:
        for h in HEIGHTS:
            img = mixed_raster(100 * w + h, h, w)
            types = F.choose(img, option)
            picked += np.bincount(types, minlength=5)
            try:
                files = []
                for rows in P.BAND_ROWS:
                    with band_rows(rows):
                        files.append(encode(img, option))
                        held(encode(img, option, DYN), img, types, tmp)      # (other bytes for other cuts: each is decoded)
                held(files[0], img, types, tmp)
                assert all(f == files[0] for f in files), 'the fixed-code file depends on the band cut'
                assert len(files[0]) == F.fixed_file_size(img, option)
            except AssertionError as e:
                raise AssertionError((NAMES[option], w, h, str(e)[:2000]))
    print('%s: rows per type %s' % (NAMES[option], list(picked)))
    if option == F.ADAPTIVE:
        assert (picked[:3] > 0).all()                      # None, Sub and Up all win rows of these rasters


@pytest.mark.parametrize('option', OPTIONS, ids=NAMES)
def test_every_width_and_height_in_bands_of_1_3_and_1000_rows(option):
    """Widths 1 .. 513 around the step and the segment, heights 1, 2 and 19: fixed codes give one file for the three band
    heights, of the model's length; dynamic codes give the raster and the model's types for each."""
    print(_run('child_geometry(%d)' % option))


# ---- alignment -----------------------------------------------------------------------------------------------------------
def child_alignment():
    tmp = _tmp()
    for w in (5, 65):
        img = mixed_raster(300 + w, 7, w)
        for option in OPTIONS:
            types = F.choose(img, option)
            files = [encode(img, option, offset=o) for o in range(4)]
            held(files[0], img, types, tmp)
            assert all(f == files[0] for f in files), (w, NAMES[option])
            for o in range(4):
                held(encode(img, option, DYN, offset=o), img, types, tmp)


def test_source_at_byte_offsets_0_to_3():
    """w = 5 and w = 65: rows 15 and 195 bytes apart, so the row and the row above it are aligned differently at every offset."""
    _run('child_alignment()')


# ---- the rasters ---------------------------------------------------------------------------------------------------------
def rasters():
    out = [('random 37 x 65', P.random_bytes(0, 37, 65)), ('random 5 x 700', P.random_bytes(1, 5, 700))]
    out += P.run_rasters()
    out += [('alphabet 19 x 65', F.alphabet_raster(1, 19, 65)), ('alphabet 19 x 257', F.alphabet_raster(2, 19, 257)), ('ramp 64 x 700', F.ramp())]
    return out


def child_rasters(option):
    tmp = _tmp()
    for name, img in rasters():
        try:
            types = F.choose(img, option)
            png = encode(img, option)
            held(png, img, types, tmp)
            with band_rows(2):
                assert encode(img, option) == png, 'the fixed-code file depends on the band cut'
                dyn2 = encode(img, option, DYN)
            dyn = encode(img, option, DYN)
            held(dyn, img, types, tmp)
            held(dyn2, img, types, tmp)
            # size with fixed codes: the model's, exactly; ADAPTIVE never above filter 0 (the guarantee)
            none = len(encode(img, F.NONE))
            assert len(png) == F.fixed_file_size(img, option), (len(png), F.fixed_file_size(img, option))
            print('%-34s %-8s fixed %8d (none %8d)  dynamic %8d, in bands of 2 rows %8d' % (name, NAMES[option], len(png), none, len(dyn), len(dyn2)))
            if option == F.ADAPTIVE:
                assert len(png) <= none
                if name.startswith('ramp'):
                    assert len(png) < none
                    assert (types[1:] == 2).all()
        except AssertionError as e:
            raise AssertionError((NAMES[option], name, str(e)[:2000]))


@pytest.mark.parametrize('option', OPTIONS, ids=NAMES)
def test_random_bytes_runs_the_tie_alphabet_and_the_ramp(option):
    """Random bytes, tests/png_stream.py's run rasters, rasters over {0, 1, 2, 127, 128, 254, 255} (Paeth's ties, Average's odd
    and 9-bit sums, wrap-around) and the 64 x 700 ramp, whole and in bands of 2 rows, with both codes."""
    print(_run('child_rasters(%d)' % option))


# ---- filter NONE through the _opts entry points ------------------------------------------------------------------------------
def child_none_is_the_plain_call():
    img = mixed_raster(31, 40, 300)
    buf, ptr = on_device(img)
    L = M.lib()
    p, sz = C.c_void_p(), C.c_size_t()
    assert L.maray_hip_png_encode_device(0, ptr, 300, 40, None, C.byref(p), C.byref(sz)) == 0
    plain = C.string_at(p, sz.value)
    L.maray_free(p)
    assert L.maray_hip_png_encode_device_ex(0, ptr, 300, 40, DYN, None, C.byref(p), C.byref(sz)) == 0
    plain_dyn = C.string_at(p, sz.value)
    L.maray_free(p)
    assert M.png_encode_device(ptr, 300, 40, png_filter=F.NONE) == plain
    assert M.png_encode_device(ptr, 300, 40, codes=DYN, png_filter=F.NONE) == plain_dyn
    assert L.maray_hip_png_encode_device_opts(0, ptr, 300, 40, None, None, C.byref(p), C.byref(sz)) == 0      # null options: all zeros
    assert C.string_at(p, sz.value) == plain
    L.maray_free(p)
    assert np.array_equal(P.decode(plain), img) and np.array_equal(P.decode(plain_dyn), img)
    ms, nb = C.c_float(), C.c_uint64()
    assert L.maray_hip_time_png_encode(0, ptr, 300, 40, 2, C.byref(ms), C.byref(nb)) == 0
    assert M.time_png_encode(ptr, 300, 40, reps=2, png_filter=F.NONE) [1] == nb.value == len(P.idat_stream(plain)) - F.ZLIB_FRAME
    for option in OPTIONS[1:]:                            # and with a filter the timed kernels make the file's stream
        ms2, nb2 = M.time_png_encode(ptr, 300, 40, reps=2, png_filter=option)
        assert ms2 > 0 and nb2 == len(P.idat_stream(M.png_encode_device(ptr, 300, 40, png_filter=option))) - F.ZLIB_FRAME, NAMES[option]
        ms2, nb2 = M.time_png_encode(ptr, 300, 40, reps=2, codes=DYN, png_filter=option)
        assert ms2 > 0 and nb2 == len(P.idat_stream(M.png_encode_device(ptr, 300, 40, codes=DYN, png_filter=option))) - F.ZLIB_FRAME, NAMES[option]


def test_filter_none_through_the_opts_entry_points_is_the_plain_call():
    _run('child_none_is_the_plain_call()')


def test_render_png_with_filter_none_is_the_plain_call():
    data, w, h, tex = scene_case('all_ops')
    ctx = M.Context(M.Scene(data).lower(), textures=tex, backend=M.BACKEND_TAPE_SMEM)
    L = M.lib()
    p, sz = C.c_void_p(), C.c_size_t()
    assert L.maray_hip_render_png(ctx._h, w, h, None, 0, C.byref(p), C.byref(sz)) == 0
    plain = C.string_at(p, sz.value)
    L.maray_free(p)
    assert ctx.render_png(w, h, png_filter=M.PNG_FILTER_NONE) == plain
    ctx.close()


# ---- one file through both entry points --------------------------------------------------------------------------------------
CONFIGS = ((M.BACKEND_TAPE_SMEM, 1, M.FILTER_BOX), (M.BACKEND_JIT, 1, M.FILTER_BOX), (M.BACKEND_TAPE_SMEM, 2, M.FILTER_TENT))


def child_encode_rasters(folder, option):
    """png_encode_device of the rasters <folder>/want<i>.npy in bands of 1, 3 and 1000 rows -> <folder>/enc<i>_<rows>.png."""
    for i in range(len(CONFIGS)):
        want = np.load(os.path.join(folder, 'want%d.npy' % i))
        for rows in P.BAND_ROWS:
            with band_rows(rows):
                with open(os.path.join(folder, 'enc%d_%d.png' % (i, rows)), 'wb') as f:
                    f.write(encode(want, option))


@pytest.mark.parametrize('option', OPTIONS, ids=NAMES)
def test_png_encode_device_and_render_png_write_one_file(option, tmp_path):
    """A scene through the scalar-cache interpreter, the JIT, and supersampled with the tent filter: png_encode_device of the
    rendered raster (a torch tensor: in a child process) and Context.render_png, whose bands carry their last row over, in
    bands of 1, 3 and 1000 rows -- one fixed-code file; with dynamic codes the raster and the model's types."""
    data, w, h, tex = scene_case('all_ops')

    def context(backend, k, filt):
        scene = supersampled(data, k) if k > 1 else M.Scene(data)
        return M.Context(scene.lower(), textures=tex, backend=backend, samples=k, filter=filt)
    wants = []
    for i, cfg in enumerate(CONFIGS):
        ctx = context(*cfg)
        wants.append(ctx.render_rows(w, h, 0, h, want_f64=False)[0])
        ctx.close()
        np.save(str(tmp_path / ('want%d.npy' % i)), wants[i])
    _run('child_encode_rasters(%r, %d)' % (str(tmp_path), option))
    for i, (backend, k, filt) in enumerate(CONFIGS):
        want, types, files = wants[i], F.choose(wants[i], option), []
        for rows in P.BAND_ROWS:
            files.append(open(str(tmp_path / ('enc%d_%d.png' % (i, rows))), 'rb').read())
            with band_rows(rows):
                ctx = context(backend, k, filt)
                files.append(ctx.render_png(w, h, png_filter=option))
                held(ctx.render_png(w, h, codes=DYN, png_filter=option), want, types, tmp_path)
                ctx.close()
        held(files[0], want, types, tmp_path)
        assert all(f == files[0] for f in files), (NAMES[option], backend, k, [len(f) for f in files])
        assert len(files[0]) == F.fixed_file_size(want, option)

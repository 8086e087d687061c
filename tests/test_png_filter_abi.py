"""The row filters of the device PNG encoder, as far as they can be checked without a device (include/maray_hip.h, "Row
filters"): the constants and the options struct, every argument error (raised before a device is looked for), the Python
defaults, and tests/png_filter_model.py pinned against itself -- its filtered rows decode back through tests/png_stream.py
in every type, and its filter-0 sizes are the fixed coder's known ones."""
import ctypes as C
import inspect
import os
import zlib

import numpy as np
import pytest

import maray_amd as M
import png_filter_model as F
import png_stream as P

E_ARG = -1
HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), 'include', 'maray_hip.h')


# ---- constants and layout --------------------------------------------------------------------------------------------------
def test_constants():
    assert (M.PNG_FILTER_NONE, M.PNG_FILTER_ADAPTIVE, M.PNG_FILTER_SUB, M.PNG_FILTER_UP, M.PNG_FILTER_AVERAGE, M.PNG_FILTER_PAETH) == (0, 1, 2, 3, 4, 5)
    assert (F.NONE, F.ADAPTIVE, F.SUB, F.UP, F.AVERAGE, F.PAETH) == (0, 1, 2, 3, 4, 5)
    header = open(HEADER).read()
    assert ('enum { MARAY_PNG_FILTER_NONE = 0, MARAY_PNG_FILTER_ADAPTIVE = 1, MARAY_PNG_FILTER_SUB = 2, MARAY_PNG_FILTER_UP = 3, '
            'MARAY_PNG_FILTER_AVERAGE = 4, MARAY_PNG_FILTER_PAETH = 5 };') in header
    assert 'typedef struct { uint32_t codes, filter, reserved[6]; } maray_png_opts;' in header


def test_the_options_struct_and_the_entry_points():
    assert C.sizeof(M.PngOpts) == 32
    assert [getattr(M.PngOpts, f).offset for f in ('codes', 'filter', 'reserved')] == [0, 4, 8]
    L = M.lib()
    vp, u32 = C.c_void_p, C.c_uint32
    assert L.maray_hip_png_encode_device_opts.argtypes == [C.c_int, vp, u32, u32, vp, vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    assert L.maray_hip_render_png_opts.argtypes == [vp, u32, u32, vp, u32, vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    assert L.maray_hip_time_png_encode_opts.argtypes == [C.c_int, vp, u32, u32, vp, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_uint64)]
    header = open(HEADER).read()
    for name in ('maray_hip_png_encode_device_opts(int device, const void *d_rgb8, uint32_t w, uint32_t h, const maray_png_opts *opts, void *stream,',
                 'maray_hip_render_png_opts(maray_ctx *c, uint32_t w, uint32_t h, const double *values, uint32_t n_frames, const maray_png_opts *opts,',
                 'maray_hip_time_png_encode_opts(int device, const void *d_rgb8, uint32_t w, uint32_t h, const maray_png_opts *opts, int reps,'):
        assert name in header


def test_python_defaults():
    for f in (M.png_encode_device, M.Context.render_png, M.time_png_encode):
        assert inspect.signature(f).parameters['png_filter'].default == M.PNG_FILTER_NONE
        assert 'filter' not in inspect.signature(f).parameters                     # `filter` is the reconstruction filter
    for f in (M.gen, M.gen_animation, M.Context.render_apng, M.apng_encode_device):      # gen and the animation writer do not take it
        assert 'png_filter' not in inspect.signature(f).parameters


# ---- argument errors ---------------------------------------------------------------------------------------------------------
def _opts(codes=0, filt=0, reserved=None):
    o = M.PngOpts()
    o.codes, o.filter = codes, filt
    if reserved is not None:
        o.reserved[reserved] = 1
    return o


def _three_calls(o):
    """The three _opts entry points on pointers that are never dereferenced: [(return code, message)]."""
    fake = C.c_void_p(0x1000)
    p, sz, ms, nb = C.c_void_p(), C.c_size_t(), C.c_float(), C.c_uint64()
    L = M.lib()
    out = []
    out.append((L.maray_hip_png_encode_device_opts(0, fake, 4, 4, C.byref(o), None, C.byref(p), C.byref(sz)), L.maray_last_error().decode()))
    out.append((L.maray_hip_render_png_opts(fake, 4, 4, None, 0, C.byref(o), C.byref(p), C.byref(sz)), L.maray_last_error().decode()))
    out.append((L.maray_hip_time_png_encode_opts(0, fake, 4, 4, C.byref(o), 1, C.byref(ms), C.byref(nb)), L.maray_last_error().decode()))
    return out


@pytest.mark.parametrize('filt', [6, 7, 0x1000, 0xFFFFFFFF])
def test_an_unknown_filter_is_an_argument_error_before_a_device_is_looked_for(filt):
    for codes in (M.CODES_FIXED, M.CODES_DYNAMIC):
        for rc, msg in _three_calls(_opts(codes, filt)):
            assert rc == E_ARG and 'filter' in msg


@pytest.mark.parametrize('word', range(6))
def test_a_reserved_word_that_is_not_zero_is_an_argument_error(word):
    for filt in (M.PNG_FILTER_NONE, M.PNG_FILTER_ADAPTIVE):
        for rc, msg in _three_calls(_opts(0, filt, reserved=word)):
            assert rc == E_ARG and 'reserved' in msg


def test_unknown_codes_in_the_options_are_an_argument_error():
    for rc, msg in _three_calls(_opts(2, M.PNG_FILTER_UP)):
        assert rc == E_ARG and 'codes' in msg
    with pytest.raises(M.MarayError) as e:
        M.png_encode_device(0x1000, 4, 4, png_filter=6)
    assert e.value.code == E_ARG
    with pytest.raises(M.MarayError) as e:
        M.time_png_encode(0x1000, 4, 4, png_filter=9)
    assert e.value.code == E_ARG


# ---- the model, pinned against itself -------------------------------------------------------------------------------------------
def _filtered_rows_of(png, h, w):
    raw = np.frombuffer(zlib.decompress(P.idat_stream(png)), np.uint8).reshape(h, 3 * w + 1)
    return raw[:, 0], raw[:, 1:].reshape(h, w, 3)


@pytest.mark.parametrize('t', range(5))
def test_the_models_filtered_rows_are_png_streams_filtered_rows_and_decode_back(t):
    for img in (F.alphabet_raster(3, 19, 65), P.random_bytes(4, 5, 33), F.ramp(9, 300), P.random_bytes(5, 1, 1), P.random_bytes(6, 3, 1)):
        h, w, _ = img.shape
        png = P.encode_filtered(img, [t])
        types, rows = _filtered_rows_of(png, h, w)
        assert (types == t).all() and np.array_equal(rows, F.filter_raster(img, t))
        assert np.array_equal(P.decode(png), img)
        assert np.array_equal(F.filter_bytes(png), np.full(h, t))


def test_the_models_mixed_rows_decode_back():
    img = F.alphabet_raster(7, 19, 257)
    types = np.arange(19) % 5
    raw = b''.join(bytes([int(t)]) + row.tobytes() for t, row in zip(types, F.filter_rows(img, types)))
    assert np.array_equal(P.unfilter(raw, 19, 257), img)


def test_the_alphabet_rasters_hit_the_ties_and_the_wide_sums():
    img = F.alphabet_raster(1, 19, 65).astype(np.int64)
    a, b, c = img[1:, :-1], img[:-1, 1:], img[:-1, :-1]
    assert ((a == b) & (b != c)).any() and ((b == c) & (a != b)).any() and ((a == b) & (b == c)).any()
    assert ((a + b) & 1).any() and ((a + b) > 255).any()
    p = a + b - c
    assert (np.abs(p - a) == np.abs(p - b)).any() and (np.abs(p - b) == np.abs(p - c)).any()      # distances that tie
    assert set(np.unique(img)) == set(int(v) for v in F.ALPHABET)


def test_filter_0_sizes_are_the_fixed_coders():
    """tests/test_gpu_png_device.py's two rasters: 1,227 and 7,878 bytes of stream."""
    assert F.fixed_stream_size(np.full((64, 256, 3), 7, np.uint8)) == 1227
    assert F.fixed_stream_size(P.random_bytes(0, 37, 65)) == 7878
    assert F.fixed_file_size(P.random_bytes(0, 37, 65)) == 7878 + 57
    # and the token bits are the existing model's count under the fixed codes, plus 3 bits per segment
    import png_dynamic_model as D
    img = P.random_bytes(9, 6, 300)
    img[2, 10:200] = 8
    lit, dist, extra = D.token_counts(img)
    lit[256] -= 1                                        # (no end-of-block in a segment's bits)
    _, bits = F.segment_costs(F.filter_raster(img, 0))
    assert int(bits.sum()) == D.fixed_cost(lit) + extra + 5 * int(dist[2]) + 3 * bits.size


def test_the_selection_rule_on_the_ramp_and_on_ties():
    ramp = F.ramp()
    types = F.choose(ramp)
    assert types[0] == 0 and (types[1:] == 2).all()                              # 63 of 64 rows take Up
    none, adaptive = F.fixed_file_size(ramp), F.fixed_file_size(ramp, F.ADAPTIVE)
    assert (none, adaptive) == (123122, 5292)
    zeros = np.zeros((4, 70, 3), np.uint8)                                       # every type costs the same: the smallest type wins
    assert (F.choose(zeros) == 0).all()
    for seed in range(4):                                                        # never larger than filter 0, row by row
        img = F.alphabet_raster(seed, 9, 300) if seed & 1 else P.random_bytes(seed, 9, 300)
        by, _ = F.row_costs(img)
        t = F.choose(img)
        assert (by[np.arange(9), t] <= by[:, 0]).all()
    assert list(F.choose(ramp, F.NONE)) == [0] * 64 and list(F.choose(ramp, F.PAETH)) == [4] * 64

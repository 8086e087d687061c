"""The dynamic-Huffman coder of the device PNG encoder, as far as it can be checked without a device (include/maray_hip.h,
"device PNG encoder": MARAY_PNG_CODES_DYNAMIC): the constants, the `_ex` entry points and their argument errors, the encoder
word's flag, the CLI option, and the host's part on its own -- maray_png_dynamic_codes on random and on edge counts, checked
against tests/png_dynamic_model.py's unrestricted Huffman tree and against zlib's inflate."""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest

import maray_amd as M
import png_dynamic_model as D

E_ARG = -1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def test_constants():
    assert (M.CODES_FIXED, M.CODES_DYNAMIC) == (0, 1)
    assert M.ENCODER_DYNAMIC == 0x100
    assert (M.ENCODER_HOST, M.ENCODER_DEVICE) == (0, 1)
    header = open(os.path.join(os.path.dirname(GOLDEN), '..', 'include', 'maray_hip.h')).read()
    assert 'enum { MARAY_PNG_CODES_FIXED = 0, MARAY_PNG_CODES_DYNAMIC = 1 };' in header
    assert '#define MARAY_ENCODER_DYNAMIC 0x100' in header


def test_gen_opts_keeps_its_size_and_offsets():
    assert C.sizeof(M.GenOpts) == 32
    assert [getattr(M.GenOpts, f).offset for f in ('backend', 'n_devices', 'tile_rows', 'samples', 'shutter', 'filter', 'encoder', 'transfer')] == \
        [0, 4, 8, 12, 16, 20, 24, 28]


def test_the_ex_entry_points_exist_with_their_signatures():
    L = M.lib()
    vp, u32 = C.c_void_p, C.c_uint32
    assert L.maray_hip_png_encode_device_ex.argtypes == [C.c_int, vp, u32, u32, u32, vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    assert L.maray_hip_render_png_ex.argtypes == [vp, u32, u32, vp, u32, u32, C.POINTER(vp), C.POINTER(C.c_size_t)]
    assert L.maray_hip_time_png_encode_ex.argtypes == [C.c_int, vp, u32, u32, u32, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_uint64)]
    assert L.maray_png_dynamic_codes.argtypes == [vp, vp, vp, vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    header = open(os.path.join(os.path.dirname(GOLDEN), '..', 'include', 'maray_hip.h')).read()
    for name in ('maray_hip_png_encode_device_ex(int device, const void *d_rgb8, uint32_t w, uint32_t h, uint32_t codes, void *stream,',
                 'maray_hip_render_png_ex(maray_ctx *c, uint32_t w, uint32_t h, const double *values, uint32_t n_frames, uint32_t codes,',
                 'maray_hip_time_png_encode_ex(int device, const void *d_rgb8, uint32_t w, uint32_t h, uint32_t codes, int reps,'):
        assert name in header
    import inspect
    for f in (M.png_encode_device, M.Context.render_png, M.time_png_encode, M.gen_animation):
        assert inspect.signature(f).parameters['codes'].default == M.CODES_FIXED


def test_unknown_codes_are_argument_errors_before_a_device_is_looked_for():
    fake = C.c_void_p(0x1000)           # never dereferenced: the checks come first
    p, sz, ms, nb = C.c_void_p(), C.c_size_t(), C.c_float(), C.c_uint64()
    L = M.lib()
    for codes in (2, 0x100, 0xFFFFFFFF):
        assert L.maray_hip_png_encode_device_ex(0, fake, 4, 4, codes, None, C.byref(p), C.byref(sz)) == E_ARG
        assert 'codes' in L.maray_last_error().decode()
        assert L.maray_hip_render_png_ex(fake, 4, 4, None, 0, codes, C.byref(p), C.byref(sz)) == E_ARG
        assert 'codes' in L.maray_last_error().decode()
        assert L.maray_hip_time_png_encode_ex(0, fake, 4, 4, codes, 1, C.byref(ms), C.byref(nb)) == E_ARG
        assert 'codes' in L.maray_last_error().decode()
    with pytest.raises(M.MarayError) as e:
        M.png_encode_device(0x1000, 4, 4, codes=2)
    assert e.value.code == E_ARG


@pytest.mark.parametrize('word', [2, 7, 0x100, 0x102, 0x201])
def test_gen_refuses_every_encoder_word_but_the_three(chess_bytes, word, tmp_path):
    s = M.Scene(chess_bytes)
    out = str(tmp_path / 'x.png')
    with pytest.raises(M.MarayError) as e:
        M.gen(s, out, encoder=word)
    assert e.value.code == E_ARG and 'encoder' in str(e.value)
    assert not os.path.exists(out)
    go = M.GenOpts()
    go.backend, go.encoder = M.BACKEND_TAPE_SMEM, word
    img = np.zeros((8, 8, 3), np.uint8)
    assert M.lib().maray_gen_to_image(s._h, None, 0, C.byref(go), M.api.Report(0, 0), M.api.REPORT_FN(0), None, img.ctypes.data, 8, 8) == E_ARG


def _cli(*args):
    exe = os.path.join(os.path.dirname(M.lib_path()), 'maray')
    return subprocess.run([exe] + list(args), capture_output=True, text=True)


def test_cli_usage_errors_and_help(tmp_path):
    scene, out = os.path.join(GOLDEN, 'chess.maray'), str(tmp_path / 'x.png')
    r = _cli('-i', scene, '-o', out, '--png-codes', 'dynamic')                      # without --encoder device or --apng
    assert r.returncode == 2 and '--png-codes' in r.stderr and '--encoder device' in r.stderr
    r = _cli('-i', scene, '-o', out, '--png-codes', 'fixed')                        # the default value too: the option has no meaning there
    assert r.returncode == 2 and '--png-codes' in r.stderr
    r = _cli('-i', scene, '-o', out, '--encoder', 'host', '--png-codes', 'dynamic')
    assert r.returncode == 2
    r = _cli('-i', scene, '-o', out, '--encoder', 'device', '--png-codes', 'huffman')
    assert r.returncode == 2 and '--png-codes takes fixed or dynamic' in r.stderr and 'huffman' in r.stderr
    r = _cli('-i', scene, '-o', out, '--encoder', 'device', '--png-codes')          # no value
    assert r.returncode == 2
    r = _cli('-i', scene, '-o', out, '--encoder', 'bogus', '--png-codes', 'dynamic')
    assert r.returncode == 2 and '--encoder takes host or device' in r.stderr and 'bogus' in r.stderr
    assert not os.path.exists(out)
    r = _cli('--help')
    assert r.returncode == 0 and '--png-codes' in r.stderr and 'fixed | dynamic' in r.stderr


# ---- maray_png_dynamic_codes ------------------------------------------------------------------------------------------------
def _canonical(lens):
    """{symbol: code} of the lengths (RFC 1951, 3.2.2)."""
    codes, code = {}, 0
    for bits in range(1, 16):
        for s, l in enumerate(lens):
            if l == bits:
                codes[s] = code
                code += 1
        code <<= 1
    return codes


def _inflate_header_and_end(header, bits, lit_lens):
    """header + symbol 256 + the sync flush + a final empty stored block through a raw inflate: b'' and the stream's end."""
    z = bytearray(header) + bytearray(8)
    code, n = _canonical(lit_lens)[256], int(lit_lens[256])
    at = bits
    for i in range(n):                                   # a Huffman code goes most significant bit first
        z[at >> 3] |= ((code >> (n - 1 - i)) & 1) << (at & 7)
        at += 1
    at += 3                                              # BFINAL = 0, BTYPE = 00
    z = bytes(z[:(at + 7) // 8]) + b'\x00\x00\xff\xff' + b'\x01\x00\x00\xff\xff'
    d = zlib.decompressobj(-15)
    out = d.decompress(z)
    assert d.eof and not d.unused_data
    return out


def _check_codes(lit, dist):
    lit, dist = np.asarray(lit, np.uint32), np.asarray(dist, np.uint32)
    lit_lens, dist_lens, header, bits = M.png_dynamic_codes(lit, dist)
    assert lit_lens.max() <= 15 and dist_lens.max() <= 15
    assert np.array_equal(lit_lens == 0, lit == 0), 'length 0 goes to exactly the unused symbols'
    assert D.kraft(lit_lens) == 1 << 15, 'the literal/length code is complete'
    assert list(dist_lens) == ([0, 0, 1] + [0] * 27 if dist[2] else [0] * 30)
    cost = int((lit.astype(np.int64) * lit_lens).sum())
    best, depth = D.huffman(lit)
    if depth <= 15:
        assert cost == best, (cost, best)
    else:
        assert cost >= best
    assert 0 < bits <= D.HEADER_MAX_BITS and len(header) == (bits + 7) // 8
    assert _inflate_header_and_end(header, bits, lit_lens) == b''
    return cost, depth


@pytest.mark.parametrize('seed', range(12))
def test_codes_of_random_counts(seed):
    rng = np.random.default_rng(seed)
    lit = rng.integers(0, [2, 50, 1000, 1 << 20][seed % 4], 286)
    lit[rng.random(286) < (seed % 3) * 0.4] = 0
    lit[0] = max(lit[0], 1)
    lit[256] = 1
    lit[257:] *= seed & 1                                # with and without matches
    dist = np.zeros(30, np.int64)
    dist[2] = lit[257:].sum()
    _check_codes(lit, dist)


def test_codes_of_edge_counts():
    none = np.zeros(30, np.int64)
    lit = np.zeros(286, np.int64)
    lit[0] = lit[256] = 1
    _check_codes(lit, none)                              # only 0 and 256
    lit[0] = 1 << 20
    _check_codes(lit, none)
    full = np.arange(1, 287)
    some = none.copy()
    some[2] = full[257:].sum()
    _check_codes(full, some)                             # all 286 symbols
    _check_codes(np.ones(286, np.int64), some)
    nomatch = full.copy()
    nomatch[257:] = 0
    _check_codes(nomatch, none)                          # no distance
    big = np.ones(286, np.int64)
    big[257:] = 0
    big[77] = 1 << 31
    _check_codes(big, none)                              # one symbol with count 2^31


def test_codes_past_the_length_limit_are_valid_and_beat_the_fixed_codes():
    """Counts 1, 1, 2, 3, 5, ... over 30 symbols: the unrestricted tree is far deeper than 15."""
    fib = [1, 1]
    while len(fib) < 30:
        fib.append(fib[-1] + fib[-2])
    lit = np.zeros(286, np.int64)
    lit[100:130] = fib
    lit[0] += 1
    lit[256] = 1
    cost, depth = _check_codes(lit, np.zeros(30, np.int64))
    assert depth > 15
    assert cost < D.fixed_cost(lit)


def test_counts_no_band_has_are_argument_errors():
    lit = np.zeros(286, np.int64)
    lit[0] = 3
    with pytest.raises(M.MarayError) as e:
        M.png_dynamic_codes(lit, np.zeros(30, np.int64))                 # symbol 256 does not occur
    assert e.value.code == E_ARG
    lit[256] = 1
    dist = np.zeros(30, np.int64)
    dist[5] = 1
    with pytest.raises(M.MarayError) as e:
        M.png_dynamic_codes(lit, dist)                                   # a distance other than 3
    assert e.value.code == E_ARG
    out = np.zeros(4, np.uint8)
    bits = C.c_size_t()
    l32, d32, ll, dl = lit.astype(np.uint32), np.zeros(30, np.uint32), np.zeros(286, np.uint8), np.zeros(30, np.uint8)
    assert M.lib().maray_png_dynamic_codes(l32.ctypes.data, d32.ctypes.data, ll.ctypes.data, dl.ctypes.data, out.ctypes.data, 4, C.byref(bits)) == E_ARG


def test_the_model_counts_a_small_raster_by_hand():
    """2 x 70 pixels: row 0 is one colour (a literal pixel, a match of 63 pixels to the step's end, a match of 6), row 1 is all
    different but for its last two pixels."""
    img = np.zeros((2, 70, 3), np.uint8)
    img[0] = (9, 9, 9)
    img[1, :, 0] = 100 + np.arange(70)
    img[1, 69] = img[1, 68]
    lit, dist, extra = D.token_counts(img)
    assert lit[9] == 3 and lit[256] == 1 and dist[2] == 3 and dist.sum() == 3
    assert lit[0] == 2 + 2 * 69 and lit[:256].sum() == 2 + 3 + 3 * 69
    s63, e63 = D.length_symbol(189)
    s6, e6 = D.length_symbol(18)
    s1, e1 = D.length_symbol(3)
    assert lit[s63] == 1 and lit[s6] == 1 and lit[s1] == 1 and extra == e63 + e6 + e1
    assert (D.length_symbol(3), D.length_symbol(10), D.length_symbol(11), D.length_symbol(257), D.length_symbol(258)) == \
        ((257, 0), (264, 0), (265, 1), (284, 5), (285, 0))

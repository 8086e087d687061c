"""The indexed-colour form of the device PNG encoder, as far as it can be checked without a device (include/maray_hip.h,
"Indexed colour"): the constants, the options struct and the entry points, every argument error (raised before a device is
looked for), the Python defaults and refusals, and tests/png_indexed.py pinned against decoders that know nothing of it -- its
own strict one, zlib, the library's reader and, where it is installed, PIL -- and against the truecolour file's size."""
import ctypes as C
import inspect
import os
import zlib

import numpy as np
import pytest

import maray_amd as M
import png_filter_model as F
import png_indexed as X
import png_stream as P

E_ARG = -1
HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), 'include', 'maray_hip.h')


# ---- constants and layout --------------------------------------------------------------------------------------------------
def test_constants():
    assert (M.PNG_COLOR_RGB, M.PNG_COLOR_INDEXED, M.PNG_COLOR_AUTO) == (0, 1, 2)
    header = open(HEADER).read()
    assert 'enum { MARAY_PNG_COLOR_RGB = 0, MARAY_PNG_COLOR_INDEXED = 1, MARAY_PNG_COLOR_AUTO = 2 };' in header
    assert 'typedef struct { uint32_t color, reserved[7]; } maray_png_color_opts;' in header
    assert 'typedef struct { uint32_t codes, filter, reserved[6]; } maray_png_opts;' in header          # (it did not grow)


def test_the_options_struct_and_the_entry_points():
    assert C.sizeof(M.PngColorOpts) == 32
    assert [getattr(M.PngColorOpts, f).offset for f in ('color', 'reserved')] == [0, 4]
    L = M.lib()
    vp, u32 = C.c_void_p, C.c_uint32
    assert L.maray_hip_png_encode_device_color.argtypes == [C.c_int, vp, u32, u32, vp, vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    assert L.maray_hip_render_png_color.argtypes == [vp, u32, u32, vp, u32, vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    assert L.maray_hip_time_png_encode_color.argtypes == [C.c_int, vp, u32, u32, vp, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_uint64)]
    assert L.maray_hip_png_palette.argtypes == [C.c_int, vp, u32, u32, vp, C.POINTER(u32), vp]
    header = open(HEADER).read()
    for proto in ('int maray_hip_png_encode_device_color(int device, const void *d_rgb8, uint32_t w, uint32_t h, const maray_png_color_opts *opts, '
                  'void *stream, uint8_t **png_out, size_t *n_out);',
                  'int maray_hip_render_png_color(maray_ctx *c, uint32_t w, uint32_t h, const double *values, uint32_t n_frames, '
                  'const maray_png_color_opts *opts, uint8_t **png_out, size_t *n_out);',
                  'int maray_hip_time_png_encode_color(int device, const void *d_rgb8, uint32_t w, uint32_t h, const maray_png_color_opts *opts, '
                  'int reps, float *ms_avg, uint64_t *stream_bytes);',
                  'int maray_hip_png_palette(int device, const void *d_rgb8, uint32_t w, uint32_t h, void *stream, uint32_t *n_colors, '
                  'uint8_t palette[768]);'):
        assert proto in header


def test_python_defaults():
    for f in (M.png_encode_device, M.Context.render_png, M.time_png_encode):
        assert inspect.signature(f).parameters['png_color'].default == M.PNG_COLOR_RGB
    for f in (M.gen, M.gen_animation, M.Context.render_apng, M.apng_encode_device, M.y4m_encode_device):      # they do not take the mode
        assert 'png_color' not in inspect.signature(f).parameters
    assert list(inspect.signature(M.png_palette).parameters) == ['d_ptr', 'w', 'h', 'device', 'stream']


# ---- argument errors ---------------------------------------------------------------------------------------------------------
def _opts(color=0, reserved=None):
    o = M.PngColorOpts()
    o.color = color
    if reserved is not None:
        o.reserved[reserved] = 1
    return o


def _three_calls(o):
    """The three _color entry points on pointers that are never dereferenced: [(return code, message)]."""
    fake = C.c_void_p(0x1000)
    p, sz, ms, nb = C.c_void_p(), C.c_size_t(), C.c_float(), C.c_uint64()
    L = M.lib()
    out = []
    out.append((L.maray_hip_png_encode_device_color(0, fake, 4, 4, C.byref(o), None, C.byref(p), C.byref(sz)), L.maray_last_error().decode()))
    out.append((L.maray_hip_render_png_color(fake, 4, 4, None, 0, C.byref(o), C.byref(p), C.byref(sz)), L.maray_last_error().decode()))
    out.append((L.maray_hip_time_png_encode_color(0, fake, 4, 4, C.byref(o), 1, C.byref(ms), C.byref(nb)), L.maray_last_error().decode()))
    return out


@pytest.mark.parametrize('color', [3, 4, 0x100, 0xFFFFFFFF])
def test_an_unknown_mode_is_an_argument_error_before_a_device_is_looked_for(color):
    for rc, msg in _three_calls(_opts(color)):
        assert rc == E_ARG and 'color' in msg
    with pytest.raises(M.MarayError) as e:
        M.png_encode_device(0x1000, 4, 4, png_color=color)
    assert e.value.code == E_ARG and 'color' in str(e.value)
    with pytest.raises(M.MarayError) as e:
        M.time_png_encode(0x1000, 4, 4, png_color=color)
    assert e.value.code == E_ARG


@pytest.mark.parametrize('word', range(7))
def test_a_reserved_word_that_is_not_zero_is_an_argument_error(word):
    for color in (M.PNG_COLOR_RGB, M.PNG_COLOR_INDEXED, M.PNG_COLOR_AUTO):
        for rc, msg in _three_calls(_opts(color, reserved=word)):
            assert rc == E_ARG and 'reserved' in msg


def test_null_outputs_are_argument_errors():
    L = M.lib()
    fake = C.c_void_p(0x1000)
    o = _opts(M.PNG_COLOR_AUTO)
    assert L.maray_hip_png_encode_device_color(0, fake, 4, 4, C.byref(o), None, None, None) == E_ARG
    assert L.maray_hip_render_png_color(fake, 4, 4, None, 0, C.byref(o), None, None) == E_ARG
    assert L.maray_hip_time_png_encode_color(0, fake, 4, 4, C.byref(o), 1, None, None) == E_ARG
    n, pal = C.c_uint32(), (C.c_uint8 * 768)()
    assert L.maray_hip_png_palette(0, fake, 4, 4, None, None, pal) == E_ARG
    assert L.maray_hip_png_palette(0, fake, 4, 4, None, C.byref(n), None) == E_ARG
    assert L.maray_hip_png_palette(0, None, 4, 4, None, C.byref(n), pal) == E_ARG
    assert L.maray_hip_png_palette(0, fake, 0, 4, None, C.byref(n), pal) == E_ARG


@pytest.mark.parametrize('color', [M.PNG_COLOR_INDEXED, M.PNG_COLOR_AUTO])
def test_python_refuses_codes_and_png_filter_with_a_colour_mode(color):
    """The _color family is fixed codes and filter 0 only; refused in Python, before the library is called."""
    for kw in (dict(codes=M.CODES_DYNAMIC), dict(png_filter=M.PNG_FILTER_ADAPTIVE), dict(codes=M.CODES_DYNAMIC, png_filter=M.PNG_FILTER_UP)):
        with pytest.raises(M.MarayError) as e:
            M.png_encode_device(0x1000, 4, 4, png_color=color, **kw)
        assert e.value.code == E_ARG
        with pytest.raises(M.MarayError) as e:
            M.time_png_encode(0x1000, 4, 4, png_color=color, **kw)
        assert e.value.code == E_ARG
        ctx = M.Context.__new__(M.Context)            # (never initialised: the refusal comes first)
        ctx._h = None
        with pytest.raises(M.MarayError) as e:
            M.Context.render_png(ctx, 4, 4, png_color=color, **kw)
        assert e.value.code == E_ARG


# ---- the model, pinned against decoders that know nothing of it -------------------------------------------------------------
def _model_rasters():
    out = X.byte_runs() + X.small_rasters()
    out += [(name, X.of_colours(keys, 9, 70, seed=i)) for i, (name, keys) in enumerate(X.colour_sets())]
    out += [('%d colours, w %d' % (n, w), X.of_colours(X.n_colours(n, n), 5, w, seed=n)) for n in (1, 2, 3, 4, 5, 16, 17, 255, 256) for w in (1, 7, 64, 300)
            if 5 * w >= n]
    return out


def test_depths():
    assert [X.depth(n) for n in (1, 2, 3, 4, 5, 16, 17, 255, 256)] == [1, 1, 2, 2, 4, 4, 8, 8, 8]
    assert [X.row_bytes(w, 1) for w in (1, 8, 9, 8 * 769 - 7)] == [1, 1, 2, 769]


def test_the_tokeniser_on_hand_made_segments():
    lit, match = (lambda v: ('lit', v)), (lambda n: ('match', n))
    assert X.tokens([5]) == [lit(5)]
    assert X.tokens([5, 5]) == [lit(5), lit(5)]                               # one repeated byte: a literal
    assert X.tokens([5, 5, 5]) == [lit(5), lit(5), lit(5)]                    # two: two literals
    assert X.tokens([5, 5, 5, 5]) == [lit(5), match(3)]
    assert X.tokens([5] * 64) == [lit(5), match(63)]
    assert X.tokens([5] * 65) == [lit(5), match(63), lit(5)]                  # a run is closed at a step's end
    assert X.tokens([5] * 67) == [lit(5), match(63), match(3)]
    assert X.tokens([5] * 130) == [lit(5), match(63), match(64), lit(5), lit(5)]
    assert X.tokens([1, 2, 2, 3, 3, 3, 4, 4, 4, 4]) == [lit(1), lit(2), lit(2), lit(3), lit(3), lit(3), lit(4), match(3)]


def test_the_models_files_pass_every_decoder(tmp_path):
    try:
        from PIL import Image
    except ImportError:
        Image = None
    path = str(tmp_path / 'model.png')
    for name, img in _model_rasters():
        png = X.model_file(img)
        got, pal = X.decode_indexed(png)
        assert np.array_equal(got, img), name
        assert np.array_equal(pal, X.palette(img)), name
        raw = zlib.decompress(P.idat_stream(png))
        assert raw == b''.join(b'\x00' + row.tobytes() for row in X.pack_rows(img)), name
        with open(path, 'wb') as f:
            f.write(png)
        assert np.array_equal(M.png_read(path), img), name
        if Image is not None:
            with Image.open(path) as im:
                assert im.mode == 'P', name
                assert np.array_equal(np.asarray(im.convert('RGB')), img), name


def test_pil_reads_the_models_files(tmp_path):
    Image = pytest.importorskip('PIL.Image')
    path = str(tmp_path / 'model.png')
    for n in (2, 4, 16, 256):
        img = X.of_colours(X.n_colours(n, n), 19, 131, seed=n)
        with open(path, 'wb') as f:
            f.write(X.model_file(img))
        with Image.open(path) as im:
            assert im.mode == 'P' and im.size == (131, 19)
            assert np.array_equal(np.asarray(im.convert('RGB')), img)


def test_the_strict_decoder_refuses_what_is_wrong():
    import struct
    img = X.of_colours(X.n_colours(3), 4, 9)
    png = X.model_file(img)
    cs = P.chunks(png)

    def rebuilt(chunks):
        return P.SIGNATURE + b''.join(X._chunk(k, d) for k, d in chunks)
    assert np.array_equal(X.decode_indexed(rebuilt(cs))[0], img)
    wrong = [
        rebuilt([cs[0], cs[2], cs[1], cs[3]]),                                                        # PLTE behind IDAT
        rebuilt([(b'IHDR', struct.pack('>IIBBBBB', 9, 4, 4, 3, 0, 0, 0))] + cs[1:]),                  # a depth PNG allows, but not the smallest
        rebuilt([cs[0], (b'PLTE', cs[1][1] + b'\x00')] + cs[2:]),                                    # PLTE not a multiple of 3
        rebuilt([cs[0], (b'PLTE', cs[1][1][:6])] + cs[2:]),                                           # an index past the palette
        rebuilt([cs[0], cs[1], (b'IDAT', zlib.compress(b'\x01' + bytes(3) + bytes(12)))] + cs[3:]),   # a filter byte that is not 0
        rebuilt([cs[0], cs[1], (b'IDAT', zlib.compress((b'\x00\x00\x00\x3f') * 4))] + cs[3:]),        # pad bits that are not 0
        rebuilt([cs[0], cs[1], (b'IDAT', zlib.compress(bytes(15)))] + cs[3:]),                        # a short stream
        rebuilt([cs[0], cs[1], (b'IDAT', cs[2][1][:-1] + bytes([cs[2][1][-1] ^ 1]))] + cs[3:]),       # a wrong Adler-32
        png[:40] + bytes([png[40] ^ 1]) + png[41:],                                                   # a wrong CRC
    ]
    for i, bad in enumerate(wrong):
        with pytest.raises((AssertionError, zlib.error)):
            X.decode_indexed(bad)
            pytest.fail('case %d was accepted' % i)


def test_the_chess_fixture_is_smaller_indexed_than_truecolour():
    """The size condition, on the CPU: the model's file of tests/golden/chess.png against the fixed-code truecolour file."""
    chess = M.png_read(os.path.join(HERE, 'golden', 'chess.png'))
    assert chess.shape == (1024, 1024, 3) and len(X.palette(chess)) == 2
    png = X.model_file(chess)
    truecolour = F.fixed_file_size(chess, F.NONE)
    print('chess 1024 x 1024: indexed %d bytes (stream %d), truecolour fixed codes %d' % (len(png), len(P.idat_stream(png)), truecolour))
    assert truecolour == 87109
    assert (len(P.idat_stream(png)), len(png)) == (20429, 20504)
    assert len(png) < truecolour
    assert np.array_equal(X.decode_indexed(png)[0], chess)

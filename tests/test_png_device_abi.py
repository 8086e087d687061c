"""The device PNG encoder's interface, as far as it can be checked without a device (include/maray_hip.h, "device PNG
encoder"): the option word's place in maray_gen_opts, the constants, the argument errors that are reported before a device
is looked for, the CLI flag -- and tests/png_stream.py's decoder itself, pinned against the host writer and against zlib
streams in every filter type."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import maray_amd as M
import png_stream as P

E_ARG, E_LIMIT = -1, -7


def test_gen_opts_keeps_its_size_and_the_encoder_is_its_first_reserved_word():
    assert C.sizeof(M.GenOpts) == 32
    assert M.GenOpts.encoder.offset == 24
    assert M.GenOpts.filter.offset == 20


def test_constants():
    assert (M.ENCODER_HOST, M.ENCODER_DEVICE) == (0, 1)
    assert P.SEG >= 256


def _encode_rc(d_ptr, w, h, out=True, n=True):
    p, sz = C.c_void_p(), C.c_size_t()
    return M.lib().maray_hip_png_encode_device(0, d_ptr, w, h, None, C.byref(p) if out else None, C.byref(sz) if n else None)


def _render_rc(ctx, w, h, out=True, n=True):
    p, sz = C.c_void_p(), C.c_size_t()
    return M.lib().maray_hip_render_png(ctx, w, h, None, 0, C.byref(p) if out else None, C.byref(sz) if n else None)


def test_null_arguments_and_empty_images_are_argument_errors_before_any_device():
    fake = C.c_void_p(0x1000)           # never dereferenced: the checks come first
    assert _encode_rc(None, 4, 4) == E_ARG
    assert _encode_rc(fake, 4, 4, out=False) == E_ARG
    assert _encode_rc(fake, 4, 4, n=False) == E_ARG
    assert _encode_rc(fake, 0, 4) == E_ARG
    assert _encode_rc(fake, 4, 0) == E_ARG
    assert 'empty' in M.lib().maray_last_error().decode()
    assert _render_rc(None, 4, 4) == E_ARG
    assert _render_rc(None, 0, 4) == E_ARG
    assert _render_rc(None, 4, 0) == E_ARG
    assert _render_rc(fake, 4, 4, out=False) == E_ARG
    assert _render_rc(fake, 4, 4, n=False) == E_ARG
    with pytest.raises(M.MarayError) as e:
        M.png_encode_device(0, 4, 4)
    assert e.value.code == E_ARG


def test_sizes_past_the_writers_limits_are_limit_errors_before_any_device():
    fake = C.c_void_p(0x1000)
    assert _encode_rc(fake, (1 << 20) + 1, 1) == E_LIMIT
    assert _encode_rc(fake, 1, (1 << 20) + 1) == E_LIMIT
    assert _encode_rc(fake, 1 << 20, 1 << 20) == E_LIMIT          # (3 w + 1) h > 2^34


def test_gen_refuses_an_unknown_encoder_word(chess_bytes, tmp_path):
    s = M.Scene(chess_bytes)
    with pytest.raises(M.MarayError) as e:
        M.gen(s, str(tmp_path / 'x.png'), encoder=2)
    assert e.value.code == E_ARG
    with pytest.raises(M.MarayError) as e:
        _gen_to_image_with_encoder(s, 7)          # gen_to_image checks the word too (and otherwise ignores it)
    assert e.value.code == E_ARG
    assert not os.path.exists(str(tmp_path / 'x.png'))


def _gen_to_image_with_encoder(scene, word):
    go = M.GenOpts()
    go.backend, go.encoder = M.BACKEND_TAPE_SMEM, word
    img = np.zeros((8, 8, 3), np.uint8)
    rc = M.lib().maray_gen_to_image(scene._h, None, 0, C.byref(go), M.api.Report(0, 0), M.api.REPORT_FN(0), None, img.ctypes.data, 8, 8)
    if rc:
        raise M.MarayError(rc, M.lib().maray_last_error().decode())


def test_cli_refuses_an_unknown_encoder(tmp_path):
    exe = os.path.join(os.path.dirname(M.lib_path()), 'maray')
    out = str(tmp_path / 'x.png')
    r = subprocess.run([exe, '-i', os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'chess.maray'), '-o', out, '--encoder', 'bogus'],
                       capture_output=True, text=True)
    assert r.returncode == 2
    assert '--encoder takes host or device' in r.stderr and 'bogus' in r.stderr
    assert not os.path.exists(out)


@pytest.mark.parametrize('shape', [(1, 1), (3, 5), (37, 65), (2, 300)])
def test_decode_round_trips_the_host_writer(shape, tmp_path):
    img = P.random_bytes(shape[0] * 1000 + shape[1], *shape)
    path = str(tmp_path / 'a.png')
    M.png_write(path, img)
    data = open(path, 'rb').read()
    assert np.array_equal(P.decode(data), img)
    assert np.array_equal(M.png_read(path), img)


def test_decode_unfilters_every_type_like_the_library_reader(tmp_path):
    img = P.random_bytes(5, 11, 23)
    for filters in ([0], [1], [2], [3], [4], [4, 3, 2, 1, 0]):
        data = P.encode_filtered(img, filters)
        assert np.array_equal(P.decode(data), img), filters
        path = str(tmp_path / 'f.png')
        open(path, 'wb').write(data)
        assert np.array_equal(M.png_read(path), img), filters


def test_decode_notices_a_damaged_file(tmp_path):
    img = P.random_bytes(6, 4, 9)
    path = str(tmp_path / 'a.png')
    M.png_write(path, img)
    data = bytearray(open(path, 'rb').read())
    for at in (3, 20, 45, len(data) - 6):
        bad = bytearray(data)
        bad[at] ^= 0x40
        with pytest.raises((AssertionError, Exception)):
            P.decode(bytes(bad))


def test_the_run_rasters_hold_what_they_are_for():
    lengths = set()
    for row in P.all_run_lengths():
        change = np.flatnonzero(np.any(row[1:] != row[:-1], axis=1)) + 1
        lengths |= set(np.diff(np.concatenate([[0], change, [len(row)]])).tolist())
    assert set(range(1, 201)) <= lengths
    starts, ends = set(), set()
    for row in P.runs_modulo_64():
        eq = np.all(row[1:] == row[:-1], axis=1)
        at = np.flatnonzero(eq)
        if len(at):
            starts.add(int(at[0]) % 64)             # the first pixel that equals the one before it
            ends.add(int(at[-1] + 2) % 64)          # the first pixel after the run
    assert len(starts) == 64 and len(ends) == 64
    for c in range(3):
        img = P.one_channel_steps(c)
        other = [k for k in range(3) if k != c]
        assert np.all(img[0, 1:, other] == img[0, :-1, other]) and np.all(img[0, 1:, c] != img[0, :-1, c])
    wrap = P.row_wrap()
    assert all(np.array_equal(wrap[y, -1], wrap[y + 1, 0]) for y in range(8))

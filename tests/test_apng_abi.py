"""The animation writer's interface, as far as it can be checked without a device (include/maray_hip.h, "animation"): the
ctypes signatures, the argument and limit errors that are reported before a device is looked for, the CLI's usage errors --
and tests/apng_stream.py's decoder itself, pinned against APNGs built in Python with zlib.compress and against the mutants
it must reject."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import apng_stream as A
import maray_amd as M
import png_stream as P

E_ARG, E_LIMIT = -1, -7
HERE = os.path.dirname(os.path.abspath(__file__))
CHESS = os.path.join(HERE, 'golden', 'chess.maray')


# ---- the decoder -----------------------------------------------------------------------------------------------------------
def moving_frames(n=4, h=9, w=13, seed=3):
    """n frames: a random first one, then each the one before with a random sub-rectangle replaced (one frame unchanged)."""
    rng = np.random.default_rng(seed)
    frames = [P.random_bytes(seed, h, w)]
    for i in range(1, n):
        f = frames[-1].copy()
        if i != 2:
            y0, x0 = int(rng.integers(0, h - 1)), int(rng.integers(0, w - 1))
            y1, x1 = int(rng.integers(y0 + 1, h + 1)), int(rng.integers(x0 + 1, w + 1))
            f[y0:y1, x0:x1] = 255 - f[y0:y1, x0:x1]
        frames.append(f)
    return frames


@pytest.mark.parametrize('filters', [(0,), (1,), (2,), (3,), (4,), (4, 3, 2, 1, 0)])
def test_decode_composes_frames_of_every_filter_type(filters):
    frames = moving_frames()
    d = A.decode(A.build(frames, filters=filters, delay=(2, 50), plays=7))
    assert len(d.frames) == len(frames) and all(np.array_equal(a, b) for a, b in zip(d.frames, frames))
    assert d.rects == [(0, 0, 13, 9)] + [A.rect_of(A.bounding_box(frames[i - 1], frames[i])) for i in range(1, 4)]
    assert d.rects[2] == (0, 0, 1, 1)               # the unchanged frame
    assert d.delay == (2, 50) and d.plays == 7


def test_decode_joins_fdat_chunks():
    frames = [P.random_bytes(s, 30, 40) for s in (5, 6, 7)]           # every stream some kilobytes long
    whole, split = A.build(frames), A.build(frames, fdat_limit=17)
    assert sum(k == b'fdAT' for k, _ in P.chunks(split)) > sum(k == b'fdAT' for k, _ in P.chunks(whole)) + 2
    d = A.decode(split)
    assert all(np.array_equal(a, b) for a, b in zip(d.frames, frames))
    assert d.streams == A.decode(whole).streams


def test_decode_takes_a_single_frame_and_a_one_by_one_canvas():
    one = [P.random_bytes(1, 1, 1)]
    assert np.array_equal(A.decode(A.build(one)).frames[0], one[0])
    two = [P.random_bytes(1, 1, 1), P.random_bytes(2, 1, 1)]
    d = A.decode(A.build(two))
    assert d.rects == [(0, 0, 1, 1)] * 2 and np.array_equal(d.frames[1], two[1])
    assert np.array_equal(P.decode(A.build(one)), one[0])           # a PNG reader that skips unknown chunks shows frame 0


@pytest.mark.parametrize('mutant', [dict(seq_gap_at=1), dict(seq_gap_at=2), dict(bad_crc=b'fcTL'), dict(bad_crc=b'fdAT'), dict(bad_crc=b'acTL'),
                                    dict(grow_rect=1), dict(actl_count=5), dict(actl_count=3), dict(trailing=0), dict(trailing=3)],
                         ids=lambda m: '%s=%s' % next(iter(m.items())))
def test_decode_rejects(mutant):
    frames = moving_frames()
    A.decode(A.build(frames))
    with pytest.raises(AssertionError):
        A.decode(A.build(frames, **mutant))


def test_decode_rejects_a_damaged_adler():
    data = bytearray(A.build(moving_frames()))
    cs = P.chunks(bytes(data))
    at = 8
    for kind, body in cs:               # the last fdAT: spoil its stream's last byte and mend the chunk's CRC
        if kind == b'fdAT':
            last = at
            n = len(body)
        at += 12 + len(body)
    data[last + 8 + n - 1] ^= 1
    crc = __import__('zlib').crc32(bytes(data[last + 4:last + 8 + n])) & 0xFFFFFFFF
    data[last + 8 + n:last + 12 + n] = crc.to_bytes(4, 'big')
    with pytest.raises((AssertionError, Exception)):
        A.decode(bytes(data))


# ---- signatures ------------------------------------------------------------------------------------------------------------
def test_the_ctypes_signatures_are_the_headers():
    header = open(os.path.join(os.path.dirname(HERE), 'include', 'maray_hip.h')).read()
    L = M.lib()
    for name, n_args in (('maray_hip_frame_delta', 7), ('maray_hip_apng_encode_device', 11), ('maray_hip_render_apng', 11),
                         ('maray_hip_time_frame_delta', 5), ('maray_hip_time_frame_delta_copy', 6), ('maray_gen_animation', 10)):
        m = re.search(r'int %s\(([^;]*)\);' % name, header)
        assert m, name
        assert len(m.group(1).split(',')) == n_args, name
        fn = getattr(L, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == n_args, name
    assert all(callable(f) for f in (M.frame_delta, M.apng_encode_device, M.gen_animation, M.time_frame_delta, M.Context.render_apng))


# ---- errors before any device ----------------------------------------------------------------------------------------------
def _encode_rc(d_ptr, n, w, h, num=1, den=25, out=True, size=True):
    p, sz = C.c_void_p(), C.c_size_t()
    return M.lib().maray_hip_apng_encode_device(0, d_ptr, n, w, h, num, den, 0, None, C.byref(p) if out else None, C.byref(sz) if size else None)


def _render_rc(ctx, n, w=4, h=4, num=1, den=25, out=True, size=True):
    p, sz = C.c_void_p(), C.c_size_t()
    return M.lib().maray_hip_render_apng(ctx, w, h, None, n, 1, num, den, 0, C.byref(p) if out else None, C.byref(sz) if size else None)


def test_argument_errors_come_before_any_device():
    fake = C.c_void_p(0x1000)           # never dereferenced: the checks come first
    assert _encode_rc(None, 2, 4, 4) == E_ARG
    assert _encode_rc(fake, 2, 4, 4, out=False) == E_ARG
    assert _encode_rc(fake, 2, 4, 4, size=False) == E_ARG
    assert _encode_rc(fake, 0, 4, 4) == E_ARG
    assert 'at least one image' in M.lib().maray_last_error().decode()
    assert _encode_rc(fake, 2, 4, 4, num=65536) == E_ARG
    assert _encode_rc(fake, 2, 4, 4, den=65536) == E_ARG
    assert '16 bits' in M.lib().maray_last_error().decode()
    assert _encode_rc(fake, 2, 0, 4) == E_ARG
    assert _encode_rc(fake, 2, 4, 0) == E_ARG
    assert 'empty' in M.lib().maray_last_error().decode()
    assert _render_rc(None, 2) == E_ARG
    assert _render_rc(fake, 2, out=False) == E_ARG
    assert _render_rc(fake, 2, size=False) == E_ARG
    box = (C.c_uint32 * 4)()
    assert M.lib().maray_hip_frame_delta(0, None, fake, 4, 4, None, box) == E_ARG
    assert M.lib().maray_hip_frame_delta(0, fake, None, 4, 4, None, box) == E_ARG
    assert M.lib().maray_hip_frame_delta(0, fake, fake, 4, 4, None, None) == E_ARG
    assert M.lib().maray_hip_frame_delta(0, fake, fake, 0, 4, None, box) == E_ARG
    assert M.lib().maray_hip_time_frame_delta(0, 4, 4, 1, None) == E_ARG
    with pytest.raises(M.MarayError) as e:
        M.apng_encode_device(0, 2, 4, 4)
    assert e.value.code == E_ARG


def test_limit_errors_come_before_any_device():
    fake = C.c_void_p(0x1000)
    box = (C.c_uint32 * 4)()
    assert _encode_rc(fake, 2, (1 << 20) + 1, 1) == E_LIMIT
    assert _encode_rc(fake, 2, 1, (1 << 20) + 1) == E_LIMIT
    assert _encode_rc(fake, 2, 1 << 15, (1 << 15) // 3 + 1) == E_LIMIT          # 3 w h just above 2^30
    assert '2^30' in M.lib().maray_last_error().decode()
    assert M.lib().maray_hip_frame_delta(0, fake, fake, 1 << 15, (1 << 15) // 3 + 1, None, box) == E_LIMIT


def test_gen_animation_checks_its_arguments_before_any_device(chess_bytes, tmp_path):
    s = M.Scene(chess_bytes)
    out = str(tmp_path / 'a.png')
    L = M.lib()
    go = M.GenOpts()
    go.backend = M.BACKEND_TAPE_SMEM

    def rc(scene=s._h, n=2, num=1, den=25, path=os.fsencode(out)):
        return L.maray_gen_animation(scene, None, 0, C.byref(go), None, n, num, den, 0, path)
    assert rc(scene=None) == E_ARG
    assert rc(path=None) == E_ARG
    assert rc(n=0) == E_ARG
    assert rc(num=65536) == E_ARG
    assert rc(den=70000) == E_ARG
    go.n_devices = 2
    assert rc() == E_ARG
    assert 'one device' in L.maray_last_error().decode()
    go.n_devices, go.shutter = 0, 3
    assert rc() == E_ARG
    assert not os.path.exists(out)
    t = M.Scene(chess_bytes)
    t.declare_param('t', -1.0, 1.0)
    with pytest.raises(M.MarayError) as e:          # a scene with a declared parameter and no values
        M.gen_animation(t, out, np.zeros((2, 3)))
    assert e.value.code == E_ARG
    assert not os.path.exists(out)


# ---- the CLI's usage errors ------------------------------------------------------------------------------------------------
def _cli(*args):
    exe = os.path.join(os.path.dirname(M.lib_path()), 'maray')
    return subprocess.run([exe, '-i', CHESS] + list(args), capture_output=True, text=True)


def test_cli_usage_errors_in_both_directions(tmp_path):
    numbered, plain = str(tmp_path / 'f%03d.png'), str(tmp_path / 'a.png')
    r = _cli('-o', numbered, '--animate', 't=0:1:3', '--apng')
    assert r.returncode == 2 and '--apng writes one file' in r.stderr and '%d' in r.stderr
    r = _cli('-o', plain, '--apng')
    assert r.returncode == 2 and '--apng writes an animation' in r.stderr and '--animate' in r.stderr
    r = _cli('-o', plain, '--animate', 't=0:1:3', '--apng', '--gpus', '2')
    assert r.returncode == 2 and '--gpus must be 1' in r.stderr
    r = _cli('-o', plain, '--animate', 't=0:1:3')            # without --apng: the error as it always read
    assert r.returncode == 2
    assert r.stderr == 'Error: --animate writes several images: --output needs one `%d` conversion, e.g. frame%03d.png\n'
    for bad in (['--fps', '0'], ['--fps', '30/0'], ['--fps', '30/x'], ['--fps', '70000'], ['--loops', '-1'], ['--loops', 'x']):
        r = _cli('-o', plain, '--animate', 't=0:1:3', '--apng', *bad)
        assert r.returncode == 2 and bad[0] + ' takes' in r.stderr, bad
    assert not os.listdir(str(tmp_path))
    assert '--apng' in _cli('-o', plain, '--help').stdout + _cli('-o', plain, '--help').stderr

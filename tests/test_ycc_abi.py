"""The raw-video interface as far as it can be checked without a device (include/maray_hip.h, "raw video"): the ctypes
signatures, struct sizes and constants against the header, every argument and limit error that is reported before a device is
looked for, and the CLI's usage errors."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import maray_amd as M
import ycc_model as Y

E_ARG, E_LIMIT = -1, -7
HERE = os.path.dirname(os.path.abspath(__file__))
CHESS = os.path.join(HERE, 'golden', 'chess.maray')
HEADER = open(os.path.join(os.path.dirname(HERE), 'include', 'maray_hip.h')).read()


# ---- signatures, structs, constants ----------------------------------------------------------------------------------------
def test_the_ctypes_signatures_are_the_headers():
    L = M.lib()
    for name, n_args in (('maray_ycc_frame_bytes', 4), ('maray_hip_rgb_to_ycc', 7), ('maray_hip_y4m_encode_device', 11), ('maray_hip_render_y4m', 11),
                         ('maray_hip_time_rgb_to_ycc', 7), ('maray_gen_animation_ex', 11)):
        m = re.search(r'int %s\(([^;]*)\);' % name, HEADER)
        assert m, name
        assert len(m.group(1).split(',')) == n_args, name
        fn = getattr(L, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == n_args, name
    assert all(callable(f) for f in (M.ycc_frame_bytes, M.rgb_to_ycc, M.y4m_encode_device, M.time_rgb_to_ycc, M.gen_animation, M.Context.render_y4m))


def test_struct_sizes_and_constants():
    assert C.sizeof(M.YccOpts) == 32 and C.sizeof(M.AnimOpts) == 32
    assert [f[0] for f in M.YccOpts._fields_] == ['sampling', 'matrix', 'reserved']
    assert [f[0] for f in M.AnimOpts._fields_] == ['container', 'sampling', 'matrix', 'reserved']
    assert re.search(r'typedef struct maray_ycc_opts \{ uint32_t sampling, matrix, reserved\[6\]; \} maray_ycc_opts;', HEADER)
    assert re.search(r'typedef struct maray_anim_opts \{ uint32_t container, sampling, matrix, reserved\[5\]; \} maray_anim_opts;', HEADER)
    for name, value in (('MARAY_YCC_420', M.YCC_420), ('MARAY_YCC_444', M.YCC_444), ('MARAY_YCC_BT601', M.YCC_BT601), ('MARAY_YCC_BT709', M.YCC_BT709),
                        ('MARAY_CONTAINER_APNG', M.CONTAINER_APNG), ('MARAY_CONTAINER_Y4M', M.CONTAINER_Y4M)):
        m = re.search(r'#define %s (\d+)u\n' % name, HEADER)
        assert m and int(m.group(1)) == value, name
    assert (M.YCC_420, M.YCC_444, M.YCC_BT601, M.YCC_BT709, M.CONTAINER_APNG, M.CONTAINER_Y4M) == (0, 1, 0, 1, 0, 1)
    assert (Y.YCC_420, Y.YCC_444, Y.BT601, Y.BT709) == (M.YCC_420, M.YCC_444, M.YCC_BT601, M.YCC_BT709)


# ---- errors before any device ----------------------------------------------------------------------------------------------
FAKE = C.c_void_p(0x1000)               # never dereferenced: the checks come first


def opts(sampling=0, matrix=0, reserved=None):
    o = M.YccOpts()
    o.sampling, o.matrix = sampling, matrix
    if reserved is not None:
        o.reserved[reserved] = 1
    return o


def _convert_rc(src=FAKE, dst=FAKE, w=4, h=4, o=None):
    return M.lib().maray_hip_rgb_to_ycc(0, src, w, h, C.byref(o) if o is not None else None, dst, None)


def _encode_rc(d_ptr=FAKE, n=2, w=4, h=4, num=1, den=25, o=None, out=True, size=True):
    p, sz = C.c_void_p(), C.c_size_t()
    return M.lib().maray_hip_y4m_encode_device(0, d_ptr, n, w, h, num, den, C.byref(o) if o is not None else None, None,
                                               C.byref(p) if out else None, C.byref(sz) if size else None)


def _render_rc(ctx=None, n=2, w=4, h=4, num=1, den=25, o=None, out=True, size=True):
    p, sz = C.c_void_p(), C.c_size_t()
    return M.lib().maray_hip_render_y4m(ctx, w, h, None, n, 1, num, den, C.byref(o) if o is not None else None, C.byref(p) if out else None,
                                        C.byref(sz) if size else None)


def last():
    return M.lib().maray_last_error().decode()


def test_conversion_argument_errors_come_before_any_device():
    assert _convert_rc(src=None) == E_ARG and _convert_rc(dst=None) == E_ARG
    assert _convert_rc(w=0) == E_ARG and _convert_rc(h=0) == E_ARG and 'empty' in last()
    assert _convert_rc(o=opts(sampling=2)) == E_ARG and 'sampling' in last()
    assert _convert_rc(o=opts(matrix=2)) == E_ARG and 'matrix' in last()
    for r in range(6):
        assert _convert_rc(o=opts(reserved=r)) == E_ARG and 'reserved' in last()
    n = C.c_size_t()
    assert M.lib().maray_ycc_frame_bytes(4, 4, 0, None) == E_ARG
    assert M.lib().maray_ycc_frame_bytes(4, 4, 7, C.byref(n)) == E_ARG
    ms = C.c_float()
    assert M.lib().maray_hip_time_rgb_to_ycc(0, 4, 4, None, 1, None, None) == E_ARG
    assert M.lib().maray_hip_time_rgb_to_ycc(0, 4, 4, C.byref(opts(sampling=3)), 1, C.byref(ms), None) == E_ARG
    assert M.lib().maray_hip_time_rgb_to_ycc(0, 0, 4, None, 1, C.byref(ms), None) == E_ARG
    assert M.lib().maray_hip_time_rgb_to_ycc(0, 4, 4, None, 0, C.byref(ms), None) == E_ARG
    with pytest.raises(M.MarayError) as e:
        M.rgb_to_ycc(0, 4, 4, 0x1000)
    assert e.value.code == E_ARG


def test_writer_argument_errors_come_before_any_device():
    assert _encode_rc(d_ptr=None) == E_ARG
    assert _encode_rc(out=False) == E_ARG and _encode_rc(size=False) == E_ARG
    assert _encode_rc(n=0) == E_ARG and 'at least one image' in last()
    assert _encode_rc(num=0) == E_ARG and 'delay_num' in last()
    assert _encode_rc(num=65536) == E_ARG and _encode_rc(den=65536) == E_ARG and '16 bits' in last()
    assert _encode_rc(w=0) == E_ARG and _encode_rc(h=0) == E_ARG and 'empty' in last()
    assert _encode_rc(o=opts(sampling=2)) == E_ARG and _encode_rc(o=opts(matrix=5)) == E_ARG
    assert _encode_rc(o=opts(reserved=5)) == E_ARG and _encode_rc(o=opts(reserved=0)) == E_ARG
    assert _render_rc(ctx=None) == E_ARG and 'context' in last()
    assert _render_rc(ctx=FAKE, out=False) == E_ARG and _render_rc(ctx=FAKE, size=False) == E_ARG
    assert _render_rc(ctx=FAKE, n=0) == E_ARG
    assert _render_rc(ctx=FAKE, num=0) == E_ARG and _render_rc(ctx=FAKE, num=70000) == E_ARG and _render_rc(ctx=FAKE, den=70000) == E_ARG
    assert _render_rc(ctx=FAKE, w=0) == E_ARG and _render_rc(ctx=FAKE, h=0) == E_ARG
    assert _render_rc(ctx=FAKE, o=opts(sampling=9)) == E_ARG and _render_rc(ctx=FAKE, o=opts(matrix=9)) == E_ARG
    assert _render_rc(ctx=FAKE, o=opts(reserved=3)) == E_ARG
    with pytest.raises(M.MarayError) as e:
        M.y4m_encode_device(0, 2, 4, 4)
    assert e.value.code == E_ARG


def test_limit_errors_come_before_any_device():
    big = (1 << 20) + 1
    assert _convert_rc(w=big, h=1) == E_LIMIT and _convert_rc(w=1, h=big) == E_LIMIT
    assert _convert_rc(w=1 << 15, h=(1 << 15) // 3 + 1) == E_LIMIT and '2^30' in last()       # 3 w h just above 2^30
    assert _encode_rc(w=big, h=1) == E_LIMIT and _encode_rc(w=1, h=big) == E_LIMIT
    assert _encode_rc(w=1 << 15, h=(1 << 15) // 3 + 1) == E_LIMIT and '2^30' in last()
    assert _render_rc(ctx=FAKE, w=big, h=1) == E_LIMIT and _render_rc(ctx=FAKE, w=1 << 15, h=(1 << 15) // 3 + 1) == E_LIMIT
    ms = C.c_float()
    assert M.lib().maray_hip_time_rgb_to_ycc(0, big, 1, None, 1, C.byref(ms), None) == E_LIMIT


def test_gen_animation_ex_checks_its_arguments_before_any_device(chess_bytes, tmp_path):
    s = M.Scene(chess_bytes)
    out = str(tmp_path / 'a.y4m')
    L = M.lib()
    go = M.GenOpts()
    go.backend = M.BACKEND_TAPE_SMEM
    ao = M.AnimOpts()
    ao.container = M.CONTAINER_Y4M

    def rc(scene=s._h, n=2, num=1, den=25, path=os.fsencode(out), a=ao):
        return L.maray_gen_animation_ex(scene, None, 0, C.byref(go), None, n, num, den, 0, C.byref(a) if a is not None else None, path)
    assert rc(scene=None) == E_ARG and rc(path=None) == E_ARG
    assert rc(n=0) == E_ARG
    assert rc(num=0) == E_ARG and 'delay_num' in last()
    assert rc(num=65536) == E_ARG and rc(den=70000) == E_ARG
    for field, word in (('container', 'container'), ('sampling', 'sampling'), ('matrix', 'matrix')):
        bad = M.AnimOpts()
        bad.container = M.CONTAINER_Y4M
        setattr(bad, field, 2)
        assert rc(a=bad) == E_ARG and word in last(), field
    for r in range(5):
        bad = M.AnimOpts()
        bad.container = M.CONTAINER_Y4M
        bad.reserved[r] = 1
        assert rc(a=bad) == E_ARG and 'reserved' in last()
    go.n_devices = 2
    assert rc() == E_ARG and 'one device' in last()
    go.n_devices, go.shutter = 0, 3
    assert rc() == E_ARG
    go.shutter = 0
    # the APNG container takes delay_num = 0, as maray_gen_animation does: the check is the Y4M container's
    apng = M.AnimOpts()
    if M.device_count() == 0:
        assert rc(num=0, a=apng) not in (0, E_ARG) and rc(num=0, a=None) not in (0, E_ARG)
        assert rc() not in (0, E_ARG, E_LIMIT)             # well-formed: it gets as far as the device
    t = M.Scene(chess_bytes)
    t.declare_param('t', -1.0, 1.0)
    with pytest.raises(M.MarayError) as e:          # a scene with a declared parameter and no values
        M.gen_animation(t, out, np.zeros((2, 3)), container=M.CONTAINER_Y4M)
    assert e.value.code == E_ARG
    assert not os.path.exists(out)


# ---- the CLI's usage errors ------------------------------------------------------------------------------------------------
def _cli(*args):
    exe = os.path.join(os.path.dirname(M.lib_path()), 'maray')
    return subprocess.run([exe, '-i', CHESS] + list(args), capture_output=True, text=True)


def test_cli_usage_errors(tmp_path):
    numbered, plain = str(tmp_path / 'f%03d.y4m'), str(tmp_path / 'a.y4m')
    anim = ('--animate', 't=0:1:3')
    for args, word in ((('-o', plain, '--y4m'), '--animate'),
                       (('-o', plain, '--y4m', '--apng') + anim, '--apng'),
                       (('-o', numbered, '--y4m') + anim, '%d'),
                       (('-o', plain, '--y4m', '--gpus', '2') + anim, '--gpus must be 1'),
                       (('-o', plain, '--y4m-sampling', '444') + anim, 'need --y4m'),
                       (('-o', plain, '--y4m-matrix', '709', '--apng') + anim, 'need --y4m'),
                       (('-o', plain, '--y4m', '--y4m-sampling', '422') + anim, '--y4m-sampling takes'),
                       (('-o', plain, '--y4m', '--y4m-matrix', '2020') + anim, '--y4m-matrix takes'),
                       (('-o', plain, '--y4m', '--fps', '0') + anim, '--fps takes')):
        r = _cli(*args)
        assert r.returncode == 2 and word in r.stderr and 'Usage' in r.stderr, (args, r.stderr[:300])
    assert not os.listdir(str(tmp_path))
    text = _cli('-o', plain, '--help')
    assert text.returncode == 0
    for option in ('--y4m ', '--y4m-sampling', '--y4m-matrix'):
        assert option in text.stdout + text.stderr, option


def test_a_well_formed_y4m_line_reaches_the_device(tmp_path):
    """Without a device that is where it ends (exit 1, no file); with one, the file is the model's of the library's own renders
    -- the same command line is compared frame by frame in tests/test_gpu_ycc.py."""
    out = str(tmp_path / 'a.y4m')
    r = _cli('-o', out, '--y4m', '--animate', 't=0:1:2', '--y4m-sampling', '444', '--y4m-matrix', '709', '--fps', '30000/1001', '--gpus', '1',
             '--backend', 'tape-smem')
    if M.device_count() == 0:
        assert r.returncode == 1 and 'no HIP device' in r.stderr and 'Usage' not in r.stderr
        assert not os.path.exists(out)
    else:
        assert r.returncode == 0, r.stderr[-2000:]
        d = Y.parse(open(out, 'rb').read())
        assert (d.w, d.h, d.fps, d.sampling, len(d.frames)) == M.Scene(open(CHESS, 'rb').read()).size + ((30000, 1001), Y.YCC_444, 2)

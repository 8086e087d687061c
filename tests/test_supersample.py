"""Supersampling without a GPU: the scene transform (maray_scene_supersample), its exactness in the oracle, the
argument checks that precede any device, and the CLI's option.  The device side is tests/test_gpu_supersample.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import maray_amd as M
import scenes
from marayb import add, decode, encode, let_, mul, nat, neg, recip, sin, sqrt, step, ln, subst_xy_deep, var, x, y
from oracle_ffi import Scene as OScene

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
E_ARG, E_LIMIT = -1, -7


def chess_bytes():
    with open(os.path.join(HERE, 'golden', 'chess.maray'), 'rb') as f:
        return f.read()


def expected_transform(data, k):
    """The substitution of include/maray_hip.h built independently: X -> X * 1/k + -((k-1) * 1/(2k)), Y alike, size * k."""
    (w, h), color = decode(data)
    def centred(v):
        return add(mul(v, recip(nat(k))), neg(mul(nat(k - 1), recip(nat(2 * k)))))
    p = [centred(x()), centred(y())]
    return encode((w * k, h * k), [subst_xy_deep(c, p) for c in color])


def let_scene():
    u = var('u')
    body = let_([(u[1], mul(sin(x()), sqrt(y())))], add(u, step(add(x(), neg(y())))))
    return encode((13, 9), [body, mul(x(), y()), let_([(u[1], ln(add(x(), nat(1))))], mul(u, nat(40)))])


@pytest.mark.parametrize('k', [2, 4, 8])
@pytest.mark.parametrize('name', ['chess', 'all_ops', 'let'])
def test_transform_bytes_equal_the_substitution_built_independently(name, k):
    data = {'chess': chess_bytes, 'all_ops': lambda: encode((31, 17), scenes.all_ops(31, 17)), 'let': let_scene}[name]()
    s = M.Scene(data)
    w, h = s.size
    s.supersample(k)
    assert s.size == (w * k, h * k)
    assert s.encode() == expected_transform(data, k)


def test_supersample_by_one_or_zero_changes_nothing():
    data = encode((13, 9), scenes.all_ops(13, 9))
    for k in (0, 1):
        s = M.Scene(data)
        s.supersample(k)
        assert s.encode() == data


def sample_coords(n, k):
    """Sample index -> exact coordinate px + (2i + 1 - k) / (2k)."""
    idx = np.arange(n * k)
    return (idx // k) + (2 * (idx % k) + 1 - k) / (2.0 * k)


def same_f64(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.array_equal(a.view(np.uint64), b.view(np.uint64)) or np.array_equal(a, b, equal_nan=True) and \
        np.array_equal(np.signbit(a), np.signbit(b))


SMALL = {
    'all_ops': (lambda: (encode((7, 5), scenes.all_ops(7, 5)), None)),
    'shapes_through_inf_and_nan': (lambda: (encode((9, 6), scenes.shapes_through_inf_and_nan()), None)),
    'ops_on_a_guarded_mask': (lambda: (encode((11, 7), scenes.ops_on_a_guarded_mask(11, 7)), scenes.textures(8))),
    'textured': (lambda: (encode((9, 5), scenes.textured(9)), scenes.textures(8))),
    'transforms': (lambda: (encode((8, 8), scenes.transforms(8)), None)),
}


@pytest.mark.parametrize('k', [2, 4, 8])
@pytest.mark.parametrize('name', sorted(SMALL))
def test_oracle_sees_the_exact_sample_coordinates(name, k):
    """The oracle's plain render of the supersampled scene = eval2 of the ORIGINAL scene at px + (2i+1-k)/(2k), on every
    sample: the transform is exact, so any back-end that renders it right samples the right points."""
    data, tex = SMALL[name]()
    s = M.Scene(data)
    w, h = s.size
    s.supersample(k)
    _, got = OScene(s.encode()).render_rows(w * k, h * k, 0, h * k, textures=tex)
    orig = OScene(data)
    xs, ys = sample_coords(w, k), sample_coords(h, k)
    want = np.array([[[orig.eval2(c, float(xv), float(yv), textures=tex) for c in range(3)] for xv in xs] for yv in ys])
    assert same_f64(got, want)


def test_bad_factor_and_overflow_leave_the_scene_unchanged():
    data = encode((13, 9), scenes.all_ops(13, 9))
    s = M.Scene(data)
    for k in (3, 5, 16, 0x80000002):
        with pytest.raises(M.MarayError) as e:
            s.supersample(k)
        assert e.value.code == E_ARG
        assert s.encode() == data
    big = M.Scene(data)
    big.set_size(1 << 31, 4)
    before = big.encode()
    with pytest.raises(M.MarayError):
        big.supersample(2)
    assert big.encode() == before


def rc_of(fn):
    try:
        fn()
    except M.MarayError as e:
        return e.code
    return 0


def test_gen_to_image_checks_samples_before_any_device():
    s = M.Scene(encode((13, 9), scenes.all_ops(13, 9)))
    assert rc_of(lambda: M.gen_to_image(s, size=(13, 9), samples=3)) == E_ARG
    assert rc_of(lambda: M.gen_to_image(s, size=(13, 9), samples=5, backend=M.BACKEND_JIT)) == E_ARG
    assert rc_of(lambda: M.gen_to_image(s, size=((1 << 20) // 4 + 1, 1), samples=4)) == E_LIMIT
    assert rc_of(lambda: M.gen_to_image(s, size=(1, (1 << 19) + 1), samples=2)) == E_LIMIT


def test_context_checks_samples_before_any_device():
    tape = M.Scene(encode((13, 9), scenes.all_ops(13, 9))).lower()
    assert rc_of(lambda: M.Context(tape, samples=3)) == E_ARG
    assert rc_of(lambda: M.Context(tape, samples=16)) == E_ARG
    assert rc_of(lambda: M.Context(tape, samples=6, backend=M.BACKEND_JIT)) == E_ARG


def jit_samples(tape, k):
    L = M.lib()
    L.maray_jit_source_samples.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]
    L.maray_jit_build_samples.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    src = C.c_void_p()
    rc = L.maray_jit_source_samples(C.byref(tape.program), k, C.byref(src))
    if rc:
        return rc, None, None
    text = C.string_at(src).decode()
    L.maray_free(src)
    code, n = C.c_void_p(), C.c_size_t()
    assert L.maray_jit_build_samples(C.byref(tape.program), k, C.byref(code), C.byref(n)) == 0, L.maray_last_error().decode()
    blob = C.string_at(code, n.value)
    L.maray_free(code)
    return 0, text, blob


def offline_scenes():
    from test_gpu_launches import tri_soup
    return {'all_ops': encode((64, 64), scenes.all_ops(64, 64)), 'textured': encode((64, 64), scenes.textured(64)),
            'chess': chess_bytes(), 'tri_soup': encode((150, 70), tri_soup(2, [(0, 150, 0, 70, 12, 30)], 150, 70))}


@pytest.mark.parametrize('k', [2, 4, 8])
@pytest.mark.parametrize('name', ['all_ops', 'textured', 'chess', 'tri_soup'])
def test_jit_supersampling_kernel_builds_offline(name, k, tmp_path, monkeypatch):
    monkeypatch.setenv('MARAY_CACHE_DIR', str(tmp_path))
    s = M.Scene(offline_scenes()[name])
    s.supersample(k)
    tape = s.lower()
    L = M.lib()
    L.maray_jit_source.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    plain = C.c_void_p()
    assert L.maray_jit_source(C.byref(tape.program), C.byref(plain)) == 0
    plain_text = C.string_at(plain).decode()
    L.maray_free(plain)
    rc, text, blob = jit_samples(tape, k)
    assert rc == 0
    assert 'maray_jit_pixels_ss' in text and 'maray_jit_pixels_ss' not in plain_text
    assert 'mr_j < %du' % k in text and 'MR_SIN_HUGE' not in text and 'mr_stepsin_fast' not in text
    assert blob[:4] == b'\x7fELF' and len(blob) > 4096
    assert any(f.endswith('.mrss') for f in os.listdir(tmp_path))


def test_jit_supersampling_source_refuses_other_factors():
    tape = M.Scene(encode((13, 9), scenes.all_ops(13, 9))).lower()
    for k in (0, 1, 3, 16):
        assert jit_samples(tape, k)[0] == E_ARG


def test_ctypes_option_structs_keep_their_size():
    from maray_amd.api import CtxOpts, GenOpts
    assert C.sizeof(CtxOpts) == 32 and CtxOpts.samples.offset == 8
    assert C.sizeof(GenOpts) == 32 and GenOpts.samples.offset == 12


@pytest.mark.parametrize('bad', ['3', '0x', '16', ''])
def test_cli_refuses_bad_samples(bad, tmp_path):
    r = subprocess.run([os.path.join(ROOT, 'maray_amd', 'maray'), '-s', bad, '-i', os.path.join(HERE, 'golden', 'chess.maray'),
                        '-o', str(tmp_path / 'out.png')], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
    assert '--samples' in r.stderr
    assert not (tmp_path / 'out.png').exists()


def test_cli_usage_lists_samples():
    r = subprocess.run([os.path.join(ROOT, 'maray_amd', 'maray'), '--help'], capture_output=True, text=True, timeout=60)
    assert '-s, --samples <k>' in r.stderr

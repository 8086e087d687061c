"""The dense-argument scenes of tests/dense_values.py on the CPU: the numpy model of their arguments is the oracle's, the
arguments fill every branch class of the device's arithmetic, the oracle's values are nearly all finite and distinct, the
lowering keeps them on every pixel, and the generated kernels name the functions, hold the constants and are built with the
contraction setting the scenes are there to test.  tests/test_gpu_dense.py runs the same scenes on the device."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import dense_values as D
import maray_amd as M
import tape_eval
from params import as_v2, same_f64
from test_edges import pixel_source
from test_gpu_launches import jit_shape

CELLS = [(n, f) for n in D.NAMES for f in D.FORMS]
IDS = ['%s-%s' % c for c in CELLS]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rows_source(tape):
    L = M.lib()
    L.maray_jit_source_rows.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)]
    src, k = C.c_void_p(), C.c_uint32()
    assert L.maray_jit_source_rows(C.byref(tape.program), C.byref(src), C.byref(k)) == 0, L.maray_last_error()
    text = C.string_at(src).decode()
    L.maray_free(src)
    return text


def v_plane(name, p=None):
    return D.arguments_np(name, 'x', p)[..., 0].ravel()


# ---- the inputs ------------------------------------------------------------------------------------------------------
def test_mantissas_are_dense():
    """Full mantissas: all 52 fraction bits take both values, about half the time each, and no two pixels share one."""
    m = D.mantissa_np(0, np.arange(D.W)[None, :], np.arange(128)[:, None])
    assert m.min() >= 1.0 and m.max() < 2.0
    frac = m.view(np.uint64).ravel() & np.uint64((1 << 52) - 1)
    assert len(np.unique(frac)) == frac.size
    for bit in range(52):
        share = float(((frac >> np.uint64(bit)) & np.uint64(1)).mean())
        assert 0.45 < share < 0.55, (bit, share)


@pytest.mark.parametrize('name,form', CELLS, ids=IDS)
def test_the_model_is_the_oracles_arguments(name, form):
    """The args scene (v, u, w * B) rendered by the oracle equals the numpy model bit for bit, in both forms."""
    for values in D.frames(name)[-3:]:
        _, got = D.oracle(name, form, values, True)
        assert same_f64(got, D.arguments_np(name, form, *values)), D.first_mismatch(got, D.arguments_np(name, form, *values))


def _census(classes, v):
    for what, mask in classes.items():
        assert int(np.count_nonzero(mask)) >= 256, (what, int(np.count_nonzero(mask)))
    fin = np.isfinite(v)
    total = sum(int(np.count_nonzero(m)) for m in classes.values())
    assert total == int(np.count_nonzero(fin)), 'the classes partition the finite arguments'


def test_census_of_the_sine_arguments():
    v = v_plane('sin_any')
    a = np.abs(v)
    bounds = [0.0, 2.0 ** -26, 0.126, 0.855469, 2.426265, 105414350.0, math.inf]
    classes = {}
    for sign, sel in (('+', ~np.signbit(v)), ('-', np.signbit(v))):
        for lo, hi in zip(bounds, bounds[1:]):
            classes['%s[%g, %g)' % (sign, lo, hi)] = sel & (a >= lo) & (a < hi)
    _census(classes, v)
    assert np.count_nonzero(np.isnan(v)) == D.W and np.count_nonzero(np.isinf(v)) == 2 * D.W
    # the bounded scene: every frame stays inside the bounded reduction's range, and the frames reach from 2^-40 to 2^26
    for (p,) in D.frames('sin_bounded'):
        assert np.abs(v_plane('sin_bounded', p)).max() + 1.0 < 105414350.0
    assert max(abs(p) for (p,) in D.frames('sin_bounded')) == 2.0 ** 25 and min(abs(p) for (p,) in D.frames('sin_bounded')) == 2.0 ** -40
    steps = sorted({math.log2(abs(p)) for (p,) in D.frames('sin_bounded') if p != 3.0})
    assert all(b - a <= 5 for a, b in zip(steps, steps[1:]))


def test_census_of_the_exp_and_ln_arguments():
    v = v_plane('exp_ln')
    over, sub, zero = 709.782712893384, -708.3964185322641, -745.1332191019411
    tiny = np.abs(v) < 2.0 ** -54
    _census({'tiny': tiny, 'overflow': v > over, 'result 0': v < zero, 'subnormal result': (v >= zero) & (v < sub),
             'normal result': ~tiny & (v >= sub) & (v <= over)}, v)
    a = np.abs(v)
    near1 = (a >= 0.9375) & (a < 1.0 + float.fromhex('0x1.09p-4'))          # the interval in which log takes its near-1 polynomial
    _census({'subnormal': a < 2.0 ** -1022, 'near 1': near1, 'elsewhere': (a >= 2.0 ** -1022) & ~near1}, v)
    assert np.count_nonzero((a >= 0.93) & (a < 0.9375)) >= 8 and np.count_nonzero((a >= 1.065) & (a < 1.07)) >= 8      # both borders


def test_census_of_the_sqrt_arguments():
    v = v_plane('algebra')
    pos = v > 0
    e = np.frexp(v)[1] - 1
    big = pos & (v >= 2.0 ** -767)
    _census({'negative': v < 0, 'subnormal': pos & (v < 2.0 ** -1022), 'below 2^-767': pos & (v >= 2.0 ** -1022) & (v < 2.0 ** -767),
             'odd exponent': big & (e % 2 == 1), 'even exponent': big & (e % 2 == 0)}, v)
    assert np.count_nonzero(v < 0) == D.W                       # the bare negative arguments: one row


def test_fusing_the_multiply_add_would_show():
    """About half of the algebra scene's (u, v, w B) triples round differently when u * v - w B is one fused operation
    (computed here in exact rational arithmetic on a sample)."""
    from fractions import Fraction
    args = D.arguments_np('algebra', 'x')
    rows = D.rows_of('algebra')
    differ = n = 0
    for yy in range(0, len(rows), 7):
        for xx in range(0, D.W, 16):
            v, u, wb = (float(t) for t in args[yy, xx])
            if not (math.isfinite(u * v) and abs(u * v) > 1e-290 and abs(u * v) < 1e290):
                continue
            fused = Fraction(u) * Fraction(v) - Fraction(wb)
            n += 1
            differ += float(fused) != u * v - wb                # (Fraction -> float rounds to nearest even)
    assert n >= 200 and differ >= n // 4, (differ, n)


@pytest.mark.parametrize('name', D.NAMES)
def test_reference_values_are_finite_and_distinct(name):
    """At least 90 % of the oracle's values are finite in every channel of both forms; in the x-varying form every channel
    holds 10,000 distinct bit patterns or more -- but the two-valued channel 255 * step(sin v), which has to show each of its
    values on 256 pixels or more.  (Of the parameterised scene the frames with |p| >= 3 are counted: under a tiny p
    every v + 1 lies within a few thousand doubles of 1 and every v has the sign of p.)"""
    for values in D.frames(name):
        for form in D.FORMS:
            _, want64 = D.oracle(name, form, values)
            for c in range(3):
                assert float(np.isfinite(want64[..., c]).mean()) >= 0.9, (name, form, c, values)
        if values and abs(values[0]) not in (3.0, 2.0 ** 25):
            continue
        _, want64 = D.oracle(name, 'x', values)
        for c in range(3):
            plane = want64[..., c]
            if name.startswith('sin') and c == 1:
                assert set(np.unique(plane)) == {0.0, 255.0} and min(np.count_nonzero(plane == 0.0), np.count_nonzero(plane == 255.0)) >= 256, (name, values)
            else:
                assert len(np.unique(plane.view(np.uint64))) >= 10000, (name, c, values)


# ---- the lowering ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,form', CELLS, ids=IDS)
def test_host_evaluator_equals_the_oracle(name, form):
    """The lowered program under the numpy evaluator against the oracle on every pixel: f64 planes bit for bit and RGB8; the
    parameterised scene lowered once and evaluated per frame (params.as_v2)."""
    tape = D.scene(name, form).lower()
    w, h = D.size(name, form)
    assert tape.param_count == (1 if name == 'sin_bounded' else 0)
    for values in D.frames(name):
        want8, want64 = D.oracle(name, form, values)
        got = tape_eval.render_rows(as_v2(tape, values) if values else tape, w, 0, h, D.textures())
        assert same_f64(got, want64), (name, form, values, D.first_mismatch(got, want64))
        assert np.array_equal(tape_eval.cast_u8(got), want8), (name, form, values)


def test_every_scene_reaches_its_form_and_its_functions(monkeypatch):
    """The x-varying form runs its ops per pixel, the y-only form in the ROW section (rows as lanes, 256 or more); the
    generated sources name the functions each scene is there for; the bounded and the unbounded sine forms are told apart."""
    reach = {'algebra': ('mr_sqrt(', 'mr_recip('), 'exp_ln': ('mr_exp(', 'mr_ln('),
             'sin_any': ('mr_sin(', 'mr_stepsin_fast_k('), 'sin_bounded': ('mr_sin_bounded(', 'mr_stepsin_bounded_mk(')}
    row_reach = {'algebra': ('mr_sqrt(', 'mr_recip('), 'exp_ln': ('mr_exp(', 'mr_ln('), 'sin_any': ('mr_sin(', 'mr_stepsin('),
                 'sin_bounded': ('mr_sin_bounded(', 'mr_stepsin_bounded')}
    for name in D.NAMES:
        tx, ty = D.scene(name, 'x').lower(), D.scene(name, 'y').lower()
        src = pixel_source(tx)
        for fn in reach[name]:
            assert fn in src, (name, fn)
        if name == 'sin_any':
            assert tx.info['sin_ops'] == 3 and tx.info['sin_bounded'] == 0 and 'mr_sin_bounded(' not in src and 'mr_stepsin_bounded' not in src
        if name == 'sin_bounded':
            assert tx.info['sin_ops'] == 3 and tx.info['sin_bounded'] == 3 and 'mr_sin(' not in src and 'mr_stepsin_fast' not in src
        assert D.size(name, 'y')[1] >= 256 and ty.info['n_row_ops'] > 4 * tx.info['n_row_ops'] / 5 and ty.program.n_pix_ops <= 5, (name, ty.program.n_pix_ops)
        rows = rows_source(ty)
        for fn in row_reach[name]:
            assert fn in rows, (name, fn)
        assert 'mr_app(' in rows or 'mr_texel(' in rows, name
    # the same scene with (-inf, inf) for the parameter's range: the unbounded forms
    s = M.Scene(D.data('sin_bounded', 'x'))
    s.declare_param(D.PARAM)
    src = pixel_source(s.lower())
    assert 'mr_sin(' in src and 'mr_stepsin_fast_k(' in src and 'mr_sin_bounded(' not in src
    # algebra: four pixels per lane (mr_sqrt's and mr_recip's mr_d forms), and one pixel per lane under the knob that keeps texel
    # lookups from the wide form -- tests/test_gpu_dense.py runs both
    tape = D.scene('algebra', 'x').lower()
    assert jit_shape(tape) == (True, False)
    monkeypatch.setenv('MARAY_JIT_WIDE_APP', '0')
    assert jit_shape(tape) == (False, False)
    monkeypatch.delenv('MARAY_JIT_WIDE_APP')
    for name in ('exp_ln', 'sin_any', 'sin_bounded'):
        assert jit_shape(D.scene(name, 'x').lower()) == (False, False)


def libm_constants():
    """MR_HPINV .. MR_PP4 as maray_libm.h defines them."""
    with open(os.path.join(ROOT, 'maray_amd', 'csrc', 'maray_libm.h')) as f:
        text = f.read()
    return [float.fromhex(re.search(r'#define %s \((-?0x[0-9a-fp.+-]+)\)' % n, text).group(1)) for n in ('MR_HPINV', 'MR_TOINT', 'MR_MP1', 'MR_MP2', 'MR_PP3', 'MR_PP4')]


def test_the_sines_constant_table_holds_the_librarys_constants():
    """mr_stepsin_bounded_mk and mr_stepsin_fast_k read the reduction's constants from the kernel's constant table, written by
    the generator: its first seven entries are the library's six, bit for bit, and 2^-70."""
    want = libm_constants() + [2.0 ** -70]
    for name in ('sin_any', 'sin_bounded'):
        src = pixel_source(D.scene(name, 'x').lower())
        body = src[src.index('mr_kc_tab['):]
        body = body[body.index('{') + 1:body.index('}')]
        got = [float.fromhex(t.strip('() \n')) for t in body.split(',') if t.strip()][:7]
        assert [v.hex() for v in got] == [v.hex() for v in want], name
        k = re.search(r'mr_stepsin_(?:bounded_mk|fast_k)\([^;]*mr_kc \+ (\d+)\)', src)
        assert k and k.group(1) == '0', name


def _objdump():
    for d in (os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'lib', 'llvm', 'bin'), '/opt/rocm/lib/llvm/bin', '/opt/rocm/llvm/bin'):
        if os.path.exists(os.path.join(d, 'llvm-objdump')):
            return os.path.join(d, 'llvm-objdump')
    return shutil.which('llvm-objdump')


def test_the_specialised_build_does_not_fuse_multiply_and_add(tmp_path):
    """With few-bit operands a fused multiply-add is invisible; here it is looked for in the code: the kernels of a scene that
    is texel lookups, multiplications and additions only (the mantissas and u * v + w) hold v_mul_f64 and v_add_f64 and not one
    v_fma_f64 -- built with the contraction left on they hold a dozen."""
    from test_jit_offline import build
    xe, ye = D.x(), D.y()
    u, v, w = (D.mantissa(j, xe, ye) for j in range(3))
    fused = D.add(D.mul(u, v), w)
    tape = M.Scene(D.encode((D.W, 8), [fused, D.add(D.mul(v, w), u), D.add(D.mul(w, u), v)])).lower()
    _, blob = build(tape)
    path = tmp_path / 'dense.co'
    path.write_bytes(blob)
    tool = _objdump()
    assert tool, 'llvm-objdump of the ROCm installation'
    asm = subprocess.run([tool, '-d', str(path)], capture_output=True, text=True, check=True).stdout
    assert 'maray_jit_pixels' in asm and asm.count('v_mul_f64') >= 3 and asm.count('v_add_f64') >= 3
    assert 'v_fma_f64' not in asm and 'v_fmac_f64' not in asm and 'v_pk_fma' not in asm


def test_dense_scenes_build_offline():
    """Both kernels of every scene and form compile for gfx950."""
    from test_jit_offline import build
    tapes = [D.scene(n, f).lower() for n, f in CELLS]
    with ThreadPoolExecutor(4) as pool:
        blobs = list(pool.map(lambda t: build(t)[1], tapes))
    assert all(b[:4] == b'\x7fELF' for b in blobs)

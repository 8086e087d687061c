"""Scene parameters on the host (include/maray_hip.h, "scene parameters"): the lowering keeps a declared free variable as a
run-time operand, and the program computes for every value what the oracle computes for the substituted scene, bit for bit
(tests/params.py).  Needs no GPU."""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

import maray_amd as M
import params as PR
import tape_eval as TE
from marayb import add, encode, let_, mul, nat, var, var_id, x, y

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SIZE = (128, 64)
E_ARG, E_ALIASED, E_LIMIT, E_NO_DEVICE = -1, -4, -7, -8


def _setup(name, size=SIZE):
    spec = PR.SCENES[name](*size)
    scene, names = PR.declared(spec, size)
    return spec, scene, PR.scene_textures() if spec.get('textures') else None


# ---- 1. parity with the oracle's substituted scene ---------------------------------------------------------------------
@pytest.mark.parametrize('row_guards', [True, False])
@pytest.mark.parametrize('name', sorted(PR.SCENES))
def test_tape_equals_the_oracle_of_the_substituted_scene(name, row_guards):
    """Lowered once; for every value of the sweep the numpy evaluator of the program (PARAM operands read from the values)
    gives the oracle's f64 planes of the substituted scene bit for bit, NaN matching NaN, and its RGB8 -- with the SKIP ops
    ignored and with them taken wavefront by wavefront; with guards over rectangles too where the tape allows it."""
    spec, scene, tex = _setup(name)
    w, h = SIZE
    tape = scene.lower(row_guards=row_guards)
    assert tape.program.version == (2 if name == 'unused' else 3)
    assert tape.param_count == (0 if name == 'unused' else len(spec['params']))
    for k in range(tape.param_count):
        assert tape.param_range(k) == tuple(spec['params'][k][1:])
    n_guards, reading_y = TE.guards_reading_y(tape)
    for values in spec['sweep']:
        want8, want64 = PR.oracle_frame(spec, SIZE, values, tex)
        v2 = PR.as_v2(tape, values)
        plain = TE.render_rows(v2, w, 0, h, tex)
        assert PR.same_f64(plain, want64), (name, values)
        assert np.array_equal(TE.cast_u8(plain), want8), (name, values)
        assert PR.same_f64(TE.render_rows_waves(v2, w, 0, h, tex), want64), (name, values, 'skips taken')
        if n_guards and not reading_y:
            assert PR.same_f64(TE.render_rows_waves(v2, w, 0, h, tex, tile=64, yrows=32), want64), (name, values, 'rectangle guards')


def test_guards_survive_a_parameter_with_a_finite_range():
    """What the declared range is for: shapes that a parameter moves keep their rectangle guards, a bounded parameter inside a
    Sin keeps the proof that the argument is bounded, and a parameter that may be anything loses it."""
    spec, scene, _ = _setup('slide')
    tape = scene.lower()
    fixed = M.Scene(encode(SIZE, PR.substituted(spec['color'], ['t', 'u'], (3.0, 33.0)))).lower()      # the scene with constants in the parameters' place
    assert tape.info['skip_ops'] == fixed.info['skip_ops'] >= 12            # a guarded region per triangle at least: none lost
    assert tape.info['n_yvals'] - TE.guards_reading_y(tape)[0] >= fixed.info['n_yvals'] - TE.guards_reading_y(fixed)[0]
    assert TE.guards_reading_y(tape)[1] == 0                                 # ... and every guard bounded over rectangles
    assert _setup('phase')[1].lower().info['sin_bounded'] == 2
    assert _setup('phase_inf')[1].lower().info['sin_bounded'] == 0
    fade, signed = _setup('fade')[1].lower(), _setup('fade_signed')[1].lower()
    assert TE.guards_reading_y(fade)[0] >= TE.guards_reading_y(signed)[0] >= 0
    assert tape.info['alg_ops_uniform'] > 0


# ---- 2. one tape, many values -----------------------------------------------------------------------------------------
def test_one_tape_for_every_value():
    spec, scene, _ = _setup('slide')
    before = [a.tobytes() for a in scene.lower().arrays()]
    for values in spec['sweep']:
        for k, v in enumerate(values):
            scene.set_param(k, v)
        assert [a.tobytes() for a in scene.lower().arrays()] == before
    assert scene.param_info(0)[3] == spec['sweep'][-1][0]


# ---- 3. sources, key and offline build do not depend on values -------------------------------------------------------------
def _sources(tape):
    L = M.lib()
    L.maray_jit_source.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    L.maray_jit_source_rows.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)]
    L.maray_jit_source_samples.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]
    out = []
    for call in (lambda p: L.maray_jit_source(C.byref(tape.program), C.byref(p)),
                 lambda p: L.maray_jit_source_rows(C.byref(tape.program), C.byref(p), C.byref(C.c_uint32())),
                 lambda p: L.maray_jit_source_samples(C.byref(tape.program), 2, C.byref(p))):
        p = C.c_void_p()
        assert call(p) == 0, L.maray_last_error()
        out.append(C.string_at(p).decode())
        L.maray_free(p)
    return out


@pytest.mark.parametrize('name', ['slide', 'phase', 'phase_inf', 'fade', 'texshift', 'three'])
def test_sources_and_key_do_not_depend_on_values(name, tmp_path, monkeypatch):
    monkeypatch.setenv('MARAY_CACHE_DIR', str(tmp_path))
    spec, scene, _ = _setup(name, (384, 320))
    loud = float.fromhex('0x1.23456789abcdp+7')  # 145.63..., inside no scene's constants
    texts, keys = [], []
    for value in (spec['sweep'][1][0], loud if spec['params'][0][1] <= loud <= spec['params'][0][2] else spec['sweep'][2][0]):
        scene.set_param(0, value)
        tape = scene.lower()
        texts.append(_sources(tape))
        keys.append(tape.jit_code_key)
    assert texts[0] == texts[1] and keys[0] == keys[1]
    joined = '\n'.join(texts[0])
    for needle in ('0x1.23456789abcdp+7', '145.63', '1.23456789abcd'):
        assert needle not in joined
    assert 'mr_par_tab[%d]' % len(spec['params']) in texts[0][0] and 'mr_par_tab[%d]' % len(spec['params']) in texts[0][1]
    assert 'from a v3 tape' in texts[0][0]
    L = M.lib()
    L.maray_jit_build.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.maray_jit_build_samples.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    code, n = C.c_void_p(), C.c_size_t()
    assert L.maray_jit_build(C.byref(tape.program), C.byref(code), C.byref(n)) == 0, L.maray_last_error().decode()[-2000:]
    assert C.string_at(code, 4) == b'\x7fELF'
    L.maray_free(code)
    assert L.maray_jit_build_samples(C.byref(tape.program), 2, C.byref(code), C.byref(n)) == 0, L.maray_last_error().decode()[-2000:]
    L.maray_free(code)


# ---- 4. programs without parameters do not change -------------------------------------------------------------------------
def test_an_unused_declaration_leaves_every_pinned_tape_as_it_is(monkeypatch):
    """Every scene of tests/golden/tape_hashes.json, built as tools/gen_tape_hashes.py builds it but with a parameter declared
    that the scene does not use: the same hashes, i.e. the same ops and constants byte for byte, in a version-2 program."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import gen_tape_hashes
    with open(os.path.join(HERE, 'golden', 'tape_hashes.json')) as f:
        want = json.load(f)
    made = []
    lower = M.Scene.lower

    def declared_lower(self, *a, **kw):
        k = self.declare_param('a name no pinned scene uses', -3.0, 5.0)
        self.set_param(k, 4.0)
        tape = lower(self, *a, **kw)
        made.append((tape.program.version, tape.param_count))
        return tape
    monkeypatch.setattr(M.Scene, 'lower', declared_lower)
    got = gen_tape_hashes.all_hashes()
    assert got == want
    assert len(made) >= len(want) and set(made) == {(2, 0)}


# ---- 5. errors ---------------------------------------------------------------------------------------------------------------
def test_declaration_errors_and_limits():
    s = M.Scene(encode((8, 8), [x(), y(), var('t')]))
    assert s.param_count == 0
    assert s.declare_param('t', -1.0, 1.0) == 0
    assert s.declare_param('t', -1.0, 1.0) == 0               # again, same range: the same index
    with pytest.raises(M.MarayError) as e:
        s.declare_param('t', -1.0, 2.0)                        # again with another range
    assert e.value.code == E_ARG
    for lo, hi in ((2.0, 1.0), (math.nan, 1.0), (0.0, math.nan)):
        with pytest.raises(M.MarayError) as e:
            s.declare_param('u', lo, hi)
        assert e.value.code == E_ARG
    assert s.param_count == 1
    assert math.isnan(s.param_info(0)[3]) and s.param_info(0)[:3] == (var('t')[1], -1.0, 1.0)
    assert M.var_id('t') == var('t')[1] and M.var_id('board offset') == var('board offset')[1]
    for bad in (1.5, -1.0000001, math.nan, math.inf):
        with pytest.raises(M.MarayError) as e:
            s.set_param(0, bad)
        assert e.value.code == E_ARG
        assert math.isnan(s.param_info(0)[3])                  # the old value stays
    s.set_param(0, 0.5)
    with pytest.raises(M.MarayError):
        s.set_param(0, 7.0)
    assert s.param_info(0)[3] == 0.5
    with pytest.raises(M.MarayError) as e:
        s.set_param(1, 0.0)
    assert e.value.code == E_ARG
    for k in range(1, 64):
        assert s.declare_param(1000 + k) == k
    with pytest.raises(M.MarayError) as e:
        s.declare_param(5000)
    assert e.value.code == E_LIMIT and s.param_count == 64
    # a range that starts at +0.0 excludes -0.0 (its sign would break "sign bit clear" statements), one from -0.0 does not
    z = M.Scene(encode((8, 8), [x(), y(), var('t')]))
    z.declare_param('t', 0.0, 1.0)
    z.set_param(0, 0.0)
    with pytest.raises(M.MarayError):
        z.set_param(0, -0.0)
    # an infinite range takes anything
    f = M.Scene(encode((8, 8), [x(), y(), var('t')]))
    f.declare_param('t')
    for v in (math.nan, math.inf, -math.inf, -0.0, 1e300):
        f.set_param(0, v)


def test_a_parameter_id_that_a_let_defines_elsewhere_is_aliased():
    """fix_color numbers Let variables 0, 1, ... (src/var_fixer.rs:49-66); a free Var(0) next to a Let is then one id with two
    meanings, and stays an error when the id is a declared parameter."""
    color = [add(var_id(0), let_([(77, x())], var_id(77))), y(), nat(1)]
    s = M.Scene(encode((8, 8), color))
    s.declare_param(0, -1.0, 1.0)
    with pytest.raises(M.MarayError) as e:
        s.lower()
    assert e.value.code == E_ALIASED
    # ... while a name that is free here and a Let's own variable there is two variables after fix_color: no error, and the
    # Let keeps its definition
    t = var('t')
    spec = dict(color=[add(t, let_([(t[1], mul(x(), nat(2)))], t)), y(), nat(1)], params=[('t', -8.0, 8.0)])
    s2, names = PR.declared(spec, (16, 8))
    tape = s2.lower()
    want8, want64 = PR.oracle_frame(spec, (16, 8), (3.5,))
    assert PR.same_f64(TE.render_rows(PR.as_v2(tape, (3.5,)), 16, 0, 8), want64)
    assert want64[2, 5, 0] == 3.5 + 10.0


def test_hand_made_programs_and_struct_layout():
    """PARAM operands are accepted only below n_params; the version-3 struct is the version-2 one with two fields appended."""
    assert C.sizeof(M.Program) == 80
    assert [(getattr(M.Program, n).offset, getattr(M.Program, n).size) for n in ('version', 'n_consts', 'consts', 'n_row_ops', 'row_ops', 'n_row_slots',
            'n_yvals', 'n_pix_ops', 'pix_ops', 'n_pix_slots', 'n_app', 'n_params', 'param_ranges')] == \
        [(0, 4), (4, 4), (8, 8), (16, 4), (24, 8), (32, 4), (36, 4), (40, 4), (48, 8), (56, 4), (60, 4), (64, 4), (72, 8)]
    _, scene, _ = _setup('three')
    tape = scene.lower()
    p = tape.program
    assert (p.version, p.n_params) == (3, 3)
    assert [p.param_ranges[i] for i in range(6)] == [-math.inf, math.inf] * 3
    L = M.lib()
    L.maray_row_cone.argtypes = [C.POINTER(M.Program), C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]

    def validates(prog):          # maray_row_cone validates a program and needs no device
        ops, n, slots = C.c_void_p(), C.c_uint32(), C.c_uint32()
        rc = L.maray_row_cone(C.byref(prog), 0, 1, C.byref(ops), C.byref(n), C.byref(slots))
        if rc == 0:
            L.maray_free(ops)
        return rc
    assert validates(p) == 0

    def copy(**kw):
        q = M.Program()
        C.memmove(C.byref(q), C.byref(p), C.sizeof(M.Program))
        for k, v in kw.items():
            setattr(q, k, v)
        return q
    assert validates(copy(n_params=2)) == E_ARG                 # PARAM 2 with p >= n_params
    assert validates(copy(version=2)) == E_ARG                  # a version-2 program has no parameters at all
    assert validates(copy(n_params=0)) == E_ARG
    assert validates(copy(n_params=65)) == E_ARG
    assert validates(copy(version=7)) == E_ARG
    bad = (C.c_double * 6)(0.0, 1.0, 2.0, 1.0, 0.0, 1.0)        # lo > hi
    assert validates(copy(param_ranges=C.cast(bad, C.POINTER(C.c_double)))) == E_ARG
    # a version-2 struct from an older caller ends at n_app: nothing behind it is read
    _, plain, _ = _setup('unused')
    t2 = plain.lower()
    buf = (C.c_uint8 * 64)()
    C.memmove(buf, C.byref(t2.program), 64)
    assert validates(C.cast(buf, C.POINTER(M.Program)).contents) == 0


# ---- 6. the cache name ---------------------------------------------------------------------------------------------------
def test_declarations_are_part_of_the_name_and_values_are_not(tmp_path):
    """No device here: gen_to_image fails with NO_DEVICE after it has lowered and named the program, so the names are read
    from the context-free side: two scenes with the same declarations lower to one program whatever their values, and
    rescale / supersample keep the declarations."""
    spec, scene, _ = _setup('slide')
    scene.set_param(0, 3.0)
    scene.rescale(2, 2)
    scene.supersample(2)
    assert scene.param_count == 2 and scene.param_info(0)[3] == 3.0 and scene.param_info(1)[:3] == (var('u')[1], -512.0, 512.0)
    tape = scene.lower()
    assert tape.param_count == 2 and tape.param_range(0) == (-512.0, 512.0)
    scene.simplify()
    assert scene.param_count == 2 and scene.lower().param_count == 2
    key = tape.jit_code_key
    scene2 = _setup('slide')[1]
    scene2.set_param(1, -77.0)
    scene2.rescale(2, 2)
    scene2.supersample(2)
    assert scene2.lower().jit_code_key == key


# ---- 7. the command line ---------------------------------------------------------------------------------------------------
def _cli(*args):
    return subprocess.run([os.path.join(ROOT, 'maray_amd', 'maray')] + list(args), capture_output=True, text=True, timeout=300,
                          env=dict(os.environ, HIP_VISIBLE_DEVICES='-1', ROCR_VISIBLE_DEVICES='-1'))


def test_cli_parses_parameters_as_far_as_it_goes_without_a_device(tmp_path):
    spec = PR.SCENES['slide'](64, 32)
    path = tmp_path / 'slide.maray'
    path.write_bytes(encode((64, 32), spec['color']))
    ok = _cli('-i', str(path), '-o', str(tmp_path / 'o.png'), '-p', 't=3.5:-512:512', '-p', 'u=-2')
    assert ok.returncode == 1 and 'no HIP device' in ok.stderr and 'usage' not in ok.stderr.lower(), ok.stderr
    ok = _cli('-i', str(path), '-o', str(tmp_path / 'f%03d.png'), '-p', 'u=0:-64:64', '--animate', 't=0:100:5')
    assert ok.returncode == 1 and 'no HIP device' in ok.stderr and 'usage' not in ok.stderr.lower(), ok.stderr
    for bad in (['-p', 't'], ['-p', 't=x'], ['-p', 't=1:2'], ['-p', 't=5:0:1'], ['--animate', 't=0:1'], ['--animate', 't=0:1:0']):
        r = _cli('-i', str(path), '-o', str(tmp_path / 'f%d.png'), *bad)
        assert r.returncode == 2, (bad, r.stderr)
    r = _cli('-i', str(path), '-o', str(tmp_path / 'o.png'), '--animate', 't=0:100:5')       # frames need a numbered output
    assert r.returncode == 2 and '%' in r.stderr

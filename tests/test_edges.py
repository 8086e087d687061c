"""The edge-value matrix of tests/edge_values.py on the CPU: each (op, form) cell reaches the form it is meant to test,
the lowering keeps the oracle's values on every pixel of it, and both specialised kernels of every cell compile for
gfx950.  tests/test_gpu_edges.py runs the same cells on the device."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import edge_values as E
import maray_amd as M
import tape_eval
from oracle_ffi import Scene as OScene
from test_gpu_launches import jit_shape
from test_lowering import same_f64

CASES = E.cases()


def pixel_source(tape):
    L = M.lib()
    L.maray_jit_source.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    src = C.c_void_p()
    assert L.maray_jit_source(C.byref(tape.program), C.byref(src)) == 0, L.maray_last_error()
    text = C.string_at(src).decode()
    L.maray_free(src)
    return text


def operand_kinds(ops, opcode):
    """The operand kinds (tape_eval.K_*) the ops with this opcode read, as a set of tuples (kind of a, kind of b)."""
    out = set()
    for ins in ops:
        op, _, _, ra, rb = tape_eval.decode(ins)
        if op == opcode:
            out.add((ra >> 14, rb >> 14))
    return out


def check_form(case, tape):
    """The cell reached its form: from the tape's sections and operand kinds and from the generated PIXEL kernel."""
    _, row_ops, pix_ops = tape.arrays()
    wide, guarded = jit_shape(tape)
    code = E.OPCODE.get(case.op)
    pix, row = operand_kinds(pix_ops, code), operand_kinds(row_ops, code)
    const, yval = tape_eval.K_CONST, tape_eval.K_YVAL
    varying = (tape_eval.K_SLOT, tape_eval.K_SPEC)          # a value slot or ACC: computed per pixel
    f = case.form
    if f in ('x-narrow', 'x-wide', 'cross'):
        # the op runs per pixel on an operand that varies along the row (a slot), one pixel per lane or four
        assert any(k[0] in varying for k in pix), (case.id, pix)
        assert wide == (f == 'x-wide') and not guarded, (case.id, wide, guarded)
        if case.op in E.BINARY:     # right operand: the cross product's y table is a y value too, read by a varying op
            assert any(k[0] in varying and k[1] == yval for k in pix), (case.id, pix)
    elif f == 'y-row':
        # computed once per row in the ROW kernel; the PIXEL kernel reads its result
        assert row and not tape.info['skip_ops'] and not guarded, (case.id, row)
        assert case.op in ('neg', 'step', 'add', 'mul') or not pix, (case.id, pix)      # (the byte channels use those per pixel)
    elif f == 'y-pixel':
        assert pix and not row and tape.info['n_row_ops'] == 0, (case.id, pix)
    elif f == 'const-row':
        assert row == {(const, 0)} and not pix, (case.id, row, pix)
    elif f == 'const-pixel':
        assert pix == {(const, 0)} and not row, (case.id, row, pix)
    elif f == 'guarded':
        # guarded shapes, and a variant for tiles without a guard bit in which their values are the literal 0.0
        assert guarded and not wide and tape.info['skip_ops'] > 0
        text = pixel_source(tape)
        sky = text[text.index('mr_d o0 = 0.0'):]
        sky = sky[:sky.index('mr_u3')]
        for fn in ('mr_sin', 'mr_stepsin', 'mr_exp(', 'mr_ln(', 'mr_sqrt(', 'mr_recip(', 'mr_texel('):
            assert fn in sky, (case.id, fn)
    elif f == 'bool':
        assert tape.info['bool_ops'] > 0 and not guarded
        assert 'mr_ym(yw, ' in pixel_source(tape)                    # a y-only boolean read as a lane mask
    elif f in ('texel', 'texel-wide'):
        assert tape.info['n_app'] >= 3 and wide == (f == 'texel-wide') and not guarded, (case.id, wide)
    else:
        raise AssertionError(f)
    if 'wide' in f:
        assert 'general variant four pixels per lane' in pixel_source(tape).split('\n', 1)[0]


def test_the_matrix_covers_every_op_in_every_form_it_has():
    """The cells the GPU matrix runs: every op x-varying (one pixel per lane), every op but sin, exp and ln also four pixels
    per lane, every op on a y-only operand with and without the ROW kernel, sin / step(sin) / exp / ln on constants."""
    have = {(c.op, c.form) for c in CASES}
    for op in list(E.UNARY) + list(E.BINARY):
        for form in ('x-narrow', 'y-row', 'y-pixel') + (() if op in E.LIBM else ('x-wide',)) + (('cross',) if op in E.BINARY else ()):
            assert (op, form) in have, (op, form)
    for op in E.LIBM:
        assert (op, 'const-row') in have and (op, 'const-pixel') in have
    assert {'guarded', 'bool', 'texel', 'texel-wide'} <= {c.form for c in CASES}
    assert len({c.id for c in CASES}) == len(CASES)


def test_edge_constants_are_exact():
    """const(v) is v bit for bit (the oracle evaluates it), NaN a NaN, every value of the tables."""
    from marayb import encode
    vals = E.VALUES + [r[1] for r in E.ROWS] + [r[2] for r in E.ROWS] + sum(E.CONST_VALUES.values(), [])
    for i in range(0, len(vals), 3):
        chunk = (vals[i:i + 3] + [0.0, 0.0])[:3]
        s = OScene(encode((1, 1), [E.const(v) for v in chunk]))
        for c, v in enumerate(chunk):
            got = s.eval2(c, 0.0, 0.0)
            assert (got != got and v != v) or E.bits(got) == E.bits(v), (v, got)
    # the tables too: row i of a table is entry i, on every row
    ys = np.arange(len(E.VALUES), dtype=np.float64)
    s = OScene(encode((1, len(E.VALUES)), [E.table(E.y(), E.VALUES), E.nat(0), E.nat(0)]))
    for yy, v in zip(ys, E.VALUES):
        got = s.eval2(0, 0.0, yy)
        assert (got != got and v != v) or E.bits(got) == E.bits(v), (yy, v, got)


@pytest.mark.parametrize('case', CASES, ids=lambda c: c.id)
def test_edge_cell_reaches_its_form_and_lowers_to_the_oracle(case):
    """The cell's form (check_form), then the lowering against the oracle on every pixel, f64 planes and bytes, with the
    SKIP ops ignored and taken per wavefront."""
    tape = M.Scene(case.data()).lower(hoist_rows=case.hoist)
    check_form(case, tape)
    tex = E.textures() if case.textures else None
    want8, want64 = OScene(case.data()).render_rows(case.w, case.h, 0, case.h, tex)
    got = tape_eval.render_rows(tape, case.w, 0, case.h, tex)
    assert same_f64(got, want64), case.id
    assert np.array_equal(tape_eval.cast_u8(got), want8), case.id
    if tape.info['skip_ops']:
        assert same_f64(tape_eval.render_rows_waves(tape, case.w, 0, case.h, tex, tile=64), want64), case.id


def test_edge_scenes_show_their_values_in_the_bytes():
    """The byte channels carry the cells' edges: a zero of each sign, NaN and both infinities give distinct sign bytes in
    the neighbourhood scene of recip, and the distance byte moves along every row of sin's."""
    from marayb import encode
    w, h = 64, len(E.ROWS)
    by_name = {r[0]: i for i, r in enumerate(E.ROWS)}
    want8, want64 = OScene(encode((w, h), E.scene_x('recip', w, heavy=False))).render_rows(w, h, 0, h)
    r = by_name['x inf']                              # (x - 32) * inf: -inf, NaN at x = 32, +inf -> recip: -0, NaN, +0
    assert np.isnan(want64[r, 32, 0]) and np.signbit(want64[r, 0, 0]) and not np.signbit(want64[r, 40, 0])
    assert len({int(want8[r, 0, 1]), int(want8[r, 32, 1]), int(want8[r, 40, 1])}) == 3
    want8, _ = OScene(encode((w, h), E.scene_x('sin', w, heavy=False))).render_rows(w, h, 0, h)
    moving = sum(len(np.unique(want8[i, :, 2])) > 8 for i in range(h))
    assert moving >= h // 2, moving


def _build(tape):
    from test_jit_offline import build
    return build(tape)


def test_edge_scenes_build_offline():
    """Both kernels of every cell compile for gfx950 with hiprtc."""
    tapes = [M.Scene(c.data()).lower(hoist_rows=c.hoist) for c in CASES]
    with ThreadPoolExecutor(4) as pool:
        blobs = list(pool.map(lambda t: _build(t)[1], tapes))
    assert all(b[:4] == b'\x7fELF' for b in blobs)

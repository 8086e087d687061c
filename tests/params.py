"""Scene parameters: the helpers and the authored scenes of tests/test_params.py and tests/test_gpu_params.py.

The contract under test (include/maray_hip.h, "scene parameters"): a scene with parameter Var(id) set to v renders the
image the oracle renders for the scene in which every occurrence of Var(id) that resolves to no definition has been
replaced by an expression whose value is exactly v.  `subst_free` + `dyadic` build that scene; `as_v2` turns a lowered
parameterised program into the version-2 program the numpy evaluator (tests/tape_eval.py) runs unchanged.
"""
import math

import numpy as np

from marayb import (BINARY, UNARY, abs_, add, app, channel, div, encode, inside_triangle, let_, max_, min_, mul, nat, neg,
                    p2_len, recip, sd_box, sd_circle, sd_inside, sin, step, sub, translate, var, x, y)

INF = math.inf
K_CONST, K_SPEC, SPEC_PARAM0 = 1, 3, 7


# ---- the substituted scene -------------------------------------------------------------------------------------------
def subst_free(ex, id_, value, bound=False):
    """`ex` with every occurrence of Var(id_) that resolves to no definition replaced by `value` (None: left free, which
    is NaN).  Descends into Let definitions and bodies.  Which occurrences are free is what the renderers see after
    var_fixer::fix_color (src/var_fixer.rs:25-70): a Let's BODY sees that Let's variables and nothing else (the context is
    replaced, src/lib.rs:659-662), its DEFINITIONS are fixed under the enclosing context."""
    if value is None:
        return ex
    t = ex[0]
    if t == 'Var':
        return value if (ex[1] == id_ and not bound) else ex
    if t in ('X', 'Y', 'Tau', 'E', 'Nat'):
        return ex
    if t == 'Arc' or t in UNARY:
        return (t, subst_free(ex[1], id_, value, bound))
    if t in BINARY:
        return (t, subst_free(ex[1], id_, value, bound), subst_free(ex[2], id_, value, bound))
    if t == 'Decor':
        return ('Decor', subst_free(ex[1], id_, value, bound), ex[2])
    if t == 'App':
        return ('App', ex[1], subst_free(ex[2], id_, value, bound), subst_free(ex[3], id_, value, bound))
    if t == 'Let':
        defs = tuple((i, subst_free(d, id_, value, bound)) for i, d in ex[1])
        return ('Let', defs, subst_free(ex[2], id_, value, any(i == id_ for i, _ in ex[1])))
    raise ValueError(t)


def dyadic(v):
    """An expression whose value is exactly v: +-n / 2^m as (Neg of) Mul(Nat n, Recip(Nat 2^m)), +-inf as (Neg of)
    Recip(Nat 0); None for NaN (the variable stays free)."""
    if v != v:
        return None
    if math.isinf(v):
        e = recip(nat(0))
    else:
        a, m = abs(v), 0
        while a != math.floor(a):
            a, m = a * 2.0, m + 1
            assert m < 1000
        assert a < 2.0 ** 53
        e = nat(int(a)) if m == 0 else mul(nat(int(a)), recip(nat(1 << m)))
    return neg(e) if (v < 0 or (v == 0 and math.copysign(1.0, v) < 0)) else e


def substituted(color, names, values):
    out = list(color)
    for n, v in zip(names, values):
        out = [subst_free(c, var(n)[1], dyadic(v)) for c in out]
    return out


def substituted_exact(color, ids, values):
    """The same for any double (edge_values.const builds every one exactly) and for numeric ids; NaN leaves the variable free."""
    from edge_values import const
    out = list(color)
    for i, v in zip(ids, values):
        out = [subst_free(c, i, None if v != v else const(v)) for c in out]
    return out


# ---- ranges and values of the parameter fuzz (tests/fuzz_scenes.py: param_scene and the parameterised soups) ---------------
TINY, HUGE = 5e-324, 1e300
RANGES = [(-64.0, 64.0),                                                  # symmetric, finite
          (0.0, 1.0), (-0.0, 1.0), (-8.0, -0.0), (0.0, 0.0),              # the four zero ends
          (3.5, 3.5),                                                     # degenerate, not zero
          (0.25, 100.0), (-300.0, -0.5),                                  # strictly positive, strictly negative
          (TINY, 1e-300), (-HUGE, HUGE),
          (0.0, INF), (-INF, 0.0), (-INF, -1.0),                          # half-infinite
          (-INF, INF)]


def value_ok(v, lo, hi):
    """param_value_ok of the library (api.cpp), restated: inside the range, the sign of a zero end counting."""
    if lo == -INF and hi == INF:
        return True
    if not (lo <= v <= hi):
        return False
    neg0 = v == 0 and math.copysign(1.0, v) < 0
    if v == 0 and lo == 0 and neg0 and math.copysign(1.0, lo) > 0:
        return False
    if v == 0 and hi == 0 and not neg0 and math.copysign(1.0, hi) < 0:
        return False
    return True


def candidate_values(rng, lo, hi):
    """The values a fuzz vector draws from for one range: both ends, the doubles next to them inward, both zeros where the
    range admits them, interior doubles; the infinite end and 1e300 of a half-infinite range; NaN, +-inf, 2^40 and +-0 of
    the full one."""
    if lo == -INF and hi == INF:
        return [math.nan, INF, -INF, 2.0 ** 40, 0.0, -0.0, rng.uniform(-100.0, 100.0), rng.choice([-1, 1]) * 10.0 ** rng.uniform(-8, 8)]
    out = [lo, hi]
    if lo != hi:
        out += [math.nextafter(lo, hi), math.nextafter(hi, lo)]
    for end, sign in ((lo, 1.0), (hi, -1.0)):
        if math.isinf(end):
            out.append(sign * -HUGE)
    flo, fhi = max(lo, -HUGE), min(hi, HUGE)
    for _ in range(3):
        if math.isinf(lo) or math.isinf(hi):                 # a few decades away from the finite end
            v = (hi - 10.0 ** rng.uniform(-3, 6)) if math.isinf(lo) else (lo + 10.0 ** rng.uniform(-3, 6))
        else:
            v = flo + (fhi - flo) * rng.random() if fhi - flo < INF else rng.uniform(-1.0, 1.0) * fhi
        out.append(min(max(v, flo), fhi))
    out += [0.0, -0.0]
    out = [v for v in out if value_ok(v, lo, hi)]
    assert out, (lo, hi)
    return out


def admits_negative_zero(lo, hi):
    return value_ok(-0.0, lo, hi)


def value_vectors(rng, decl, n):
    """n vectors of values for decl = [(id, lo, hi), ...]; vector 1 has -0.0 in every parameter whose range admits it, vector
    2 NaN in every parameter that may be anything."""
    out = []
    for k in range(n):
        vec = []
        for _, lo, hi in decl:
            c = candidate_values(rng, lo, hi)
            v = rng.choice(c)
            if admits_negative_zero(lo, hi) and (k == 1 or rng.random() < 0.15):
                v = -0.0
            if k == 2 and lo == -INF and hi == INF:
                v = math.nan
            vec.append(v)
        out.append(tuple(vec))
    return out


def declared_ids(data, decl):
    """maray_amd.Scene of the encoded scene with decl = [(id, lo, hi), ...] declared in that order."""
    import maray_amd as M
    s = M.Scene(data)
    for k, (i, lo, hi) in enumerate(decl):
        assert s.declare_param(i, lo, hi) == k
    return s


def fuzz_check(color, decl, vectors, size, textures=None, yrows=(4, 8, 32), threads=None):
    """One parameterised scene against the oracle (tests/test_fuzz_params.py, tools/gpu_fuzz_params.py --cpu).  Lowered ONCE;
    for every vector the program (as_v2) under the numpy evaluator must equal the oracle's f64 planes and RGB8 of the
    substituted scene: plain, with skips taken per wavefront, per 64-pixel span, and per rectangle of `yrows` rows where no
    guard reads y; the guard-free lowering too; and lowering again with the values set gives the same arrays byte for byte.
    Returns None for a scene the library refuses as aliased / self-referent, else a dict: version, guards, reading_y, differ
    (two frames differ), failures (a list of (vector, what))."""
    import os
    import maray_amd as M
    import tape_eval as TE
    from oracle_ffi import Scene as OScene
    w, h = size
    data = encode(size, color)
    scene = declared_ids(data, decl)
    try:
        tape = scene.lower()
        bare = scene.lower(skips=False)
    except M.MarayError as e:
        if e.code in (-4, -5):
            return None
        raise
    ids = [i for i, _, _ in decl]
    n_guards, reading_y = TE.guards_reading_y(tape)
    before = [a.tobytes() for a in tape.arrays()]
    fails, frames = [], []
    threads = threads or min(16, os.cpu_count() or 1)
    for values in vectors:
        want8, want64 = OScene(encode(size, substituted_exact(color, ids, values))).render_rows(w, h, 0, h, textures, threads=threads)
        frames.append(want64)
        v2 = as_v2(tape, values) if tape.param_count else tape

        def check(what, got):
            if not same_f64(got, want64):
                fails.append((values, what))
            elif what == 'plain' and not np.array_equal(TE.cast_u8(got), want8):
                fails.append((values, 'rgb8'))
        check('plain', TE.render_rows(v2, w, 0, h, textures))
        if tape.info['skip_ops']:
            check('skips per wavefront', TE.render_rows_waves(v2, w, 0, h, textures))
            check('skips per span', TE.render_rows_waves(v2, w, 0, h, textures, tile=64))
            if n_guards and not reading_y:
                for yr in yrows:
                    check('skips per rectangle of %d rows' % yr, TE.render_rows_waves(v2, w, 0, h, textures, tile=64, yrows=yr))
        check('guard-free lowering', TE.render_rows(as_v2(bare, values) if bare.param_count else bare, w, 0, h, textures))
        for k, v in enumerate(values):
            scene.set_param(k, v)
        if [a.tobytes() for a in scene.lower().arrays()] != before:
            fails.append((values, 'lowered again'))
    differ = any(not same_f64(frames[0], f) for f in frames[1:])
    return dict(version=tape.program.version, param_count=tape.param_count, guards=n_guards, reading_y=reading_y, differ=differ,
                failures=fails, info=tape.info)


# ---- a parameterised program as a version-2 one ----------------------------------------------------------------------
class TapeV2:
    """Stands in for maray_amd.Tape where tests/tape_eval.py wants one: every PARAM operand rewritten to a CONST operand on
    the pool extended by the values."""

    def __init__(self, tape, values):
        consts, row, pix = tape.arrays()
        n = len(consts)
        assert tape.program.version == 3 and len(values) == tape.program.n_params

        def fix(ops):
            out = ops.copy()
            for j, ins in enumerate(ops):
                ins = int(ins)
                op = ins & 0x7F
                if op in (0, 15):
                    continue
                refs = [(ins >> 32) & 0xFFFF, (ins >> 48) & 0xFFFF]
                for k in range(2 if 10 <= op <= 14 else 1):
                    kind, idx = refs[k] >> 14, refs[k] & 0x3FFF
                    if kind == K_SPEC and idx >= SPEC_PARAM0:
                        refs[k] = (K_CONST << 14) | (n + idx - SPEC_PARAM0)
                out[j] = np.uint64((ins & 0xFFFFFFFF) | (refs[0] << 32) | (refs[1] << 48))
            return out
        self._arrays = (np.concatenate([consts, np.asarray(values, np.float64)]), fix(row), fix(pix))
        self.info = tape.info

    def arrays(self):
        return self._arrays


def as_v2(tape, values):
    return TapeV2(tape, values) if tape.program.version == 3 else tape


def same_f64(a, b):
    """Bit for bit, NaN matching NaN."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


# ---- the scenes ------------------------------------------------------------------------------------------------------
# Each: dict(color=[r, g, b], params=[(name, lo, hi), ...], sweep=[tuple of values per frame], textures=n) for a (w, h)
# picture.  Sweeps hold one pair of frames that differ by less than a pixel and one that moves the shape by more than 64
# pixels and 32 rows (at the GPU tests' size, 384 x 320).
def _tri(ax, ay, bx, by, cx, cy, p):
    return inside_triangle([(nat(ax), nat(ay)), (nat(bx), nat(by)), (nat(cx), nat(cy))], p)


def slide(w, h):
    """A grid of triangles under translate(var t, var u)."""
    p = [x(), y()]
    m = None
    nx, ny = 4, 3
    for j in range(ny):
        for i in range(nx):
            x0, y0 = w * (2 * i + 1) // (2 * nx + 2), h * (2 * j + 1) // (2 * ny + 2)
            t = _tri(x0, y0, x0 + w // (nx + 2), y0 + h // 20, x0 + w // 30, y0 + h // (ny + 1), p) if (i + j) % 2 else \
                _tri(x0, y0 + h // 8, x0 + w // 8, y0, x0 + w // 7, y0 + h // 6, p)
            m = t if m is None else max_(m, t)
    m = translate(m, [var('t'), var('u')])
    sweep = [(0.0, 0.0), (0.5, 0.25), (100.0, 70.0), (-37.5, 12.75), (200.125, -40.0), (-512.0, 512.0), (3.0, 33.0)]
    return dict(color=[mul(m, nat(255)), mul(m, nat(100)), add(mul(m, nat(50)), nat(20))],
                params=[('t', -512.0, 512.0), ('u', -512.0, 512.0)], sweep=sweep)


def _phase(lo, hi, sweep):
    t = var('t')
    r = mul(step(sin(add(mul(x(), div(nat(1), nat(16))), t))), nat(255))
    g = add(mul(sin(add(mul(y(), div(nat(1), nat(8))), t)), nat(127)), nat(128))
    b = mul(step(sin(add(t, mul(mul(x(), y()), div(nat(1), nat(256)))))), nat(200))
    return dict(color=[r, g, b], params=[('t', lo, hi)], sweep=[(v,) for v in sweep])


def phase(w, h):
    """Step(Sin(a x + t)) bands, finite range: the sines are proven bounded (fused STEPSIN, no huge-argument path)."""
    return _phase(-64.0, 64.0, [0.0, 0.001953125, 1.5, -3.25, 40.0, -64.0])


def phase_inf(w, h):
    """The same with the range (-inf, +inf): unbounded sines, and values that take the huge-argument path, inf and NaN."""
    return _phase(-INF, INF, [0.0, 0.001953125, 1.5, 2.0 ** 40, INF, math.nan, -3.25])


def _fade(w, h, lo, hi, sweep):
    p = [x(), y()]
    t = var('t')
    s1 = _tri(w // 8, h // 8, w // 2, h // 6, w // 5, h - h // 8, p)
    s2 = _tri(w // 2, h // 3, w - w // 8, h // 8, w - w // 6, h - h // 6, p)
    r = max_(mul(s1, mul(t, nat(255))), mul(s2, mul(t, nat(90))))
    g = mul(t, x())
    b = add(mul(max_(s1, s2), nat(77)), mul(t, nat(16)))
    return dict(color=[r, g, b], params=[('t', lo, hi)], sweep=[(v,) for v in sweep])


def fade(w, h):
    """shape x (t . colour), t in [0, 1]: a parameter as a sign-clear factor."""
    return _fade(w, h, 0.0, 1.0, [0.0, 0.5, 0.50390625, 1.0, 0.00390625, 0.75])


def fade_signed(w, h):
    """The same with t in [-1, 1]: no sign class."""
    return _fade(w, h, -1.0, 1.0, [-1.0, -0.5, 0.0, 1.0, 0.25, 0.251953125])


def grow(w, h):
    """A signed-distance circle and a rounded box of radius t (sqrt / abs / square rules), t = 0 included."""
    t = var('t')
    circle = translate(sd_inside(sub(sd_circle(nat(0)), t)), [nat(w // 3), nat(h // 2)])
    box = translate(sd_inside(sub(sd_box([nat(w // 10), nat(h // 12)]), t)), [nat(2 * w // 3), nat(h // 2)])
    return dict(color=[mul(circle, nat(255)), mul(box, nat(255)), mul(max_(circle, box), nat(128))],
                params=[('t', 0.0, 256.0)], sweep=[(v,) for v in [0.0, 0.5, 1.0, 70.25, 33.0, 256.0, 1.25]])


def in_let(w, h):
    """The parameter only inside Let definitions that the three channels share."""
    t = var('t')
    a, b = var('a'), var('b')
    defs = [(a[1], add(mul(x(), div(nat(1), nat(4))), t)), (b[1], mul(step(sub(y(), t)), nat(200)))]
    r = let_(defs, add(a, b))
    g = let_(defs, mul(a, nat(2)))
    bl = let_(defs, max_(b, min_(a, nat(99))))
    return dict(color=[r, g, bl], params=[('t', -256.0, 256.0)], sweep=[(v,) for v in [0.0, 0.25, 100.0, -70.5, 35.0, 256.0]])


def texshift(w, h):
    """A textured triangle whose u offset is a parameter (the App path)."""
    p = [x(), y()]
    t = var('t')
    mask = _tri(w // 10, h // 10, w - w // 10, h // 5, w // 3, h - h // 10, p)
    u, v = add(mul(x(), div(nat(1), nat(2))), t), mul(y(), div(nat(1), nat(2)))
    col = [mul(mask, app(channel(0, c), u, v)) for c in range(3)]
    return dict(color=col, params=[('t', -128.0, 128.0)], sweep=[(v,) for v in [0.0, 0.5, 70.0, -33.25, 128.0, 1.0]], textures=True)


def unused(w, h):
    """A declared parameter nothing reads: the scene's version-2 program."""
    p = [x(), y()]
    m = max_(_tri(w // 8, h // 8, w // 2, h // 6, w // 5, h - h // 8, p), _tri(w // 2, h // 3, w - w // 8, h // 8, w - w // 6, h - h // 6, p))
    return dict(color=[mul(m, nat(255)), mul(x(), div(nat(1), nat(2))), y()], params=[('t', -1.0, 1.0)], sweep=[(0.5,), (-1.0,)])


def three(w, h):
    """Three parameters, the last of which is never set (NaN)."""
    a, b, c = var('a'), var('b'), var('c')
    return dict(color=[add(x(), a), mul(y(), b), add(c, x())], params=[('a', -INF, INF), ('b', -INF, INF), ('c', -INF, INF)],
                sweep=[(1.0, 2.0, math.nan), (1.5, -0.5, math.nan), (200.0, 0.0, math.nan)])


SCENES = dict(slide=slide, phase=phase, phase_inf=phase_inf, fade=fade, fade_signed=fade_signed, grow=grow, in_let=in_let,
              texshift=texshift, unused=unused, three=three)


def scene_textures():
    from scenes import textures
    return textures(8)[:1]          # T0, 128 x 128


def declared(spec, size):
    """(maray_amd.Scene with the parameters declared, names)."""
    import maray_amd as M
    s = M.Scene(encode(size, spec['color']))
    names = [n for n, _, _ in spec['params']]
    for k, (n, lo, hi) in enumerate(spec['params']):
        assert s.declare_param(n, lo, hi) == k
    return s, names


def oracle_frame(spec, size, values, textures=None, want_f64=True):
    """The oracle's render of the substituted scene: (rgb8, f64 planes)."""
    from oracle_ffi import Scene as OScene
    names = [n for n, _, _ in spec['params']]
    w, h = size
    import os
    return OScene(encode(size, substituted(spec['color'], names, values))).render_rows(w, h, 0, h, textures, threads=min(16, os.cpu_count() or 1),
                                                                                        want_f64=want_f64)

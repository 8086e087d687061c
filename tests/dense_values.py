"""Dense-argument scenes: sqrt, recip, a multiply-add, exp, ln and the sine forms fed with full 53-bit mantissas whose
every bit is known, in the binades and windows where the device's arithmetic changes branch.

edge_values.py walks the doubles next to the hard points; the structured sweeps feed arguments of a few significant bits, on
which a * b is exact and a fused multiply-add cannot be told from a * b + c.  Here the bits are random and come from
textures (App is the scene language's only source of data):

    m(x, y) = 1 + sum_{k = 1..6} byte_k * 2^(-8 k) + nib * 2^-52

with the six bytes the three channels of the texels (x, y + 2 j HT) and (x, y + (2 j + 1) HT) of image 0 and nib in 0 .. 15 a
texel of image 1 (channel j); j = 0, 1, 2 gives three independent mantissas v, u, w.  Every partial sum is a multiple of 2^-52
below 2 and so exact in any order: m is uniform over the 2^52 doubles of [1, 2), and numpy computes the same doubles from the
same arrays (`mantissa_np`).

The argument is v(x, y) = A(y) + m * B(y), A and B exact per-row tables (edge_values.table).  A binade row has A = 0 and
B = +-2^e (the product is exact while the result is normal); a window row maps [1, 2) onto [lo, hi) with B = hi - lo and
A = lo - B, both operations rounded -- numpy performs the same two IEEE operations (`arguments_np`).  The numpy planes only
classify the arguments (the census of tests/test_dense.py); no result is judged by them.

Two forms of every scene: x-varying (W = 320 pixels: a full 256-pixel tile and a ragged one, one row of the table per image
row) and y-only (the mantissa read from column 3, so the ops land in the ROW section with rows as lanes; the table is walked
three times over, each time with other mantissas)."""
import functools
import math

import numpy as np

from edge_values import table
from marayb import abs_, add, app, channel, encode, exp, ln, mul, nat, neg, recip, sin, sqrt, step, var, x, y

INF, NAN = math.inf, math.nan
W = 320
HT = 384                     # the height of one block of texture rows: no form is taller
SEED = 0x0DE25E
COLUMN = 3                   # the y-only form's column
REPEATS = 3                  # ... and how often it walks the table
PARAM_ROWS = {'x': 64, 'y': 288}      # the heights of the table-less scene (sin_bounded)


@functools.lru_cache(None)
def textures():
    """Image 0: 6 HT x W random bytes (two blocks of rows per mantissa); image 1: HT x W, values 0 .. 15."""
    rng = np.random.default_rng(SEED)
    return [rng.integers(0, 256, (6 * HT, W, 3), dtype=np.uint8), rng.integers(0, 16, (HT, W, 3), dtype=np.uint8)]


# ---- the mantissas ---------------------------------------------------------------------------------------------------
def mantissa(j, xe, ye):
    """m_j in [1, 2) at texel column xe, row ye (expressions)."""
    acc = nat(1)
    for k in range(6):
        texel = app(channel(0, k % 3), xe, add(ye, nat((2 * j + k // 3) * HT)))
        acc = add(acc, mul(texel, recip(nat(1 << (8 * (k + 1))))))
    return add(acc, mul(app(channel(1, j), xe, ye), recip(nat(1 << 52))))


def mantissa_np(j, xs, ys):
    """The same doubles from the arrays: xs, ys integer index arrays (broadcast against one another)."""
    t0, t1 = textures()
    acc = np.ones(np.broadcast(xs, ys).shape)
    for k in range(6):
        acc = acc + t0[ys + (2 * j + k // 3) * HT, xs, k % 3].astype(np.float64) * 2.0 ** (-8 * (k + 1))
    return acc + t1[ys, xs, j].astype(np.float64) * 2.0 ** -52


# ---- rows ------------------------------------------------------------------------------------------------------------
def binade(e, sign=1.0):
    return (0.0, math.copysign(math.ldexp(1.0, e), sign))


def window(lo, hi):
    b = hi - lo
    return (lo - b, b)


def _both(rows):
    return [r for a, b in rows for r in ((a, b), (-a, -b))]


def _algebra_rows():
    es = sorted(set(range(-1074, 1024, 23)) | {-1060, -1040, -1030, -1023, -1022, -768, -767, -1, 0, 1, 2, 1022, 1023})
    return [binade(e) for e in es] + [window(2.0 ** -768, 2.0 ** -766), window(2.0 ** -767, 2.0 ** -766 + 2.0 ** -767), binade(0, -1.0)]


def _exp_ln_rows():
    rows = _both([binade(e) for e in range(-60, 10, 3)] + [binade(9)])
    rows += [binade(10), window(709.0, 710.0), window(-745.2, -708.3), window(-1e-10, 1e-10), window(0.93, 1.07), window(0.9375, 1.0647)]
    # ln: every stretch of binades, the subnormal ones included; those past exp's range are negative (exp gives 0, not inf)
    es = sorted(set(range(-1074, 1024, 41)) | {-1060, -1040, -1023, -1022, 1023})
    rows += [binade(e, -1.0 if e >= 10 else 1.0) for e in es if not -60 <= e < 10]
    return rows


def _sin_rows():
    es = list(range(-60, 31, 3)) + list(range(33, 1024, 45)) + [1023]
    rows = [binade(e) for e in es] + [window(105414350.0 - 100.0, 105414350.0 + 100.0), window(0.126, 0.855469), window(0.855469, 2.426265),
                                      window(2.0 ** -27, 2.0 ** -25)]
    return _both(rows) + [(0.0, INF), (0.0, -INF), (0.0, NAN)]


def _channels_algebra(v, u, w, b):
    return [sqrt(v), recip(v), add(mul(u, v), neg(mul(w, b)))]        # (a difference: the product's rounding shows in the result's last bits)


def _channels_exp_ln(v, u, w, b):
    return [exp(v), ln(abs_(v)), exp(ln(abs_(v)))]


def _channels_sin(v, u, w, b):
    return [sin(v), mul(nat(255), step(sin(v))), sin(add(v, nat(1)))]


SCENES = {'algebra': (_algebra_rows(), _channels_algebra), 'exp_ln': (_exp_ln_rows(), _channels_exp_ln), 'sin_any': (_sin_rows(), _channels_sin)}
NAMES = ('algebra', 'exp_ln', 'sin_any', 'sin_bounded')
FORMS = ('x', 'y')
# the parameter of sin_bounded: |m p| < 2^26, inside the range in which the sine's reduction is the bounded one
PARAM, PARAM_RANGE = 'p', (-2.0 ** 25, 2.0 ** 25)
FRAMES = [s * 2.0 ** e for e in range(-40, 26, 5) for s in (1.0, -1.0)] + [3.0]


def rows_of(name):
    return SCENES[name][0]


def size(name, form):
    """(w, h) of a scene's form."""
    if name == 'sin_bounded':
        return W, PARAM_ROWS[form]
    n = len(rows_of(name))
    return W, n if form == 'x' else REPEATS * n


def _coords(form):
    return (x(), y()) if form == 'x' else (nat(COLUMN), y())


def _row_index(name, form):
    """The table row of image row y: y itself, or y modulo the table's length in the y-only form."""
    n = len(rows_of(name))
    if form == 'x':
        return y()
    wraps = None
    for k in range(1, REPEATS):
        s = step(add(y(), neg(nat(k * n))))
        wraps = s if wraps is None else add(wraps, s)
    return add(y(), neg(mul(nat(n), wraps)))


def operands(name, form):
    """(v, u, w, B) as expressions."""
    xe, ye = _coords(form)
    m, u, w = (mantissa(j, xe, ye) for j in range(3))
    if name == 'sin_bounded':
        return mul(m, var(PARAM)), u, w, nat(1)
    t = _row_index(name, form)
    a, b = table(t, [r[0] for r in rows_of(name)]), table(t, [r[1] for r in rows_of(name)])
    return add(a, mul(m, b)), u, w, b


def channels(name, form):
    fn = _channels_sin if name == 'sin_bounded' else SCENES[name][1]
    return fn(*operands(name, form))


def args_channels(name, form):
    """The `args` scene: v, u and w * B themselves."""
    v, u, w, b = operands(name, form)
    return [v, u, mul(w, b)]


def data(name, form, args=False):
    return encode(size(name, form), (args_channels if args else channels)(name, form))


def arguments_np(name, form, p=None):
    """The numpy model of the args scene: an (h, w, 3) f64 array (v, u, w * B); sin_bounded takes the parameter's value."""
    w, h = size(name, form)
    ys = np.arange(h)[:, None]
    xs = np.arange(w)[None, :] if form == 'x' else np.full((1, w), COLUMN)
    m, u, ww = (mantissa_np(j, xs, ys) for j in range(3))
    with np.errstate(all='ignore'):
        if name == 'sin_bounded':
            return np.stack([m * p, u, ww * 1.0], axis=-1)
        rows = rows_of(name)
        a = np.array([rows[i % len(rows)][0] for i in range(h)])[:, None]
        b = np.array([rows[i % len(rows)][1] for i in range(h)])[:, None]
        return np.stack([a + m * b, u, ww * b], axis=-1)


# ---- scenes, declared and lowered --------------------------------------------------------------------------------------
def scene(name, form):
    """maray_amd.Scene, with the parameter declared where the scene has one."""
    import maray_amd as M
    s = M.Scene(data(name, form))
    if name == 'sin_bounded':
        assert s.declare_param(PARAM, *PARAM_RANGE) == 0
    return s


def frames(name):
    """The parameter vectors a scene is rendered with: [()] for a scene without parameters."""
    return [(p,) for p in FRAMES] if name == 'sin_bounded' else [()]


def frame_data(name, form, values=(), args=False):
    """The scene the oracle renders for a frame: the parameter replaced by an exact constant."""
    if not values:
        return data(name, form, args)
    from params import substituted_exact
    ch = (args_channels if args else channels)(name, form)
    return encode(size(name, form), substituted_exact(ch, [var(PARAM)[1]], values))


@functools.lru_cache(None)
def oracle(name, form, values=(), args=False):
    """(rgb8, f64 planes) of the oracle, computed once per process and shared (do not write to them)."""
    import os
    from oracle_ffi import Scene as OScene
    w, h = size(name, form)
    want8, want64 = OScene(frame_data(name, form, values, args)).render_rows(w, h, 0, h, textures(), threads=min(16, os.cpu_count() or 1))
    want8.setflags(write=False)
    want64.setflags(write=False)
    return want8, want64


def first_mismatch(got64, want64):
    """'' or a description of the first pixel whose f64 bits differ (the mismatching value in hex pins the branch)."""
    g, w_ = np.ascontiguousarray(got64, np.float64), np.ascontiguousarray(want64, np.float64)
    bad = ~((g.view(np.uint64) == w_.view(np.uint64)) | (np.isnan(g) & np.isnan(w_)))
    if not bad.any():
        return ''
    yy, xx, c = (int(i) for i in np.argwhere(bad)[0])
    return '%d differ; first at x %d y %d channel %d: got %s want %s' % (int(bad.sum()), xx, yy, c, float(g[yy, xx, c]).hex(), float(w_[yy, xx, c]).hex())

"""Exact edge-value scenes: every op of the tape fed with IEEE edge values (zeros of both signs, subnormals, the ends of
the finite range, infinities, NaN) and with the neighbourhoods of the points where the device's libm, sqrt and casts
change branch -- in each form the lowering and the specialised kernels produce.

Every double is built exactly from the scene language: a 53-bit mantissa as hi * 2^26 + lo (Nat, Mul, Add) scaled by
powers of two (Nat(2^k), Recip(Nat(2^30))) in an order in which no intermediate rounds; -0 is Neg(+0), +-inf Recip(+-0),
NaN inf + -inf.  Per-row and per-pixel tables are sums of c_i * [t == i] with [t == i] = min(step(t - i), step(i - t)),
exact for finite c_i; infinities, NaN and -0 are composed on top (inf * 0 would be NaN).

A neighbourhood row y runs the 64 (or more) consecutive doubles around one hard point:
v(x, y) = (M(y) + (x - 32)) * S(y), with S(y) the hard point's ulp (its sign carrying the sign of the point) and
M(y) = h / S(y); rows of NaN, +-inf and +-0 are in the table too.  M and S read only y: the table work is done per row.

Each op's scene has three channels: the raw result r (its f64 plane compared bit for bit), and two channels whose RGB8
bytes show what matters when there is no f64 plane: the sign pattern of r (step(r), step(-r), step(1/r): NaN shows as
neither sign, +0 and -0 as +inf and -inf), and r's distance from a reference value of the row in units that make the
low bits move the byte (a layout bug that hands a lane another pixel's value moves it too)."""
import math
import struct

from marayb import add, app, channel, max_, min_, mul, nat, neg, recip, sin, exp, ln, sqrt, step, abs_, x, y

INF, NAN = math.inf, math.nan


def f64(bits):
    return struct.unpack('<d', struct.pack('<Q', bits))[0]


def bits(v):
    return struct.unpack('<Q', struct.pack('<d', v))[0]


def ulp_below(h):
    """The distance from |h| to the next double towards zero (2^-1074 for the smallest magnitudes)."""
    a = abs(h)
    return a - f64(bits(a) - 1) if a > 5e-324 else 5e-324


# ---- exact constants --------------------------------------------------------------------------------------------
def const(v):
    """An Expr whose value is exactly the double v (every double, NaN, +-inf and -0 included)."""
    if v != v:
        return add(recip(nat(0)), neg(recip(nat(0))))           # inf + -inf
    if v == INF:
        return recip(nat(0))
    if v == -INF:
        return recip(neg(nat(0)))
    if v == 0:
        return neg(nat(0)) if math.copysign(1.0, v) < 0 else nat(0)
    m, e = math.frexp(abs(v))
    m, e = int(m * (1 << 53)), e - 53                          # |v| = m * 2^e, m < 2^53
    while m % 2 == 0:
        m, e = m // 2, e + 1
    hi, lo = divmod(m, 1 << 26)
    c = nat(lo) if hi == 0 else add(mul(nat(hi), nat(1 << 26)), nat(lo))
    # scale by 2^e: every intermediate lies between m and |v|, so all are doubles and no step rounds
    while e > 0:
        k = min(e, 30)
        c, e = mul(c, nat(1 << k)), e - k
    while e < 0:
        k = min(-e, 30)
        c, e = mul(c, recip(nat(1 << k))), e + k
    return neg(c) if v < 0 else c


def is_(t, i):
    """[t == i] for an integer-valued t: 1.0 or 0.0."""
    return min_(step(add(t, neg(nat(i)))), step(add(nat(i), neg(t))))


def table(t, vals):
    """v(t) = vals[t] for t = 0 .. len(vals) - 1, exactly; 0.0 elsewhere.  Infinities, NaN and -0 by composition."""
    acc = None
    flip = None                                               # -1 where the entry is -0 or -inf
    for i, v in enumerate(vals):
        b = is_(t, i)
        if v != v:
            term = add(recip(add(nat(1), neg(b))), neg(recip(add(nat(1), neg(b)))))      # inf - inf at i, 1 - 1 elsewhere
        elif math.isinf(v):
            term = add(recip(add(nat(1), neg(b))), neg(nat(1)))                           # inf at i, +0 elsewhere
        elif v == 0:
            term = None
        else:
            term = mul(const(v), b)
        if term is not None:
            acc = term if acc is None else add(acc, term)
        if math.copysign(1.0, v) < 0 and (v == 0 or math.isinf(v)):
            flip = b if flip is None else add(flip, b)
    acc = nat(0) if acc is None else acc
    if flip is not None:
        acc = mul(acc, add(nat(1), mul(flip, neg(nat(2)))))                               # x (1 - 2 [negative special])
    return acc


# ---- the edge table ---------------------------------------------------------------------------------------------
H = float.fromhex
MIN_SUB, MAX_SUB, MIN_NORM, MAX_FIN = 5e-324, H('0x0.fffffffffffffp-1022'), H('0x1p-1022'), H('0x1.fffffffffffffp+1023')
# (name, hard point): each gives a neighbourhood row of each sign; sources: libm_check.cpp's specials and the branch points
# of maray_libm.h / device_math.h
HARD = [
    ('min subnormal', MIN_SUB), ('max subnormal', MAX_SUB), ('min normal', MIN_NORM), ('max finite', MAX_FIN),
    ('1', 1.0), ('0.5', 0.5), ('2', 2.0),
    ('sqrt scaling 2^-767', H('0x1p-767')),
    ('exp overflow', 709.782712893384), ('exp subnormal results', -708.3964185322641), ('exp last nonzero', -745.1332191019411),
    ('ln 0.93', 0.93), ('ln 0.9375', 0.9375), ('ln 1.0647', 1.0647), ('ln 1.07', 1.07),
    ('2^-26', H('0x1p-26')), ('2^-27', H('0x1p-27')), ('0.126', 0.126), ('do_cos 0.855469', 0.855469), ('2.426265', 2.426265),
    ('pi/2', math.pi / 2), ('pi', math.pi), ('3pi/2', 3 * math.pi / 2), ('2pi', 2 * math.pi), ('1e6 pi/2', H('0x1.7f6a7a2955385p+20')),
    ('22', 22.0), ('355', 355.0),
    ('reduce_sincos edge', 105414350.0), ('1e22', 1e22), ('0x1.6ac5b262ca1ffp+849', H('0x1.6ac5b262ca1ffp+849')),
    ('1e300', 1e300), ('1e-300', 1e-300),
]
# the rows of the neighbourhood scene: (name, M, S); v = (M + (x - 32)) * S
ROWS = []
for _name, _h in HARD:
    _s = ulp_below(_h)
    ROWS.append((_name, _h / _s, _s))
    ROWS.append(('-' + _name, _h / _s, -_s))
ROWS += [('integers', 0.0, 1.0), ('-integers', 0.0, -1.0), ('x inf', 0.0, INF), ('x -inf', 0.0, -INF),
         ('inf', INF, 1.0), ('-inf', -INF, 1.0), ('nan', NAN, 1.0)]

# single values (the cross product of the binary ops, the y-only and constant operands)
VALUES = [0.0, -0.0, INF, -INF, NAN]
for _name, _h in HARD:
    _u = ulp_below(_h)
    VALUES += [_h, -_h, f64(bits(_h) + 1), f64(bits(_h) - 1), -f64(bits(_h) + 2)]
VALUES += [math.pi / 2 * k for k in (5, 9, 1001)] + [f64(bits(105414350.0) + 7), -f64(bits(105414350.0) - 3), 1024.0, -1024.0, 709.79, -745.14]


def rows_table(col):
    """M(y) (col 1) or S(y) (col 2) of ROWS as a y table."""
    return table(y(), [r[col] for r in ROWS])


def neighbourhood():
    """v(x, y) = (M(y) + (x - 32)) * S(y): x-varying, its tables y-only."""
    return mul(add(rows_table(1), add(x(), neg(nat(32)))), rows_table(2))


# ---- the ops ----------------------------------------------------------------------------------------------------
UNARY = {'neg': neg, 'abs': abs_, 'recip': recip, 'sqrt': sqrt, 'step': step, 'sin': sin, 'stepsin': lambda a: step(sin(a)),
         'exp': exp, 'ln': ln}
BINARY = {'add': add, 'mul': mul, 'max': max_, 'min': min_}
LIBM = ('sin', 'stepsin', 'exp', 'ln')
# tape opcode of each op (include/maray_tape.h)
OPCODE = dict(neg=2, abs=3, recip=4, sqrt=5, step=6, sin=7, exp=8, ln=9, add=10, mul=11, max=12, min=13, app=14, stepsin=17)


def py_op(name, a, b=None):
    """The op in Python, for picking reference values and scales only (no result is compared against it)."""
    try:
        if name == 'neg': return -a
        if name == 'abs': return abs(a)
        if name == 'recip': return 1.0 / a if a != 0 else math.copysign(INF, a)
        if name == 'sqrt': return math.sqrt(a) if a >= 0 else NAN
        if name == 'step': return 1.0 if a >= 0 else 0.0
        if name == 'sin': return math.sin(a)
        if name == 'stepsin': return 1.0 if math.sin(a) >= 0 else 0.0
        if name == 'exp': return math.exp(a)
        if name == 'ln': return math.log(a) if a > 0 else (-INF if a == 0 else NAN)
        if name == 'add': return a + b
        if name == 'mul': return a * b
        if name == 'max': return max(a, b)
        if name == 'min': return min(a, b)
    except (ValueError, OverflowError):
        return NAN
    raise ValueError(name)


def pow2_at_most(v):
    """The largest power of two <= v (v > 0 finite), as a double that const() builds exactly."""
    return math.ldexp(1.0, math.frexp(v)[1] - 1)


def fingerprint(r, ref, unit):
    """Two channels whose RGB8 bytes show r: its sign pattern and its distance from `ref` in `unit`s (both exprs)."""
    signs = add(add(mul(step(r), nat(64)), mul(step(neg(r)), nat(128))), mul(step(recip(r)), nat(32)))
    dist = add(mul(add(r, neg(ref)), unit), nat(128))                        # not clamped: the cast saturates (and NaN -> 0)
    return [add(signs, add(mul(add(r, neg(ref)), mul(unit, recip(nat(1 << 10)))), nat(16))), dist]


def _row_refs(name, width, arg_of_row):
    """Per neighbourhood row: a reference value (the op at the row's hard point) and a unit in which r's spread over the
    row is about 100 -- both exact powers of two or exact doubles, as y tables."""
    refs, units = [], []
    for i, (_, m, s) in enumerate(ROWS):
        vals = []
        for xx in (0, min(width, 64) - 1, 32):
            a = (m + (xx - 32)) * s
            vals.append(py_op(name, *arg_of_row(i, a)))
        ref = vals[2] if math.isfinite(vals[2]) else 0.0
        spread = max((abs(v - ref) for v in vals[:2] if math.isfinite(v - ref)), default=0.0)
        scale = abs(ref) * 2.0 ** -52 if ref else 0.0
        unit = 100.0 / spread if spread > 0 and math.isfinite(100.0 / spread) else (1.0 / scale if scale > MIN_NORM and math.isfinite(1.0 / scale) else 1.0)
        refs.append(ref)
        units.append(pow2_at_most(min(unit, 2.0 ** 1000)))
    return table(y(), refs), table(y(), units)


def partner(i):
    """The right operand of a binary op on neighbourhood row i: the hard point of another row, or a special."""
    return VALUES[(7 * i + 3) % len(VALUES)]


def op_on(name, a, b=None):
    return BINARY[name](a, b) if name in BINARY else UNARY[name](a)


def scene_x(name, width, heavy):
    """Form (a) / (b): the op on the x-varying neighbourhood operand (binary ops: left = neighbourhood, right = a y-only
    value of the edge table).  heavy: a Step(Sin) of x joins the second channel, which keeps the program from the
    four-pixels-per-lane form (jit_wide_general).  Height len(ROWS)."""
    v = neighbourhood()
    if name in BINARY:
        rhs = table(y(), [partner(i) for i in range(len(ROWS))])
        r = op_on(name, v, rhs)
        ref, unit = _row_refs(name, width, lambda i, a: (a, partner(i)))
    else:
        r = op_on(name, v)
        ref, unit = _row_refs(name, width, lambda i, a: (a,))
    fp = fingerprint(r, ref, unit)
    if heavy:
        fp[0] = add(fp[0], step(sin(mul(x(), recip(nat(7))))))
    return [r] + fp


def scene_cross(name):
    """Binary ops, narrow form (a): the full cross product of VALUES, x selects the left operand, y the right one."""
    n = len(VALUES)
    r = op_on(name, table(x(), VALUES), table(y(), VALUES))
    ref = table(y(), [v if math.isfinite(v) else 0.0 for v in VALUES])
    unit = table(y(), [pow2_at_most(2.0 ** 40 / abs(v)) if v and math.isfinite(v) and abs(v) > 2.0 ** -900 else 1.0 for v in VALUES])
    return [r] + fingerprint(r, ref, unit), n


def scene_y(name):
    """Form (c): the op on a y-only operand (VALUES by row; binary ops: the right operand is VALUES by row too, shifted).
    x enters only outside the op, so every pixel of a row shows the row's result; height len(VALUES)."""
    n = len(VALUES)
    a = table(y(), VALUES)
    if name in BINARY:
        r = op_on(name, a, table(y(), [VALUES[(5 * i + 1) % n] for i in range(n)]))
    else:
        r = op_on(name, a)
    xs = mul(add(x(), neg(nat(1))), recip(nat(1 << 20)))         # tiny, per pixel: the byte channels vary along the row
    return [r] + fingerprint(r, xs, nat(1 << 27))


def scene_const(name, vals):
    """Form (d): the op on constant operands (never folded for sin, exp, ln: lower.cpp), up to three channels' worth."""
    return [UNARY[name](const(v)) for v in vals]


def guarded_mask_scene(w, h, vals):
    """Form (e): scenes.ops_on_a_guarded_mask with edge values in the ops' operands: each op reads the value of a guarded
    shape (a literal 0.0 in tiles outside every guard) combined with an edge value, so the literal-zero variant and the
    busy variant both meet them."""
    import scenes
    return scenes.ops_on_a_guarded_mask(w, h, edge=[const(v) for v in vals])


def bool_scene():
    """Form (f): boolean masks (x-varying) and y-only booleans as operands of non-boolean ops, against edge values."""
    bx = step(add(nat(31), neg(x())))                            # 1 for x <= 31
    by = step(add(y(), neg(nat(len(VALUES) // 2))))              # 1 for the lower half of the rows
    v = table(y(), VALUES)
    c0 = add(mul(bx, v), recip(add(by, neg(nat(1)))))             # bool * edge, + recip(0 or -1): -inf / -1
    c1 = max_(min_(by, v), mul(bx, by))
    c2 = add(sqrt(mul(add(bx, by), v)), ln(add(bx, abs_(v))))
    return [c0, c1, c2]


def texel_scene():
    """Form (g): texel lookups whose coordinates come from the edge table (x selects the column coordinate, y the row's)."""
    u = table(x(), VALUES[:48] + [-0.5, -0.25, 0.5, 36.5, 37.0, 22.9999, 23.0, 1e9])
    v = table(y(), [0.0, -0.0, 0.5, -0.5, 22.0, 22.5, 23.0, INF, -INF, NAN, MIN_SUB, -MIN_SUB, 4294967295.0, 4294967296.0, 1e300])
    return [app(channel(0, 0), u, v), add(app(channel(0, 1), v, u), app(channel(0, 2), u, nat(3))), app(channel(0, 2), add(u, nat(1)), v)]


# ---- the matrix ---------------------------------------------------------------------------------------------------
# Constant operands of sin, exp and ln (never folded on the host): the hard points of each, three to a scene.
CONST_VALUES = {
    'sin': [0.0, -0.0, INF, NAN, H('0x1p-26'), H('0x1p-27'), f64(bits(math.pi) + 2), f64(bits(math.pi / 2) - 2), 0.855469,
            2.426265, 105414350.0, f64(bits(105414350.0) - 1), 1e22, H('0x1.6ac5b262ca1ffp+849'), -MIN_SUB],
    'exp': [709.782712893384, f64(bits(709.782712893384) + 1), -708.3964185322641, f64(bits(-708.3964185322641) + 1),
            -745.1332191019411, f64(bits(-745.1332191019411) + 1), -0.0, -INF, INF, NAN, MIN_SUB, -1024.0],
    'ln': [MIN_SUB, MAX_SUB, MIN_NORM, MAX_FIN, f64(bits(1.0) - 1), f64(bits(1.0) + 1), 0.93, 1.07, -0.0, -1.0, INF, NAN],
}
CONST_VALUES['stepsin'] = CONST_VALUES['sin']
GUARDED_EDGES = [(-0.0, INF, NAN), (MIN_SUB, -MAX_FIN, H('0x1p-767')), (709.782712893384, -745.1332191019411, 105414350.0)]
WIDTHS = (1, 3, 63, 65, 257, 302)


class Case:
    """One (op, form) cell: the scene's channels, its size, the lowering option, and the form the product must reach."""

    def __init__(self, op, form, channels, w, h, hoist=True, textures=False, tag=''):
        self.op, self.form, self.channels, self.w, self.h, self.hoist, self.textures = op, form, channels, w, h, hoist, textures
        self.id = '%s-%s%s' % (op, form, tag)

    def data(self):
        from marayb import encode
        return encode((self.w, self.h), self.channels)


def cases():
    """Every (op, form) cell of the matrix."""
    out = []
    for op in list(UNARY) + list(BINARY):
        out.append(Case(op, 'x-narrow', scene_x(op, 64, heavy=True), 64, len(ROWS)))
        if op not in LIBM:
            out.append(Case(op, 'x-wide', scene_x(op, 64, heavy=False), 64, len(ROWS)))
        if op in BINARY:
            ch, n = scene_cross(op)
            out.append(Case(op, 'cross', ch, n, n))
        out.append(Case(op, 'y-row', scene_y(op), 64, len(VALUES)))
        out.append(Case(op, 'y-pixel', scene_y(op), 64, len(VALUES), hoist=False))
    for op in LIBM:
        vals = CONST_VALUES[op]
        for i in range(0, len(vals), 3):
            out.append(Case(op, 'const-row', scene_const(op, vals[i:i + 3]), 4, 2, tag=str(i // 3)))
            out.append(Case(op, 'const-pixel', scene_const(op, vals[i:i + 3]), 4, 2, hoist=False, tag=str(i // 3)))
    for i, vals in enumerate(GUARDED_EDGES):
        out.append(Case('all', 'guarded', guarded_mask_scene(512, 256, vals), 512, 256, textures=True, tag=str(i)))
    out.append(Case('all', 'bool', bool_scene(), 64, len(VALUES)))
    out.append(Case('app', 'texel', texel_scene(), 56, 15, textures=True))
    ch, n = texel_wide_scene()
    out.append(Case('app', 'texel-wide', ch, 64, n, textures=True))
    return out


def texel_wide_scene():
    """Form (g) in a program small enough for the four-pixels-per-lane form: u = (x + A(y)) * B(y), v = V(y) -- negative,
    fractional (-1 < u < 0 included), -0, +-inf, NaN and past-2^32 coordinates from row tables."""
    rows = [(-32.0, 1.0, 0.0), (-32.0, 0.25, 3.0), (0.0, -0.5, -0.0), (-32.0, INF, 22.0), (NAN, 1.0, 1.0),
            (4294967295.0 - 32.0, 1.0, 2.0), (-32.0, -1.0 / 64, 22.9999), (0.0, 1.0, 23.0), (0.0, 1.0, -0.5),
            (0.0, 1.0, NAN), (0.0, 1.0, INF), (-4.0, 1.0, 4294967296.0), (0.0, MIN_SUB, 5.0), (-1.0, 0.5, -MIN_SUB)]
    u = mul(add(x(), table(y(), [r[0] for r in rows])), table(y(), [r[1] for r in rows]))
    v = table(y(), [r[2] for r in rows])
    return [app(channel(0, 0), u, v), app(channel(0, 1), v, u), app(channel(0, 2), u, add(v, nat(1)))], len(rows)


def textures():
    """The two images of the texel and guarded scenes: 37 x 23 and the scale-8 pair's second."""
    import numpy as np
    import scenes
    t = scenes.textures(scale=8)
    rng = np.random.default_rng(5)
    return [rng.integers(0, 256, (23, 37, 3), dtype=np.uint8), t[1]]

"""Random scene generator for the parity fuzz tests (deterministic per seed)."""
import math
import random

from marayb import (abs_, add, app, arc, channel, decor, div, exp, image_height, image_width, let_, ln, max_, min_, mul,
                    nat, neg, recip, sin, sqrt, step, sub, var_id, x, y)

UN = [neg, abs_, recip, sqrt, step, sin, exp, ln]
BIN = [add, mul, max_, min_]


def _leaf(rng, vars_):
    r = rng.random()
    if vars_ and r < 0.25: return var_id(rng.choice(vars_))
    if r < 0.50: return x()
    if r < 0.70: return y()
    if r < 0.90: return nat(rng.choice([0, 1, 2, 3, 5, 7, 16, 100, 255, 1024, 10 ** 6, 10 ** 12]))
    return rng.choice([('Tau',), ('E',)])


def _expr(rng, depth, vars_, n_tex):
    if depth <= 0 or rng.random() < 0.12:
        return _leaf(rng, vars_)
    r = rng.random()
    if r < 0.08:   # scaled coordinate, keeps many arguments in a moderate range
        return mul(_leaf(rng, vars_), div(nat(1), nat(rng.choice([3, 7, 64, 1000]))))
    if r < 0.40:
        f = rng.choice(UN)
        return f(_expr(rng, depth - 1, vars_, n_tex))
    if r < 0.80:
        f = rng.choice(BIN)
        return f(_expr(rng, depth - 1, vars_, n_tex), _expr(rng, depth - 1, vars_, n_tex))
    if r < 0.86:   # boolean algebra, the shapes the skip regions look for
        a = step(_expr(rng, depth - 1, vars_, n_tex)); b = step(_expr(rng, depth - 1, vars_, n_tex))
        c = rng.choice([min_, max_, mul])(a, rng.choice([b, sub(nat(1), b)]))
        return c if rng.random() < 0.5 else mul(c, _expr(rng, depth - 2, vars_, n_tex))
    if r < 0.885:   # half-plane polygons gating a heavier cone: what the row bounds and SKIP regions target
        def half_plane():
            a, b, c = rng.choice([1, 2, 3, 7]), rng.choice([0, 1, 2, 5]), rng.randrange(0, 200)
            e_ = sub(add(mul(x(), nat(a)), mul(y(), nat(b))), nat(c))
            e_ = mul(e_, div(nat(1), nat(rng.choice([1, 3, 16]))))
            return step(e_ if rng.random() < 0.5 else neg(e_))
        poly = min_(min_(half_plane(), half_plane()), half_plane())
        heavy = _expr(rng, depth - 1, vars_, n_tex)
        for _ in range(3):
            heavy = add(mul(heavy, heavy), sin(add(heavy, x())))
        body = step(heavy) if rng.random() < 0.5 else heavy
        return rng.choice([mul, min_])(poly, body) if body[0] == 'Step' else mul(poly, body)
    if r < 0.90 and n_tex:
        t = rng.randrange(n_tex)
        sel = rng.choice([channel(t, 0), channel(t, 1), channel(t, 2), image_width(t), image_height(t)])
        return app(sel, _expr(rng, depth - 1, vars_, n_tex), _expr(rng, depth - 1, vars_, n_tex))
    if r < 0.93:
        return arc(_expr(rng, depth - 1, vars_, n_tex))
    if r < 0.95:
        return decor(_expr(rng, depth - 1, vars_, n_tex), ['note', 2, ('TokenExpr', x())])
    # Let with definitions that reference earlier ones (like the compressor's output, src/compressor.rs:226-232)
    base = rng.randrange(0, 1000) * 10
    ids, defs = [], []
    for k in range(rng.randint(1, 4)):
        defs.append((base + k, _expr(rng, depth - 2, ids[:], n_tex)))
        ids.append(base + k)
    return let_(defs, _expr(rng, depth - 1, ids, n_tex))


def scene(seed, depth=6, n_tex=0):
    """Three channel expressions.  Let ids are unique per Let (base chosen at random), so the reference's
    id-keyed Cache stays value-transparent; scenes that still alias are skipped by the caller."""
    rng = random.Random(seed)
    return [_expr(rng, depth, [], n_tex) for _ in range(3)]


class _Plain:
    """What the soups are built with when no parameter is planted: every hook is the identity."""
    def coord(self, e): return e
    def radius(self, e): return e
    def level(self, e): return e
    def colour(self, e): return e


def polygon_soup(seed, n, w, h, mixed=True, plant=_Plain()):
    """n random textured triangles painted over one another (max chain), the kind of scene `examples/chess.rs` builds
    and the lowering's shape machinery targets: balanced OR trees, group and shape guards, private regions.  Vertices
    are integers inside (and a little outside) the w x h image; each triangle carries a chess pattern in its own
    barycentric frame; channels differ in a gradient term and, with `mixed`, in which triangles they paint (every shape
    is then shared by two OR trees)."""
    from marayb import chess, inside_triangle, to_uv
    rng = random.Random(0x50117 + seed)
    p = [x(), y()]
    tris = []
    for _ in range(n):
        cx, cy = rng.randrange(0, w), rng.randrange(0, h)
        r = rng.choice([6, 12, 25, 60])
        pts = [(nat(max(0, cx + rng.randrange(-r, r + 1))), nat(max(0, cy + rng.randrange(-r, r + 1)))) for _ in range(3)]
        if len({(a[1], b[1]) for a, b in pts}) < 3:
            continue
        pts = [(plant.coord(a), plant.coord(b)) for a, b in pts]
        inside = inside_triangle(pts, p)
        uv = to_uv(pts, [(nat(0), nat(0)), (nat(1), nat(0)), (nat(0), nat(1))], p)
        pattern = subst_xy(chess(rng.choice([2, 4, 6])), uv[0], uv[1])
        tris.append(min_(inside, pattern) if rng.random() < 0.7 else inside)
    if not tris:
        tris = [step(sub(x(), nat(w)))]

    def paint(items):
        acc = items[0]
        for t in items[1:]:
            acc = max_(acc, t)
        return acc
    grad = mul(add(x(), mul(y(), nat(3))), div(nat(1), nat(w + 3 * h)))
    if mixed == 'colours':      # every shape has its own colour: channel = max_i(shape_i * c_i), a max chain of non-booleans
        cols = [[plant.colour(div(nat(rng.randrange(1, 9)), nat(8))) for _ in range(3)] for _ in tris]
        return [mul(max_(paint([mul(t, c[k]) for t, c in zip(tris, cols)]), mul(grad, div(nat(1), nat(8)))), nat(255)) for k in range(3)]
    if not mixed:       # one mask for the three channels, like examples/chess.rs: the shapes belong to one tree
        m = paint(tris)
        return [mul(m, nat(255)), mul(max_(m, mul(grad, div(nat(1), nat(2)))), nat(255)), mul(add(mul(m, div(nat(3), nat(4))), mul(grad, div(nat(1), nat(4)))), nat(255))]
    return [mul(paint(tris), nat(255)), mul(max_(paint(tris[::2]), mul(grad, div(nat(1), nat(2)))), nat(255)),
            mul(add(mul(paint(tris[1::2] or tris), div(nat(3), nat(4))), mul(grad, div(nat(1), nat(4)))), nat(255))]


def subst_xy(e, ex, ey):
    """e with X -> ex and Y -> ey (tuple expression trees)."""
    if e[0] == 'X': return ex
    if e[0] == 'Y': return ey
    return tuple(subst_xy(c, ex, ey) if isinstance(c, tuple) and c and isinstance(c[0], str) else c for c in e)


def curved_soup(seed, n, w, h, mixed=False, plant=_Plain()):
    """n random CURVED shapes painted over one another: the gating shapes are not half-planes but signed-distance
    circles, boxes and rounded boxes (Sd2, /root/reference/src/sd.rs:28-48: sqrt, abs, max / min of differences), cubic
    Bezier strokes (p2_cbez, src/lib.rs:1061-1065, the curve's y at a clamped parameter of x, a band of |y - c(t)|
    around it) and 1/(1 + d^2) falloffs cut at a level -- so that the sqrt / recip / abs / corner-product paths of the
    lowering's interval bounds (RowBounds::ival, lower.cpp) decide which rectangles of pixels skip a shape.  Each
    shape carries a pattern in its own frame (a cone worth guarding); `mixed`: False = one mask for the three channels,
    True = channels paint different subsets, 'colours' = channel = max_i(shape_i * falloff_i): max trees of non-booleans."""
    from marayb import (abs_, chess, clamp_unit, p2_cbez, p2_lerp, p2_pos, p4_xy, p4_zw, pos, range_, sd_box, sd_circle, sd_inside,
                        set_inv, subst2, translate)
    rng = random.Random(0xC0FFEE + seed)
    shapes, falloffs = [], []
    for _ in range(n):
        cx, cy = rng.randrange(0, w), rng.randrange(0, h)
        r = rng.choice([5, 9, 17, 33, 70])
        off = [plant.coord(nat(cx)), plant.coord(nat(cy))]
        kind = rng.choice(['circle', 'box', 'rbox', 'stroke', 'falloff', 'ring'])
        dx, dy = sub(x(), off[0]), sub(y(), off[1])
        d2 = add(mul(dx, dx), mul(dy, dy))
        if kind == 'circle':
            inside = sd_inside(translate(sd_circle(plant.radius(nat(r))), off))
        elif kind == 'box':
            inside = sd_inside(translate(sd_box([plant.radius(nat(r)), nat(max(2, r // rng.choice([1, 2, 3])))]), off))
        elif kind == 'rbox':                              # Sd2::RoundedBox, src/sd.rs:39-47
            b = [nat(r), nat(max(3, r // 2))]
            rr = [div(nat(rng.randrange(1, 5)), nat(2)) for _ in range(4)]
            rxy = p2_pos(x(), p4_xy(rr), p4_zw(rr))
            rx = pos(y(), rxy[0], rxy[1])
            q = [add(sub(abs_(x()), b[0]), rx), add(sub(abs_(y()), b[1]), rx)]
            sd = sub(add(min_(max_(q[0], q[1]), nat(0)), sqrt(add(mul(max_(q[0], nat(0)), max_(q[0], nat(0))), mul(max_(q[1], nat(0)), max_(q[1], nat(0)))))), rx)
            inside = sd_inside(translate(sd, off))
        elif kind == 'stroke':                            # the band |y - c_y(t(x))| <= th over x in [x0, x0 + L)
            L = rng.choice([40, 90, 200])
            x0 = max(0, cx - L // 2)
            t = clamp_unit(mul(sub(x(), nat(x0)), div(nat(1), nat(L))))
            pts = [[nat(x0 + L * k // 3), nat(max(0, cy + rng.randrange(-r, r + 1)))] for k in range(4)]
            c = p2_cbez(pts[0], pts[1], pts[2], pts[3], t)
            th = plant.radius(nat(rng.choice([2, 4, 7])))
            inside = min_(step(sub(th, abs_(sub(y(), c[1])))), range_(nat(x0), nat(x0 + L), x()))
        elif kind == 'falloff':                           # 1 / (1 + d^2 / s) >= 1/k  <=>  d^2 <= (k - 1) s
            s_, k = rng.choice([4, 16, 50]), rng.choice([2, 5, 17])
            inside = step(sub(recip(add(nat(1), mul(d2, div(nat(1), nat(s_))))), plant.level(div(nat(1), nat(k)))))
        else:                                             # ring: r/2 <= d <= r, through two sqrt tests
            d = sqrt(d2)
            inside = min_(step(sub(plant.radius(nat(r)), d)), step(sub(d, div(nat(r), nat(2)))))
        u, v = mul(dx, div(nat(1), nat(max(2, r // 2)))), mul(dy, div(nat(1), nat(max(2, r // 2))))
        pat = rng.random()
        if pat < 0.45:
            pattern = subst_xy(chess(rng.choice([2, 4])), u, v)
        elif pat < 0.75:
            pattern = step(sin(add(mul(u, nat(3)), mul(v, v))))
        else:
            pattern = None
        shapes.append(inside if pattern is None else min_(inside, pattern))
        falloffs.append(recip(add(nat(1), mul(d2, div(nat(1), nat(4 * r * r))))))

    def paint(items):
        acc = items[0]
        for t in items[1:]:
            acc = max_(acc, t)
        return acc
    grad = mul(add(x(), mul(y(), nat(3))), div(nat(1), nat(w + 3 * h)))
    if mixed == 'colours':
        return [mul(max_(paint([mul(s_, mul(f, div(nat(k + 2), nat(4)))) for s_, f in zip(shapes, falloffs)]), mul(grad, div(nat(1), nat(8)))), nat(200))
                for k in range(3)]
    if not mixed:
        m = paint(shapes)
        return [mul(m, nat(255)), mul(max_(m, mul(grad, div(nat(1), nat(2)))), nat(255)), mul(add(mul(m, div(nat(3), nat(4))), mul(grad, div(nat(1), nat(4)))), nat(255))]
    return [mul(paint(shapes), nat(255)), mul(max_(paint(shapes[::2]), mul(grad, div(nat(1), nat(2)))), nat(255)),
            mul(add(mul(paint(shapes[1::2] or shapes), div(nat(3), nat(4))), mul(grad, div(nat(1), nat(4)))), nat(255))]


def product_soup(seed, n, w, h, plant=_Plain()):
    """n shapes whose edge tests are Steps of PRODUCTS, SQUARES, ROOTS and RECIPROCALS of terms that are monotone in x and in y --
    what the lowering's monotonicity rule for two varying factors, its square and abs rules and the end-point bounds decide
    on (lower.cpp: monotonicity, RowBounds): (x + a)(x + b) <= k, (x + a)(y + b) >= k, sqrt(x + a)(y + b) <= k, products of
    two non-positive factors, a factor that changes sign inside the image (no monotone bound: interval corners), 1/(x + a)
    against y.  Each shape carries a Step(Sin) pattern, so that skipping it matters."""
    rng = random.Random(0xBEEF + seed)
    shapes = []
    for _ in range(n):
        a, b = rng.randrange(1, 40), rng.randrange(1, 40)
        k = rng.randrange(1, w * h // 4)
        kind = rng.randrange(8)
        X, Y = x(), y()
        na, nb, nk = plant.coord(nat(a)), plant.coord(nat(b)), plant.level(nat(k))
        if kind == 0:
            e_ = sub(nk, mul(add(X, na), add(X, nb)))                          # (x+a)(x+b) <= k: both factors >= 0, increasing
        elif kind == 1:
            e_ = sub(mul(add(X, na), add(Y, nb)), nk)                          # (x+a)(y+b) >= k
        elif kind == 2:
            e_ = sub(nk, mul(sqrt(add(X, na)), add(Y, nb)))                     # sqrt(x+a)(y+b) <= k
        elif kind == 3:
            e_ = sub(nk, mul(neg(add(X, na)), neg(add(Y, nb))))                 # two non-positive factors
        elif kind == 4:
            e_ = sub(nk, mul(sub(X, nat(rng.randrange(0, w))), sub(X, nat(rng.randrange(0, w)))))      # factors that change sign inside the image
        elif kind == 5:
            c = rng.randrange(0, w)
            e_ = sub(nat(rng.randrange(1, 60) ** 2), add(mul(sub(X, nat(c)), sub(X, nat(c))), mul(sub(Y, nb), sub(Y, nb))))   # a disc, written with squares
        elif kind == 6:
            e_ = sub(mul(recip(add(X, na)), nk), add(Y, nb))                    # k / (x+a) >= y + b
        else:
            e_ = sub(nk, mul(mul(add(X, na), add(X, nb)), add(Y, nat(1))))      # a product of three
        inside = step(e_)
        from marayb import chess
        pattern = subst_xy(chess(rng.choice([2, 3])), mul(add(X, Y), div(nat(1), nat(rng.randrange(5, 19)))), mul(sub(X, Y), div(nat(1), nat(rng.randrange(5, 19)))))
        shapes.append(min_(inside, pattern))
    acc = shapes[0]
    for t in shapes[1:]:
        acc = max_(acc, t)
    grad = mul(add(x(), y()), div(nat(1), nat(w + h)))
    return [mul(acc, nat(255)), mul(max_(acc, mul(grad, div(nat(1), nat(2)))), nat(255)), mul(add(mul(acc, div(nat(1), nat(2))), mul(grad, div(nat(1), nat(2)))), nat(255))]


# ---- scenes with parameters (tests/params.py holds the ranges, the values and the checks) ----------------------------------
PARAM_ID0 = 900000          # fix_color numbers Let variables 0, 1, ...: a parameter id up here meets none of them


def _plant(ex, rng, ids):
    """ex with some constant leaves replaced by a parameter and some X / Y by X + parameter -- inside Let definitions and
    bodies, Arc, Decor and App coordinates alike."""
    t = ex[0]
    if t in ('Nat', 'Tau', 'E'):
        return var_id(rng.choice(ids)) if rng.random() < 0.30 else ex
    if t in ('X', 'Y'):
        return add(ex, var_id(rng.choice(ids))) if rng.random() < 0.12 else ex
    if t == 'Var':
        return ex
    if t == 'Let':
        return ('Let', tuple((i, _plant(d, rng, ids)) for i, d in ex[1]), _plant(ex[2], rng, ids))
    if t == 'Decor':
        return ('Decor', _plant(ex[1], rng, ids), ex[2])
    if t == 'App':
        return ('App', ex[1], _plant(ex[2], rng, ids), _plant(ex[3], rng, ids))
    return (t,) + tuple(_plant(c, rng, ids) for c in ex[1:])


def _observers(color, rng, ids):
    """Terms that show what a max or a sum with +0.0 hides, on a shape large enough to get a guard of its own.  In about a
    quarter of the channels 1 / (shape * p), cut at 1: where the shape is 0 the product is a zero with p's sign, and
    1 / -0.0 = -inf shows a region that was skipped as +0.0.  In about a seventh a band |x + p| < -1, empty for every number
    and the whole plane for p = NaN (the comparison is the inverse of one that NaN fails): a bound that drops the NaN of an
    abs is wrong there."""
    from marayb import lt

    def shape():
        def half_plane():
            e_ = sub(add(mul(x(), nat(rng.choice([1, 2, 3]))), mul(y(), nat(rng.choice([0, 1, 2])))), nat(rng.randrange(10, 160)))
            return step(e_ if rng.random() < 0.5 else neg(e_))
        pattern = step(sin(mul(add(x(), mul(y(), nat(3))), div(nat(1), nat(rng.choice([3, 5, 7]))))))
        return min_(min_(half_plane(), half_plane()), pattern)
    out = []
    for c in color:
        q, p = rng.random(), var_id(rng.choice(ids))
        if q < 0.25:
            c = add(c, min_(recip(mul(shape(), p)), nat(1)))
        elif q < 0.40:
            c = max_(c, mul(min_(lt(abs_(add(x(), p)), neg(nat(1))), shape()), nat(200)))
        out.append(c)
    return out


def param_scene(seed, n_tex=0, n_params=3, n_vectors=5, ranges=None):
    """The random scene of scene(seed, n_tex) with parameters planted: (channels, [(id, lo, hi), ...], value vectors).
    The planting, the ranges, the vectors and the observers (_observers) come from a generator of their own, seeded by
    seed * 7919 + 1."""
    import params as PR
    rng = random.Random(seed * 7919 + 1)
    ids = [PARAM_ID0 + k for k in range(n_params)]
    color = [_plant(c, rng, ids) for c in scene(seed, n_tex=n_tex)]
    decl = [(i,) + tuple(ranges[k] if ranges else rng.choice(PR.RANGES)) for k, i in enumerate(ids)]
    vectors = PR.value_vectors(rng, decl, n_vectors)
    return _observers(color, rng, ids), decl, vectors


class _Planted:
    """The soups' hooks with parameters in them: t, u translate (x + t), s scales (x * s), r changes radii and levels, c is a
    colour factor.  A hook leaves most of what it is given alone, so that most shapes keep the guards a constant gives."""

    def __init__(self, rng, ids):
        self.rng, (self.t, self.u, self.s, self.r, self.c) = rng, [var_id(i) for i in ids]

    def coord(self, e):
        q = self.rng.random()
        if q < 0.10: return add(e, self.t)
        if q < 0.18: return add(e, self.u)
        if q < 0.26: return mul(e, self.s)
        if q < 0.30: return add(mul(e, self.s), self.t)
        return e

    def radius(self, e):
        q = self.rng.random()
        return add(e, self.r) if q < 0.3 else (mul(e, self.s) if q < 0.4 else e)

    def level(self, e):
        return add(e, self.r) if self.rng.random() < 0.3 else e

    def colour(self, e):
        return mul(e, self.c) if self.rng.random() < 0.5 else e


SOUP_RANGES = dict(t=[(-16.0, 16.0), (-64.0, 64.0), (0.0, 40.0), (-0.0, 8.0)], u=[(-24.0, -0.0), (-8.0, 8.0), (3.5, 3.5)],
                   s=[(1.0, 1.0), (-1.0, 2.0), (0.5, 2.0), (-0.0, 1.5)], r=[(0.0, 8.0), (-4.0, 4.0), (-0.0, 0.25)],
                   c=[(0.0, 1.0), (-0.0, 1.0), (-1.0, 1.0), (0.25, 2.0)])


def param_soup(family, seed, n, w, h, n_vectors=4):
    """polygon_soup / curved_soup / product_soup (family 0 / 1 / 2) with parameters planted in vertices, radii and levels and
    as colour factors of the three channels: (channels, [(id, lo, hi), ...], value vectors).  Five parameters with finite
    ranges (the scale's include one across zero and the degenerate [1, 1]) and a sixth that may be anything, NaN included."""
    import params as PR
    rng = random.Random(0x9A2A + 31 * seed + family)
    ids = [PARAM_ID0 + k for k in range(5)]
    plant = _Planted(rng, ids)
    if family == 0:
        color = polygon_soup(seed, n, w, h, mixed=(True, False, 'colours')[seed % 3], plant=plant)
    elif family == 1:
        color = curved_soup(seed, n, w, h, mixed=(False, True, 'colours')[seed % 3], plant=plant)
    else:
        color = product_soup(seed, n, w, h, plant=plant)
    color = [mul(c, plant.c) if k != 1 else add(c, mul(plant.r, nat(3))) for k, c in enumerate(color)]
    # a shape of its own times the colour factor, read through a reciprocal: where the shape is 0 the product is a zero with
    # the factor's sign, and 1 / -0.0 = -inf shows a region that was skipped as +0.0 (a max or a sum with +0.0 would hide it)
    from marayb import chess, inside_triangle
    cx, cy = rng.randrange(w // 3, 2 * w // 3), rng.randrange(h // 3, 2 * h // 3)
    tri = [(nat(cx - 20), nat(cy - 10)), (nat(cx + 25), nat(cy - 5)), (nat(cx), nat(cy + 15))]
    own = min_(inside_triangle(tri, [x(), y()]), subst_xy(chess(2), mul(x(), div(nat(1), nat(9))), mul(y(), div(nat(1), nat(7)))))
    color[2] = add(color[2], min_(recip(mul(own, plant.c)), nat(1)))
    # and a band |x + v - cx| < r - 9 with v anything: empty for every number (r <= 8), the whole plane for v = NaN, as
    # lt() is the inverse of a comparison that NaN fails -- a bound that drops the NaN (max(lo, -hi, +0) of an abs) is wrong there
    from marayb import abs_, lt
    v = var_id(PARAM_ID0 + 5)
    band = min_(lt(abs_(add(x(), sub(v, nat(cx)))), sub(plant.r, nat(9))), subst_xy(chess(2), mul(x(), div(nat(1), nat(5))), mul(y(), div(nat(1), nat(11)))))
    color[0] = max_(color[0], mul(band, nat(200)))
    decl = [(i,) + SOUP_RANGES[name][(seed + k) % len(SOUP_RANGES[name])] for k, (i, name) in enumerate(zip(ids, 'tusrc'))]
    decl.append((PARAM_ID0 + 5, -math.inf, math.inf))
    return color, decl, PR.value_vectors(rng, decl, n_vectors)

"""Seeded scenes for the second bounds of Step(Sin) factors (the REFINE section: maray_amd/csrc/lower.cpp, build_refine; DESIGN 2
item 10, 4.3, 5.3): the generator and the committed cases of tests/test_refine_fuzz.py (numpy alone: the soundness claim and
the conditions that keep it from being empty) and tests/test_gpu_refine_fuzz.py (the device's words against the numpy model,
its rasters against the oracle).  tools/cpu_fuzz_refine.py runs the same generator over fresh seeds.

A scene is guarded shapes -- a triangle AND a pattern, two triangles to a quad (refine_scenes._quad) -- each times a colour
under max; the red channel gives shape n the colour 250 - n and nothing else, which is how a test finds the guard of a shape
(guard_shapes).  Every kind takes a seed and a geometry (w, h, y0, y1) and makes (channels, declarations, value vectors)
and one record per shape: what its pattern is there for.

  near3      Step(Sin(A (x - m) + B y + C)) whose span over a rectangle, |A| 63 + |B| (gh - 1), is drawn from [2.5, 3.4]:
             round the rule's width 3 and round pi.  Both signs of A and B, B = 0 too; m on 64 n, 64 n - 1, 64 n + 63 and
             anywhere; C = 0, anything, or placed so that a rectangle's corners lie just outside a positive half-wave
  edge       periods >= 300 pixels, the sine's sign change between two named neighbouring columns or rows, single or as a
             slit one column (row) wide in a rectangle's corner column (row): 64 n - 1 | 64 n, 64 n - 2 | 64 n - 1,
             w - 2 | w - 1, and in y the launch's groups and its last row
  offset     constant offsets up to the bounded-Sin limit 105414350: under it over the whole 2^20 domain, and just over it
  nonaffine  c (x - m)^2, c x y, c |x - m|, min / max of two affine arguments, sqrt of a value that goes negative
  arith      factors combined above the patterns: NOT, weighted thresholds, a product, nests, a boolean without a pattern
  param      a parameter in the argument: a ROW-read offset, a frequency (a parameter times x), PIXEL-only ones
  many       >= 70 guarded shapes (two guard words), pattern kinds alternating bit by bit
  rows       near3 and edge patterns in y in scenes whose guards read Y (rectangles of one row)

Seeded and deterministic.  No GPU in here."""
import math
import os
import random
import re

import numpy as np

import params as PR
from fuzz_scenes import PARAM_ID0
from marayb import abs_, add, div, encode, half, max_, min_, mul, nat, neg, recip, set_and, set_inv, set_or, set_xor, sin, sqrt, step, sub, tau, translate, var_id, x, y
from refine_scenes import _quad

KINDS = ('near3', 'edge', 'offset', 'nonaffine', 'arith', 'param', 'many', 'rows')
GW = 64
LIMIT = 105414350                       # the bounded-Sin range (lower.cpp)
DOMAIN = 1 << 20                        # MARAY_DOMAIN_MAX
Q = 1 << 40                             # denominator of a real constant: n / 2^40, exact in f64
T_ID, F_ID, U_ID = PARAM_ID0, PARAM_ID0 + 1, PARAM_ID0 + 2

G320 = (320, 72, 0, 72)                 # five rectangles of 64, the second tile ragged; groups of 32, 32 and 8 rows
G449 = (449, 100, 0, 100)               # a ragged row whose last rectangle holds one pixel
G449R = (449, 100, 37, 93)              # ... and a launch whose first row is on no group boundary of the picture
G1100 = (1100, 200, 0, 200)             # 20 rectangles of 64 a row; 5 of 256: the blinds-like `rows` case on it is 1000 work-items of maray_jit_refine


def _num(v):
    return nat(v) if v >= 0 else neg(nat(-v))


def real(v):
    """(expression, the double it evaluates to): v rounded to n / 2^40."""
    n = int(round(v * Q))
    return mul(_num(n), recip(nat(Q))), n / Q


def affine(a, m, b, c):
    """(A (x - m) + B y + C, f(x, y) in Python floats, (A, m, B, C) as the doubles used)."""
    ea, a = real(a)
    eb, b = real(b)
    ec, c = real(c)
    ex = mul(ea, sub(x(), _num(m)))
    if b != 0.0:
        ex = add(ex, mul(eb, y()))
    if c != 0.0:
        ex = add(ex, ec)
    return ex, (a, m, b, c)


def f_of(coef, xs, ys):
    a, m, b, c = coef
    return a * (np.asarray(xs, np.float64) - m) + b * np.asarray(ys, np.float64) + c


def wave(ex):
    return step(sin(ex))


# ---- quads -------------------------------------------------------------------------------------------------------------------
def cells(geo, rng, limit=None):
    """Boxes (x0, y0, x1, y1, skew) of quads on a grid of 104 x 35 cells over the launch's rows, jittered as refine_scenes does."""
    w, h, y0, y1 = geo
    out = []
    for j in range(max(1, (y1 - y0) // 35)):
        for i in range(max(1, w // 104)):
            bx, by = 6 + 104 * i + rng.randrange(8), y0 + 3 + 35 * j + rng.randrange(4)
            out.append((bx, by, bx + 90 + rng.randrange(12), by + 28 + rng.randrange(5), rng.randrange(-5, 6)))
    if limit is not None and len(out) > limit:
        out = [out[k] for k in sorted(rng.sample(range(len(out)), limit))]
    return out


def box_around(rng, geo, cx=None, cy=None):
    """A quad's box that holds column cx and/or row cy well inside."""
    w, h, y0, y1 = geo
    bx = max(6, cx - 20 - rng.randrange(50)) if cx is not None else rng.randrange(6, max(7, w - 100))
    by = max(y0, cy - 8 - rng.randrange(14)) if cy is not None else rng.randrange(y0, max(y0 + 1, y1 - 30))
    return (bx, by, bx + 90 + rng.randrange(12), by + 28 + rng.randrange(5), rng.randrange(-5, 6))


class Made:
    """A scene in the making: shapes (a quad adds two), one record per shape."""

    def __init__(self, kind, seed, geo):
        self.kind, self.seed, self.geo = kind, seed, geo
        self.shapes, self.recs = [], []
        self.decl, self.vectors = [], [None]
        self.extra = None                       # a fourth channel's worth of expression added to blue (a PIXEL-read ramp)
        self.move = None                        # a translation of the whole picture

    def quad(self, box, pat, **rec):
        for tri in _quad(*box):
            self.shapes.append(set_and(tri, pat))
            self.recs.append(dict(rec, box=box))

    def color(self):
        assert 0 < len(self.shapes) <= 100
        r = g = b = None
        for n, s in enumerate(self.shapes):
            col = self.recs[n].get('colour')
            t = mul(s, nat(250 - n)) if col is None else mul(mul(s, col), nat(250 - n))       # (s u) c: u is an operand of a PIXEL op
            r = t if r is None else max_(r, t)
            if n % 2:
                g = mul(s, nat(100)) if g is None else max_(g, mul(s, nat(100)))
            if n % 3 == 0:
                b = mul(s, nat(20 + n % 50)) if b is None else max_(b, mul(s, nat(20 + n % 50)))
        out = [r, g if g is not None else nat(0), b]
        if self.move is not None:
            out = [translate(c, self.move) for c in out]
        if self.extra is not None:
            out[2] = add(out[2], self.extra)
        return out


# ---- the kinds ---------------------------------------------------------------------------------------------------------------
def near3_coef(rng, box, gh, in_y=False, gw=GW, y0=0):
    """Coefficients of a near3 pattern for a quad in `box`; the phase modes are what makes decided rectangles frequent."""
    span = rng.uniform(2.5, 3.4)
    mode = rng.randrange(4)
    share = 1.0 if mode == 0 or gh == 1 else rng.uniform(0.35, 0.9)          # B = 0 in a quarter of them
    a = span * share / (gw - 1) * rng.choice([-1, 1])
    b = 0.0 if share == 1.0 else span * (1.0 - share) / (gh - 1) * rng.choice([-1, 1])
    if in_y:                                                                    # the pattern varies over y alone (rows)
        a, b = 0.0, rng.uniform(0.05, 0.4) * rng.choice([-1, 1])
    n64 = (box[0] + box[2]) // 2 // gw * gw
    m = rng.choice([n64, n64 - 1, n64 + gw - 1, rng.randrange(box[0], box[2])])
    pm = rng.randrange(4)
    if pm == 0:
        c = 0.0
    elif pm == 1:
        c = rng.uniform(-math.pi, math.pi)
    else:
        # the rectangle round the quad's middle starts a little before a zero of the sine, rising or falling: with a span
        # above pi its corners are both negative round a whole positive half-wave; with one below, it is cleared or kept by little
        _, coef = affine(a, m, b, 0.0)
        x0, ya = n64, y0 + (box[1] + 4 - y0) // gh * gh
        corners = [f_of(coef, xx, yy) for xx in (x0, x0 + gw - 1) for yy in (ya, ya + gh - 1)]
        lo = float(min(corners))
        over = abs(a) * (gw - 1) + abs(b) * (gh - 1) - math.pi
        c = -lo - (rng.uniform(0.1, 0.9) * over if over > 0.02 else rng.uniform(0.01, 0.3)) + rng.choice([0.0, 0.0, math.pi])
    return a, m, b, c


def near3(made, rng):
    for box in cells(made.geo, rng, 12):
        gh = rng.choice([8, 32])
        ex, coef = affine(*near3_coef(rng, box, gh, y0=made.geo[2]))
        pat = wave(ex)
        how = rng.randrange(5)
        if how == 1:
            pat = set_inv(pat)
        elif how == 2:
            ex2, _ = affine(*near3_coef(rng, box, gh))
            pat = set_xor(pat, wave(ex2))
        elif how == 3:
            pat = step(sub(sin(ex), real(rng.uniform(-0.9, 0.9))[0]))              # thresholded: not a Step(Sin), no bound of its own
        made.quad(box, pat, tag=('plain', 'inverted', 'xor', 'threshold', 'plain')[how], coef=coef if how in (0, 4) else None)


def long_wave(rng, geo, e=None, rising=True, in_y=False):
    """A long pattern whose sine changes sign between e - 1 and e (x or y): 1 from e on if rising, 1 up to e - 1 if not."""
    w, h, y0, y1 = geo
    per = rng.randrange(300, 700)
    if e is None:
        e = rng.randrange(0, w) if not in_y else rng.randrange(y0, y1)
    t = add(sub(y() if in_y else x(), nat(e)), half())
    return wave(mul(div(tau(), nat(per)), t if rising else neg(t)))


def box_wave(rng, geo, box, in_y=False):
    """A long pattern whose sign change lies inside the quad's box, the 1 side towards the nearer end: both values show in the quad,
    and the rectangles of its far side are 0 on every pixel."""
    if in_y:
        e = rng.randrange(box[1] + 6, box[3] - 6)
        return long_wave(rng, geo, e, e > (box[1] + box[3]) // 2, True)
    e = rng.randrange(box[0] + 15, box[2] - 15)
    return long_wave(rng, geo, e, e > (box[0] + box[2]) // 2)


EDGE_PLACEMENTS = ('x64', 'x63', 'xw', 'ygroup', 'ylast')


def edge(made, rng):
    """One quad per placement and form.  The records carry the column (row) of a slit and where its cleared neighbours are."""
    w, h, y0, y1 = made.geo
    for place in EDGE_PLACEMENTS:
        for form in ('slit', 'rise', 'fall'):
            if place in ('x64', 'x63'):
                n = rng.randrange(1, (w - 40) // GW + 1)
                col = GW * n if place == 'x64' else GW * n - 1             # the slit's column: first of rectangle n / last of n - 1
                e, box, in_y = col, box_around(rng, made.geo, cx=col), False
            elif place == 'xw':
                if w % GW == 0:
                    continue
                col = w - 1                                                # the sign change between w - 2 and w - 1
                e, in_y = col, False
                box = box_around(rng, made.geo)
                box = (w - 60 - rng.randrange(30), box[1], w + 20, box[3], 0)
            elif place == 'ygroup':
                n = rng.randrange(1, (y1 - y0 - 6) // 32 + 1)
                row = y0 + 32 * n - rng.randrange(2)                       # first row of a group of 8 and of 32, or the last of one
                e, box, in_y = row, box_around(rng, made.geo, cy=row), True
            else:
                row = y1 - 1
                e, in_y = row, True
                box = box_around(rng, made.geo)
                box = (box[0], y1 - 20 - rng.randrange(10), box[2], y1 + 9, box[4])
            if form == 'slit':
                pat = set_and(long_wave(rng, made.geo, e, True, in_y), long_wave(rng, made.geo, e + 1, False, in_y))
            else:
                pat = long_wave(rng, made.geo, e, form == 'rise', in_y)
            made.quad(box, pat, tag=place, form=form, at=e, in_y=in_y)


def offset(made, rng):
    for k, box in enumerate(cells(made.geo, rng, 12)):
        per = rng.randrange(300, 600)
        a = math.tau / per
        reach = int(a * DOMAIN) + 2
        which = ('under', 'over', 'log', 'under_neg', 'over_domain', 'log')[k % 6]
        if which == 'under':
            off = LIMIT - reach - rng.randrange(1, 2000)                   # |a| < limit over the whole domain
        elif which == 'under_neg':
            off = -(LIMIT - rng.randrange(1, 2000))                        # a in [-limit + ..., -limit + ... + reach]
        elif which == 'over':
            off = LIMIT + rng.randrange(0, 3000)                           # over it everywhere
        elif which == 'over_domain':
            off = LIMIT - rng.randrange(1, reach - 1)                      # under it in the picture, over it at the domain's end
        else:
            off = int(10.0 ** rng.uniform(3, 8))
            which = 'log_under' if off + reach < LIMIT else 'log_over'
        pat = wave(add(mul(div(tau(), nat(per)), x()), _num(off)))
        made.quad(box, pat, tag=which, bounded=which in ('under', 'under_neg', 'log_under'))


NONAFFINE = ('square', 'square_corner', 'xy', 'abs', 'min', 'max', 'sqrt')


def nonaffine(made, rng):
    w, h, y0, y1 = made.geo
    for k, box in enumerate(cells(made.geo, rng, 14)):
        which = NONAFFINE[(k + made.seed) % len(NONAFFINE)]
        mid = (box[0] + box[2]) // 2
        if which in ('square', 'square_corner'):
            # c = 1 / 16384 keeps the argument inside the bounded-Sin range over the whole domain (2^40 / 16384 < 105414350).
            # c (x - m)^2 is 3 pi / 2, the middle of a negative half-wave, 278 pixels from m, and grows by about 2 over a
            # rectangle there: m that far from the quad's middle where the picture has the room, else at its far end
            c = div(nat(1), nat(16384))
            d = 278 + rng.randrange(-25, 25)
            room = [v for v in (mid - d, mid + d) if 0 <= v < w]
            m = rng.choice(room) if room else (0 if mid > w // 2 else w - 1)
            if which == 'square_corner':
                m = (m + GW // 2) // GW * GW
            dx = sub(x(), nat(m))
            arg = mul(c, mul(dx, dx))
        elif which == 'xy':
            arg = add(mul(div(nat(1), nat(16384)), mul(x(), y())), real(rng.uniform(2.0, 5.5))[0])       # (2^40 / 16384: inside the range)
        elif which == 'abs':
            arg = mul(div(tau(), nat(rng.randrange(140, 220))), abs_(sub(x(), nat(max(0, mid + rng.choice([-1, 1]) * rng.randrange(50, 100))))))
        elif which in ('min', 'max'):
            f1, _ = affine(math.tau / rng.randrange(300, 600) * rng.choice([-1, 1]), rng.randrange(w), 0.0, rng.uniform(-3, 3))
            f2, _ = affine(math.tau / rng.randrange(300, 600) * rng.choice([-1, 1]), rng.randrange(w), rng.uniform(-0.02, 0.02), rng.uniform(-3, 3))
            arg = (min_ if which == 'min' else max_)(f1, f2)
        else:
            arg = mul(div(nat(1), nat(4)), sqrt(sub(x(), nat(mid))))          # NaN left of mid: not NaN-free, no bound
        made.quad(box, wave(arg), tag=which)


ARITH = ('not', 'sum', 'weighted', 'negstep', 'product', 'nest', 'plain_bool')


def arith(made, rng):
    w, h, y0, y1 = made.geo
    for k, box in enumerate(cells(made.geo, rng, 14)):
        which = ARITH[(k + made.seed) % len(ARITH)]
        # two long patterns that change sign inside the quad
        p1 = box_wave(rng, made.geo, box)
        p2 = box_wave(rng, made.geo, box, in_y=rng.random() < 0.5)
        p3 = long_wave(rng, made.geo, rng.randrange(0, w), rng.random() < 0.5)
        if which == 'not':
            pat = set_inv(p1)
        elif which == 'sum':
            pat = step(sub(add(p1, p2), div(nat(3), nat(2))))
        elif which == 'weighted':
            pat = step(sub(sub(mul(nat(2), p1), p2), half()))
        elif which == 'negstep':
            pat = step(add(neg(p1), half()))
        elif which == 'product':
            pat = mul(p1, p2)
        elif which == 'nest':
            pat = rng.choice([set_and(set_or(p1, p2), set_xor(p2, p3)), set_xor(set_and(p1, set_or(p2, p3)), p3), set_or(set_and(p1, p2), set_and(set_inv(p1), p3))])
        else:
            pat = set_and(p1, step(sub(x(), nat((box[0] + box[2]) // 2))))
        made.quad(box, pat, tag=which)


PARAM_FORMS = ('offset', 'frequency', 'colour', 'phase')


def param(made, rng):
    """seed % 4 picks the parameter's place.  offset: the picture translated by t, which the guards and the bounds read in the
    ROW stage; frequency: Step(Sin(f x)), a parameter times x (not affine for the lowering: MUL wants a literal); colour: a
    colour scale u that only PIXEL ops read; phase: u inside the sine's argument with x alone."""
    w, h, y0, y1 = made.geo
    form = PARAM_FORMS[made.seed % 4]
    made.form = form
    boxes = cells(made.geo, rng, 8)
    if form == 'offset':
        made.decl = [(T_ID, -64.0, 64.0)]
        e0 = GW * rng.randrange(1, w // GW) + rng.randrange(3, 20)          # the first pattern's sign change, before the translation
        for k, box in enumerate(boxes):
            pat = long_wave(rng, made.geo, e0, rng.random() < 0.5) if k == 0 else box_wave(rng, made.geo, box)
            made.quad(box, pat, tag='offset')
        made.move = [var_id(T_ID), nat(0)]
        corner = float(-(e0 % GW))                                         # moves that sign change onto a multiple of 64
        made.vectors = [(-64.0,), (64.0,), (corner,), (rng.uniform(-64, 64),), (float(rng.randrange(-60, 60)) + 0.5,)]
    elif form == 'frequency':
        lo, hi = math.tau / 640, math.tau / 320
        made.decl = [(F_ID, lo, hi)]
        for box in boxes:
            made.quad(box, wave(mul(var_id(F_ID), sub(x(), nat(rng.choice([0, 64, 100]))))), tag='frequency')
        made.vectors = [(lo,), (hi,), (math.pi / 256,), (rng.uniform(lo, hi),)]     # pi / 256: sin(f (x - 0)) changes sign at x = 256
    elif form == 'colour':
        made.decl = [(U_ID, 0.25, 2.0)]
        for k, box in enumerate(boxes):
            made.quad(box, box_wave(rng, made.geo, box), tag='colour' if k % 2 == 0 else 'plain',
                      colour=var_id(U_ID) if k % 2 == 0 else None)
        made.vectors = [(0.25,), (2.0,), (1.0,), (rng.uniform(0.25, 2.0),)]
    else:
        made.decl = [(U_ID, -3.0, 3.0)]
        for k, box in enumerate(boxes):
            if k % 2 == 0:
                pat = wave(add(mul(div(tau(), nat(rng.randrange(300, 600))), x()), var_id(U_ID)))
            else:
                pat = box_wave(rng, made.geo, box)
            made.quad(box, pat, tag='phase' if k % 2 == 0 else 'plain')
        made.vectors = [(-3.0,), (3.0,), (0.0,), (rng.uniform(-3, 3),)]


def many(made, rng):
    """40 quads, 80 guarded shapes: with the groups' own guards more than 64 bits.  The kinds alternate quad by quad, and a quad's
    two shapes are neighbouring bits: a byte holds bits with a second bound and bits without."""
    w, h, y0, y1 = made.geo
    for k, box in enumerate(cells(made.geo, rng, 40)):
        which = ('long', 'over', 'short', 'long_xy', 'sqrt')[k % 5]
        if which == 'long':
            pat = box_wave(rng, made.geo, box)
        elif which == 'long_xy':
            pat = wave(mul(div(tau(), nat(rng.randrange(300, 600))), sub(add(x(), y()), nat(rng.randrange(w)))))
        elif which == 'short':
            pat = wave(mul(div(tau(), nat(rng.choice([6, 11, 24]))), x()))
        elif which == 'over':
            pat = wave(add(mul(div(tau(), nat(rng.randrange(300, 600))), x()), nat(LIMIT + rng.randrange(0, 3000))))
        else:
            pat = wave(mul(div(nat(1), nat(4)), sqrt(sub(x(), nat((box[0] + box[2]) // 2)))))
        made.quad(box, pat, tag=which, bounded=which in ('long', 'long_xy', 'short'))


def rows(made, rng):
    """Guards that read Y: rectangles of 256 pixels x 1 row.  A pattern in y alone is a ROW value there, part of the guard itself;
    what is left to a second bound is a pattern in x, so every shape has one: a near3 pattern whose span is taken over 255
    pixels, or a long one.  seed % 2 == 0: quads whose patterns are such a pattern in x AND a near3 or edge pattern in y, lowered
    with y_spans=False; else a blinds-like scene under the default lowering: row bands Step(Sin) that have no monotone bound
    over y (lowering_forms.blinds), each AND an XOR of two patterns in x."""
    w, h, y0, y1 = made.geo

    def in_x(box):
        if rng.random() < 0.5:
            ex, coef = affine(*near3_coef(rng, box, 1, gw=256))
            return wave(ex), coef
        t = add(sub(x(), nat(rng.randrange(0, w))), half())
        return wave(mul(div(tau(), nat(rng.randrange(560, 900))), t if rng.random() < 0.5 else neg(t))), None

    if made.seed % 2 == 0:
        made.lower = dict(y_spans=False)
        for k, box in enumerate(cells(made.geo, rng, 10)):
            px, coef = in_x(box)
            if k % 3 == 0:
                ex, _ = affine(*near3_coef(rng, box, 1, in_y=True))
                made.quad(box, set_and(px, wave(ex)), tag='near3_y', coef=coef)
            elif k % 3 == 1:
                row = rng.randrange(box[1] + 3, box[3] - 3)
                form = rng.choice(['slit', 'rise', 'fall'])
                py = set_and(long_wave(rng, made.geo, row, True, True), long_wave(rng, made.geo, row + 1, False, True)) if form == 'slit' else \
                    long_wave(rng, made.geo, row, form == 'rise', True)
                made.quad(box, set_and(px, py), tag='edge_y', form=form, at=row, in_y=True, coef=coef)
            else:
                made.quad(box, px, tag='x_only', coef=coef)
    else:
        made.blinds = True
        for i in range(6):
            band = wave(mul(add(y(), nat(7 * i + rng.randrange(5))), div(nat(1), nat(3 + 2 * i))))
            pat = set_xor(in_x((0, 0, w, h, 0))[0], in_x((0, 0, w, h, 0))[0])
            made.shapes.append(min_(band, pat))
            made.recs.append(dict(tag='blinds', box=None))


_KIND = dict(near3=near3, edge=edge, offset=offset, nonaffine=nonaffine, arith=arith, param=param, many=many, rows=rows)


def make(kind, seed, geo):
    made = Made(kind, seed, geo)
    made.lower, made.blinds, made.form = {}, False, None
    _KIND[kind](made, random.Random(0x5EF1 + 7919 * KINDS.index(kind) + seed))
    return made


def scene(kind, seed, geo):
    """(channels, [(id, lo, hi), ...], value vectors) -- [None] for a scene without parameters."""
    made = make(kind, seed, geo)
    return made.color(), made.decl, made.vectors


# ---- the cases: (kind, seed, geometry, k) ------------------------------------------------------------------------------------
# k: 1, or the factor of a supersampled lowering (Scene.supersample: the sections cover the k w x k h sample grid).  A seed
# that fails a condition of tests/test_refine_fuzz.py is replaced here, never skipped there.
CASES = [('near3', 0, G320, 1), ('near3', 27, G449, 1), ('near3', 9, G449R, 1), ('near3', 3, G320, 2), ('near3', 4, G320, 4), ('near3', 5, G1100, 1),
         ('near3', 30, G449R, 1), ('near3', 7, G320, 1),
         ('edge', 0, G320, 1), ('edge', 1, G449, 1), ('edge', 2, G449R, 1), ('edge', 3, G320, 2), ('edge', 4, G449, 1), ('edge', 5, G320, 4),
         ('offset', 0, G320, 1), ('offset', 1, G449, 1), ('offset', 2, G449R, 1), ('offset', 3, G320, 1),
         ('nonaffine', 0, G320, 1), ('nonaffine', 1, G449, 1), ('nonaffine', 2, G449R, 1), ('nonaffine', 3, G449, 1),
         ('arith', 0, G320, 1), ('arith', 1, G449, 1), ('arith', 2, G449R, 1), ('arith', 3, G320, 2), ('arith', 4, G449, 1), ('arith', 5, G320, 4),
         ('param', 0, G320, 1), ('param', 1, G449, 1), ('param', 2, G449R, 1), ('param', 3, G320, 1), ('param', 4, G449R, 1), ('param', 5, G320, 1),
         ('many', 0, G1100, 1), ('many', 1, G1100, 1),
         ('rows', 0, G320, 1), ('rows', 1, G320, 1), ('rows', 2, G449R, 1), ('rows', 3, G449, 1), ('rows', 7, G1100, 1)]


def lowered(case):
    """(tape, made) of a case: the scene encoded at its picture's size, its parameters declared, supersampled if the case says so."""
    kind, seed, geo, k = case
    made = make(kind, seed, geo)
    s = PR.declared_ids(encode(geo[:2], made.color()), made.decl)
    if k > 1:
        s.supersample(k)
    made.encoded = s.encode()
    return s.lower(**made.lower), made


def sample_geo(case):
    """(w, y0, rows) of the grid the sections of a case cover: the picture's, k times for a supersampled one."""
    _, _, (w, h, y0, y1), k = case
    return k * w, k * y0, k * (y1 - y0)


# ---- what belongs to which shape ---------------------------------------------------------------------------------------------
def guard_shapes(tape, w, y0, rows_, params=None):
    """{guard: shape} for the guards whose regions are != 0 somewhere and take one value there that is a red colour 250 - n:
    the guard of shape n alone (a group's guard sees several colours; a shape that is 0 everywhere has no entry)."""
    import refine_eval as RE
    consts, _, pix = tape.arrays()
    n_ynum = RE.n_numeric(tape)
    yv = RE.numeric_yvals_of_rows(tape, w, y0, rows_, params)
    ry, rx = np.divmod(np.arange(rows_ * w), w)
    # a guard's regions on the pixels of the rectangles whose geometric bit is set, as the kernels read it
    _, _, gw, gh = tape.guard_layout()
    only = as_read(tape, RE.guard_bits(tape, w, y0, rows_, gw, gh, params=params)[0])
    rect_of = (ry // gh) * ((w + 255) // 256 * (256 // gw)) + rx // gw
    out = {}
    for k, ends in RE.guarded_regions(tape).items():
        seen = set()
        sel = np.nonzero(only[rect_of, k - n_ynum])[0]
        for end in ends if len(sel) else []:
            v = RE.run(RE.cone(pix, end), consts, tape.info['n_pix_slots'], len(sel), {0: rx[sel].astype(np.float64), 1: (y0 + ry[sel]).astype(np.float64)},
                       yvals=yv[ry[sel]], params=params, want=end)
            seen |= set(np.unique(v[v != 0.0]).tolist())
        reds = [v for v in seen if 150.0 <= v <= 250.0 and v == int(v)]
        if len(reds) == 1 and not [v for v in seen if v > 250.0]:
            out[k - n_ynum] = 250 - int(reds[0])
    return out


def row_block():
    """ROW_BLOCK of jit_parts.hpp: the work-items of a block of maray_jit_refine."""
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'maray_amd', 'csrc', 'jit_parts.hpp')).read()
    m = re.findall(r'static const unsigned ROW_BLOCK = (\d+);', text)
    assert len(m) == 1
    return int(m[0])


# ---- the model's view of a case ----------------------------------------------------------------------------------------------
def as_read(tape, bits):
    """The bits as the kernels read them: a guard without a bit of its own is the OR of its members'."""
    import refine_eval as RE
    members = RE.derived_members(tape)
    assert sorted(members) == np.nonzero(tape.guard_layout()[0] < 0)[0].tolist()
    return RE.effective(bits, members)


def examine(tape, case, gh, values=None, gw=GW, full=True):
    """The rectangles of a case at guard height gh under one value vector: a dict of geo, second, has (refine_eval.guard_bits),
    refined = geo & second, exact (every pixel: refine_eval.nonzero_per_rectangle; full=False: every pixel of the rectangles whose
    geometric bit is set, as the kernels read it), bad = exact & ~as_read(refined) -- the
    soundness claim is that it is empty -- and the rectangles' xlo, xhi, y of the first and last row."""
    import refine_eval as RE
    w, y0, rows_ = sample_geo(case)
    geo, second, has = RE.guard_bits(tape, w, y0, rows_, gw, gh, params=values)
    refined = geo & second
    exact = RE.nonzero_per_rectangle(tape, w, y0, rows_, gw, gh, params=values, only=None if full else as_read(tape, geo))
    _, xlo, xhi, r0, r1 = RE.rectangles(w, rows_, gw, gh)
    return dict(geo=geo, second=second, has=has, refined=refined, exact=exact, bad=exact & ~as_read(tape, refined),
                xlo=xlo, xhi=xhi, ylo=y0 + r0, yhi=y0 + r1, n_rect=(w + 255) // 256 * (256 // gw))


def near3_counts(e, tape, made, shape_of):
    """(cleared rectangles whose span is in [2.5, 3), humps, humps whose span is under 3.3) of one examined near3 scene.  The span
    of a rectangle is |A| (xhi - xlo) + |B| (yhi - ylo); a hump has a span in (pi, 3.4], a negative sine of the generator's own f
    at both corners the bound is taken at (picked by the signs of A and B), a conjunction != 0 on some pixel, and its bit kept."""
    leaf = tape.guard_layout()[0] >= 0
    near = hump = hump33 = 0
    for g, n in shape_of.items():
        coef = made.recs[n].get('coef')
        if coef is None or not leaf[g]:
            continue
        a, m, b, c = coef
        sp = abs(a) * (e['xhi'] - e['xlo']) + abs(b) * (e['yhi'] - e['ylo'])
        xl, xh = (e['xlo'], e['xhi']) if a >= 0 else (e['xhi'], e['xlo'])
        yl, yh = (e['ylo'], e['yhi']) if b >= 0 else (e['yhi'], e['ylo'])
        neg_ = (np.sin(f_of(coef, xl, yl)) < 0) & (np.sin(f_of(coef, xh, yh)) < 0)
        h = (sp > math.pi) & (sp <= 3.4) & neg_ & e['exact'][:, g] & e['refined'][:, g]
        near += int((e['geo'][:, g] & ~e['refined'][:, g] & (sp >= 2.5) & (sp < 3.0)).sum())
        hump += int(h.sum())
        hump33 += int((h & (sp < 3.3)).sum())
    return near, hump, hump33


def refine_items(tape, case):
    """The work-items of the maray_jit_refine launch of a case on the device: one per rectangle of the tape's own layout."""
    import refine_eval as RE
    _, _, gw, gh = tape.guard_layout()
    w, y0, rows_ = sample_geo(case)
    return RE.rectangles(w, rows_, gw, gh)[1].size

"""Sine-patterned quads for tests/test_refine_bounds.py and tests/test_gpu_refine.py: a seeded family at 320 x 72.

320 pixels are five guard rectangles of 64, so the row's second 256-pixel tile is ragged; 72 rows are two full groups of 32
rows and one of 8 (nine groups of 8).  A shape is a triangle AND a pattern, a quad two of them; the pattern is Step(Sin(a))
or, like the chess board's, the XOR of two.  What a kind is there for:

  long      periods of 257 or 400 pixels, longer than a rectangle: some quad lies in the half where the sine is negative
  short     periods of 6 .. 24 pixels: every rectangle spans whole periods, the second bound has to stay "unknown"
  zero      the argument runs from negative to positive through 0 inside the picture, falling and rising
  huge      the argument sits just below the bounded-Sin limit (105414350) over the whole pixel domain
  yonly     a pattern in y alone: a ROW-section value, bounded over the rows of the rectangle
  slanted   coefficients of both signs in x and y: each end of the interval is another corner of the rectangle
  square    an argument that is not affine (x^2 / 16384): bounded by interval arithmetic, not by end points
  mixed     a seeded draw of all of them, some as XOR pairs
"""
import random

from marayb import add, div, encode, inside_triangle, max_, mul, nat, neg, set_and, set_xor, sin, step, sub, tau, translate, var, x, y

W, H = 320, 72
KINDS = ('long', 'short', 'zero', 'huge', 'yonly', 'slanted', 'square', 'mixed')


def _quad(x0, y0, x1, y1, skew):
    """Two triangles that tile the (skewed) box x0..x1 x y0..y1."""
    p = [x(), y()]
    a, b, c, d = (nat(x0 + skew), nat(y0)), (nat(x1 + skew), nat(y0)), (nat(x0), nat(y1)), (nat(x1), nat(y1))
    return [inside_triangle([a, b, c], p), inside_triangle([b, c, d], p)]


def _wave(per, of):
    return step(sin(mul(div(tau(), nat(per)), of)))


def pattern(kind, rng):
    if kind == 'long':
        return _wave(rng.choice([257, 400]), rng.choice([x(), add(x(), y())]))
    if kind == 'short':
        return _wave(rng.choice([6, 11, 24]), rng.choice([x(), add(x(), y())]))
    if kind == 'zero':
        m = nat(rng.choice([100, 160, 231]))
        return _wave(rng.choice([300, 500]), rng.choice([sub(x(), m), sub(m, x())]))
    if kind == 'huge':
        # (tau / 300) 2^20 + 105384350 < 105414350: proven bounded over the whole domain
        return step(sin(add(mul(div(tau(), nat(300)), x()), nat(105384350))))
    if kind == 'yonly':
        return _wave(rng.choice([70, 110, 200]), y())
    if kind == 'slanted':
        return _wave(rng.choice([400, 700]), add(mul(nat(3), x()), neg(mul(nat(rng.choice([2, 5])), y()))))
    if kind == 'square':
        return step(sin(mul(mul(x(), x()), div(nat(1), nat(16384)))))
    raise ValueError(kind)


def scene(kind, seed):
    """Three channels of a 320 x 72 picture of six quads (twelve guarded shapes) whose patterns are of `kind`."""
    rng = random.Random(1000 * KINDS.index(kind) + seed)
    shapes = []
    for j in range(2):
        for i in range(3):
            x0, y0 = 6 + 104 * i + rng.randrange(8), 3 + 35 * j + rng.randrange(4)
            k = kind if kind != 'mixed' else rng.choice(KINDS[:-1])
            pat = pattern(k, rng)
            if kind == 'mixed' and rng.random() < 0.5:
                pat = set_xor(pat, pattern(rng.choice(('long', 'yonly', 'zero')), rng))
            for tri in _quad(x0, y0, x0 + 90 + rng.randrange(12), y0 + 28 + rng.randrange(5), rng.randrange(-5, 6)):
                shapes.append(set_and(tri, pat))
    # a channel is the max over shapes times a colour: every shape is a guarded conjunction of its own (one conjunction
    # around a whole channel would get one guard for all of them)
    r = g = b = None
    for n, s in enumerate(shapes):
        r = mul(s, nat(255 - n)) if r is None else max_(r, mul(s, nat(255 - n)))
        if n % 2:
            g = mul(s, nat(200)) if g is None else max_(g, mul(s, nat(200)))
        if n % 3 == 0:
            b = mul(s, nat(90 + n)) if b is None else max_(b, mul(s, nat(90 + n)))
    return [r, g, b]


def data(kind, seed):
    return encode((W, H), scene(kind, seed))


def moving():
    """(color, [(name, lo, hi), ...]): the 'long' quads of seed 0 moved in x by parameter t -- the guards and their second
    bounds read it, in the ROW stage -- and a ramp scaled by parameter u, which only PIXEL ops read."""
    r, g, _ = scene('long', 0)
    off = [var('t'), nat(0)]
    return [translate(r, off), translate(g, off), mul(x(), var('u'))], [('t', -64.0, 64.0), ('u', 0.0, 1.0)]


def shared_bound():
    """Three shapes behind ONE geometric bound (a band of rows), each with a pattern of its own, in one max group; the first
    is too small to get a SKIP of its own, so only the group's SKIP -- which reads the shared guard's bit -- ever skips it.
    A second bound made from the shapes that do have a SKIP alone would clear the bit where the first is 1."""
    b = set_and(step(sub(y(), nat(10))), step(sub(nat(50), y())))
    s1 = set_and(b, _wave(300, x()))
    s2 = set_and(b, set_xor(_wave(257, x()), _wave(400, add(x(), y()))))
    s3 = set_and(b, _wave(500, sub(x(), nat(100))))
    return [max_(max_(mul(s1, nat(255)), mul(s2, nat(200))), mul(s3, nat(120))), mul(s2, nat(100)), nat(0)]

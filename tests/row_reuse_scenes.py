"""Scenes of tests/test_row_reuse.py and tests/test_gpu_row_reuse.py: small pictures (256 x 96: three guard groups of 32 rows)
whose parameters reach the ROW section, or do not.

What puts a parameter into the ROW section: the lowering hoists every op that does not depend on X, so a parameter that enters
a y value, a guard's bound (x bounds too: a guard is evaluated per rectangle, in the ROW stage) or any op whose other operands
are constants (t * 255 is uniform, hence a ROW op) is ROW-read.  A parameter multiplied into a pixel-dependent value is not."""
import maray_amd as M
from marayb import encode, max_, mul, nat, sin, step, add, div, translate, var, x, y
from params import _tri

W, H = 256, 96


def shapes(w=W, h=H):
    p = [x(), y()]
    s1 = _tri(w // 8, h // 8, w // 2, h // 6, w // 5, h - h // 8, p)
    s2 = _tri(w // 2, h // 3, w - w // 8, h // 8, w - w // 6, h - h // 6, p)
    return s1, s2


def plain():
    """No parameters."""
    s1, s2 = shapes()
    return [mul(s1, nat(255)), mul(s2, nat(255)), mul(max_(s1, s2), nat(77))], []


def colour():
    """max_i(shape_i . c_i): both parameters scale a shape's colour, in PIXEL ops only."""
    s1, s2 = shapes()
    t, u = var('t'), var('u')
    return [max_(mul(mul(s1, t), nat(255)), mul(mul(s2, u), nat(90))), mul(mul(s1, u), nat(200)), mul(max_(s1, s2), nat(77))], \
        [('t', 0.0, 1.0), ('u', 0.0, 1.0)]


def move_y():
    s1, s2 = shapes()
    return [mul(translate(max_(s1, s2), [nat(0), var('t')]), nat(255)), mul(s1, nat(99)), y()], [('t', -64.0, 64.0)]


def move_x():
    s1, s2 = shapes()
    return [mul(translate(max_(s1, s2), [var('t'), nat(0)]), nat(255)), mul(s1, nat(99)), y()], [('t', -64.0, 64.0)]


def move_and_colour():
    """Parameter 0 moves the shapes in x (ROW-read: the guards' bounds), parameter 1 scales the colour (PIXEL only)."""
    s1, s2 = shapes()
    return [mul(mul(translate(max_(s1, s2), [var('t'), nat(0)]), var('u')), nat(255)), mul(s1, nat(99)), y()], \
        [('t', -64.0, 64.0), ('u', 0.0, 1.0)]


def unread():
    """Two declared parameters, the first of which nothing reads; the second scales a colour."""
    s1, s2 = shapes()
    return [mul(mul(max_(s1, s2), var('u')), nat(255)), mul(s1, nat(99)), y()], [('t', -64.0, 64.0), ('u', 0.0, 1.0)]


def unread_only():
    """One declared parameter that nothing reads: the version-2 program."""
    s1, s2 = shapes()
    return [mul(max_(s1, s2), nat(255)), mul(s1, nat(99)), y()], [('t', -64.0, 64.0)]


def sines():
    """Sines whose argument is not proven bounded (the range is everything): tiles may be deferred to the interpreter behind the
    specialised context.  The phase is a pixel-level operand of the first channel and a ROW-level one of the second."""
    t = var('t')
    r = mul(step(sin(add(mul(mul(x(), y()), div(nat(1), nat(256))), t))), nat(255))
    g = add(mul(sin(add(mul(y(), div(nat(1), nat(8))), t)), nat(127)), nat(128))
    return [r, g, mul(x(), div(nat(1), nat(2)))], [('t', -float('inf'), float('inf'))]


def lowered(spec, size=(W, H), samples=0):
    """(scene, tape) with the parameters declared in order."""
    color, decl = spec
    s = M.Scene(encode(size, color))
    for k, (n, lo, hi) in enumerate(decl):
        assert s.declare_param(n, lo, hi) == k
    if samples:
        s.supersample(samples)
    return s, s.lower()

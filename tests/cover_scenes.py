"""Scenes and the numpy side of tests/test_cover_policy.py and tests/test_gpu_cover.py (the cover of guarded ORs):
what a set's third table of guard words must hold once maray_jit_cover has been through it.

Per rectangle and per boolean OR of guarded shapes that has a cover bit (Tape.cover_plan): the OR is covered when the rectangle
has pixels inside the picture and inside the rendered rows, and on every one of them some untainted guarded leaf of the OR
whose bit the census left set is != 0.  The third table is the census'd words (census_scenes.words) with, in a covered
rectangle, the OR's cover bit set and those of its leaves' bits cleared that the census may decide.  No GPU in here."""
import numpy as np

import census_scenes as CS
import refine_eval as RE
import refine_scenes as RS
from marayb import add, eq, recip, sin, inside_triangle, max_, mul, nat, neg, set_and, set_inv, step, sub, translate, var, x, y

W, H = RS.W, RS.H


def _pixels(w, rows, gw, gh):
    (n_groups, n_rect), _, _, _, _ = RE.rectangles(w, rows, gw, gh)
    ry, rx = np.divmod(np.arange(rows * w), w)
    return n_groups * n_rect, ry, rx, (ry // gh) * n_rect + rx // gw


def leaf_masks(tape, w, y0, rows, params=None, cbits=None):
    """[per OR of tape.cover_plan(): (rows * w,) booleans, the OR of its untainted guarded leaves whose bit is set in the census'd
    words of the pixel's rectangle]"""
    consts, _, pix = tape.arrays()
    _, _, gw, gh = tape.guard_layout()
    cb = CS.words(tape, w, y0, rows, params=params) if cbits is None else cbits
    _, ry, rx, rect_of = _pixels(w, rows, gw, gh)
    yv_rows = RE.numeric_yvals_of_rows(tape, w, y0, rows, params)
    out = []
    for red in tape.cover_plan():
        acc = np.zeros(rows * w, bool)
        for end, bit, tainted, _ in red['leaves']:
            if tainted:
                continue
            has = ((cb[:, bit // 64] >> np.uint64(bit % 64)) & np.uint64(1)).astype(bool)
            sel = np.nonzero(has[rect_of] & ~acc)[0]
            if not len(sel):
                continue
            v = RE.run(RE.cone(pix, end), consts, tape.info['n_pix_slots'], len(sel), {0: rx[sel].astype(np.float64), 1: (y0 + ry[sel]).astype(np.float64)},
                       yvals=yv_rows[ry[sel]], params=params, want=end)
            acc[sel[v != 0.0]] = True
        out.append(acc)
    return out


def covered(tape, w, y0, rows, params=None, cbits=None):
    """(rectangles, ORs with a cover bit) booleans."""
    _, _, gw, gh = tape.guard_layout()
    n, _, _, rect_of = _pixels(w, rows, gw, gh)
    inside = np.bincount(rect_of, minlength=n)
    masks = leaf_masks(tape, w, y0, rows, params, cbits)
    out = np.zeros((n, len(masks)), bool)
    for j, acc in enumerate(masks):
        out[:, j] = (inside > 0) & (np.bincount(rect_of[acc], minlength=n) == inside)
    return out


def words(tape, w, y0, rows, params=None):
    """(the third table, the census'd words, covered): (rectangles, words per rectangle) uint64 twice and covered()."""
    cb = CS.words(tape, w, y0, rows, params=params)
    cov = covered(tape, w, y0, rows, params, cbits=cb)
    vb = cb.copy()
    for j, red in enumerate(tape.cover_plan()):
        for _, bit, _, eligible in red['leaves']:
            if eligible:
                vb[cov[:, j], bit // 64] &= ~(np.uint64(1) << np.uint64(bit % 64))
        vb[cov[:, j], red['bit'] // 64] |= np.uint64(1) << np.uint64(red['bit'] % 64)
    return vb, cb, cov


def counts(tape, w, y0, rows, params=None):
    """What the issue's estimate is replaced by: rectangles with a leaf bit of an OR, those of them that are covered, the
    leaf bits the census leaves in the words and those of them that covered rectangles hold."""
    vb, cb, cov = words(tape, w, y0, rows, params)
    out = []
    for j, red in enumerate(tape.cover_plan()):
        leaf = np.zeros(cb.shape[1], np.uint64)
        for _, bit, _, _ in red['leaves']:
            leaf[bit // 64] |= np.uint64(1) << np.uint64(bit % 64)
        pc = lambda a: int(sum(bin(int(v)).count('1') for v in a.reshape(-1)))
        busy = ((cb & leaf[None, :]) != 0).any(axis=1)
        out.append({'rectangles': int(cb.shape[0]), 'with_leaf_bit': int(busy.sum()), 'covered': int(cov[:, j].sum()),
                    'leaf_bits': pc(cb & leaf[None, :]), 'leaf_bits_in_covered': pc(cb[cov[:, j]] & leaf[None, :]),
                    'leaf_bits_left': pc(vb & leaf[None, :])})
    return out


# ---- scenes, 320 x 72 like census_scenes': rectangles of 64 x 32, the second tile ragged, groups of 32, 32 and 8 rows ----------
def _num(v):
    return nat(v) if v >= 0 else neg(nat(-v))


def _tri(pts):
    return inside_triangle([(_num(a), _num(b)) for a, b in pts], [x(), y()])


def _or(shapes):
    u = None
    for s in shapes:
        u = s if u is None else max_(u, s)
    return u


def _paint(u, k=100):
    """(u + 1) times a colour: u times a colour would be ONE guarded conjunction, not an OR of shapes (census_scenes.covered)."""
    return mul(add(u, nat(1)), nat(k))


def _scene(shapes):
    u = _or(list(shapes) + CS._filler())
    return [_paint(u), _paint(u, 50), nat(0)]


WHOLE = [(-8, -8), (2000, -8), (-8, 2000)]           # a triangle over the whole picture


def one_shape():
    """A solid triangle that holds the whole rectangle x 64..127, rows 0..31 (and parts of its neighbours)."""
    return _scene([_tri([(60, -4), (260, -4), (60, 196)])])


def two_together():
    """Two solid triangles that hold that rectangle only together: one below x + y = 126, one above x + y = 120."""
    return _scene([_tri([(60, -4), (130, -4), (60, 66)]), _tri([(130, 40), (80, 40), (130, -10)])])


HOLES = ((64, 0), (191, 31), (70, 45))               # lane 0 of a first row, lane 63 of a last row, a middle row


def holes():
    """A triangle over the whole picture but for three pixels, in three rectangles."""
    s = _tri(WHOLE)
    for px, py in HOLES:
        s = set_and(s, set_inv(set_and(eq(x(), nat(px)), eq(y(), nat(py)))))
    return _scene([s])


def whole():
    """A triangle over the whole picture: every rectangle with a pixel is covered -- the ragged one, the 8-row group."""
    return _scene([_tri(WHOLE)])


def row_out():
    """... but for row 10: a y factor of the leaf fails there, and the rectangles of the first group are not covered."""
    return _scene([set_and(_tri(WHOLE), set_inv(eq(y(), nat(10))))])


def pixel_param():
    """(color, params): the whole-picture triangle AND Step(c - x / 1000) -- at c = 1 all of the picture, at c = 1/4 its first 250 columns --, c a parameter only PIXEL ops read: tainted, never counted.
    t moves the picture in x: the ROW section reads it."""
    color = _scene([set_and(_tri(WHOLE), step(sub(var('c'), mul(x(), recip(nat(1000))))))])
    return [translate(c, [var('t'), nat(0)]) for c in color], [('t', -64.0, 64.0), ('c', 0.0, 1.0)]


def row_param():
    """(color, params): one_shape() moved in x by t, which the ROW section reads."""
    return [translate(c, [var('t'), nat(0)]) for c in one_shape()], [('t', -64.0, 64.0)]


def with_colours():
    """An f64 max reduction (red: shapes times colours) beside a boolean OR of the same kind of shapes (green)."""
    red = CS._channels(CS._filler(), [250, 170, 250, 170])[0]
    u = _or([_tri([(60, -4), (260, -4), (60, 196)])] + [translate(s, [nat(3), nat(1)]) for s in CS._filler()])
    return [red, _paint(u), nat(0)]


def two_ors():
    """Two boolean ORs: green's holds the whole-picture triangle, red's the triangle of one_shape()."""
    u1 = _or([_tri([(60, -4), (260, -4), (60, 196)])] + CS._filler())
    u2 = _or([_tri(WHOLE)] + [translate(s, [nat(5), nat(2)]) for s in CS._filler()])
    return [_paint(u1), _paint(u2, 70), nat(0)]


def three_leaves():
    """A tree of three guarded leaves is walked as written: no reduction, no cover bit."""
    u = _or(CS._filler()[:3])
    return [_paint(u), _paint(u, 50), nat(0)]


def _other_waves():
    """census_scenes._filler()'s four triangles AND other waves: the same geometry, so the same bounds and the same guard bits."""
    return [set_and(CS._tri(10 + 75 * i, 4 + 9 * i, 95 + 75 * i, 40 + 9 * i), RS._wave((310, 450, 280, 520)[i], x() if i % 2 else add(x(), y()))) for i in range(4)]


def shared_ors():
    """Two boolean ORs over the same four triangles (other patterns): their leaves share guard bits.  Green's also holds the
    whole-picture triangle and is covered everywhere; red's is covered nowhere and must keep every leaf."""
    u1 = _or(CS._filler())
    u2 = _or([_tri(WHOLE)] + _other_waves())
    return [_paint(u1), _paint(u2, 70), nat(0)]


def shared_with_colours():
    """An f64 max reduction (red) and a boolean OR (green) over the same four triangles; green also holds the whole-picture triangle."""
    red = CS._channels(CS._filler(), [250, 170, 250, 170])[0]
    u = _or([_tri(WHOLE)] + _other_waves())
    return [red, _paint(u), nat(0)]


def tainted():
    """The whole-picture triangle AND Step(Sin(10^6 x) + 2): 1 on every pixel, but the Sin's argument is not provably bounded, so it
    may send its tile to the interpreter: the leaf is tainted and the measurement leaves it out -- nothing is covered."""
    return _scene([set_and(_tri(WHOLE), step(add(sin(mul(x(), nat(1000000))), nat(2))))])

"""Scenes and the numpy side of tests/test_gpu_census.py (the census of guard bits): what the guard words of a set
must hold once maray_jit_census has been through them,

    pack_words(effective(geo & second & (exact | ~eligible)))

with geo / second the ROW section's guards and the REFINE section's second bounds per rectangle (tests/refine_eval.py), exact
= "the guarded conjunction is != 0 on some pixel of the rectangle" (refine_eval.nonzero_per_rectangle) and eligible the bits
the library says a census may clear (Tape.census_eligible).  Scenes are 320 x 72 like refine_scenes': five rectangles of 64
pixels (the second 256-pixel tile is ragged), two groups of 32 rows and one of 8.  No GPU in here."""
import numpy as np

import refine_eval as RE
import refine_scenes as RS
from marayb import add, eq, inside_triangle, max_, mul, nat, neg, set_and, translate, var, x, y

W, H = RS.W, RS.H


def eligible_guards(tape):
    """Per guard: it has a bit of its own and the census may clear it."""
    pos, n_words, _, _ = tape.guard_layout()
    el = tape.census_eligible()
    assert len(el) == n_words
    return np.array([p >= 0 and bool((int(el[p // 64]) >> (p % 64)) & 1) for p in map(int, pos)], bool)


def words(tape, w, y0, rows, params=None, census=True):
    """(rectangles, words per rectangle) uint64: the refined words, or what the census leaves of them."""
    pos, n_words, gw, gh = tape.guard_layout()
    geo, second, _ = RE.guard_bits(tape, w, y0, rows, gw, gh, params=params)
    bits = geo & second
    if census:
        exact = RE.nonzero_per_rectangle(tape, w, y0, rows, gw, gh, params=params, only=geo)
        bits = bits & (exact | ~eligible_guards(tape)[None, :])
    return RE.pack_words(RE.effective(bits, RE.derived_members(tape)), pos, n_words)


def nonzero_counts(tape, w, y0, rows, params=None):
    """(rectangles, n_guards) integers: on how many pixels of the rectangle a conjunction guarded by that guard is != 0 (the
    largest count among the guard's regions); every pixel evaluated, as refine_eval.nonzero_per_rectangle does without `only`."""
    consts, _, pix = tape.arrays()
    pos, _, gw, gh = tape.guard_layout()
    n_ynum = RE.n_numeric(tape)
    (n_groups, n_rect), _, _, _, _ = RE.rectangles(w, rows, gw, gh)
    yv_rows = RE.numeric_yvals_of_rows(tape, w, y0, rows, params)
    ry, rx = np.divmod(np.arange(rows * w), w)
    rect_of = (ry // gh) * n_rect + rx // gw
    out = np.zeros((n_groups * n_rect, len(pos)), np.int64)
    for k, ends in RE.guarded_regions(tape).items():
        for end in ends:
            v = RE.run(RE.cone(pix, end), consts, tape.info['n_pix_slots'], rows * w, {0: rx.astype(np.float64), 1: (y0 + ry).astype(np.float64)},
                       yvals=yv_rows[ry], params=params, want=end)
            out[:, k - n_ynum] = np.maximum(out[:, k - n_ynum], np.bincount(rect_of[v != 0.0], minlength=n_groups * n_rect))
    return out


def _num(v):
    return nat(v) if v >= 0 else neg(nat(-v))


def _tri(x0, y0, x1, y1):
    """The half of the box x0..x1 x y0..y1 above its falling diagonal, corner (x0, y0)."""
    return inside_triangle([(_num(x0), _num(y0)), (_num(x1), _num(y0)), (_num(x0), _num(y1))], [x(), y()])


def _channels(shapes, colours):
    """Red and green are the max over ALL shapes times a colour each (green's at half strength), blue is 0: two f64 max
    reductions in which every shape is a guarded leaf -- a tree of fewer than four such leaves is walked as written, and a
    shape it shares with one would keep its bit for that walk's SKIP."""
    out = []
    for ch in range(2):
        c = None
        for s, col in zip(shapes, colours):
            if isinstance(col, tuple):          # (a parameter, a number): multiplied into the shape first, a PIXEL op (times a constant it would be a ROW op)
                s, col = mul(s, col[0]), col[1]
            t = mul(s, nat(col if ch == 0 else col // 2 + 1))
            c = t if c is None else max_(c, t)
        out.append(c)
    return out + [nat(0)]


def _filler():
    """Four patterned triangles, so that a tree has the leaves a reduction asks for whatever the shapes under test turn into."""
    return [set_and(_tri(10 + 75 * i, 4 + 9 * i, 95 + 75 * i, 40 + 9 * i), RS._wave((257, 400, 300, 500)[i], add(x(), y()) if i % 2 else x())) for i in range(4)]


# (x, y) of the single pixels: lane 0 and lane 63 of a pass, the first and the last row of a group of 32, and the ragged last
# rectangle (x >= 256) in the ragged last group (rows 64 .. 71)
ONE_PIXELS = ((128, 5), (191, 40), (100, 32), (100, 63), (300, 70))


def one_pixel():
    """Five shapes that are != 0 on exactly one pixel each (a triangle over the whole picture AND a long wave AND x == px AND
    y == py) beside four ordinary ones."""
    whole = _tri(-8, -8, 2000, 2000)
    shapes = _filler()
    for n, (px, py) in enumerate(ONE_PIXELS):
        on = set_and(set_and(whole, RS._wave(4000 + 100 * n, add(x(), nat(7)))), set_and(eq(x(), nat(px)), eq(y(), nat(py))))
        shapes.append(on)
    return _channels(shapes, [255 - 9 * n for n in range(len(shapes))])


def covered():
    """An OR of booleans (one colour for all shapes) in which two shapes are 1 on every pixel of the picture: whichever comes
    second in a pass is != 0 only under the first, and a loop that left on "every lane covered" would never enter it."""
    box = lambda n: set_and(set_and(_tri(-400 - n, -400 - n, 3000, 3000), RS._wave(5000 + 500 * n, add(x(), nat(11)))), RS._wave(7000, add(y(), nat(3 + n))))
    shapes = [box(0), box(1)] + _filler()
    u = None
    for s in shapes:
        u = s if u is None else max_(u, s)
    return [mul(add(u, nat(1)), nat(100)), mul(add(u, nat(1)), nat(50)), nat(0)]         # (u times a colour would be ONE guarded conjunction)


def pixel_param():
    """(color, params): the filler, its first shape's colour scaled by parameter c, which only PIXEL ops read -- inside the
    leaf, so that leaf's bit is never cleared (at c = 0 it is zero everywhere) -- and moved in x by t, which the ROW section reads."""
    shapes = _filler()
    colours = [(var('c'), 120), 200, 150, 100]
    return [translate(c, [var('t'), nat(0)]) for c in _channels(shapes, colours)], [('t', -64.0, 64.0), ('c', 0.0, 1.0)]


def three_colours():
    """An f64 max reduction over shapes of three colours; the third colour sits on a shape whose pattern is negative
    on the left of the picture: its triangle reaches rectangles where it shows in no pixel."""
    shapes = _filler() + [set_and(_tri(2, 2, 318, 70), RS._wave(300, add(x(), nat(160))))]
    return _channels(shapes, [250, 170, 250, 170, 90])

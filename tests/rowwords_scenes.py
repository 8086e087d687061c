"""Scenes and the numpy side of tests/test_rowwords_policy.py and tests/test_gpu_rowwords.py (row words): what a
set's fourth table of guard words and its row words must hold once maray_jit_rowscan and maray_jit_rowscan_apply have been
through it.

Per (rectangle, row) with a pixel inside the picture, the row's words are the band's -- the third table, cover_scenes.words
-- with
  * every census-eligible bit cleared whose guarded conjunctions are 0 on every pixel of the row inside the rectangle, and
  * for every OR with a cover bit whose untainted guarded leaves (those whose bit the band's words hold) cover every such
    pixel: the cover bit set and those of the OR's leaf bits cleared that the cover may clear.
A rectangle is flagged where at least `threshold` of its rows differ from the band; the fourth table is the third with the
row flag (Tape.rowwords_flag) in the flagged rectangles' last word.  A rectangle without a leaf bit of a reduction, and a
(rectangle, row) without a pixel, keep the band's words.  No GPU in here."""
import numpy as np

import census_scenes as CS
import cover_scenes as CV
import refine_eval as RE
from marayb import eq, nat, neg, set_and, set_inv, step, sub, add, mul, recip, sin, translate, var, x, y

W, H = CV.W, CV.H


def _bit(a, b):
    return ((a[..., b // 64] >> np.uint64(b % 64)) & np.uint64(1)).astype(bool)


def reduction_bits(tape):
    """The guard bits that are a leaf of some reduction (boolean OR or f64 max) of the PIXEL section: the eligible bits and
    the leaves of the ORs with a cover bit -- what the library calls a rectangle's 'leaf bits'."""
    _, n_words, _, _ = tape.guard_layout()
    m = np.array([int(v) for v in tape.census_eligible()], dtype=np.uint64)
    for red in tape.cover_plan():
        for _, bit, _, _ in red['leaves']:
            m[bit // 64] |= np.uint64(1) << np.uint64(bit % 64)
    assert len(m) == n_words
    return m


def row_words(tape, w, y0, rows, params=None, threshold=None):
    """-> dict: xbits (rectangles, words), rwords (rows, rectangles per row, words), changed (rectangles, rows per band) bool,
    flagged (rectangles,) bool, band (the third table), hit_rows / cover_rows (for the soundness test)."""
    pos, n_words, gw, gh = tape.guard_layout()
    flag = tape.rowwords_flag()
    assert flag >= 0, 'the program gets no row words'
    threshold = max(1, gh // 4) if threshold is None else threshold
    vb, cb, _ = CV.words(tape, w, y0, rows, params=params)
    (n_groups, n_rect), _, _, _, _ = RE.rectangles(w, rows, gw, gh)
    consts, _, pix = tape.arrays()
    n_ynum = RE.n_numeric(tape)
    el = [int(v) for v in tape.census_eligible()]
    yv_rows = RE.numeric_yvals_of_rows(tape, w, y0, rows, params)
    ry, rx = np.divmod(np.arange(rows * w), w)
    rect_of = (ry // gh) * n_rect + rx // gw            # band rectangle of a pixel
    rr_of = ry * n_rect + rx // gw                      # (row, rectangle) of a pixel
    inside = np.bincount(rr_of, minlength=rows * n_rect)
    band_of_rr = (np.arange(rows) // gh)[:, None] * n_rect + np.arange(n_rect)[None, :]      # (rows, n_rect) -> band rectangle
    band = vb[band_of_rr]                               # (rows, n_rect, words)
    rw = band.copy()
    # eligible bits: hit on the row?
    hit_rows = {}
    for k, ends in RE.guarded_regions(tape).items():
        p = int(pos[k - n_ynum])
        if p < 0 or not (el[p // 64] >> (p % 64)) & 1:
            continue
        sel = np.nonzero(_bit(vb, p)[rect_of])[0]
        hit = np.zeros(rows * n_rect, bool)
        for end in ends:
            if not len(sel):
                break
            v = RE.run(RE.cone(pix, end), consts, tape.info['n_pix_slots'], len(sel), {0: rx[sel].astype(np.float64), 1: (y0 + ry[sel]).astype(np.float64)},
                       yvals=yv_rows[ry[sel]], params=params, want=end)
            hit[rr_of[sel][v != 0.0]] = True
        hit_rows[p] = hit.reshape(rows, n_rect)
        rw[..., p // 64] &= ~np.where(hit_rows[p], np.uint64(0), np.uint64(1) << np.uint64(p % 64))
    # ORs with a cover bit: covered on the row?
    cover_rows = []
    masks = CV.leaf_masks(tape, w, y0, rows, params, cbits=vb)
    for j, red in enumerate(tape.cover_plan()):
        cov = ((inside > 0) & (np.bincount(rr_of[masks[j]], minlength=rows * n_rect) == inside)).reshape(rows, n_rect)
        cover_rows.append(cov)
        for _, bit, _, eligible in red['leaves']:
            if eligible:
                rw[..., bit // 64] &= ~np.where(cov, np.uint64(1) << np.uint64(bit % 64), np.uint64(0))
        rw[..., red['bit'] // 64] |= np.where(cov, np.uint64(1) << np.uint64(red['bit'] % 64), np.uint64(0))
    # what no pass refines keeps the band's words: no pixel on the row, or no leaf bit of a reduction in the band's words
    redm = reduction_bits(tape)
    quiet = ~((band & redm[None, None, :]) != 0).any(axis=2) | (inside.reshape(rows, n_rect) == 0)
    rw[quiet] = band[quiet]
    differs = (rw != band).any(axis=2)                  # (rows, n_rect)
    changed = np.zeros((n_groups * n_rect, gh), bool)
    for r in range(rows):
        changed[(r // gh) * n_rect + np.arange(n_rect), r % gh] = differs[r]
    flagged = changed.sum(axis=1) >= threshold
    xb = vb.copy()
    xb[flagged, flag // 64] |= np.uint64(1) << np.uint64(flag % 64)
    return {'xbits': xb, 'rwords': rw, 'changed': changed, 'flagged': flagged, 'band': vb, 'hit_rows': hit_rows, 'cover_rows': cover_rows,
            'n_rect': n_rect, 'gh': gh}


def flagged_rows(model):
    """(rows, rectangles per row) booleans: the (row, rectangle) pairs whose row words a launch reads."""
    rows = model['rwords'].shape[0]
    return model['flagged'][(np.arange(rows) // model['gh'])[:, None] * model['n_rect'] + np.arange(model['n_rect'])[None, :]]


# ---- scenes, 320 x 72 like cover_scenes': five rectangles per row, two whole bands and a ragged 8-row one -----------------------
def _box_rows(ya, yb):
    """1 on the rows ya <= y < yb, over the whole width: a shape whose edges are horizontal (y factors of its leaf)."""
    return set_and(CV._tri(CV.WHOLE), set_and(step(sub(y(), CV._num(ya))), set_inv(step(sub(y(), CV._num(yb))))))


def edge_mid_band():
    """Rows 0 .. 15 covered, the rows below empty: the edge is horizontal in the middle of the first band."""
    return CV._scene([_box_rows(-4, 16)])


def edge_on_boundary():
    """The same with the edge on the band boundary at row 32: no row differs from its band."""
    return CV._scene([_box_rows(-4, 32)])


def _steep(c):
    """The part of the picture left of a steep line from (c, -8) down to the left: 26 pixels over the picture's 72 rows at c = 290."""
    return CV._tri([(-8, -8), (c, -8), (-8, 800)])


def _steep_scene(more=()):
    """Four such shapes and no other: the widest holds the rectangles x < 256 whole, and its edge crosses the rectangle x = 256 ..
    319 on every row of every band."""
    u = CV._or([_steep(c) for c in (290, 200, 140, 80)] + list(more))
    return [CV._paint(u), CV._paint(u, 50), nat(0)]


def slanted():
    """Slanted edges alone: every row of a rectangle is mixed, or covered, like its band -- nothing changes, nothing is flagged."""
    return _steep_scene()


def all_but_one():
    """Every row covered but row 10 (cover_scenes.row_out): the band is mixed, 31 of its rows are covered."""
    return CV.row_out()


def one_row():
    """Row 40 alone: 31 rows of the second band are emptied."""
    return CV._scene([_box_rows(40, 41)])


def few_rows():
    """slanted() and a small triangle right of the slanted edge that ends a few rows above the first band's last row: its bit
    is cleared on those rows alone, in the one rectangle the slanted edge keeps mixed -- fewer rows than a threshold of 8, more
    than one of 1.  (A shape with a horizontal edge inside a band changes EVERY row of its rectangles: covered above, cleared below.)"""
    return _steep_scene([CV._tri([(300, -8), (318, -8), (300, 28)])])


def ragged():
    """Rows 60 .. 67 over the whole width: the edge crosses the second band and the ragged 8-row band, in the ragged right
    rectangle too."""
    return CV._scene([_box_rows(60, 68)])


def tainted_rows():
    """edge_mid_band() AND Step(Sin(10^6 x) + 2), 1 everywhere but not provably bounded: the leaf is tainted, its rows are
    never counted as covered and its bit is never cleared."""
    return CV._scene([set_and(_box_rows(-4, 16), step(add(sin(mul(x(), nat(1000000))), nat(2))))])


def pixel_param():
    """(color, params): edge_mid_band()'s shape AND Step(c - x / 1000), c a parameter only PIXEL ops read (tainted); t moves
    the picture in x, which the ROW section reads."""
    color = CV._scene([set_and(_box_rows(-4, 16), step(sub(var('c'), mul(x(), recip(nat(1000))))))])
    return [translate(c, [var('t'), nat(0)]) for c in color], [('t', -64.0, 64.0), ('c', 0.0, 1.0)]


def row_param():
    """(color, params): edge_mid_band() moved in y by t, which the ROW section reads."""
    return [translate(c, [nat(0), var('t')]) for c in edge_mid_band()], [('t', -16.0, 16.0)]


def two_ors():
    """Two boolean ORs: red's holds rows 0 .. 15, green's rows 40 .. 71."""
    u1 = CV._or([_box_rows(-4, 16)] + CS._filler())
    u2 = CV._or([_box_rows(40, 80)] + [translate(s, [nat(5), nat(2)]) for s in CS._filler()])
    return [CV._paint(u1), CV._paint(u2, 70), nat(0)]


def shared_ors():
    """Two boolean ORs over the same four triangles (their leaves share guard bits: never cleared by a cover); green's also
    holds rows 0 .. 15."""
    u1 = CV._or(CS._filler())
    u2 = CV._or([_box_rows(-4, 16)] + CV._other_waves())
    return [CV._paint(u1), CV._paint(u2, 70), nat(0)]


def with_colours():
    """An f64 max reduction (red) beside a boolean OR that holds rows 0 .. 15 (green)."""
    red = CS._channels(CS._filler(), [250, 170, 250, 170])[0]
    u = CV._or([_box_rows(-4, 16)] + [translate(s, [nat(3), nat(1)]) for s in CS._filler()])
    return [red, CV._paint(u), nat(0)]


PLAIN = {'edge_mid_band': edge_mid_band, 'edge_on_boundary': edge_on_boundary, 'slanted': slanted, 'all_but_one': all_but_one, 'one_row': one_row,
         'few_rows': few_rows, 'ragged': ragged, 'row_out': CV.row_out, 'tainted_rows': tainted_rows, 'two_ors': two_ors, 'shared_ors': shared_ors,
         'with_colours': with_colours}

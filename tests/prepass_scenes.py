"""Scenes and the numpy side of tests/test_prepass_policy.py and tests/test_gpu_prepass.py (the wide pre-pass of a busy tile's
leafless rectangles, maray_jit_pixels_pp).

The model works on the guard words a launch reads -- the fourth table and the row words (tests/rowwords_scenes.py's row_words,
or Context.debug_row_words), or the third table alone for a covered set without flags:
  * a (rectangle, row) is LEAFY when its words -- the row's, where the rectangle carries the row flag, else the band's without
    the flag -- hold a bit that is no cover bit, and leafless otherwise;
  * a tile-row (a 256-pixel tile on one row: four rectangles) is `all_zero` when no bit at all is set (the wide variant, as
    before), `all_leafy` (the narrow loop, as before), `mixed` (the pre-pass, then narrow passes for the leafy rectangles) or
    `leafless_only` (the pre-pass alone).
No GPU in here."""
import numpy as np

import census_scenes as CS
import cover_scenes as CV
import refine_scenes as RS
import rowwords_scenes as RW
from marayb import add, mul, nat, recip, set_and, set_inv, sin, step, sub, translate, var, x, y

W, H = 512, 64          # two whole tiles, two bands of 32 rows
CLASSES = ('all_zero', 'all_leafy', 'mixed', 'leafless_only')


def launch_words(xbits, rwords, flag, rows, gh):
    """(rows, rectangles per row, words): the words maray_jit_pixels_pp holds per (row, rectangle) behind its strip's fetch.
    xbits: (rectangles, words), band by band; rwords: (rows x rectangles per row, words) or empty (a set without row words)."""
    n_groups = (rows + gh - 1) // gh
    n_rect = xbits.shape[0] // n_groups
    band = xbits[(np.arange(rows) // gh)[:, None] * n_rect + np.arange(n_rect)[None, :]].copy()
    if flag < 0:
        return band
    bit = np.uint64(1) << np.uint64(flag % 64)
    flagged = (band[..., flag // 64] & bit) != 0
    band[..., flag // 64] &= ~bit
    if rwords.size:
        band[flagged] = rwords.reshape(rows, n_rect, -1)[flagged]
    else:
        assert not flagged.any()
    return band


def leafy_masks(words, cover_bits):
    """(rows, tiles) integers, bit e: rectangle e of the tile is leafy; and (rows, tiles) booleans: some bit of the tile is set."""
    other = words.copy()
    for b in cover_bits:
        other[..., b // 64] &= ~(np.uint64(1) << np.uint64(b % 64))
    rows, n_rect, _ = words.shape
    leafy = (other != 0).any(axis=2).reshape(rows, n_rect // 4, 4)
    some = (words != 0).any(axis=2).reshape(rows, n_rect // 4, 4).any(axis=2)
    return (leafy * (1 << np.arange(4))[None, None, :]).sum(axis=2), some


def classify(words, cover_bits):
    """-> dict: tile_rows and passes by class, narrow passes run with and without the pre-pass."""
    mask, some = leafy_masks(words, cover_bits)
    n_leafy = np.array([bin(v).count('1') for v in range(16)])[mask]
    cls = {'all_zero': ~some, 'all_leafy': mask == 15, 'leafless_only': some & (mask == 0)}
    cls['mixed'] = ~cls['all_zero'] & ~cls['all_leafy'] & ~cls['leafless_only']
    out = {'tile_rows': {k: int(cls[k].sum()) for k in CLASSES}}
    out['narrow_passes_before'] = int(4 * some.sum())
    out['narrow_passes_after'] = int(n_leafy[some].sum())
    out['leafless_passes'] = {k: int((4 - n_leafy)[cls[k]].sum()) for k in ('mixed', 'leafless_only')}
    out['leafy_passes'] = {k: int(n_leafy[cls[k]].sum()) for k in ('mixed', 'all_leafy')}
    out['pre_passes'] = int(cls['mixed'].sum() + cls['leafless_only'].sum())
    return out


def model(tape, w, y0, rows, params=None, threshold=None):
    """classify() of the launch's words by tests/rowwords_scenes.py's model."""
    m = RW.row_words(tape, w, y0, rows, params=params, threshold=threshold)
    words = launch_words(m['xbits'], m['rwords'].reshape(-1, m['rwords'].shape[2]), tape.rowwords_flag(), rows, m['gh'])
    return classify(words, tape.cover_bits()), m


# ---- scenes, 512 x 64 (also rendered at 600 x 72 and as rows 37 .. 101 of 200) ----------------------------------------------------
# census_scenes._filler()'s four patterned triangles hold x 10 .. 320, rows 4 .. 67: tile 0 is mixed on the upper rows and all
# leafy around row 35.  The shapes under test sit in tile 1 (x 256 .. 511), whose rows 0 .. 30 the filler leaves alone.
def gradient():
    """A background that varies in x and in y: (x + 3 y) / 8, at most 102 over 600 x 72."""
    return mul(add(x(), mul(y(), nat(3))), recip(nat(8)))


def _box(xa, xb, ya, yb):
    """1 on xa <= x < xb, ya <= y < yb: every edge horizontal or vertical."""
    whole = CV._tri([(-8, -8), (2000 + xa + 3 * ya, -8), (-8, 2000 + xb + 5 * yb)])      # (over the whole picture; one of its own per box: no shared bound)
    s = set_and(whole, set_and(step(sub(y(), CV._num(ya))), set_inv(step(sub(y(), CV._num(yb))))))
    return set_and(s, set_and(step(sub(x(), CV._num(xa))), set_inv(step(sub(x(), CV._num(xb))))))


def _wavy(x0, y0, x1, y1, period=300):
    """A patterned triangle (never covered: leafy where it shows)."""
    return set_and(CS._tri(x0, y0, x1, y1), RS._wave(period, add(x(), y())))


def _paint(u, k=60):
    return add(CV._paint(u, k), gradient())


def _stripe():
    """Four patterned triangles, one in each rectangle of tile 1 on the rows 50 .. 62: an all-leafy tile-row."""
    return [_wavy(258 + 64 * k, 50, 316 + 64 * k, 63, 280 + 37 * k) for k in range(4)]


def _scene(shapes, free=None):
    # (a free leaf goes inside the tree: as the root's own operand the whole tree sits behind its guard, a bit the census cannot clear)
    stripe = _stripe()
    u = CV._or(list(shapes) + stripe[:3] + ([free] if free is not None else []) + stripe[3:] + CS._filler())
    return [_paint(u), _paint(u, 40), gradient()]


COVER_TOP = (256, 512, -4, 16)      # tile 1, rows 0 .. 15: covered on those rows, empty below -- a leafless-only tile-row


def one_leafy():
    """Case 1: one leafy rectangle (x 320 .. 383) beside three empty ones, rows 18 .. 30."""
    return _scene([_box(*COVER_TOP), _wavy(330, 18, 370, 31)])


def covered_leafy_empty():
    """Case 2: rectangle 6 of the row (x 384 .. 447) covered on the whole first band, rectangle 5 leafy, 4 and 7 empty."""
    return _scene([_box(384, 448, -4, 32), _wavy(330, 2, 370, 30), _box(256, 512, 40, 48)])


def covered_and_empty():
    """Case 3: covered and empty rectangles only in tile 1: no narrow pass there."""
    return _scene([_box(384, 448, -4, 32), _box(256, 320, 40, 48)])


def two_ors():
    """Case 5: two ORs with cover bits; rectangle 6 is covered by red's and leafy in green's."""
    u1 = CV._or([_box(384, 448, -4, 32), _box(*COVER_TOP)] + CS._filler())
    u2 = CV._or([_wavy(390, 2, 440, 30), _box(256, 320, 40, 48)] + _stripe() + [translate(s, [nat(5), nat(2)]) for s in CS._filler()])
    return [_paint(u1), _paint(u2, 40), gradient()]


def with_colours():
    """Case 6: an f64 max tree (red) beside a boolean OR (green)."""
    red = CS._channels(CS._filler(), [250, 170, 250, 170])[0]
    u = CV._or([_box(*COVER_TOP), _box(384, 448, 20, 32)] + _stripe() + [translate(s, [nat(3), nat(1)]) for s in CS._filler()])
    return [add(red, gradient()), _paint(u), gradient()]


def free_leaf():
    """Case 7: the OR holds a free (unguarded) leaf, a y value: 1 on the rows 56 and below."""
    return _scene([_box(*COVER_TOP), _wavy(330, 18, 370, 31)], free=step(sub(y(), nat(56))))


def edge_in_band():
    """Case 8: a horizontal edge inside the first band over tile 1: leaflessness is decided per row from row words.  (Rendered
    96 rows high, tile 1 is covered on the whole third band: the set has a cover bit whatever the row scan flags.)"""
    return _scene([_box(*COVER_TOP), _box(256, 512, 64, 100)])


def sin_in_leaf():
    """Case 9a: a Sin that defers its tile inside a leafy rectangle (x 320 .. 383) next to leafless ones."""
    return _scene([_box(*COVER_TOP), set_and(CS._tri(330, 18, 370, 31), step(add(sin(mul(x(), nat(1000000))), nat(2))))])


def sin_in_background():
    """Case 9b: the background holds a Sin whose argument is huge from x = 106 on: those tiles are deferred, pre-pass or not."""
    u = CV._or([_box(*COVER_TOP), _wavy(330, 18, 370, 31)] + _stripe() + CS._filler())
    wobble = mul(add(sin(mul(x(), nat(1000000))), nat(1)), nat(8))
    return [add(_paint(u), wobble), _paint(u, 40), gradient()]


def pixel_param():
    """Case 10 (color, params): c scales the background, read by PIXEL ops alone; t moves the picture in y, read by the ROW section."""
    u = CV._or([_box(*COVER_TOP), _wavy(330, 18, 370, 31)] + _stripe() + CS._filler())
    color = [add(CV._paint(u, 60), mul(gradient(), var('c'))), _paint(u, 40), gradient()]
    return [translate(c, [nat(0), var('t')]) for c in color], [('t', -16.0, 16.0), ('c', 0.0, 2.0)]


PLAIN = {'one_leafy': one_leafy, 'covered_leafy_empty': covered_leafy_empty, 'covered_and_empty': covered_and_empty, 'two_ors': two_ors,
         'with_colours': with_colours, 'free_leaf': free_leaf, 'edge_in_band': edge_in_band, 'sin_in_leaf': sin_in_leaf,
         'sin_in_background': sin_in_background}

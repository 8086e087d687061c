#!/usr/bin/env python3
"""tools/census_rows.py [SCALE] [BAND0 BAND1] -- the CPU census behind the row words: chess at (1024 SCALE)^2
(default SCALE = 4), evaluated band by band with the tests' numpy model (tests/rowwords_scenes.py), no GPU.

Per band of guard rows it looks inside each rectangle that still holds a leaf bit of a reduction in the cover's words at single
rows, and prints, summed over the bands BAND0 <= band < BAND1 (default: all): the rectangles with a leaf bit, their (rectangle,
row) pairs, how many of those the OR of the set leaves covers on every pixel, leaves empty, or leaves mixed, the leaf bits a
pass walks with the band's words and with the row's, the pairs whose row words are all zero (the wide path), and the
rectangles a threshold of a quarter of the band's rows flags.  One JSON line per band with --bands, one for the sum."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import maray_amd as M  # noqa: E402
import rowwords_scenes as RW  # noqa: E402


def popcount(a):
    a = a.astype(np.uint64).copy()
    n = np.zeros(a.shape, np.int64)
    while a.any():
        n += (a & np.uint64(1)).astype(np.int64)
        a >>= np.uint64(1)
    return n


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    per_band = '--bands' in sys.argv
    scale = int(args[0]) if args else 4
    s = M.Scene(open(os.path.join(ROOT, 'tests', 'golden', 'chess.maray'), 'rb').read())
    if scale > 1:
        s.rescale(scale, scale)
    tape = s.lower()
    w = h = 1024 * scale
    _, n_words, gw, gh = tape.guard_layout()
    b0, b1 = (int(args[1]), int(args[2])) if len(args) > 2 else (0, (h + gh - 1) // gh)
    leaf = RW.reduction_bits(tape)
    cover = tape.cover_plan()
    total = {}
    for band in range(b0, b1):
        y0, rows = band * gh, min(gh, h - band * gh)
        m = RW.row_words(tape, w, y0, rows)
        bandw, roww = m['band'][None, :, :] & leaf[None, None, :], m['rwords'] & leaf[None, None, :]
        busy = (bandw != 0).any(axis=2)[0]                                   # rectangles with a leaf bit
        covered = np.zeros(m['rwords'].shape[:2], bool)
        for red in cover:
            covered |= RW._bit(m['rwords'], red['bit']) & ~RW._bit(m['band'], red['bit'])[None, :]
        empty = ~(roww != 0).any(axis=2) & ~covered
        rec = {'band': band, 'rectangles_with_leaf_bit': int(busy.sum()), 'pairs': int(busy.sum()) * rows,
               'pairs_covered': int(covered[:, busy].sum()), 'pairs_empty': int(empty[:, busy].sum()),
               'leaf_bits_band_words': int(popcount(np.broadcast_to(bandw, roww.shape)[:, busy]).sum()), 'leaf_bits_row_words': int(popcount(roww[:, busy]).sum()),
               'pairs_all_zero_words': int((~(m['rwords'] != 0).any(axis=2))[:, busy].sum()), 'rectangles_flagged': int(m['flagged'].sum())}
        rec['pairs_mixed'] = rec['pairs'] - rec['pairs_covered'] - rec['pairs_empty']
        if per_band and rec['rectangles_with_leaf_bit']:
            print(json.dumps(rec), flush=True)
        for k, v in rec.items():
            if k != 'band':
                total[k] = total.get(k, 0) + v
    total.update(scene='chess', size=w, bands=[b0, b1], rows_per_band=gh, pixels_per_rectangle_row=gw)
    print(json.dumps(total))


if __name__ == '__main__':
    main()

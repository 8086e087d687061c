#!/usr/bin/env python3
"""Census of the guard bits of chess @4096^2 (CPU, numpy): what the ROW section's guards set per rectangle, what the real
REFINE section (include/maray_tape.h, maray_refine) leaves of it, and -- with --exact -- on how many
(rectangle, leaf) pairs the leaf is != 0 on some pixel at all.

    python3 tools/census_refine.py [--scale 4] [--exact]

Rectangles are the specialised kernels' (Tape.guard_layout: 64 pixels x 32 rows for chess); leaves are the guards that have
a bit of their own.  One JSON line.  --exact evaluates every leaf on every pixel of the rectangles whose geometric bit is
set (minutes at scale 4).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import numpy as np                                  # noqa: E402

import maray_amd as M                               # noqa: E402
import refine_eval as RE                            # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scale', type=int, default=4, help='chess.maray (1024^2) rescaled by this factor')
    ap.add_argument('--exact', action='store_true')
    args = ap.parse_args()
    s = M.Scene(open(os.path.join(ROOT, 'tests', 'golden', 'chess.maray'), 'rb').read())
    s.rescale(args.scale, args.scale)
    w, h = s.size
    tape = s.lower()
    pos, n_words, gw, gh = tape.guard_layout()
    geo, second, has = RE.guard_bits(tape, w, 0, h, gw, gh)
    leaf = pos >= 0
    g, r = geo[:, leaf], (geo & second)[:, leaf]
    busy = g.any(axis=1)
    n_rect = (w + 255) // 256 * (256 // gw)
    tiles = lambda bits: bits.any(axis=1).reshape(-1, n_rect // (256 // gw), 256 // gw).any(axis=2)      # per 256-pixel tile-band
    out = {'scene': 'chess @%dx%d' % (w, h), 'rectangle': [gw, gh], 'leaves': int(leaf.sum()), 'leaves_with_a_second_bound': int((leaf & has).sum()),
           'refine_ops': int(tape.refine.n_ops), 'busy_rectangles': int(busy.sum()),
           'geometric_bits': int(g.sum()), 'refined_bits': int(r.sum()), 'ratio': round(float(r.sum()) / float(g.sum()), 4),
           'busy_rectangles_without_a_bit': int((busy & ~r.any(axis=1)).sum()),
           'busy_tile_bands': int(tiles(g).sum()), 'busy_tile_bands_without_a_bit': int((tiles(g) & ~tiles(r)).sum())}
    if args.exact:
        exact = RE.nonzero_per_rectangle(tape, w, 0, h, gw, gh, only=geo)[:, leaf]
        assert not (exact & ~r).any(), 'a leaf is != 0 in a rectangle whose refined bit is clear'
        out.update(exact_bits=int(exact.sum()), busy_rectangles_without_an_exact_bit=int((busy & ~exact.any(axis=1)).sum()))
    print(json.dumps(out))


if __name__ == '__main__':
    main()

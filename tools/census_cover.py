#!/usr/bin/env python3
"""Census of the cover of guarded ORs (CPU, numpy): on chess rescaled to 4096^2, per boolean OR with a cover bit,
how many rectangles of 64 x 32 pixels hold one of its leaf bits after the census of guard bits, how many of those the OR covers
on every pixel, and how many leaf bits such rectangles hold -- what maray_jit_cover finds on the device, by the evaluator the
tests compare it with (tests/cover_scenes.py).

    python3 tools/census_cover.py [--scale 4] [--soup 300 --band 32]

One JSON line.  Minutes at scale 4."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import maray_amd as M       # noqa: E402
import cover_scenes as CV   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scale', type=int, default=4, help='chess.maray (1024^2) rescaled by this factor')
    ap.add_argument('--soup', type=int, default=0, help='N > 0: tests/fuzz_scenes.py polygon_soup(1, N) at 4096^2 instead of chess')
    ap.add_argument('--band', type=int, default=0, help='rows per evaluation (a multiple of the rectangle height; 0: all at once)')
    args = ap.parse_args()
    if args.soup:
        import fuzz_scenes
        from marayb import encode
        w = h = 4096
        s = M.Scene(encode((w, h), fuzz_scenes.polygon_soup(1, args.soup, w, h, mixed=False)))
        name = 'polygon_soup(1, %d) at %d^2' % (args.soup, w)
    else:
        s = M.Scene(open(os.path.join(ROOT, 'tests', 'golden', 'chess.maray'), 'rb').read())
        s.rescale(args.scale, args.scale)
        w = h = 1024 * args.scale
        name = 'chess rescaled to %d^2' % w
    tape = s.lower()
    band = args.band or h
    total = None
    for y0 in range(0, h, band):        # rectangles do not cross a band: the counts add up
        part = CV.counts(tape, w, y0, min(band, h - y0))
        total = part if total is None else [{k: a[k] + b[k] for k in a} for a, b in zip(total, part)]
    print(json.dumps({'scene': name, 'cover_bits': tape.cover_bits(), 'ors': total}))


if __name__ == '__main__':
    main()

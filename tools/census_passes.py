#!/usr/bin/env python3
"""tools/census_passes.py [SCALE] [BAND0 BAND1] [--sy=N] [--every=K] -- the CPU census behind the wide pre-pass: chess at
(1024 SCALE)^2 (default SCALE = 4), band by band with the tests' numpy models (tests/rowwords_scenes.py's row_words,
tests/prepass_scenes.py's classify), no GPU.

Prints, summed over the bands BAND0 <= band < BAND1 (default: all), the tile-rows (a 256-pixel tile on one row) by class --
all zero (the wide variant), all leafy (the narrow loop), mixed (pre-pass + the leafy passes), leafless only (the pre-pass
alone) -- and the 64-pixel passes by class: the narrow passes a frame runs without and with the pre-pass, the leafless passes
it replaces and the pre-passes it adds.  One JSON line per band with --bands, one for the sum.  --sy=N stretches the scene N times
vertically instead of SCALE (tools/run_crop.py's board crop is SCALE 4, --sy=16, bands 256 .. 384); --every=K takes every K-th band."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import maray_amd as M  # noqa: E402
import prepass_scenes as PP  # noqa: E402


def merge(total, rec):
    for k, v in rec.items():
        if isinstance(v, dict):
            merge(total.setdefault(k, {}), v)
        else:
            total[k] = total.get(k, 0) + v


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    per_band = '--bands' in sys.argv
    scale = int(args[0]) if args else 4
    s = M.Scene(open(os.path.join(ROOT, 'tests', 'golden', 'chess.maray'), 'rb').read())
    opt = {a.split('=')[0]: int(a.split('=')[1]) for a in sys.argv[1:] if a.startswith('--') and '=' in a}
    sy, every = opt.get('--sy', scale), opt.get('--every', 1)
    if scale > 1 or sy > 1:
        s.rescale(scale, sy)
    tape = s.lower()
    w, h = 1024 * scale, 1024 * sy
    _, _, gw, gh = tape.guard_layout()
    b0, b1 = (int(args[1]), int(args[2])) if len(args) > 2 else (0, (h + gh - 1) // gh)
    total = {}
    for band in range(b0, b1, every):
        rec, _ = PP.model(tape, w, band * gh, min(gh, h - band * gh))
        if per_band and rec['narrow_passes_before']:
            print(json.dumps(dict(rec, band=band)), flush=True)
        merge(total, rec)
    total['narrow_passes_saved_share'] = round(1.0 - total['narrow_passes_after'] / max(1, total['narrow_passes_before']), 4)
    total.update(scene='chess', size=w, height=h, every=every, bands=[b0, b1], rows_per_band=gh, pixels_per_pass=gw)
    print(json.dumps(total))


if __name__ == '__main__':
    main()

"""The second bounds of Step(Sin) factors over fresh seeds of tests/refine_fuzz_scenes.py, on the host: every scene lowered, its
guards and second bounds evaluated per rectangle (tests/refine_eval.py) at guard heights 8 and 32 (1 where the guards read Y)
under every value vector, every pixel through nonzero_per_rectangle.  A violation is a rectangle whose refined bit is clear
while a conjunction the guard skips is != 0 on one of its pixels.

    python tools/cpu_fuzz_refine.py FIRST_SEED N_SCENES [PROCESSES] > profiles/refine_fuzz_cpu.txt

Scene i is of kind KINDS[i % 8] (`many`, on 1100 x 200, once in 64 scenes; near3 takes its other turns), on 320 x 72, 449 x 100 and
its rows 37 .. 92 in turn; every fourth near3, edge and arith scene is supersampled, k = 2 and k = 4 in turn.  Prints a line for every scene that holds a hump or a violation, and the totals per kind; every scene's line goes to stderr."""
import os
import sys
import time
from multiprocessing import Pool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]


def case_of(first, i):
    import refine_fuzz_scenes as F
    n = len(F.KINDS)
    kind = F.KINDS[i % n]
    if kind == 'many' and (i // n) % 8:                 # 80 shapes on 1100 x 200 take a minute of numpy: one scene in 64, the others near3
        kind = 'near3'
    geo = F.G1100 if kind == 'many' else (F.G320, F.G449, F.G449R)[(i // n) % 3]
    k = (4 if (i // n) % 8 == 7 else 2) if kind in ('near3', 'edge', 'arith') and (i // n) % 4 == 3 else 1
    return (kind, first + i + i // n, geo, k)          # (i // n: a kind meets every residue of the seeds its forms are picked by)


def one(case):
    import refine_fuzz_scenes as F
    tape, made = F.lowered(case)
    gw, gh0 = tape.guard_layout()[2:]
    leaf = tape.guard_layout()[0] >= 0
    out = dict(kind=case[0], scenes=1, rectangles=0, cleared=0, near=0, humps=0, violations=0)
    w, y0, rows = F.sample_geo(case)
    shape_of = F.guard_shapes(tape, w, y0, rows) if case[0] == 'near3' and case[3] == 1 else {}
    for gh in ((1,) if gh0 == 1 else (8, 32)):
        for v in made.vectors:
            e = F.examine(tape, case, gh, v, gw=gw)
            out['rectangles'] += e['geo'].shape[0]
            out['cleared'] += int((e['geo'] & ~e['refined'] & leaf[None, :]).sum())
            out['violations'] += int(e['bad'].sum()) + int((e['refined'] & ~e['geo']).sum()) + int((~e['second'][:, ~e['has']]).sum())
            if shape_of:
                near, hump, _ = F.near3_counts(e, tape, made, shape_of)
                out['near'] += near
                out['humps'] += hump
    out['line'] = '%s seed %d %dx%d rows %d-%d k=%d: rectangles %d cleared %d humps %d violations %d' % (
        case[:2] + case[2] + (case[3], out['rectangles'], out['cleared'], out['humps'], out['violations']))
    out['k'] = case[3]
    return out


def main():
    import refine_fuzz_scenes as F
    first, n = int(sys.argv[1]), int(sys.argv[2])
    procs = int(sys.argv[3]) if len(sys.argv) > 3 else 16
    t0 = time.time()
    total = {k: dict(scenes=0, rectangles=0, cleared=0, near=0, humps=0, violations=0) for k in F.KINDS}
    by_k = {}
    with Pool(procs) as pool:
        for out in pool.imap(one, [case_of(first, i) for i in range(n)], chunksize=1):
            print(out['line'], file=sys.stderr, flush=True)
            if out['humps'] or out['violations']:
                print(out['line'], flush=True)
            by_k[out['k']] = by_k.get(out['k'], 0) + 1
            for k in total[out['kind']]:
                total[out['kind']][k] += out[k]
    print('# totals per kind: scenes, rectangles examined (both guard heights, every vector), bits cleared, cleared near3 rectangles of span [2.5, 3), humps kept, violations')
    for kind in F.KINDS:
        t = total[kind]
        print('%-10s scenes %5d  rectangles %8d  cleared %7d  near %5d  humps %5d  violations %d' % (kind, t['scenes'], t['rectangles'], t['cleared'], t['near'], t['humps'], t['violations']))
    print('all        scenes %5d  rectangles %8d  cleared %7d  violations %d   (%.0f s on %d processes)' % (
        sum(t['scenes'] for t in total.values()), sum(t['rectangles'] for t in total.values()), sum(t['cleared'] for t in total.values()),
        sum(t['violations'] for t in total.values()), time.time() - t0, procs))
    print('scenes by supersampling factor: %s' % sorted(by_k.items()))


if __name__ == '__main__':
    main()

"""The cases of the row words' fuzz (tests/test_rowwords_fuzz.py on the model alone, tests/test_gpu_rowwords_fuzz.py on the
device): twenty seeded soups of tests/cover_fuzz_scenes.py -- sixteen shapes, triangles, discs and boxes, half of them patterned
-- over its two geometries.  Every case has a flagged rectangle that holds a covered row, an emptied row and a mixed row at
once: a condition on the seeds, which were chosen on the CPU until it held (tools: `python tests/rowwords_fuzz_scenes.py`
prints the seeds that meet it); a seed that stops meeting it is replaced here, never skipped in a test.  No GPU in here."""
import numpy as np

import cover_fuzz_scenes as F
import rowwords_scenes as RW

A, B = F.A, F.B

# (kind, seed, geometry): five soups of each kind, three at 320 x 136 and two at 300 pixels of rows 37-141 of a 200-row picture
CASES = [('one', 44, A), ('one', 50, A), ('one', 58, A), ('one', 21, B), ('one', 23, B),
         ('two', 11, A), ('two', 15, A), ('two', 25, A), ('two', 0, B), ('two', 4, B),
         ('shared', 40, A), ('shared', 44, A), ('shared', 50, A), ('shared', 21, B), ('shared', 23, B),
         ('colours', 35, A), ('colours', 59, A), ('colours', 105, A), ('colours', 0, B), ('colours', 4, B)]


def model(case):
    """(tape, channels, the model's tables of the case)."""
    tape, color, _, _, _ = F.lowered(case)
    w, _, y0, y1 = case[2]
    return tape, color, RW.row_words(tape, w, y0, y1 - y0)


def row_kinds(tape, m):
    """(covered, emptied, mixed): (rows, rectangles per row) booleans over the (row, rectangle) pairs with a pixel and a leaf bit
    in the band's words.  covered: the row's words hold a cover bit the band's do not; emptied: no leaf bit is left and no
    cover bit was set; mixed: leaf bits are left and no cover bit was set."""
    leaf = RW.reduction_bits(tape)
    rows = m['rwords'].shape[0]
    band = m['band'][(np.arange(rows) // m['gh'])[:, None] * m['n_rect'] + np.arange(m['n_rect'])[None, :]]
    busy = ((band & leaf[None, None, :]) != 0).any(axis=2)
    covered = np.zeros(busy.shape, bool)
    for red in tape.cover_plan():
        covered |= RW._bit(m['rwords'], red['bit']) & ~RW._bit(band, red['bit'])
    left = ((m['rwords'] & leaf[None, None, :]) != 0).any(axis=2)
    differs = (m['rwords'] != band).any(axis=2)
    return covered & busy, ~left & ~covered & busy & differs, left & ~covered & busy


def full_rectangles(tape, m):
    """The flagged rectangles (band rectangle numbers) that hold a covered, an emptied and a mixed row."""
    covered, emptied, mixed = row_kinds(tape, m)
    rows, gh, n_rect = m['rwords'].shape[0], m['gh'], m['n_rect']
    out = []
    for r in np.nonzero(m['flagged'])[0]:
        g, t = divmod(int(r), n_rect)
        sl = slice(g * gh, min(rows, (g + 1) * gh))
        if covered[sl, t].any() and emptied[sl, t].any() and mixed[sl, t].any():
            out.append(int(r))
    return out


if __name__ == '__main__':
    import sys
    found = []
    for seed in range(int(sys.argv[1]) if len(sys.argv) > 1 else 0, 400):
        for kind in F.KINDS:
            case = (kind, seed, A if (seed + F.KINDS.index(kind)) % 2 == 0 else B)
            try:
                tape, _, m = model(case)
            except AssertionError:
                continue
            if full_rectangles(tape, m):
                found.append(case)
                print(case, flush=True)
        if len(found) >= 24:
            break

"""Conditions on the cases of tests/cover_fuzz_scenes.py, on the numpy model alone (tests/census_scenes.py, tests/cover_scenes.py,
tests/refine_eval.py): that the soups hold what tests/test_gpu_cover_fuzz.py is there to exercise -- cover bits, bits a census
clears, covered rectangles beside uncovered ones of the same OR, shared and tainted leaves, keys with tables of their own -- so
that the device tests cannot pass on empty scenes.  The thresholds are caps on emptiness, not measurements.  One cross-check of
the model itself: the census's "!= 0 on some pixel", which evaluates a guard's regions only where its geometric bit is set,
against a count over every pixel."""
import numpy as np

import census_scenes as CS
import cover_fuzz_scenes as F
import refine_eval as RE

_model = {}


def model(case, n_vectors=None):
    """(tape, vectors, [tables per vector]) of a case, computed once and never written to."""
    key = (case, n_vectors)
    if key not in _model:
        tape, _, _, vectors, _ = F.lowered(case, n_vectors)
        tabs = [F.tables(tape, case[2], v) for v in vectors]
        for t in tabs:
            for a in t.values():
                a.setflags(write=False)
        _model[key] = (tape, vectors, tabs)
    return _model[key]


def all_cases():
    return [(c, None) for c in F.PLAIN] + [(c, 4) for c in F.PLANTED]


def leaf_words(red, n_words, pick=lambda tainted, eligible: True):
    return F.bit_mask([bit for _, bit, tainted, eligible in red['leaves'] if pick(tainted, eligible)], n_words)


def test_the_table():
    assert len(F.PLAIN) == 12 and len(F.PLANTED) == 8 and len(set(F.PLAIN)) == 12 and len(set(F.PLANTED)) == 8
    for kind, seed, geo in F.PLAIN + F.PLANTED:
        assert kind in F.KINDS and geo in (F.A, F.B)
    for kind in F.KINDS:
        assert sum(c[0] == kind for c in F.PLAIN) == 3 and sum(c[0] == kind for c in F.PLANTED) == 2
    for cases in (F.PLAIN, F.PLANTED):
        assert {c[2] for c in cases} == {F.A, F.B}
    assert F.MANY_KEYS[0] in F.PLANTED and F.MANY_KEYS[1] > 8
    assert F.ENTRY_POINTS in F.PLAIN and F.ENTRY_POINTS in F.PLANTED and F.ENTRY_POINTS[0] == 'one' and F.ENTRY_POINTS[2] == F.A
    assert F.plain(F.PLAIN[0]) == F.plain(F.PLAIN[0]) and F.planted(F.PLANTED[0]) == F.planted(F.PLANTED[0])      # seeded: the same twice


def test_every_case_has_a_cover_bit_and_a_bit_its_census_clears():
    ran = 0
    for case, n in all_cases():
        tape, vectors, tabs = model(case, n)
        assert tape.cover_bits(), case
        for t in tabs:
            assert not (t['census'] & ~t['refined']).any() and (t['refined'] != t['census']).any(), case
        ran += 1
    assert ran == 20


def test_covered_and_partly_covered_cases():
    """At least 40 % of the cases have a covered rectangle; at least 25 % are partial: some rectangle is covered and some rectangle
    that holds a leaf bit of the same OR is not; at least two have two cover bits that both cover somewhere."""
    ran = covered = partial = both = 0
    for case, n in all_cases():
        tape, _, tabs = model(case, n)
        t = tabs[0]
        plan = tape.cover_plan()
        assert t['covered'].shape[1] == len(plan) == len(tape.cover_bits())
        covered += bool(t['covered'].any())
        for j, red in enumerate(plan):
            busy = ((t['census'] & leaf_words(red, t['census'].shape[1])[None, :]) != 0).any(axis=1)
            if t['covered'][:, j].any() and (busy & ~t['covered'][:, j]).any():
                partial += 1
                break
        both += int(t['covered'].any(axis=0).sum() >= 2)
        ran += 1
    assert ran == 20
    assert covered >= 0.40 * ran and partial >= 0.25 * ran and both >= 2, (covered, partial, both)


def test_shared_bits_stay_set_inside_covered_rectangles():
    """In at least two `shared` cases a leaf bit that two reductions share -- not eligible, not tainted -- is set in the third table
    inside a rectangle that its OR covers."""
    ran = stays = 0
    for case, n in all_cases():
        if case[0] != 'shared':
            continue
        tape, _, tabs = model(case, n)
        t = tabs[0]
        hit = False
        for j, red in enumerate(tape.cover_plan()):
            shared = leaf_words(red, t['cover'].shape[1], lambda tainted, eligible: not tainted and not eligible)
            hit = hit or bool((t['cover'][t['covered'][:, j]] & shared[None, :]).any())
        stays += hit
        ran += 1
    assert ran == 5 and stays >= 2, (ran, stays)


def test_planted_cases_have_tainted_leaves_and_a_table_per_key():
    """At least two planted cases have a tainted leaf in cover_plan(); in every one the translation is what the ROW section reads
    and the factor is not, and the third tables of its vectors are pairwise different."""
    ran = tainted = 0
    for case in F.PLANTED:
        tape, vectors, tabs = model(case, 4)
        assert tape.param_count == 3 and tape.info['row_params'] in (1, 3), case        # t (and u, unless its range is one value); never c
        tainted += any(l[2] for red in tape.cover_plan() for l in red['leaves'])
        assert len({t['cover'].tobytes() for t in tabs}) == len(vectors) == 4, case
        assert len({v[:2] for v in vectors}) == 4, case
        ran += 1
    assert ran == 8 and tainted >= 2, tainted


def test_more_keys_than_kept_sets():
    case, n = F.MANY_KEYS
    tape, vectors, tabs = model(case, n)
    assert len(vectors) == n and vectors[:4] == model(case, 4)[1]
    assert len({t['cover'].tobytes() for t in tabs}) == n and len({t['census'].tobytes() for t in tabs}) == n and len({t['refined'].tobytes() for t in tabs}) == n
    # no table of one key is any table of another
    every = [t[k].tobytes() for t in tabs for k in ('refined', 'census', 'cover')]
    assert len({(i // 3, b) for i, b in enumerate(every)}) == len(set(every))


def test_nonzero_per_rectangle_agrees_with_a_count_over_every_pixel():
    """refine_eval.nonzero_per_rectangle(..., only=geo) -- what census_scenes.words clears bits by -- against
    census_scenes.nonzero_counts(...) > 0, which evaluates every pixel, wherever geo is set; every case, its first vector."""
    ran = 0
    for case, n in all_cases():
        tape, vectors, _ = model(case, n)
        w, _, y0, y1 = case[2]
        _, _, gw, gh = tape.guard_layout()
        geo, _, _ = RE.guard_bits(tape, w, y0, y1 - y0, gw, gh, params=vectors[0])
        exact = RE.nonzero_per_rectangle(tape, w, y0, y1 - y0, gw, gh, params=vectors[0], only=geo)
        counts = CS.nonzero_counts(tape, w, y0, y1 - y0, params=vectors[0])
        assert geo.any() and np.array_equal(exact[geo], (counts > 0)[geo]), case
        ran += 1
    assert ran == 20

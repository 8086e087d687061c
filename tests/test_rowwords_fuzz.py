"""The row words' fuzz, on the model alone (tests/rowwords_fuzz_scenes.py): no case of tests/test_gpu_rowwords_fuzz.py is
empty.  Every one of the twenty soups gets a row flag and has a flagged rectangle that holds a covered row, an emptied row and
a mixed row at once; the cases are distinct and cover the four kinds of soup and both geometries."""
import numpy as np
import pytest

import cover_fuzz_scenes as F
import rowwords_fuzz_scenes as RF
import rowwords_scenes as RW


def test_the_table_of_cases():
    assert len(RF.CASES) == len(set(RF.CASES)) == 20
    for kind in F.KINDS:
        mine = [c for c in RF.CASES if c[0] == kind]
        assert len(mine) == 5 and {c[2] for c in mine} == {F.A, F.B}, kind


@pytest.mark.parametrize('case', RF.CASES, ids=lambda c: '%s-%d-%d' % (c[0], c[1], c[2][0]))
def test_no_case_is_empty(case):
    tape, _, m = RF.model(case)
    assert tape.rowwords_flag() >= 0 and tape.cover_bits()
    full = RF.full_rectangles(tape, m)
    assert full, case
    covered, emptied, mixed = RF.row_kinds(tape, m)
    assert not (covered & emptied).any() and not (covered & mixed).any() and not (emptied & mixed).any()
    # the flagged rectangles' rows are what a launch reads: some differ from the band's words, and the flag is in no row word
    sel = RW.flagged_rows(m)
    flag = tape.rowwords_flag()
    assert sel.any() and not RW._bit(m['rwords'], flag).any() and RW._bit(m['xbits'], flag).sum() == m['flagged'].sum()
    assert m['changed'].sum(axis=1)[m['flagged']].min() >= max(1, m['gh'] // 4) > m['changed'].sum(axis=1)[~m['flagged']].max(initial=0)

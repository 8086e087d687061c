"""The REFINE section of the lowering (include/maray_tape.h, maray_refine), on the CPU.

A guard's second bound may clear the guard's bit for a rectangle only if the guarded conjunction is +0.0 on every pixel of
it.  tests/refine_eval.py evaluates the ROW section's guards and the REFINE section per rectangle the way maray_jit_rows and
maray_jit_refine do, and every guarded conjunction per pixel; the sine is the platform libm's, which is the oracle's and,
bit for bit, the device's.
"""
import os

import numpy as np
import pytest

import maray_amd as M
import refine_eval as RE
import refine_scenes as RS
import row_reuse_scenes as RR
from marayb import encode
from conftest import GOLDEN

GW = 64


def lowered(kind, seed=0):
    if kind == 'shared_bound':
        return M.Scene(encode((RS.W, RS.H), RS.shared_bound())).lower()
    return M.Scene(RS.data(kind, seed)).lower()


def as_read(tape, bits):
    """The bits as the kernels read them: a guard without a bit of its own is the OR of its members' (and the numpy model of
    which guards those are agrees with the library's layout)."""
    members = RE.derived_members(tape)
    assert sorted(members) == np.nonzero(tape.guard_layout()[0] < 0)[0].tolist()
    return RE.effective(bits, members)


def leaves(tape):
    """The guards that have a bit of their own (jit_guard_plan): the ones a second bound can clear."""
    return tape.guard_layout()[0] >= 0


@pytest.mark.parametrize('gh', [8, 32])
@pytest.mark.parametrize('kind', RS.KINDS + ('shared_bound',))
def test_no_pixel_of_a_cleared_rectangle_is_set(kind, gh):
    """Every pixel, every guarded region (a shape's, and a group's: its guard is read as the OR of its members' bits), seeds 0
    and 1: value != 0 => the refined bit of the pixel's rectangle is set; and the refined bits are a subset of the geometric
    ones.  shared_bound: several shapes behind one geometric bound, one of them skipped only through their group."""
    cleared = 0
    for seed in (0, 1):
        tape = lowered(kind, seed)
        assert tape.refine.n_ops and tape.refine.n_outs, (kind, seed)
        geo, second, has = RE.guard_bits(tape, RS.W, 0, RS.H, GW, gh)
        refined = geo & second
        assert not (refined & ~geo).any()
        assert not (~second[:, ~has]).any()             # a guard without a second bound keeps its bit
        exact = RE.nonzero_per_rectangle(tape, RS.W, 0, RS.H, GW, gh)
        assert exact.any()
        bad = exact & ~as_read(tape, refined)
        assert not bad.any(), (kind, seed, np.argwhere(bad)[:8].tolist())
        cleared += int((geo & ~refined).sum())
    if kind == 'short':
        assert cleared == 0                             # a rectangle spans whole periods: nothing may be decided
    elif kind in ('long', 'zero', 'huge', 'yonly', 'slanted'):
        assert cleared > 0, kind                        # ... and these must not be vacuous


def test_chess_1024_bands_where_the_geometric_bit_is_set():
    """The committed chess at 1024^2, every 32-row band -- narrower than "every pixel and leaf": on the pixels of every
    rectangle whose geometric bit is set, a leaf or a group that is != 0 somewhere has its refined bit.  (Where the
    geometric bit is clear the refined one is too, and the leaf is 0 there by the ROW section's own guard, which the rectangle renders of test_lowering.py hold against the oracle.)"""
    tape = M.Scene(open(os.path.join(GOLDEN, 'chess.maray'), 'rb').read()).lower()
    geo, second, has = RE.guard_bits(tape, 1024, 0, 1024, GW, 32)
    refined = geo & second
    assert has[tape.guard_layout()[0] >= 0].sum() >= 100 and not (refined & ~geo).any()
    exact = RE.nonzero_per_rectangle(tape, 1024, 0, 1024, GW, 32, only=as_read(tape, geo))
    assert exact.any() and not (exact & ~as_read(tape, refined)).any()
    assert (geo & ~refined).sum() > 0


def test_chess_4096_keeps_at_most_four_fifths_of_the_bits():
    """The flagship frame: refined bits <= 0.80 x geometric bits, over every guard that has a bit -- the 128 leaves and one
    group that keeps a bit of its own, which no second bound clears (the census on the true range of each sine's argument
    gave 0.74 over the leaves; measured here: 0.760, 3,072 of 4,040; over the leaves alone 3,029 of 3,997, 0.758)."""
    s = M.Scene(open(os.path.join(GOLDEN, 'chess.maray'), 'rb').read())
    s.rescale(4, 4)
    tape = s.lower()
    pos, n_words, gw, gh = tape.guard_layout()
    assert (gw, gh) == (64, 32)
    geo, second, has = RE.guard_bits(tape, 4096, 0, 4096, gw, gh)
    leaf = pos >= 0
    n_geo, n_ref = int(geo[:, leaf].sum()), int((geo & second)[:, leaf].sum())
    print('chess @4096^2: geometric bits %d, refined bits %d, ratio %.4f' % (n_geo, n_ref, n_ref / n_geo))
    assert n_ref <= 0.80 * n_geo


def test_a_program_without_step_sin_has_no_section_and_no_source():
    _, tape = RR.lowered(RR.plain())
    assert tape.refine.n_ops == 0 and tape.refine.n_outs == 0 and tape.refine_arrays() is None
    assert tape.jit_source_refine == ''
    assert tape.jit_build_refine() == b''
    # ... and one whose only sine has no proven range (a parameter of any value) has none either
    _, tape = RR.lowered(RR.sines())
    assert tape.refine.n_ops == 0 and tape.jit_source_refine == ''


def test_the_section_reads_no_coordinate_and_only_row_read_parameters():
    import tape_eval as TE
    for kind in ('mixed', 'square'):
        tape = lowered(kind)
        consts, ops, n_slots = tape.refine_arrays()
        n_ynum = RE.n_numeric(tape)
        outs = set()
        for ins in ops:
            op, aux, dst, ra, rb = TE.decode(ins)
            if op == TE.OP['OUT']:
                assert aux >= n_ynum and aux not in outs
                outs.add(aux)
            for r in ([ra, rb] if TE.OP['ADD'] <= op <= TE.OP['APP'] else [ra]):
                assert r >> 14 != TE.K_YVAL and not (r >> 14 == TE.K_SPEC and (r & 0x3FFF) in (0, 1)), 'reads X, Y or a y value'
        assert len(outs) == tape.refine.n_outs
        src = tape.jit_source_refine
        assert 'maray_jit_refine' in src and 'maray_jit_rows' not in src

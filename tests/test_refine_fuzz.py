"""The second bounds of Step(Sin) factors on the seeded scenes of tests/refine_fuzz_scenes.py, on the CPU.

The claim is that of tests/test_refine_bounds.py -- a guarded conjunction that is != 0 on some pixel of a rectangle has its
refined bit set there, the refined bits are a subset of the geometric ones, a guard without a second bound keeps its bit --
on every case of the committed list, at guard heights 8 and 32 (1 where the guards read Y), under every value vector of a
parameterised scene and on the k-times sample grid of a supersampled one.  The tests below it hold, kind by kind, what keeps
the claim from being empty: rectangles cleared at spans just under the rule's width 3, rectangles KEPT at spans just over pi
whose corners both have a negative sine round a whole positive half-wave (what a width above pi would clear), slits in a
rectangle's corner column or row beside a cleared neighbour, rectangles cleared through NOT, a weighted threshold and a
product, no second bound where there must be none.  A seed that fails a condition is replaced in the case list."""
import functools

import numpy as np
import pytest

import refine_eval as RE
import refine_fuzz_scenes as F
import tape_eval as TE



@functools.lru_cache(maxsize=None)
def lowered(case):
    return F.lowered(case)


@functools.lru_cache(maxsize=None)
def shapes_of(case):
    """{guard: shape} of a case that is not supersampled (under the vector whose colour scale is 1)."""
    tape, made = lowered(case)
    w, y0, rows = F.sample_geo(case)
    v = made.vectors[2] if made.form == 'colour' else made.vectors[0]
    return F.guard_shapes(tape, w, y0, rows, params=v)


def heights(tape):
    gh = tape.guard_layout()[3]
    return (1,) if gh == 1 else (8, 32)


@functools.lru_cache(maxsize=None)
def examined(case, gh, vi):
    tape, made = lowered(case)
    w, y0, rows = F.sample_geo(case)
    return F.examine(tape, case, gh, made.vectors[vi], gw=tape.guard_layout()[2], full=case[0] != 'many')      # `many` (126 guards on 1100 x 200): the pixels of the rectangles whose geometric bit is set


def leaves(tape):
    return tape.guard_layout()[0] >= 0


def cleared(e, tape):
    return e['geo'] & ~e['refined'] & leaves(tape)[None, :]


def cases(kind, plain=False):
    return [c for c in F.CASES if c[0] == kind and (c[3] == 1 or not plain)]


def test_the_case_list():
    assert len(F.CASES) == len(set(F.CASES)) >= 38 and {c[0] for c in F.CASES} == set(F.KINDS)
    assert {c[2] for c in F.CASES} == {F.G320, F.G449, F.G449R, F.G1100}
    for kind in ('near3', 'edge', 'arith'):
        assert {c[3] for c in cases(kind)} == {1, 2, 4}


def test_a_case_launches_more_than_two_blocks_of_the_pass():
    """maray_jit_refine takes one work-item per rectangle, ROW_BLOCK (jit_parts.hpp, read by regex) to a block.  With the layouts
    the library gives these tapes -- 64 x 32, or 256 x 1 where the guards read Y -- every other case is one block (1100 x 200 is
    140 rectangles of 64 x 32; at a guard height of 8 it would be 500, still under two blocks); the blinds-like `rows` case on
    1100 x 200 is 1000: three full blocks and a partial one, with second bounds that clear bits in each of them."""
    rb = F.row_block()
    big = [c for c in F.CASES if F.refine_items(lowered(c)[0], c) > 2 * rb]
    assert big == [('rows', 7, F.G1100, 1)]
    tape, made = lowered(big[0])
    assert made.blinds and tape.refine.n_outs and tape.guard_layout()[2:] == (256, 1)
    items = F.refine_items(tape, big[0])
    assert items == 1000 and items % rb
    cl = cleared(examined(big[0], 1, 0), tape).any(axis=1)
    per_block = [int(cl[i:i + rb].sum()) for i in range(0, items, rb)]
    print('blocks: %d work-items, rectangles with a cleared bit per block of %d: %s' % (items, rb, per_block))
    assert len(per_block) == 4 and all(per_block)


@pytest.mark.parametrize('case', F.CASES, ids=lambda c: '%s-%d-%dx%d-%d-k%d' % (c[0], c[1], c[2][0], c[2][1], c[2][2], c[3]))
def test_no_pixel_of_a_cleared_rectangle_is_set(case):
    tape, made = lowered(case)
    n_cleared, n_rect = 0, 0
    for gh in heights(tape):
        for vi, v in enumerate(made.vectors):
            e = examined(case, gh, vi)
            assert not (e['refined'] & ~e['geo']).any()
            assert not (~e['second'][:, ~e['has']]).any()                  # a guard without a second bound keeps its bit
            assert e['exact'].any(), (case, gh, v)
            assert not e['bad'].any(), (case, gh, v, np.argwhere(e['bad'])[:8].tolist())
            n_cleared += int(cleared(e, tape).sum())
            n_rect += e['geo'].shape[0]
    print('refine-fuzz (cpu): %s seed %d %dx%d rows %d-%d k=%d: %d rectangles, %d bits cleared' % (case[:2] + case[2] + (case[3], n_rect, n_cleared)))


# ---- the conditions, kind by kind --------------------------------------------------------------------------------------------
def by_tag(kind, tags, what=cleared):
    """Bits cleared in the plain cases of a kind on the guards of shapes with one of `tags`, per guard height."""
    out = {}
    for case in cases(kind, plain=True):
        tape, made = lowered(case)
        for gh in heights(tape):
            for vi in range(len(made.vectors)):
                c = what(examined(case, gh, vi), tape)
                for g, n in shapes_of(case).items():
                    if made.recs[n]['tag'] in tags:
                        out[gh] = out.get(gh, 0) + int(c[:, g].sum())
    return out


def test_near3_clears_under_3_and_keeps_the_humps():
    """Per guard height: rectangles cleared whose span |A| 63 + |B| (gh - 1) is in [2.5, 3), and "humps": span in (pi, 3.4],
    the sine of the generator's own f negative at both corners the bound is taken at, the conjunction != 0 on some pixel,
    the bit kept.  A rule whose width were above pi clears the humps whose span is under that width."""
    total = {}
    for case in cases('near3', plain=True):
        tape, made = lowered(case)
        for gh in heights(tape):
            near, hump, hump33 = F.near3_counts(examined(case, gh, 0), tape, made, shapes_of(case))
            t = total.setdefault(gh, dict(near=0, hump=0, hump_under_3_3=0))
            t['near'], t['hump'], t['hump_under_3_3'] = t['near'] + near, t['hump'] + hump, t['hump_under_3_3'] + hump33
    print('near3:', total)
    for gh in (8, 32):
        assert total[gh]['near'] > 0 and total[gh]['hump'] > 0 and total[gh]['hump_under_3_3'] > 0, (gh, total)


def test_edge_slits_in_a_corner_column_or_row_beside_a_cleared_rectangle():
    """For every placement: a slit one column (row) wide that is the first or the last of its rectangle, kept and != 0 there,
    while a rectangle beside it -- same row of rectangles (same column) -- is cleared for the same guard."""
    seen = {}
    for case in cases('edge', plain=True):
        tape, made = lowered(case)
        w, h, y0, y1 = case[2]
        for gh in heights(tape):
            e = examined(case, gh, 0)
            cl = cleared(e, tape)
            n_rect = e['n_rect']
            for g, n in shapes_of(case).items():
                rec = made.recs[n]
                if rec['form'] != 'slit' or not leaves(tape)[g]:
                    continue
                at = rec['at']
                here = (e['ylo'] <= at) & (at <= e['yhi']) if rec['in_y'] else (e['xlo'] <= at) & (at <= e['xhi']) & (np.arange(len(cl)) % n_rect == at // F.GW)
                for r in np.nonzero(here & e['exact'][:, g] & e['refined'][:, g])[0]:
                    lo, hi, step_ = (e['ylo'][r], e['yhi'][r], n_rect) if rec['in_y'] else (e['xlo'][r], e['xhi'][r], 1)
                    beside = [o for o in (r - step_, r + step_) if 0 <= o < len(cl) and (rec['in_y'] or o // n_rect == r // n_rect) and cl[o, g]]
                    if at in (lo, hi) and beside:
                        seen[(rec['tag'], gh)] = seen.get((rec['tag'], gh), 0) + 1
    print('edge:', seen)
    for place in F.EDGE_PLACEMENTS:
        for gh in (8, 32):
            assert seen.get((place, gh), 0) > 0, (place, gh, seen)


def test_arith_clears_through_not_thresholds_and_product():
    got = {name: by_tag('arith', tags) for name, tags in (('not', ('not', 'negstep')), ('thresholds', ('sum', 'weighted')), ('product', ('product',)),
                                                            ('nest', ('nest',)), ('plain_bool', ('plain_bool',)))}
    print('arith:', got)
    for name in ('not', 'thresholds', 'product'):
        for gh in (8, 32):
            assert got[name].get(gh, 0) > 0, (name, got)
    for tag in ('not', 'negstep', 'sum', 'weighted', 'product'):
        assert sum(by_tag('arith', (tag,)).values()) > 0, tag


def no_bound(kind, tags):
    """The guards of the shapes with one of `tags` have no second bound; how many such guards the plain cases hold."""
    n = 0
    for case in cases(kind, plain=True):
        tape, made = lowered(case)
        has = examined(case, heights(tape)[0], 0)['has']
        for g, s in shapes_of(case).items():
            if made.recs[s]['tag'] in tags:
                assert not has[g], (case, g, made.recs[s]['tag'])
                n += 1
    return n


def test_offset_under_the_limit_clears_and_over_it_has_no_bound():
    under = by_tag('offset', ('under', 'under_neg', 'log_under'))
    print('offset:', under, {t: sum(by_tag('offset', (t,)).values()) for t in ('under', 'under_neg', 'log_under')})
    assert all(under.get(gh, 0) > 0 for gh in (8, 32))
    assert sum(by_tag('offset', ('under',)).values()) > 0 and sum(by_tag('offset', ('under_neg',)).values()) > 0
    assert no_bound('offset', ('over', 'over_domain', 'log_over')) >= 8
    assert sum(by_tag('offset', ('over', 'over_domain', 'log_over')).values()) == 0


def test_nonaffine_clears_on_the_interval_path_and_sqrt_has_no_bound():
    got = {t: sum(by_tag('nonaffine', (t,)).values()) for t in F.NONAFFINE}
    print('nonaffine:', got)
    for t in ('square', 'square_corner', 'xy', 'abs', 'min', 'max'):
        assert got[t] > 0, (t, got)
    assert no_bound('nonaffine', ('sqrt',)) >= 2 and got['sqrt'] == 0


def section_params(tape):
    """The parameters the REFINE section reads."""
    ref = tape.refine_arrays()
    out = set()
    if ref is not None:
        for ins in ref[1]:
            op, aux, dst, ra, rb = TE.decode(ins)
            for r in ([ra, rb] if TE.OP['ADD'] <= op <= TE.OP['APP'] else [ra]):
                if r >> 14 == TE.K_SPEC and (r & 0x3FFF) >= 7:
                    out.add((r & 0x3FFF) - 7)
    return out


def test_param_the_section_reads_row_read_parameters_only():
    """offset: the section reads t, clears rectangles under at least two vectors, and the vectors' word tables differ pairwise.
    colour, phase: the parameter is read by PIXEL ops alone, the guards of the shapes it touches have no second bound, the
    others clear.  frequency: a parameter times x has no second bound (RowBounds::ival gives the product no ends): `has` is false
    for its guards and nothing is cleared; a lowering that learns to bound it has to bring the conditions that it clears soundly."""
    forms = set()
    for case in cases('param'):
        tape, made = lowered(case)
        forms.add(made.form)
        row_params = tape.info['row_params']
        assert all((row_params >> p) & 1 for p in section_params(tape)), case
        pos, n_words, gw, _ = tape.guard_layout()
        tables = [RE.pack_words(examined(case, 32, vi)['refined'], pos, n_words).tobytes() for vi in range(len(made.vectors))]
        n_cl = [int(cleared(examined(case, 32, vi), tape).sum()) for vi in range(len(made.vectors))]
        print('param: %s seed %d: bits cleared per vector %s, %d different tables, section reads %s' % (made.form, case[1], n_cl, len(set(tables)), sorted(section_params(tape))))
        assert 4 <= len(made.vectors) <= 5
        for (_, lo, hi), column in zip(made.decl, zip(*made.vectors)):
            assert lo in column and hi in column                            # a vector at each end of the declared range
        if made.form == 'offset':
            assert row_params == 1 and section_params(tape) == {0}
            assert sum(n > 0 for n in n_cl) >= 2 and len(set(tables)) == len(tables)
        if made.form in ('colour', 'phase'):
            assert row_params == 0 and not section_params(tape), case
            assert len(set(tables)) == 1 and n_cl[0] > 0
        if made.form == 'frequency':
            assert not tape.refine.n_outs and not any(n_cl) and not any(examined(case, gh, 0)['has'].any() for gh in (8, 32)), case
    assert forms == set(F.PARAM_FORMS)
    assert no_bound('param', ('colour', 'phase')) >= 6 and no_bound('param', ('frequency',)) >= 8


def test_many_two_words_and_bytes_with_both_kinds_of_bit():
    for case in cases('many'):
        tape, made = lowered(case)
        assert len(made.shapes) >= 70
        pos, n_words, gw, gh = tape.guard_layout()
        assert n_words >= 2 and (gw, gh) == (64, 32)
        e = examined(case, 32, 0)
        has = e['has']
        mixed = [b for b in range(8 * n_words) if len({bool(has[g]) for g in np.nonzero(pos // 8 == b)[0]}) == 2]
        second_word = int(cleared(e, tape)[:, pos >= 64].sum())
        print('many: seed %d: %d guards in %d words, %d with a second bound, bytes with both kinds %s, %d bits cleared in the second word' %
              (case[1], len(pos), n_words, int(has.sum()), mixed, second_word))
        assert mixed and [b for b in mixed if b >= 8] and second_word > 0
    assert no_bound('many', ('over', 'sqrt')) >= 8


def test_rows_guards_that_read_y():
    """y_spans=False: every guard reads Y and the lowering builds no REFINE section (build_refine runs under y spans only): the
    bits stay geometric.  The blinds-like scenes under the default lowering: rectangles of 256 x 1 with second bounds that clear."""
    n_cleared = 0
    for case in cases('rows'):
        tape, made = lowered(case)
        n_guards, n_read_y = TE.guards_reading_y(tape)
        assert n_read_y == n_guards > 0 and tape.guard_layout()[2:] == (256, 1), case
        e = examined(case, 1, 0)
        if made.blinds:
            assert tape.refine.n_outs and e['has'].any()
            n_cleared += int(cleared(e, tape).sum())
        else:
            assert tape.refine.n_ops == 0 and not e['has'].any() and np.array_equal(e['refined'], e['geo'])
    print('rows: %d bits cleared in rectangles of one row' % n_cleared)
    assert n_cleared > 0

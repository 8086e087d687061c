"""The walks of tests/walk_scenes.py without a GPU: the plain model of the policy (PolicyModel) against the policy itself
(maray_amd/csrc/row_reuse.hpp, driven launch by launch by tests/native/row_reuse_walk.cpp under AddressSanitizer and UBSan), for every
committed walk and every budget tests/test_gpu_walks.py runs it under; the conditions that keep the walks from being empty; and,
on the numpy models alone, that the tables of two keys of one walk differ -- which is what makes "the launch read its own key's
table" a check at all."""
import os
import subprocess

import pytest

import walk_scenes as WS
from conftest import ROOT


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('walk') / 'row_reuse_walk')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-I' + os.path.join(ROOT, 'maray_amd', 'csrc'), '-I' + os.path.join(ROOT, 'include'),
                           os.path.join(ROOT, 'tests', 'native', 'row_reuse_walk.cpp'), '-o', out])
    return out


def cases():
    """(name, steps, pool, budget, reuse) of everything tests/test_gpu_walks.py runs."""
    out = []
    for name in WS.WALKS:
        P, steps = WS.program(name), WS.steps_of(name)
        out += [(name, steps, P['pool'], b, True) for b in WS.budgets(name)]
    out.append(('plain', WS.steps_of('plain'), WS.program('plain')['pool'], None, False))
    out.append((WS.MANY[0], WS.many_steps(), WS.program(WS.MANY[0])['many'], None, True))
    return out


def native(exe, facts, steps, pool, budget, reuse):
    m = WS.PolicyModel(facts, budget=budget, reuse=reuse)
    ids, lines = {}, ['%d %d' % (m.max_bytes, reuse)]
    for s in steps:
        for launch, vec, rp in WS.launches_of(s):
            lines.append(m.native_line(launch, pool[vec], rp, ids))
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=1', UBSAN_OPTIONS='print_stacktrace=1')
    out = subprocess.run([exe], input='\n'.join(lines) + '\n', capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    return [tuple(int(v) for v in ln.split()) for ln in out.stdout.split('\n') if ln]


def test_the_model_is_the_policy_line_for_line(exe):
    """Every committed walk under every budget: set, ROW pass, census, cover, scan, order, kept_sets and kept_bytes of every
    launch, the model's against row_reuse.hpp's."""
    n = 0
    for name, steps, pool, budget, reuse in cases():
        facts = WS.program(name)['facts']
        got = native(exe, facts, steps, pool, budget, reuse)
        recs = [r for rs in WS.run(WS.PolicyModel(facts, budget=budget, reuse=reuse), steps, pool) for r in rs]
        want = [(r['set'], r['passes'], r['census'], r['cover'], r['scan'], r['order'], r['kept_sets'], r['kept_bytes']) for r in recs]
        assert len(got) == len(want), (name, budget)
        for i, (a, b) in enumerate(zip(got, want)):
            assert a == b, (name, budget, reuse, i, a, b)
        assert all(r['kept_bytes'] <= (WS.PolicyModel.MAX_BYTES if budget is None else budget) for r in recs)
        n += len(want)
    assert n > 1000


def test_walks_are_walks():
    """At most 48 steps and 14 keys (the walk of many keys: 33 or more, so that the seen-ring wraps), every entry point and every
    geometry of the menu somewhere, pools of at most four vectors of which two differ in what the ROW section reads and, for the
    planted soups, two in c alone; the planted tapes get a row flag."""
    entries, geos = set(), set()
    for name in WS.WALKS:
        P, steps = WS.program(name), WS.steps_of(name)
        assert len(steps) <= WS.MAX_STEPS and len(P['pool']) <= 4
        classes = WS.row_classes(P['facts'], P['pool'])
        keys = {(l, classes[v]) for s in steps for l, v, _ in WS.launches_of(s)}
        assert len(keys) <= WS.MAX_KEYS, name
        assert any(s['geo'] in ('R3', 'R6') for s in steps), name
        entries |= {s['entry'] for s in steps}
        geos |= {s['geo'] for s in steps}
        if name in WS.PLANTED:
            assert P['tape'].rowwords_flag() >= 0 and P['facts']['has_rw'] and P['facts']['n_cover'] >= 1
            assert len(set(classes)) >= 2 and any(classes[i] == classes[j] and P['pool'][i] != P['pool'][j] for i in range(len(classes)) for j in range(i))
            assert {WS.PLANTED[name][0] for name in WS.PLANTED} & {'shared', 'colours'} and 'one' in {k for k, _ in WS.PLANTED.values()}
    assert entries == set(WS.ENTRIES) and geos == set(WS.MENU)
    P, steps = WS.program(WS.MANY[0]), WS.many_steps()
    classes = WS.row_classes(P['facts'], P['many'])
    assert len({(l, classes[v]) for s in steps for l, v, _ in WS.launches_of(s)}) >= 33 and len(steps) <= WS.MAX_STEPS
    assert {s['geo'] for s in steps} == {'R3', 'R6'}


@pytest.fixture(scope='module')
def surveys():
    return {name: WS.survey(name) for name in WS.WALKS}


def test_every_event_occurs(surveys):
    """Over the committed walks and budgets together every event tag of the model occurs at least twice."""
    total = dict.fromkeys(WS.EVENTS, 0)
    for cond, keys, events in surveys.values():
        for k, v in events.items():
            total[k] += v
    P = WS.program(WS.MANY[0])
    for k, v in WS.census_of_events(WS.run(WS.PolicyModel(P['facts']), WS.many_steps(), P['many'])).items():
        total[k] += v
    print(total)
    assert all(v >= 2 for v in total.values()), total


@pytest.mark.parametrize('name', list(WS.PLANTED))
def test_histories_of_the_planted_walks(surveys, name):
    """Under one of its budgets each planted walk has: a take-over in place of a set whose old key has flagged and covered
    rectangles by a key of fewer rectangles per row or fewer groups that has flagged rectangles too and is then found in the set
    three more times, reading the fourth table; a return to an evicted key that is then found three times; a scan refused and
    later a scan admitted in the same set; a K2 step between two R1 or K3 steps of the same values."""
    cond, keys, _ = surveys[name]
    assert cond == dict(takeover=True, back=True, refused_then_admitted=True, k2_between=True), cond
    assert keys['flagged'] >= 3 and keys['unflagged'] >= 1 and keys['covered'] >= 2 and keys['uncovered'] >= 1 and keys['no_order'], keys


@pytest.mark.parametrize('name', [n for n in WS.WALKS if n != 'sines'])
def test_tables_of_two_keys_differ(name):
    """The numpy tables of a walk's keys: refined words and fourth tables differ between any two keys (but K3B and K3R of the same
    values, which are two keys over the same rows: walk_scenes.py), so a launch that read another key's table would be seen."""
    P, steps = WS.program(name), WS.steps_of(name)
    known = WS.Known(name, steps, P['pool'])
    keys = list(known.by_key)
    same_rows = lambda a, b: {known.by_key[a][0], known.by_key[b][0]} == {WS.MENU['K3B'], WS.MENU['K3R']} and a[6:] == b[6:]
    for i, a in enumerate(keys):
        ta = known.tables(a)
        print(name, known.by_key[a], 'covered' if ta['covered'].any() else '-', 'flagged' if ta['flagged'].any() else '-')
        for b in keys[:i]:
            if same_rows(a, b):
                continue
            tb = known.tables(b)
            assert ta['refined'].tobytes() != tb['refined'].tobytes(), (a, b)
            if 'xbits' in ta and 'xbits' in tb:
                assert ta['xbits'].tobytes() != tb['xbits'].tobytes(), (a, b)

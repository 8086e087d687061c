"""The guard census and the cover of guarded ORs on the device, on random soups (tests/cover_fuzz_scenes.py): the words
every launch read -- the refined words, what the census left of them, the third table with cover bits -- against the numpy model
(tests/census_scenes.py, tests/cover_scenes.py) bit for bit, and every raster against the oracle's render of the scene (with the
values substituted: tests/params.py), RGB8 byte for byte and f64 planes bit for bit.  tests/test_cover_fuzz.py holds the conditions
that keep these cases from being empty.

Every test body runs in a child process with a time limit of its own; nothing follows a failure inside one.  A child prints one
line per case, `cover-fuzz: ...`, with the rectangles that had a cover bit on the device; the test prints them again."""
import os
import subprocess
import sys

import numpy as np
import pytest

import maray_amd as M
import cover_fuzz_scenes as F
import params as PR

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

_CHILD = r"""
import sys
sys.path[:0] = [%(root)r, %(tests)r]
%(first)s
import test_gpu_cover_fuzz as T
T.%(call)s
print('child ok')
"""


def _run(call, timeout, torch_first=False):
    code = _CHILD % dict(root=ROOT, tests=HERE, call=call, first='import torch' if torch_first else '')
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0 and out.stdout.strip().endswith('child ok'), (out.stdout[-2000:], out.stderr[-4000:])
    lines = [ln for ln in out.stdout.split('\n') if ln.startswith('cover-fuzz:')]
    print('\n'.join(lines))
    return lines


def contexts(tapes, census=True, samples=0):
    """MARAY_BACKEND_JIT contexts of several tapes, eight builds side by side (as tests/test_gpu_fuzz_params.py), the knobs set
    around their creation (they are read when a context is created): census=False: MARAY_JIT_GUARD_CENSUS=0."""
    from concurrent.futures import ThreadPoolExecutor
    want = {'MARAY_JIT_GUARD_CENSUS': '1' if census else '0', 'MARAY_JIT_GUARD_COVER': '1', 'MARAY_JIT_ROW_REUSE': '1'}
    old = {k: os.environ.get(k) for k in want}
    os.environ.update(want)
    try:
        with ThreadPoolExecutor(8) as pool:
            return list(pool.map(lambda t: M.Context(t, backend=M.BACKEND_JIT, samples=samples), tapes))
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def oracle(color, decl, values, geo, want_f64=True):
    """The oracle's (rgb8, f64 planes) of the rows of `geo`, the values substituted exactly."""
    from marayb import encode
    from oracle_ffi import Scene as OScene
    w, h, y0, y1 = geo
    if decl:
        color = PR.substituted_exact(color, [i for i, _, _ in decl], values)
    return OScene(encode((w, h), color)).render_rows(w, h, y0, y1, threads=min(16, os.cpu_count() or 1), want_f64=want_f64)


def launch(ctx, geo, want, values=None, want_f64=True, what=None):
    """One render_rows of the rows of `geo`, against the oracle's frame `want`."""
    w, h, y0, y1 = geo
    if values is not None:
        ctx.set_params(list(values))
    got8, got64 = ctx.render_rows(w, h, y0, y1, want_f64=want_f64)
    assert np.array_equal(got8, want[0]), (what, values, 'rgb8')
    if want_f64:
        assert PR.same_f64(got64, want[1]), (what, values, 'f64')


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b)


def covered_on_device(tape, words):
    """Rectangles in which the words the last launch read have a cover bit."""
    mask = F.bit_mask(tape.cover_bits(), words.shape[1])
    return int(((words & mask[None, :]) != 0).any(axis=1).sum())


def three_launches(ctx, tape, geo, want, tabs, values, counts, what):
    """The first three launches of a key no set holds, the waiting accessor between them: the refined words, the census'd words,
    the third table; counts = (census_count, cover_count) before them."""
    for i in range(3):
        launch(ctx, geo, want, values, what=(what, i))
        # (the accessors wait for the context's work: the count of the second launch's cover has arrived by the third)
        assert same(ctx.debug_census_words(), tabs['census'] if i else tabs['refined']), (what, i)
        assert (ctx.census_count, ctx.cover_count) == ((counts[0] + 1, counts[1] + 1) if i else counts), (what, i)
    got = ctx.debug_cover_words()
    assert same(got, tabs['cover']), (what, int(tabs['covered'].sum()), [(hex(int(a)), hex(int(b))) for a, b in zip(got.reshape(-1), tabs['cover'].reshape(-1)) if a != b][:8])
    assert same(ctx.debug_census_words(), tabs['census']) and same(ctx.debug_guard_words(), tabs['refined']), what
    assert covered_on_device(tape, got) == int(tabs['covered'].any(axis=1).sum()), what


# ---- a. plain soups: words and rasters ---------------------------------------------------------------------------------------
def child_plain(kind):
    cases = [c for c in F.PLAIN if c[0] == kind]
    made = [F.lowered(c) for c in cases]
    on = contexts([m[0] for m in made])
    off = contexts([m[0] for m in made], census=False)
    ran = 0
    for case, (tape, color, _, _, _), a, b in zip(cases, made, on, off):
        geo = case[2]
        tabs, want = F.tables(tape, geo), oracle(color, None, None, geo)
        three_launches(a, tape, geo, want, tabs, None, (0, 0), case)
        launch(a, geo, want, want_f64=False, what=(case, 'four pixels per lane'))
        assert same(a.debug_cover_words(), tabs['cover']) and (a.census_count, a.cover_count) == (1, 1), case
        assert same(a.debug_guard_words(), tabs['refined']), case
        for i in range(4):
            launch(b, geo, want, want_f64=i < 3, what=(case, 'no census', i))
        assert (b.census_count, b.cover_count) == (0, 0), case
        assert same(b.debug_cover_words(), tabs['refined']) and same(b.debug_census_words(), tabs['refined']) and same(b.debug_guard_words(), tabs['refined']), case
        print('cover-fuzz: plain %s seed %d %dx%d rows %d-%d: %d of %d rectangles covered on the device' %
              (case[0], case[1], geo[0], geo[1], geo[2], geo[3], covered_on_device(tape, a.debug_cover_words()), tabs['cover'].shape[0]))
        a.close()
        b.close()
        ran += 1
    assert ran == 3


@pytest.mark.parametrize('kind', F.KINDS)
def test_plain_soups_words_and_rasters(kind):
    """Three soups of a kind: four launches on a context with the knobs on (after the first the refined words, after the second the
    census'd ones, after the third the third table; the fourth without f64 planes, four pixels per lane) and four on one created
    with MARAY_JIT_GUARD_CENSUS=0, every raster the oracle's."""
    assert len(_run('child_plain(%r)' % kind, 600)) == 3


# ---- b. planted soups: a table per key ---------------------------------------------------------------------------------------
def child_planted(kind):
    cases = [c for c in F.PLANTED if c[0] == kind]
    made = [F.lowered(c, 4) for c in cases]
    on = contexts([m[0] for m in made])
    ran = 0
    for case, (tape, color, decl, vectors, other), ctx in zip(cases, made, on):
        geo = case[2]
        v0, v1 = vectors[0], vectors[1]
        v0p = v0[:2] + (other,)
        assert v0p != v0 and v0p[:2] == v0[:2]
        tabs = {v: F.tables(tape, geo, v) for v in (v0, v1)}
        tabs[v0p] = tabs[v0]                                            # c is read by PIXEL ops only: the same key, the same tables
        want = {v: oracle(color, decl, v, geo) for v in (v0, v1, v0p)}
        three = lambda v: [tabs[v][k] for k in ('refined', 'census', 'cover')]

        def one_of_its_own(v, what):
            launch(ctx, geo, want[v], v, what=what)
            got = ctx.debug_cover_words()
            assert any(same(got, t) for t in three(v)), what

        def exactly_the_third(v, what):
            before = (ctx.census_count, ctx.cover_count, ctx.launch_counts[0])
            launch(ctx, geo, want[v], v, what=what)
            assert same(ctx.debug_cover_words(), tabs[v]['cover']) and same(ctx.debug_census_words(), tabs[v]['census']), what
            assert (ctx.census_count, ctx.cover_count, ctx.launch_counts[0]) == before, what     # no ROW pass, no census, no cover

        # v0 v0 v0 v1 v1 v1: a key no set holds, three times each
        three_launches(ctx, tape, geo, want[v0], tabs[v0], v0, (0, 0), (case, 'v0'))
        three_launches(ctx, tape, geo, want[v1], tabs[v1], v1, (1, 1), (case, 'v1'))
        # v0 v0': v1 took the scratch set that held v0 (a key gets a set of its own when it comes a second time: row_reuse.hpp),
        # so these two read v0's tables as they are made again -- one of v0's three, never one of v1's
        one_of_its_own(v0, (case, 'v0 again'))
        one_of_its_own(v0p, (case, "v0'"))
        for i in range(2):
            one_of_its_own(v0, (case, 'v0 in its own set', i))
        # now both keys are held: every return reads the key's third table, and nothing is made again
        exactly_the_third(v0, (case, 'v0 held'))
        for i in range(3):
            one_of_its_own(v1, (case, 'v1 again', i))
        exactly_the_third(v1, (case, 'v1 held'))
        exactly_the_third(v0, (case, 'the return to v0'))
        exactly_the_third(v0p, (case, "v0' keeps counts and tables"))
        exactly_the_third(v1, (case, 'the return to v1'))
        print('cover-fuzz: planted %s seed %d %dx%d rows %d-%d: %s of %d rectangles covered on the device (v0, v1)' %
              (case[0], case[1], geo[0], geo[1], geo[2], geo[3], [int(tabs[v]['covered'].any(axis=1).sum()) for v in (v0, v1)], tabs[v0]['cover'].shape[0]))
        ctx.close()
        ran += 1
    assert ran == 2


@pytest.mark.parametrize('kind', F.KINDS)
def test_planted_soups_a_table_per_key(kind):
    """Two soups of a kind with a ROW-read translation (t, u) and a PIXEL-read factor c, one context each, launched v0 v0 v0 v1 v1
    v1 v0 v0' (v0' = v0 with another c) and on: words per key as for the plain soups; the seventh and eighth launch find v0's set
    taken by v1 and read one of v0's own three tables while they are made again; once both keys are held a return to v0 reads
    v0's third table with no ROW pass, census or cover enqueued, and v0' keeps both counts and tables.  Every raster is the
    oracle's frame of its values."""
    assert len(_run('child_planted(%r)' % kind, 600)) == 2


# ---- c. more keys than kept sets ---------------------------------------------------------------------------------------------
def child_many_keys():
    case, n = F.MANY_KEYS
    tape, color, decl, vectors, _ = F.lowered(case, n)
    geo = case[2]
    assert len(vectors) == n == 10
    tabs = [F.tables(tape, geo, v) for v in vectors]
    want = [oracle(color, decl, v, geo) for v in vectors]
    own = [[t[k].tobytes() for k in ('refined', 'census', 'cover')] for t in tabs]
    assert len({b for o in own for b in o}) >= 2 * n and all(not (set(own[i]) & set(own[j])) for i in range(n) for j in range(i))
    ctx, = contexts([tape])
    for rnd in range(4):                    # no accessor: a count that arrives late is legal, rasters only
        for k in range(n):
            launch(ctx, geo, want[k], vectors[k], want_f64=rnd % 2 == 0, what=('round', rnd, k))
    seen = [0, 0, 0]
    for k in range(n):
        launch(ctx, geo, want[k], vectors[k], what=('round with the accessor', k))
        got = ctx.debug_cover_words().tobytes()
        assert got in own[k], k             # one of this key's three tables, and so none of another key's
        seen[own[k].index(got)] += 1
    for k in (0, 4, 9):
        for i in range(3):
            launch(ctx, geo, want[k], vectors[k], what=('three in a row', k, i))
            got = ctx.debug_cover_words()
        assert same(got, tabs[k]['cover']) and same(ctx.debug_census_words(), tabs[k]['census']) and same(ctx.debug_guard_words(), tabs[k]['refined']), k
    print('cover-fuzz: ten keys %s seed %d: the round with the accessor read %d refined, %d census\'d and %d third tables; %s rectangles covered' %
          (case[0], case[1], seen[0], seen[1], seen[2], [covered_on_device(tape, t['cover']) for t in tabs]))
    ctx.close()


def test_more_keys_than_kept_sets():
    """One planted soup, ten vectors on one context (RowReuse::MAX_KEPT is 8): four rounds of all ten, rasters only; a round with the
    accessor after each launch, in which the words a launch read are one of its key's three tables (they differ pairwise between
    keys: tests/test_cover_fuzz.py); then three keys three times in a row each, whose words are then exactly their third table."""
    assert len(_run('child_many_keys()', 600)) == 1


# ---- d. other entry points over the same tables ------------------------------------------------------------------------------
TILES = [(0, 32), (32, 96), (96, 136)]


def child_tiles_shutter_samples():
    from marayb import encode
    from oracle_ffi import Scene as OScene
    from test_gpu_shutter import mean
    from test_gpu_supersample import box
    case = F.ENTRY_POINTS
    geo = case[2]
    w, h = geo[:2]
    tape, color, _, _, _ = F.lowered(case)
    ptape, pcolor, decl, vectors, _ = F.lowered(case, 4)
    ss = M.Scene(encode((w, h), color))
    ss.supersample(2)
    sstape = ss.lower()
    ctx, pctx = contexts([tape, ptape])
    sctx, = contexts([sstape], samples=2)
    want8 = oracle(color, None, None, geo, want_f64=False)[0]
    # render_tiles: every tile is a geometry of its own; its fourth frame is the first that can read a third table
    for frame in range(4):
        image = np.full((h, w, 3), 9, np.uint8)
        done = []
        ctx.render_tiles(w, h, TILES, image, on_tile=lambda a, b: done.append((a, b)))
        assert done == TILES and np.array_equal(image, want8), frame
    assert ctx.census_count == 3 and ctx.cover_count == 3
    # the shutter: four frames that differ only in the PIXEL-read factor, one key
    lo, hi = decl[2][1:]
    v0 = vectors[0]
    cs = [lo + (hi - lo) * f for f in (0.0, 0.4, 0.75, 1.0)]
    rows = [v0[:2] + (c,) for c in cs]
    frames = [oracle(pcolor, decl, r, geo, want_f64=False)[0] for r in rows]
    assert len({f.tobytes() for f in frames}) >= 2
    for call in range(3):
        assert np.array_equal(pctx.render_rows_shutter(w, h, 0, h, rows), mean(frames)), call
    assert pctx.launch_counts[0] == 1 and (pctx.census_count, pctx.cover_count) == (1, 1)
    assert same(pctx.debug_cover_words(), F.tables(ptape, geo, v0)['cover'])
    # samples = 2: the supersampled kernel reads the ROW pass's words: no census, no cover
    want_ss = box(OScene(ss.encode()).render_rows(2 * w, 2 * h, 0, 2 * h, threads=min(16, os.cpu_count() or 1), want_f64=False)[0], 2)
    for i in range(3):
        assert np.array_equal(sctx.render_rows(w, h, 0, h, want_f64=False)[0], want_ss), i
        assert sctx.census_count == sctx.cover_count == 0, i
    for c in (ctx, pctx, sctx):
        c.close()
    print('cover-fuzz: entry points %s seed %d: tiles, shutter and samples = 2' % (case[0], case[1]))


def test_tiles_shutter_and_supersampled():
    """One partial `one` soup.  render_tiles with tiles (0, 32) (32, 96) (96, 136), four frames, against the oracle;
    render_rows_shutter over four frames that differ only in c, three calls, against the integer mean of the oracle's frames
    (tests/test_gpu_shutter.py); a samples = 2 context three times, which keeps both counts at 0, against the box filter of the
    oracle's 2w x 2h render."""
    assert len(_run('child_tiles_shutter_samples()', 600)) == 1


BLOCK_ROWS, BLOCK_STRIDE, N_BLOCKS, BLOCK_Y0 = 32, 64, 2, 5


def child_blocks():
    import torch
    case = F.ENTRY_POINTS
    geo = case[2]
    w, h = geo[:2]
    tape, color, _, _, _ = F.lowered(case)
    whole = oracle(color, None, None, geo, want_f64=False)[0]
    pick = (BLOCK_Y0 + np.arange(N_BLOCKS)[:, None] * BLOCK_STRIDE + np.arange(BLOCK_ROWS)[None, :]).reshape(-1)
    assert pick.max() < h
    # groups of 32 rows never straddle two blocks: the launch's words are the blocks' words one after the other
    per = [F.tables(tape, (w, h, BLOCK_Y0 + k * BLOCK_STRIDE, BLOCK_Y0 + k * BLOCK_STRIDE + BLOCK_ROWS)) for k in range(N_BLOCKS)]
    tabs = {k: np.concatenate([t[k] for t in per]) for k in ('refined', 'census', 'cover')}
    ctx, = contexts([tape])
    d = torch.zeros((N_BLOCKS * BLOCK_ROWS, w, 3), dtype=torch.uint8, device='cuda')
    for i in range(4):
        d.zero_()
        torch.cuda.synchronize()
        ctx.render_blocks_device(w, h, BLOCK_Y0, BLOCK_ROWS, BLOCK_STRIDE, N_BLOCKS, d_rgb8=d.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(d.cpu().numpy(), whole[pick]), i
        assert (ctx.census_count, ctx.cover_count) == ((1, 1) if i else (0, 0)), i
        assert same(ctx.debug_cover_words(), tabs['refined'] if i == 0 else tabs['census'] if i == 1 else tabs['cover']), i
    assert same(ctx.debug_guard_words(), tabs['refined'])
    print('cover-fuzz: blocks %s seed %d: %d of %d rectangles covered on the device' % (case[0], case[1], covered_on_device(tape, ctx.debug_cover_words()), tabs['cover'].shape[0]))
    ctx.close()


def test_interleaved_blocks():
    """render_blocks_device with two blocks of 32 rows 64 apart from row 5, four launches, against those rows of the oracle's whole
    frame; the words of the launch are the model's for the blocks one after the other.  A process of its own with PyTorch
    imported first: the device buffer is PyTorch's."""
    assert len(_run('child_blocks()', 600, torch_first=True)) == 1

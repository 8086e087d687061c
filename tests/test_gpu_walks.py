"""Random walks of launches over the kept ROW sets of one context, on the device (tests/walk_scenes.py).  A walk runs on
one MARAY_BACKEND_JIT context created with the census, the cover, the reuse and the row words on and a byte budget of its own;
after EVERY step
  * the raster is the oracle's (one whole-picture render per vector, sliced to the step's rows; the integer mean of the frames
    for a shutter; the assembled picture for tiles), RGB8 byte for byte and f64 planes bit for bit, and the guard bands round a
    device buffer are untouched;
  * launch_counts, census_count, cover_count, rowscan_count and refine_count are the running totals of the plain model of the
    policy (walk_scenes.PolicyModel);
  * debug_row_sets() is the model's set, kept_sets and accounted bytes, the accounted bytes are within the budget and the bytes
    the kept sets' tables hold are within the accounted bytes;
  * the words of the set the launch used are the numpy models' tables of ITS key: refined, census'd, third and fourth table and the
    flagged rectangles' row words, each where the model says the set has them, and `used` is the model's "reads xbits".
The accessors wait for the context's work, so after a step every pending count has arrived and the next launch's kernel choice
is the model's; inside a step of several launches (time_rows, a shutter, tiles) a count may or may not have arrived, and the
model then names the tables the last launch may have read.  tests/test_walks.py holds the conditions that keep the walks from
being empty and checks the model against row_reuse.hpp itself.

Every test body runs in a child process with a time limit of its own, one at a time; nothing follows a failure inside one.  A
child prints one line, `walk: ...`, with the events of its walk and its seconds; the test prints it again."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import walk_scenes as WS

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BAND, FILL8, FILL64 = 64, 0xA5, -12345.0

_CHILD = r"""
import sys
sys.path[:0] = [%(root)r, %(tests)r]
import torch
import test_gpu_walks as T
T.%(call)s
print('child ok')
"""


def _run(call, timeout=600):
    code = _CHILD % dict(root=ROOT, tests=HERE, call=call)
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0 and out.stdout.strip().endswith('child ok'), (out.stdout[-3000:], out.stderr[-4000:])
    lines = [ln for ln in out.stdout.split('\n') if ln.startswith('walk:')]
    print('\n'.join(lines))
    return lines


def context(tape, budget=None, reuse=True):
    """A MARAY_BACKEND_JIT context with every knob of the ROW sets on (they are read when a context is created)."""
    import maray_amd as M
    want = {'MARAY_JIT_GUARD_CENSUS': '1', 'MARAY_JIT_GUARD_COVER': '1', 'MARAY_JIT_ROW_REUSE': '1' if reuse else '0', 'MARAY_JIT_ROW_WORDS': '1',
            'MARAY_ROW_KEPT_BYTES': '' if budget is None else str(budget)}
    old = {k: os.environ.get(k) for k in want}
    os.environ.update(want)
    try:
        return M.Context(tape, backend=M.BACKEND_JIT)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


class Frames:
    """The oracle's whole picture per vector of a pool, rendered once."""

    def __init__(self, P, pool):
        self.P, self.pool, self.got = P, pool, {}

    def __call__(self, vec):
        if vec not in self.got:
            from test_gpu_cover_fuzz import oracle
            self.got[vec] = oracle(self.P['color'], self.P['decl'], self.pool[vec], (WS.W, WS.H, 0, WS.H))
        return self.got[vec]

    def rows(self, vec, launch, f64=False):
        w = launch[1]
        return self(vec)[1 if f64 else 0][WS.image_rows(launch), :w]


def banded(torch, rows, w, f64):
    """A device buffer of `rows` rows between two guard bands of BAND rows of a fill value; (tensor, pointer to the first row)."""
    t = torch.full((rows + 2 * BAND, w, 3), FILL64 if f64 else FILL8, dtype=torch.float64 if f64 else torch.uint8, device='cuda')
    return t, t.data_ptr() + BAND * w * 3 * (8 if f64 else 1)


def unbanded(t, f64, what):
    a = t.cpu().numpy()
    fill = FILL64 if f64 else FILL8
    assert (a[:BAND] == fill).all() and (a[-BAND:] == fill).all(), (what, 'a guard band was written')
    return a[BAND:-BAND]


def one_step(ctx, torch, streams, step, pool, frames, what, alternate=None):
    """Runs a step and checks its raster(s).  Returns when the step's work is complete."""
    import params as PR
    from test_gpu_shutter import mean
    e, launch, vec = step['entry'], step['launch'], step['vec']
    w = launch[1]
    if pool[vec] is not None:
        ctx.set_params(list(pool[vec]))
    if e == 'render_rows':
        got8, got64 = ctx.render_rows(w, WS.H, launch[2], launch[3], want_f64=step['f64'])
        assert np.array_equal(got8, frames.rows(vec, launch)), (what, 'rgb8')
        if step['f64']:
            assert PR.same_f64(got64, frames.rows(vec, launch, True)), (what, 'f64')
    elif e == 'render_rows_shutter':
        got = ctx.render_rows_shutter(w, WS.H, launch[2], launch[3], [list(pool[f]) for f in step['frames']])
        assert np.array_equal(got, mean([frames.rows(f, launch) for f in step['frames']])), (what, 'shutter')
    elif e == 'render_tiles':
        image = np.full((WS.H, w, 3), 9, np.uint8)
        want = image.copy()
        for t in step['tiles']:
            want[t[2]:t[3]] = frames(vec)[0][t[2]:t[3], :w]
        done = []
        tiles = [(t[2], t[3]) for t in step['tiles']]
        ctx.render_tiles(w, WS.H, tiles, image, on_tile=lambda a, b: done.append((a, b)))
        assert done == tiles and np.array_equal(image, want), (what, 'tiles')
    else:
        rows = len(WS.image_rows(launch))
        st = streams[step['stream'] if alternate is None else alternate]
        d8, p8 = banded(torch, rows, w, False)
        d64, p64 = banded(torch, rows, w, True) if step['f64'] else (None, 0)
        torch.cuda.synchronize()
        if e == 'render_rows_device':
            ctx.render_rows_device(w, WS.H, launch[2], launch[3], d_rgb8=p8, d_rgb64=p64, stream=st.cuda_stream)
        elif e == 'render_blocks_device':
            _, _, y0, brows, stride, n = launch
            ctx.render_blocks_device(w, WS.H, y0, brows, stride, n, d_rgb8=p8, d_rgb64=p64, stream=st.cuda_stream)
        else:
            assert e == 'time_rows'
            ctx.time_rows(w, WS.H, launch[2], launch[3], d_rgb8=p8, reps=WS.TIME_REPS)
        st.synchronize()
        torch.cuda.synchronize()
        assert np.array_equal(unbanded(d8, False, what), frames.rows(vec, launch)), (what, 'rgb8')
        if step['f64']:
            assert PR.same_f64(unbanded(d64, True, what), frames.rows(vec, launch, True)), (what, 'f64')


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b)


def check_words(ctx, rec, T, what):
    """The words of the set the last launch used against the tables T of its key, by the model's record of that launch."""
    reads = rec['reads'] if isinstance(rec['reads'], frozenset) else frozenset([rec['reads']])
    assert same(ctx.debug_guard_words(), T['refined']), (what, 'refined')
    census = T['census'] if rec['sets_census'] else T['refined']
    assert same(ctx.debug_census_words(), census), (what, 'census')
    third = T['cover'] if rec['covered'] else census            # what a launch of the cover's kernels read
    may = [third if r in ('cover', 'xbits') else census for r in reads]
    got = ctx.debug_cover_words()
    assert any(same(got, m) for m in may), (what, 'cover', sorted(reads))
    xb, rw, used = ctx.debug_row_words()
    assert used in [r == 'xbits' for r in reads], (what, 'used', used, sorted(reads))
    if not rec['scanned']:
        assert len(xb) == 0 and len(rw) == 0, (what, 'row words of a set that has had no scan')
        return
    assert same(xb, T['xbits']), (what, 'xbits', [(i, hex(int(a)), hex(int(b))) for i, (a, b) in enumerate(zip(xb.reshape(-1), T['xbits'].reshape(-1))) if a != b][:8])
    got = rw.reshape(T['rwords'].shape)
    assert np.array_equal(got[T['sel']], T['rwords'][T['sel']]), (what, 'rwords')


def child_walk(name, budget=0, alternate=False, reuse=True, many=False):
    import torch
    t0 = time.time()
    P = WS.program(name)
    steps, pool = (WS.many_steps(), P['many']) if many else (WS.steps_of(name), P['pool'])
    b = WS.budgets(name)[budget] if not many else None
    known = WS.Known(name, steps, pool)
    model = WS.PolicyModel(P['facts'], budget=b, reuse=reuse, known=known)
    frames = Frames(P, pool)
    ctx = context(P['tape'], b, reuse)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    words = reuse and not many and P['facts']['n_words'] > 0
    events, excess, flip = dict.fromkeys(WS.EVENTS, 0), 0, 0
    for i, step in enumerate(steps):
        what = (name, budget, i, step['entry'], step['geo'], step['vec'])
        alt = None
        if alternate and step['entry'] in ('render_rows_device', 'render_blocks_device'):
            alt, flip = flip, 1 - flip
        one_step(ctx, torch, streams, step, pool, frames, what, alt)
        recs = [model.launch(launch, pool[vec], rp) for launch, vec, rp in WS.launches_of(step)]
        model.wait()
        for r in recs:
            for e in r['events']:
                events[e] += 1
        tot = model.totals
        assert ctx.launch_counts[0] == tot['passes'], (what, 'ROW passes', ctx.launch_counts, tot)
        if not reuse:
            continue
        assert ctx.launch_counts == (tot['passes'], tot['order']), (what, ctx.launch_counts, tot)
        assert (ctx.census_count, ctx.cover_count, ctx.rowscan_count, ctx.refine_count) == (tot['census'], tot['cover'], tot['scan'], tot['refines']), \
            (what, ctx.census_count, ctx.cover_count, ctx.rowscan_count, ctx.refine_count, tot)
        s, kept_sets, kept_bytes, budget_bytes, held = ctx.debug_row_sets()
        last = recs[-1]
        assert (s, kept_sets, kept_bytes) == (last['set'], last['kept_sets'], last['kept_bytes']), (what, (s, kept_sets, kept_bytes), last)
        assert budget_bytes == model.max_bytes and kept_bytes <= budget_bytes, (what, kept_bytes, budget_bytes)
        excess = max(excess, held - kept_bytes)
        assert held <= kept_bytes and held == model.held_bytes(), (what, 'held', held, 'accounted', kept_bytes, 'model', model.held_bytes())
        if words:
            check_words(ctx, last, known.tables(last['key']), what)
    ctx.close()
    print('walk: %s budget %s%s%s: %d steps, %d launches, %d keys, %s, %.1f s' %
          (name, b, ' alternating streams' if alternate else '', '' if reuse else ' reuse off', len(steps), sum(len(WS.launches_of(s)) for s in steps), len(known.by_key),
           ' '.join('%s %d' % (k, v) for k, v in events.items() if v), time.time() - t0))


@pytest.mark.parametrize('budget', [0, 1, 2])
@pytest.mark.parametrize('name', list(WS.WALKS))
def test_walk(name, budget):
    """A program's walk under the default budget (0), one that holds about three of its sets (1), and one that admits the main
    tables of its largest key but not that key's row words (2): rasters, counters, sets and words after every step."""
    assert len(_run('child_walk(%r, %d)' % (name, budget))) == 1


def test_walk_alternating_streams():
    """A planted walk once more, every device-form step on the other of two streams than the one before."""
    assert len(_run("child_walk('planted_shared', 0, alternate=True)")) == 1


def test_walk_without_reuse():
    """The plain soup's walk on a context created with MARAY_JIT_ROW_REUSE=0: rasters, and a ROW pass for every launch that may
    run one -- the model's count with reuse off."""
    assert len(_run("child_walk('plain', 0, reuse=False)")) == 1


def test_walk_of_more_keys_than_the_seen_ring_holds():
    """R3 and R6 under eighteen values of t, most steps a shutter of four frames: more than 32 keys, so the ring of seen keys
    wraps and a key that comes back may be new again.  Rasters, counters and sets."""
    assert len(_run("child_walk(%r, many=True)" % WS.MANY[0])) == 1


def child_accessor():
    import maray_amd as M
    P = WS.program('plain')
    tape = P['tape']
    ctx = context(tape)
    assert ctx.debug_row_sets() == (-1, 0, 0, WS.PolicyModel.MAX_BYTES, 0)              # before any launch
    ctx.render_rows(WS.W, WS.H, 0, 32, want_f64=False)
    assert ctx.debug_row_sets() == (0, 0, 0, WS.PolicyModel.MAX_BYTES, 0)               # the scratch: nothing kept, nothing accounted
    ctx.close()
    small = context(tape, budget=4096)
    assert small.debug_row_sets()[3] == 4096
    small.close()
    for backend in (M.BACKEND_TAPE, M.BACKEND_TAPE_SMEM):
        slow = M.Context(tape, backend=backend)
        with pytest.raises(M.MarayError) as e:
            slow.debug_row_sets()
        assert e.value.code == -1                       # MARAY_E_ARG: an interpreter keeps no sets
        slow.close()
    print('walk: accessor')


def test_row_sets_accessor():
    """maray_hip_debug_row_sets before any launch, after a one-off launch (the scratch), under a budget from the environment, and
    on the interpreters' contexts, which answer MARAY_E_ARG."""
    assert len(_run('child_accessor()')) == 1

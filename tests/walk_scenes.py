"""Random walks of launches over the kept ROW sets of one MARAY_BACKEND_JIT context, and a plain model of the policy
that decides what each launch does to them: tests/test_walks.py (the model against maray_amd/csrc/row_reuse.hpp driven by
tests/native/row_reuse_walk.cpp, and the conditions that keep the walks from being empty) and tests/test_gpu_walks.py (the device
against the model, the numpy tables and the oracle after every step).  Seeded and deterministic.  No GPU in here.

A walk is a list of steps; a step is one call of an entry point over a geometry of the MENU with a vector of the program's pool.
A step is one or more launches (launches_of): every tile of render_tiles and every frame of a shutter is one, time_rows is two
launches that may run a ROW pass and five plus `reps` that may not.

Keys.  A set's key is the six geometry words of RowKey::geometry -- width, rows of the launch, first row, rows per block, block
stride, rows per guard group -- and the bits of the values the ROW section reads.  Two launch tuples of the MENU are one key only
if they are the same tuple, with one coincidence on purpose: K3 is four blocks of 32 rows 32 apart from row 0 and also the rows
0-128.  They cover the same rows and their tables hold the same words, but RowKey::geometry takes the block's rows (32 against
128) and the stride (32 against 0) as they are given, so they are TWO keys (K3B, K3R below)."""
import random
import struct

W, H = 320, 200

# name -> launch tuple: ('rows', w, y0, y1) or ('blocks', w, y0, block rows, stride, blocks)
MENU = {
    'R1': ('rows', 320, 0, 136),            # 5 groups, 8 rectangles a row
    'R2': ('rows', 300, 37, 141),           # ragged fifth rectangle, window off the 32-row grid
    'R3': ('rows', 320, 64, 96),            # one group: no launch order; fits inside every R1 table
    'R4': ('rows', 64, 0, 200),             # 4 rectangles a row, 7 groups: more y values than R1, fewer guard words
    'R5': ('rows', 257, 100, 200),          # second 256-tile one pixel wide
    'R6': ('rows', 320, 0, 31),             # one partial group
    'K1': ('blocks', 320, 5, 32, 64, 3),    # yrows 32
    'K2': ('blocks', 320, 0, 20, 40, 4),    # yrows 1: census, no row words
    'K3B': ('blocks', 320, 0, 32, 32, 4),   # the same rows as K3R, another key
    'K3R': ('rows', 320, 0, 128),
}
ENTRIES = ('render_rows', 'render_rows_device', 'render_blocks_device', 'render_tiles', 'render_rows_shutter', 'time_rows')
TIME_REPS = 2
MAX_STEPS, MAX_KEYS = 48, 14


def geometry_words(launch):
    """(w, rows of the launch, y0, rows per block, stride) as the entry points hand them to the backend: a range of rows is one
    block of all its rows with stride 0, and so is a single block."""
    if launch[0] == 'rows':
        _, w, y0, y1 = launch
        return w, y1 - y0, y0, y1 - y0, 0
    _, w, y0, rows, stride, n = launch
    return w, n * rows, y0, rows, stride if n > 1 else 0


def image_rows(launch):
    """The image rows of a launch, in the order of its output."""
    if launch[0] == 'rows':
        return list(range(launch[2], launch[3]))
    _, _, y0, rows, stride, n = launch
    return [y0 + b * stride + r for b in range(n) for r in range(rows)]


def blocks_of(launch):
    """[(y0, y1), ...]: the runs of consecutive image rows of a launch."""
    if launch[0] == 'rows':
        return [(launch[2], launch[3])]
    _, _, y0, rows, stride, n = launch
    return [(y0 + b * stride, y0 + b * stride + rows) for b in range(n)]


def bits(v):
    return struct.unpack('<Q', struct.pack('<d', v))[0]


# ---- the walks ---------------------------------------------------------------------------------------------------------------
def walk(seed, pool, row_classes, n_steps=MAX_STEPS, menu=None, max_keys=MAX_KEYS, many=False):
    """n_steps steps over `pool`, a list of value vectors (or [None]); row_classes[i] = what of vector i the ROW section reads
    (vectors of one class are one key on a geometry).  A step: dict(entry, geo, launch, vec, frames, tiles, f64, stream).  The
    walk dwells: about half the steps repeat the key of the step before (a key gets a set when it comes a second time, its
    census, cover and scan on the next launch, and reads them on the one after), a quarter return to a key that has been left."""
    assert n_steps <= MAX_STEPS
    rng = random.Random(0x3A1C5 + 7919 * seed)
    names = list(menu or MENU)
    keys, steps, last = [], [], None
    motif_at = None if many or menu else rng.randrange(6, 24)       # three steps X K2 X of the same values, X one of R1, K3R, K3B
    motif = []

    def key_of(launch, vec):
        return (launch, row_classes[vec])

    def room(new):
        return len(set(keys) | set(new)) <= max_keys

    for i in range(n_steps):
        r = rng.random()
        if motif_at is not None and i == motif_at:
            x = rng.choice(['R1', 'K3R', 'K3B'])
            motif = [x, 'K2', x]
        if motif:
            name, vec = motif.pop(0), (last[1] if last else 0)
        elif last is not None and r < (0.15 if many else 0.5):
            name, vec = last
            if rng.random() < 0.3:                      # the same key under another PIXEL-read value, where the pool has one
                same = [i for i in range(len(pool)) if row_classes[i] == row_classes[vec]]
                vec = rng.choice(same)
        elif steps and r < (0.3 if many else 0.75):
            s = rng.choice(steps)
            name, vec = s['geo'], s['vec']
        else:
            name, vec = rng.choice(names), rng.randrange(len(pool))
            if not room([key_of(MENU[name], vec)]):
                s = rng.choice(steps)
                name, vec = s['geo'], s['vec']
        launch = MENU[name]
        step = dict(entry=None, geo=name, launch=launch, vec=vec, frames=None, tiles=None, f64=rng.random() < 0.3, stream=rng.randrange(2))
        if launch[0] == 'blocks':
            step['entry'] = 'render_blocks_device'
        else:
            e = rng.random()
            step['entry'] = 'render_rows' if e < 0.4 or motif_at is not None and motif_at <= i < motif_at + 3 else 'render_rows_device' if e < 0.6 else 'time_rows' if e < 0.7 else 'render_rows_shutter' if e < 0.85 else 'render_tiles'
            if many and e >= 0.4:
                step['entry'] = 'render_rows_shutter'
            if step['entry'] == 'render_rows_shutter':
                if pool[0] is None:
                    step['entry'] = 'render_rows'
                else:
                    n = 4 if many else rng.choice([2, 4])
                    frames = [vec] + [rng.randrange(len(pool)) for _ in range(n - 1)]
                    if not room([key_of(launch, f) for f in frames]):
                        frames = [vec] * n
                    step['frames'], step['f64'] = frames, False
            if step['entry'] == 'render_tiles':
                others = [MENU[n] for n in names if MENU[n][0] == 'rows' and MENU[n][1] == launch[1] and MENU[n] != launch]
                if launch[1] != W or not others:
                    step['entry'] = 'render_rows'
                else:
                    tiles = [launch] + rng.sample(others, min(len(others), rng.choice([1, 2])))
                    if not room([key_of(t, vec) for t in tiles]):
                        step['entry'] = 'render_rows'
                    else:
                        step['tiles'], step['f64'] = tiles, False
            if step['entry'] == 'time_rows':
                step['f64'] = False
        for launch_, vec_, _ in launches_of(step):
            keys.append(key_of(launch_, vec_))
        steps.append(step)
        last = (name, vec)
    return steps


def launches_of(step):
    """[(launch tuple, vector index, may run a ROW pass), ...] of a step, in the order the context enqueues them."""
    e, launch, vec = step['entry'], step['launch'], step['vec']
    if e == 'render_tiles':
        return [(t, vec, True) for t in step['tiles']]
    if e == 'render_rows_shutter':
        return [(launch, f, True) for f in step['frames']]
    if e == 'time_rows':
        return [(launch, vec, True)] * 2 + [(launch, vec, False)] * (5 + TIME_REPS)
    return [(launch, vec, True)]


# ---- the policy, restated ----------------------------------------------------------------------------------------------------
NONE, PENDING, SOME, EMPTY = 'none', 'pending', 'some', 'empty'
EVENTS = ('promotion', 'eviction-by-count', 'eviction-by-bytes', 'take-over-in-place', 'release-and-regrow', 'scan-admitted', 'scan-refused',
          'return-to-evicted-key', 'scratch-census')
CAPS = ('yvals', 'gbits', 'order', 'hits', 'cbits', 'vbits', 'cflags', 'rwords', 'changed', 'xbits')
SIZE = dict(yvals=8, gbits=8, order=4, hits=1, cbits=8, vbits=8, cflags=1, rwords=8, changed=1, xbits=8)


def program_facts(tape):
    """The numbers of a tape that the policy reads (nothing else of the library enters the model)."""
    _, n_words, gw, gh = tape.guard_layout()
    rows = tape.info['n_row_ops'] > 0
    n_words = n_words if rows else 0
    census = bool(rows and n_words and tape.jit_source_census)
    n_cover = len(tape.cover_bits()) if census else 0
    flag = tape.rowwords_flag()
    return dict(n_yvals=tape.info['n_yvals'], n_row_ops=tape.info['n_row_ops'], n_words=n_words, gw=gw if rows else 256, gh=gh if rows else 1,
                has_refine=bool(rows and n_words and tape.refine.n_ops), has_census=census, n_cover=n_cover,
                has_rw=bool(census and gw == 64 and n_words <= 12 and gh > 1 and flag >= 0 and flag // 64 == n_words - 1),
                row_params=tape.info['row_params'], n_params=tape.param_count)


class _Set:
    def __init__(self):
        self.key, self.keyed, self.order, self.cover, self.census, self.rowwords = None, False, False, False, False, False
        self.rw_bytes, self.launches, self.stamp, self.bytes = 0, 0, 0, 0


class PolicyModel:
    """What a launch does to the sets of a context, from the contracts of row_reuse.hpp and of row_set() and launch() in
    jit_backend.cpp.  launch() returns a dict: set, passes / refines / census / cover / scan / order (kernels enqueued: 0 or 1), reads
    (the table the pixel kernel reads: 'refined', 'census', 'cover', 'xbits'; a set of them where a count enqueued since the
    last wait() may or may not have arrived), kept_sets, kept_bytes, events.  wait(): the caller has waited for the context's
    work -- every pending count has arrived.  known(key) -> (some rectangle covered, some rectangle flagged), the numpy models'
    word on what the counts will say; without it a count that arrives says 'some'."""
    MAX_KEPT, MAX_BYTES, SEEN, N_SETS = 8, 256 << 20, 32, 9

    def __init__(self, facts, budget=None, reuse=True, known=None):
        self.f, self.enabled, self.known = facts, reuse, known
        self.max_bytes = self.MAX_BYTES if budget is None else budget
        self.sets = [_Set() for _ in range(self.N_SETS)]
        self.cap = [dict.fromkeys(CAPS, 0) for _ in range(self.N_SETS)]
        self.cover_state, self.rw_state = [NONE] * self.N_SETS, [NONE] * self.N_SETS
        self.arrived = [[True, True] for _ in range(self.N_SETS)]         # (cover, rw): a pending count has been waited for
        self.gbits_n = [0] * self.N_SETS
        self.seen, self.seen_next, self.clock, self.kept_bytes, self.kept_sets = [None] * self.SEEN, 0, 0, 0, 0
        self.rw_module = False              # the row-word module is loaded by the first launch that is due a scan
        self.evicted = set()
        self.totals = dict(passes=0, refines=0, census=0, cover=0, scan=0, order=0)
        if not reuse:                       # a context that reuses nothing takes no census, and so no cover and no row words
            self.f = dict(facts, has_census=False, n_cover=0, has_rw=False)

    # -- the key
    def key(self, launch, values):
        w, rows, y0, blk_rows, stride = geometry_words(launch)
        gh = self.f['gh']
        yrows = gh if gh > 1 and (blk_rows >= rows or blk_rows % gh == 0) else 1
        mask = self.f['row_params'] if self.enabled else ~0
        vals = tuple(bits(v) for p, v in enumerate(values or ()) if (mask >> p) & 1)
        return (w, rows, y0, blk_rows, stride, yrows) + vals

    def sizes(self, key):
        """Elements of the ten tables a key's launch needs, and the bytes of the seven that place() is asked for."""
        w, rows, _, _, _, yrows = key[:6]
        f = self.f
        n_groups = -(-rows // yrows)
        nw = max(f['n_words'], 1)
        n_rect = -(-w // 256) * (256 // f['gw'])
        gb = n_groups * n_rect * nw
        want_order = f['n_words'] > 0 and n_groups > 1
        c, cov = f['has_census'], f['has_census'] and f['n_cover'] > 0
        n = dict(yvals=rows * max(f['n_yvals'], 1), gbits=gb, order=rows if want_order else 0, hits=gb * 64 if c else 0, cbits=gb if c else 0,
                 vbits=gb if cov else 0, cflags=gb // nw * 2 * f['n_cover'] if cov else 0,
                 rwords=rows * n_rect * nw, changed=gb // nw * yrows, xbits=gb)
        need = sum(n[k] * SIZE[k] for k in CAPS[:7])
        return n, need, want_order

    def need(self, launch, values=None):
        return self.sizes(self.key(launch, values))[1]

    def rw_bytes(self, launch, values=None):
        n = self.sizes(self.key(launch, values))[0]
        return (n['rwords'] + n['gbits']) * 8 + n['changed']

    # -- row_reuse.hpp
    def _find(self, key):
        for s, S in enumerate(self.sets):
            if S.keyed and S.key == key:
                return s
        return -1

    def _touch(self, s):
        self.clock += 1
        self.sets[s].stamp = self.clock
        self.sets[s].launches += 1

    def _lru(self):
        live = [s for s in range(1, self.MAX_KEPT + 1) if self.sets[s].bytes]
        return min(live, key=lambda s: self.sets[s].stamp) if live else -1

    def _drop(self, s, events):
        if self.sets[s].key is not None:
            self.evicted.add(self.sets[s].key)
        self.kept_bytes -= self.sets[s].bytes
        self.kept_sets -= 1
        self.sets[s] = _Set()
        self.cap[s] = dict.fromkeys(CAPS, 0)
        events.append('release-and-regrow')

    def _place(self, key, need, n, events):
        again = key in self.seen
        if not again:
            self.seen[self.seen_next] = key
            self.seen_next = (self.seen_next + 1) % self.SEEN
        s = 0
        if self.enabled and again and need <= self.max_bytes:
            by_count = self.kept_sets >= self.MAX_KEPT
            v = self._lru() if by_count or self.kept_bytes + need > self.max_bytes else -1
            if v >= 0:
                events.append('eviction-by-count' if by_count else 'eviction-by-bytes')
            if v >= 0 and all(self.cap[v][k] >= n[k] for k in CAPS[:7]):
                s = v
                self.evicted.add(self.sets[v].key)
                events.append('take-over-in-place')
            else:
                if by_count:
                    self._drop(v, events)
                while self.kept_bytes + need > self.max_bytes:
                    if 'eviction-by-bytes' not in events:
                        events.append('eviction-by-bytes')
                    self._drop(self._lru(), events)
                s = next(i for i in range(1, self.N_SETS) if not self.sets[i].bytes)
                self.sets[s].bytes = need
                self.kept_bytes += need
                self.kept_sets += 1
                events.append('promotion')
        if key in self.evicted:
            events.append('return-to-evicted-key')
            if s:
                self.evicted.discard(key)
        S = self.sets[s]
        S.keyed = S.order = S.census = S.cover = S.rowwords = False
        S.launches = 0
        S.key = key
        return s

    def _admit(self, s, nbytes):
        S = self.sets[s]
        more = max(0, nbytes - S.rw_bytes)
        kept = s > 0 and S.bytes > 0
        add = more if kept else nbytes
        if add > self.max_bytes or self.kept_bytes + add > self.max_bytes:
            return False
        if kept:
            S.bytes += more
            self.kept_bytes += more
        S.rw_bytes += more
        return True

    def _grow(self, s, n, names):
        for k in names:
            self.cap[s][k] = max(self.cap[s][k], n[k])

    # -- row_set() and launch()
    def launch(self, launch, values=None, rows_pass=True):
        f = self.f
        key = self.key(launch, values)
        n, need, want_order = self.sizes(key)
        yrows = key[5]
        out = dict(passes=0, refines=0, census=0, cover=0, scan=0, order=0, events=[], key=key)
        s = self._find(key)
        if s >= 0 and (self.enabled or not rows_pass):
            self._touch(s)
        else:
            assert rows_pass, 'a launch without a ROW pass of a key no set holds: not in these walks'
            refill = s >= 0
            if not refill:
                s = self._place(key, need, n, out['events'])
            self._grow(s, n, CAPS[:2] if s == 0 else CAPS[:7])
            if f['n_row_ops']:
                out['passes'] = 1
                out['refines'] = 1 if f['has_refine'] else 0
            self.cover_state[s] = self.rw_state[s] = NONE
            self.arrived[s] = [True, True]
            if refill:
                self._touch(s)
            else:
                self.sets[s].keyed = True
                self._touch(s)
            self.gbits_n[s] = n['gbits']
        S = self.sets[s]
        pending_before = (self.cover_state[s] == PENDING and not self.arrived[s][0]) or (self.rw_state[s] == PENDING and not self.arrived[s][1])
        has_cover = f['has_census'] and f['n_cover'] > 0
        if f['has_census'] and self.enabled and S.keyed and not S.census and S.launches >= 2 and self.gbits_n[s]:
            self._grow(s, n, ('hits', 'cbits'))
            out['census'] = 1
            S.census = True
            if s == 0:
                out['events'].append('scratch-census')
        if has_cover and self.enabled and S.keyed and S.census and not S.cover and self.gbits_n[s]:
            self._grow(s, n, ('vbits', 'cflags'))
            out['cover'] = 1
            S.cover = True
            self.cover_state[s], self.arrived[s][0] = PENDING, False
        self._arrive(s, 0)
        if f['has_rw'] and yrows > 1 and self.enabled and S.keyed and S.census and (S.cover or not has_cover) and not S.rowwords:
            self.rw_module = True
            if self.gbits_n[s] and self._admit(s, (n['rwords'] + n['gbits']) * 8 + n['changed']):
                self._grow(s, n, ('rwords', 'changed', 'xbits'))
                out['scan'] = 1
                self.rw_state[s], self.arrived[s][1] = PENDING, False
                out['events'].append('scan-admitted')
            else:
                out['events'].append('scan-refused')
            S.rowwords = True
        self._arrive(s, 1)
        certain = 'xbits' if self.rw_module and S.rowwords and self.rw_state[s] == SOME else 'cover' if S.cover and self.cover_state[s] == SOME else \
            'census' if S.census else 'refined'
        reads = {certain}
        if pending_before:                  # a count enqueued by an earlier launch since the last wait: it may have arrived
            was_cover, was_rw = self._count(key)
            if self.cover_state[s] == PENDING and was_cover:
                reads.add('cover')
            if self.rw_state[s] == PENDING and was_rw and self.rw_module:
                reads.add('xbits')
        out['reads'] = certain if len(reads) == 1 else frozenset(reads)
        if want_order and not S.order and S.launches >= 2:
            self._grow(s, n, ('order',))
            out['order'] = 1
            S.order = True
        for k in self.totals:
            self.totals[k] += out[k]
        out.update(set=s, kept_sets=self.kept_sets, kept_bytes=self.kept_bytes, scanned=S.rowwords and self.rw_state[s] != NONE, sets_census=S.census,
                   covered=S.cover)
        return out

    def _count(self, key):
        return self.known(key) if self.known else (True, True)

    def _arrive(self, s, which):
        """The count of set s's cover (0) or scan (1), if it has been waited for since it was enqueued."""
        state = self.cover_state if which == 0 else self.rw_state
        if state[s] == PENDING and self.arrived[s][which]:
            state[s] = SOME if self._count(self.sets[s].key)[which] else EMPTY

    def wait(self):
        for a in self.arrived:
            a[0] = a[1] = True

    def held_bytes(self):
        return sum(self.cap[s][k] * SIZE[k] for s in range(1, self.N_SETS) for k in CAPS)

    # -- the lines tests/native/row_reuse_walk.cpp reads
    def native_line(self, launch, values, rows_pass, ids):
        """key-id, may run a ROW pass, need, the seven capacities, rows of the order, yrows, the program's has_census / has_cover /
        has_rw, the row words' bytes."""
        key = self.key(launch, values)
        n, need, want_order = self.sizes(key)
        f = self.f
        return ' '.join(str(int(v)) for v in [ids.setdefault(key, len(ids) + 1), rows_pass, need] + [n[k] for k in CAPS[:7]] +
                        [want_order, key[5], f['has_census'], f['has_census'] and f['n_cover'] > 0, f['has_rw'], (n['rwords'] + n['gbits']) * 8 + n['changed'],
                         n['gbits'], 1 if f['n_row_ops'] else 0])


def run(model, steps, pool):
    """The model's records of a walk: a list (per step) of lists (per launch); waits after every step, as the GPU test does."""
    out = []
    for step in steps:
        recs = [model.launch(launch, pool[vec], rp) for launch, vec, rp in launches_of(step)]
        model.wait()
        out.append(recs)
    return out


def census_of_events(records):
    c = dict.fromkeys(EVENTS, 0)
    for recs in records:
        for r in recs:
            for e in r['events']:
                c[e] += 1
    return c


# ---- the programs ------------------------------------------------------------------------------------------------------------
# Two planted soups of tests/cover_fuzz_scenes.py (a ROW-read translation t, u and a PIXEL-read factor c), one plain soup (kind and
# seed of a case of rowwords_fuzz_scenes.CASES, on this picture) and row_reuse_scenes.sines(), all on a picture of 320 x 200.  The
# seeds of the planted soups and of the walks were searched on the CPU (`python tests/walk_scenes.py`) until the conditions of
# tests/test_walks.py held; a seed that stops meeting them is replaced here, never skipped there.
PLANTED = {'planted_one': ('one', 2), 'planted_shared': ('shared', 0)}
PLAIN = ('one', 21)
SINES_T = (0.0, -0.0, 2.5, -7.25)           # +0.0 and -0.0: two keys, one picture
MANY_T = 18                                 # the walk of more keys than the seen-ring holds: R3 and R6 under eighteen values of t
WALKS = {'planted_one': 2, 'planted_shared': 1, 'plain': 0, 'sines': 0}
MANY = ('planted_one', 0)
_programs = {}


def program(name):
    """dict(tape, color, decl, pool, many): a program lowered, its pool of at most four vectors ([None] without parameters) and,
    for the planted soups, the vectors of the walk of many keys."""
    if name in _programs:
        return _programs[name]
    import cover_fuzz_scenes as F
    import maray_amd as M
    import params as PR
    import row_reuse_scenes as RS
    from marayb import encode
    many = None
    if name in PLANTED:
        kind, seed = PLANTED[name]
        color, decl, (v0, v1), other = F.planted_soup(seed, F.N_SHAPES, W, H, kind, 2)
        tape = PR.declared_ids(encode((W, H), color), decl).lower()
        pool = [v0, v1, v0[:2] + (other,)]
        if other != v1[2]:
            pool.append(v1[:2] + (other,))
        lo, hi = decl[0][1:]
        many = [(lo + (hi - lo) * (k + 0.5) / MANY_T, v0[1], v0[2]) for k in range(MANY_T)]
    elif name == 'plain':
        kind, seed = PLAIN
        color, decl, pool = F.cover_soup(seed, F.N_SHAPES, W, H, kind), [], [None]
        tape = M.Scene(encode((W, H), color)).lower()
    elif name == 'sines':
        color, named = RS.sines()
        _, tape = RS.lowered((color, named), size=(W, H))
        from marayb import var
        decl, pool = [(var(n)[1], lo, hi) for n, lo, hi in named], [(t,) for t in SINES_T]
    else:
        raise KeyError(name)
    _programs[name] = dict(tape=tape, color=color, decl=decl, pool=pool, many=many, facts=program_facts(tape))
    return _programs[name]


def row_classes(facts, pool):
    """Per vector of a pool: the bits of what the ROW section reads of it."""
    return [tuple(bits(x) for p, x in enumerate(v or ()) if (facts['row_params'] >> p) & 1) for v in pool]


def steps_of(name):
    P = program(name)
    return walk(WALKS[name], P['pool'], row_classes(P['facts'], P['pool']))


def many_steps():
    P = program(MANY[0])
    return walk(1000 + MANY[1], P['many'], row_classes(P['facts'], P['many']), menu=('R3', 'R6'), max_keys=2 * MANY_T, many=True)


def budgets(name, steps=None, pool=None):
    """The three budgets of a walk: the default; one that holds about three of its sets (three times the mean need of its keys, row
    words included); one that admits the seven main tables of its largest key and not that key's row words."""
    P = program(name)
    steps, pool = steps or steps_of(name), pool or P['pool']
    m = PolicyModel(P['facts'])
    ls = {(launch, vec) for s in steps for launch, vec, _ in launches_of(s)}
    full = sorted({m.key(l, pool[v]): m.need(l, pool[v]) + (m.rw_bytes(l, pool[v]) if P['facts']['has_rw'] and m.key(l, pool[v])[5] > 1 else 0) for l, v in ls}.values())
    main = max(m.need(l, pool[v]) for l, v in ls)
    return [None, 3 * sum(full) // len(full), main + 64]


# ---- the numpy tables of a key -----------------------------------------------------------------------------------------------
class _OneRow:
    """A tape whose guard groups are one row high: what a launch evaluates whose blocks are no multiple of the group's rows."""

    def __init__(self, tape):
        self._tape = tape

    def guard_layout(self):
        pos, n_words, gw, _ = self._tape.guard_layout()
        return pos, n_words, gw, 1

    def __getattr__(self, name):
        return getattr(self._tape, name)


def tables(tape, launch, values=None):
    """The numpy models' tables of one key: refined, census, cover (None for a program without cover bits), covered, and -- for a
    program with row words and groups of more than a row -- xbits, rwords, flagged, sel (the (row, rectangle) pairs whose row
    words a launch reads).  A launch of blocks holds its blocks' tables one after the other: no group straddles two blocks."""
    import numpy as np
    import census_scenes as CS
    import cover_scenes as CV
    import rowwords_scenes as RW
    w, rows, _, blk_rows, _ = geometry_words(launch)
    gh = tape.guard_layout()[3]
    one_row = not (gh > 1 and (blk_rows >= rows or blk_rows % gh == 0))
    t = _OneRow(tape) if one_row else tape
    has_cover = bool(tape.cover_bits())
    has_rw = not one_row and tape.rowwords_flag() >= 0
    parts = []
    for y0, y1 in blocks_of(launch):
        d = dict(refined=CS.words(t, w, y0, y1 - y0, params=values, census=False))
        if has_rw:
            m = RW.row_words(t, w, y0, y1 - y0, params=values)
            d.update(xbits=m['xbits'], rwords=m['rwords'], flagged=m['flagged'], sel=RW.flagged_rows(m))
        if has_cover:
            d['cover'], d['census'], d['covered'] = CV.words(t, w, y0, y1 - y0, params=values)
            d['covered'] = np.asarray(d['covered']).any(axis=1) if np.asarray(d['covered']).ndim > 1 else np.asarray(d['covered'])
        else:
            d['census'] = CS.words(t, w, y0, y1 - y0, params=values)
        parts.append(d)
    out = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    out.setdefault('cover', None)
    out.setdefault('covered', np.zeros(len(out['refined']), bool))
    out.setdefault('flagged', np.zeros(len(out['refined']), bool))
    return out


# ---- what keeps a walk from being empty (tests/test_walks.py asserts it; `python tests/walk_scenes.py` searches seeds for it) --
class Known:
    """known(key) of a program's walk: (a rectangle is covered, a rectangle is flagged) from the numpy tables, kept per key."""

    def __init__(self, name, steps, pool):
        P = program(name)
        self.P, self.by_key, self.tabs = P, {}, {}
        m = PolicyModel(P['facts'])
        for s in steps:
            for launch, vec, _ in launches_of(s):
                self.by_key.setdefault(m.key(launch, pool[vec]), (launch, pool[vec]))

    def tables(self, key):
        if key not in self.tabs:
            launch, values = self.by_key[key]
            self.tabs[key] = tables(self.P['tape'], launch, values) if self.P['facts']['n_words'] else None
        return self.tabs[key]

    def __call__(self, key):
        t = self.tables(key)
        return (False, False) if t is None else (bool(t['covered'].any()), bool(t['flagged'].any()))


def _rects(key):
    return -(-key[0] // 256) * 4, -(-key[1] // key[5])          # rectangles per row (64 pixels wide), groups


def conditions(records, steps, known):
    """The conditions on one walk under one budget, as a dict of booleans (tests/test_walks.py says which must hold where)."""
    flat = [r for recs in records for r in recs]
    c = dict(takeover=False, back=False, refused_then_admitted=False, k2_between=False)

    def stays(i, n):            # the n launches of flat[i]'s key after i that find it in flat[i]'s set, before anything places it again
        k, s, out = flat[i]['key'], flat[i]['set'], []
        for r in flat[i + 1:]:
            if r['key'] == k:
                if r['passes'] or r['set'] != s:
                    break
                out.append(r)
        return out if len(out) >= n else None

    old = {}
    for i, r in enumerate(flat):
        if 'take-over-in-place' in r['events'] and r['set'] in old:
            was = old[r['set']]
            smaller = _rects(r['key'])[0] < _rects(was)[0] or _rects(r['key'])[1] < _rects(was)[1]
            after = stays(i, 3)
            if smaller and known(was) == (True, True) and known(r['key'])[1] and after and any(a['reads'] == 'xbits' for a in after):
                c['takeover'] = True
        if 'return-to-evicted-key' in r['events'] and stays(i, 3):
            c['back'] = True
        if 'scan-refused' in r['events'] and any('scan-admitted' in q['events'] and q['set'] == r['set'] for q in flat[i + 1:]):
            c['refused_then_admitted'] = True
        old[r['set']] = r['key']
    for a, b, d in zip(steps, steps[1:], steps[2:]):
        if b['geo'] == 'K2' and a['geo'] in ('R1', 'K3R', 'K3B') and d['geo'] in ('R1', 'K3R', 'K3B') and a['vec'] == b['vec'] == d['vec']:
            c['k2_between'] = True
    return c


def key_conditions(steps, known):
    keys = list(known.by_key)
    f = [known(k) for k in keys]
    return dict(n_keys=len(keys), flagged=sum(x[1] for x in f), unflagged=sum(not x[1] for x in f), covered=sum(x[0] for x in f), uncovered=sum(not x[0] for x in f),
                no_order=any(s['geo'] in ('R3', 'R6') for s in steps))


def survey(name, steps=None, pool=None):
    """(conditions OR-ed over the three budgets, key conditions, events summed over the budgets) of a program's walk."""
    P = program(name)
    steps, pool = steps or steps_of(name), pool or P['pool']
    known = Known(name, steps, pool)
    cond, events = {}, dict.fromkeys(EVENTS, 0)
    for b in budgets(name, steps, pool):
        recs = run(PolicyModel(P['facts'], budget=b, known=known), steps, pool)
        for k, v in conditions(recs, steps, known).items():
            cond[k] = cond.get(k, False) or v
        for k, v in census_of_events(recs).items():
            events[k] += v
    return cond, key_conditions(steps, known), events


if __name__ == '__main__':
    import sys
    sys.path[:0] = [__file__.rsplit('/', 2)[0]]
    for name in sys.argv[1:] or list(WALKS):
        P = program(name)
        for seed in range(400):
            steps = walk(seed, P['pool'], row_classes(P['facts'], P['pool']))
            cond, keys, events = survey(name, steps)
            ok = keys['n_keys'] <= MAX_KEYS and keys['no_order'] and (name not in PLANTED or (all(cond.values()) and keys['flagged'] >= 3 and keys['unflagged'] >= 1 and
                                                                                              keys['covered'] >= 2 and keys['uncovered'] >= 1))
            print(name, seed, 'OK' if ok else '--', cond, keys, events, flush=True)
            if ok:
                break

"""The guard words of a lowered program in numpy, rectangle by rectangle: the ROW section's guards, the REFINE section's
second bounds (include/maray_tape.h, maray_refine) and the exact value of every guarded conjunction on every pixel.

Test infrastructure, never on a render path.  What the specialised kernels keep per rectangle of `gw` pixels x `gh` rows is
  geometric bit of guard g = (ROW OUT of guard g, evaluated with XMIN / XMAX / YMIN / YMAX = the rectangle) != 0
  refined bit              = geometric bit AND (REFINE OUT of guard g != 0), for the guards that have one
and the claim under test is: a guarded conjunction that is != 0 on some pixel of a rectangle has its refined bit set there.
sin goes through the platform libm (math.sin, = the oracle's); where only its sign is asked (Step(Sin)) numpy's sin answers
for the arguments whose sine is far from zero -- both are within 1e-15 of the true value, so they agree on the sign of anything
larger than 1e-9 -- and math.sin for the rest.
"""
import math

import numpy as np

import tape_eval as TE

OP = TE.OP
_vsin = np.vectorize(math.sin, otypes=[np.float64])


def step_sin(a):
    with np.errstate(all='ignore'):
        s = np.sin(a)
        near = ~(np.abs(s) > 1e-9)              # (NaN and inf arguments included)
        if near.any():
            s = s.copy()
            fin = near & np.isfinite(a)
            s[near] = np.nan
            s[fin] = _vsin(a[fin])
        return np.where(s >= 0.0, 1.0, 0.0)


def run(ops, consts, n_slots, n_items, spec, yvals=None, params=None, want=None):
    """A section without its SKIP ops (an evaluator may ignore them) on n_items items.  spec: {index: array or scalar} of the
    SPEC operands X, Y, XMAX, XMIN, YMAX, YMIN (maray_tape.h); yvals: (n_items, n_yvals) or None.  Returns {aux: value} of
    the OUT ops; want = an op index: returns that op's value instead."""
    shape = (n_items,)
    slots = [None] * max(n_slots, 1)
    outs = {}
    acc = None

    def fetch(ref):
        kind, idx = ref >> 14, ref & 0x3FFF
        if kind == TE.K_SLOT: return slots[idx]
        if kind == TE.K_CONST: return np.full(shape, consts[idx])
        if kind == TE.K_YVAL: return yvals[:, idx]
        if idx == 2: return acc
        if idx >= 7: return np.full(shape, float(params[idx - 7]))
        return np.broadcast_to(np.asarray(spec[idx], np.float64), shape)

    with np.errstate(all='ignore'):
        for pc, ins in enumerate(ops):
            op, aux, dst, ra, rb = TE.decode(ins)
            if op in (OP['NOP'], OP['SKIPZ'], OP['SKIPNZ']):
                continue
            if op == OP['OUT']:
                outs[aux] = fetch(ra)
                continue
            if op == OP['MOV']: r = fetch(ra)
            elif op == OP['NEG']: r = -fetch(ra)
            elif op == OP['ABS']: r = np.abs(fetch(ra))
            elif op == OP['RECIP']: r = 1.0 / fetch(ra)
            elif op == OP['SQRT']: r = np.sqrt(fetch(ra))
            elif op == OP['STEP']: r = np.where(fetch(ra) >= 0.0, 1.0, 0.0)
            elif op == OP['STEPSIN']: r = step_sin(fetch(ra))
            elif op == OP['SIN']: r = TE._sin(fetch(ra))
            elif op == OP['EXP']: r = TE._vexp(fetch(ra))
            elif op == OP['LN']: r = TE._vlog(fetch(ra))
            elif op == OP['ADD']: r = fetch(ra) + fetch(rb)
            elif op == OP['MUL']: r = fetch(ra) * fetch(rb)
            elif op == OP['MAX']: r = TE._max(fetch(ra), fetch(rb))
            elif op == OP['MIN']: r = TE._min(fetch(ra), fetch(rb))
            else:
                raise ValueError('op %d is not evaluated here (no textures)' % op)
            acc = r
            if dst != TE.DST_NONE:
                slots[dst] = r
            if want == pc:
                return r
    return outs


def rectangles(w, rows, gw, gh):
    """The rectangles of `rows` launch rows of a w-wide image as the kernels cut them: (n_groups, n_rect) and, flattened group
    by group, xlo, xhi, first and last launch row.  A row has (w + 255) // 256 tiles of 256 // gw rectangles each; those past
    a ragged edge are clamped to the last pixel (maray_jit_rows)."""
    n_rect = (w + 255) // 256 * (256 // gw)
    n_groups = (rows + gh - 1) // gh
    grp, tile = np.divmod(np.arange(n_groups * n_rect), n_rect)
    xlo = np.minimum(tile * gw, w - 1)
    xhi = np.minimum(tile * gw + gw - 1, w - 1)
    r0 = grp * gh
    r1 = np.minimum(r0 + gh - 1, rows - 1)
    return (n_groups, n_rect), xlo, xhi, r0, r1


def n_numeric(tape):
    guards = TE.guard_yvals(tape)
    return min(guards) if guards else tape.info['n_yvals']


def guard_bits(tape, w, y0, rows, gw, gh, params=None):
    """(geometric, second, has): (rectangles, n_guards) booleans -- the ROW section's guards per rectangle, the REFINE
    section's outputs (True where a guard has none) -- and which guards have a second bound."""
    consts, row_ops, _ = tape.arrays()
    n_ynum = n_numeric(tape)
    n_g = tape.info['n_yvals'] - n_ynum
    _, xlo, xhi, r0, r1 = rectangles(w, rows, gw, gh)
    n = len(xlo)
    spec = {1: (y0 + r0).astype(np.float64), 3: xhi.astype(np.float64), 4: xlo.astype(np.float64), 5: (y0 + r1).astype(np.float64),
            6: (y0 + r0).astype(np.float64)}
    outs = run(row_ops, consts, tape.info['n_row_slots'], n, spec, params=params)
    geo = np.ones((n, n_g), bool)
    for k in range(n_g):
        if n_ynum + k in outs:
            geo[:, k] = outs[n_ynum + k] != 0.0
    second = np.ones((n, n_g), bool)
    has = np.zeros(n_g, bool)
    ref = tape.refine_arrays()
    if ref is not None:
        rc, rops, rslots = ref
        spec_r = {k: v for k, v in spec.items() if k != 1}          # the REFINE section never reads Y
        for aux, v in run(rops, rc, rslots, n, spec_r, params=params).items():
            second[:, aux - n_ynum] = v != 0.0
            has[aux - n_ynum] = True
    return geo, second, has


def derived_members(tape):
    """{guard: [guards]} for the guards the specialised kernels keep no bit for (jit_guard_plan): a guard whose ROW value is
    a MAX tree over other guards' values is read as "any of their bits".  Guards are numbered from the first guard y value."""
    _, row_ops, _ = tape.arrays()
    n_ynum = n_numeric(tape)
    writer, acc, deps, src = {}, None, {}, {}
    for j, ins in enumerate(row_ops):
        op, aux, dst, ra, rb = TE.decode(ins)
        if op in (OP['NOP'], OP['SKIPZ'], OP['SKIPNZ']):
            continue
        prod = lambda r: writer.get(r & 0x3FFF) if r >> 14 == TE.K_SLOT else (acc if (r >> 14 == TE.K_SPEC and (r & 0x3FFF) == 2) else None)
        if op == OP['OUT']:
            if aux >= n_ynum:
                src[aux - n_ynum] = prod(ra)
            continue
        deps[j] = (op, prod(ra), prod(rb) if OP['ADD'] <= op <= OP['APP'] else None)
        acc = j
        if dst != TE.DST_NONE:
            writer[dst] = j
    guard_of = {}
    for g_, o in src.items():
        if o is not None:
            guard_of.setdefault(o, g_)
    out = {}
    for g_, o in src.items():
        if o is None or deps[o][0] != OP['MAX']:
            continue
        leaves, st, ok = [], [deps[o][1], deps[o][2]], True
        while st and ok:
            v = st.pop()
            if v is None:
                ok = False
            elif v in guard_of and guard_of[v] != g_:
                leaves.append(guard_of[v])
            elif deps[v][0] == OP['MAX']:
                st += [deps[v][2], deps[v][1]]
            else:
                ok = False
        if ok and leaves:
            out[g_] = leaves
    return out


def effective(bits, members):
    """(rectangles, n_guards) booleans as the kernels read them: a derived guard is the OR of its members' bits."""
    out = bits.copy()

    def get(g_, depth=0):
        if g_ in members and depth < 64:
            return np.logical_or.reduce([get(m, depth + 1) for m in members[g_]])
        return bits[:, g_]
    for g_ in members:
        out[:, g_] = get(g_)
    return out


def pack_words(bits, pos, n_words):
    """(rectangles, n_guards) booleans -> (rectangles, n_words) uint64 with guard g at bit pos[g] (pos < 0: no bit)."""
    out = np.zeros((bits.shape[0], n_words), np.uint64)
    for g, p in enumerate(pos):
        if p >= 0:
            out[:, p // 64] |= bits[:, g].astype(np.uint64) << np.uint64(p % 64)
    return out


def guarded_regions(tape):
    """{guard y value: [op index that ends a region it guards, ...]} of the PIXEL section."""
    _, _, pix = tape.arrays()
    guards = TE.guard_yvals(tape)
    out = {}
    for j, ins in enumerate(pix):
        op, aux, dst, ra, rb = TE.decode(ins)
        if op == OP['SKIPZ'] and ra >> 14 == TE.K_YVAL and (ra & 0x3FFF) in guards:
            out.setdefault(ra & 0x3FFF, []).append(j + aux)
    return out


def cone(pix, end):
    """The ops of the PIXEL section that op `end` depends on, as a tape of their own (the rest NOPs)."""
    writer, acc, deps = {}, None, {}
    for j, ins in enumerate(pix[:end + 1]):
        op, aux, dst, ra, rb = TE.decode(ins)
        if op in (OP['NOP'], OP['SKIPZ'], OP['SKIPNZ'], OP['OUT']):
            continue
        d = []
        for r in ([ra, rb] if OP['ADD'] <= op <= OP['APP'] else [ra] if op != OP['TEXDIM'] else []):
            if r >> 14 == TE.K_SLOT: d.append(writer[r & 0x3FFF])
            elif r >> 14 == TE.K_SPEC and (r & 0x3FFF) == 2: d.append(acc)
        deps[j] = d
        acc = j
        if dst != TE.DST_NONE:
            writer[dst] = j
    need, st = set(), [end]
    while st:
        j = st.pop()
        if j not in need:
            need.add(j)
            st += deps[j]
    return [pix[j] if j in need else 0 for j in range(end + 1)]


def numeric_yvals_of_rows(tape, w, y0, rows, params=None):
    """(rows, n_yvals) with the y values PIXEL ops read as operands (the guards' columns hold what a whole row gives)."""
    consts, row_ops, _ = tape.arrays()
    ys = np.arange(y0, y0 + rows, dtype=np.float64)
    outs = run(row_ops, consts, tape.info['n_row_slots'], rows, {1: ys, 3: float(w - 1), 4: 0.0, 5: ys, 6: ys}, params=params)
    yv = np.zeros((rows, tape.info['n_yvals']))
    for k, v in outs.items():
        yv[:, k] = v
    return yv


def nonzero_per_rectangle(tape, w, y0, rows, gw, gh, params=None, only=None):
    """(rectangles, n_guards) booleans: some pixel of the rectangle has a conjunction guarded by that guard != 0 -- every
    pixel of the rows evaluated, through the cone of the op that ends the guarded region.  only: (rectangles, n_guards)
    booleans, evaluate a guard's regions on the pixels of these rectangles alone (the others report False)."""
    consts, _, pix = tape.arrays()
    n_ynum = n_numeric(tape)
    n_g = tape.info['n_yvals'] - n_ynum
    (n_groups, n_rect), _, _, _, _ = rectangles(w, rows, gw, gh)
    yv_rows = numeric_yvals_of_rows(tape, w, y0, rows, params)
    ry, rx = np.divmod(np.arange(rows * w), w)
    rect_of = (ry // gh) * n_rect + rx // gw
    out = np.zeros((n_groups * n_rect, n_g), bool)
    for k, ends in guarded_regions(tape).items():
        sel = np.arange(rows * w) if only is None else np.nonzero(only[rect_of, k - n_ynum])[0]
        if not len(sel):
            continue
        for end in ends:
            v = run(cone(pix, end), consts, tape.info['n_pix_slots'], len(sel), {0: rx[sel].astype(np.float64), 1: (y0 + ry[sel]).astype(np.float64)},
                    yvals=yv_rows[ry[sel]], params=params, want=end)
            hit = np.zeros(n_groups * n_rect, bool)
            hit[rect_of[sel][v != 0.0]] = True
            out[:, k - n_ynum] |= hit
    return out

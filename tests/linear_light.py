"""The reduces in linear light (include/maray_hip.h, "transfer") in numpy: the committed decode table, the contracts box_lin,
tent_lin and mean_lin, MUTANTS of them, and the rasters that sit on the encoder's thresholds.  The helpers of
tests/test_linear_light.py (no device) and tests/test_gpu_linear_bytes.py.

The contracts are byte_rasters.tent_general / mean_general (and the box mean) with a decode in front and an encode behind:
out = E((SUM w_i D[s_i] + W/2) >> log2 W).  Those two functions end in a cast to uint8, which a 16-bit mean does not survive,
so the sums are restated here on integers of any size; with the identity tables (TRANSFER_NONE) the restatements must BE
tent_general, mean_general and box, which tests/test_linear_light.py checks.
"""
import os
import re

import numpy as np

import byte_rasters as BR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def committed_table():
    """The 256 literals of include/maray_transfer_table.h."""
    text = open(os.path.join(ROOT, 'include', 'maray_transfer_table.h')).read()
    body = text[text.index('#define MARAY_SRGB_DECODE_LIST') + len('#define MARAY_SRGB_DECODE_LIST'):text.rindex('#endif')]
    d = [int(t) for t in re.findall(r'\d+', body)]
    assert len(d) == 256
    return np.array(d, np.int64)


def formula_table():
    c = np.arange(256) / 255.0
    return np.floor(65535 * np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4) + 0.5).astype(np.int64)


D = committed_table()
T = np.concatenate([[0], (D[:-1] + D[1:] + 1) >> 1])           # T[0] = 0: never counted
D_NONE = np.arange(256, dtype=np.int64)
T_NONE = np.arange(256, dtype=np.int64)


def encode(m, t=T):
    """E(M): the number of v in 1 .. 255 with T[v] <= M."""
    return np.searchsorted(np.asarray(t)[1:], m, side='right').astype(np.uint8)


def _finish(m, t, enc):
    return encode(m, t) if enc else (m & 0xFF).astype(np.uint8)          # a kernel that forgot E writes M's low byte


def _log2(n):
    return int(n).bit_length() - 1


# ---- the contracts, with room for one mistake ----------------------------------------------------------------------------
def box_lin(s8, k, d=D, t=T, half=None, dec=True, enc=True):
    H, W, _ = s8.shape
    x = d[s8] if dec else s8.astype(np.int64)
    s = x.reshape(H // k, k, W // k, k, 3).sum(axis=(1, 3))
    return _finish((s + (k * k // 2 if half is None else half)) >> (2 * _log2(k)), t, enc)


def tent_lin_mean(s8, k, d=D, half=None, dec=True, hbits=None):
    """M of the tent: (SUM t(u) t(v) D[s] + W/2) >> log2 W, indices clamped to the image; hbits: the bits a horizontal sum keeps."""
    H, W, _ = s8.shape
    tw = BR.tent_weights(k)
    x = d[s8] if dec else s8.astype(np.int64)
    p = np.pad(x, ((k // 2,) * 2, (k // 2,) * 2, (0, 0)), mode='edge')
    hs = sum(tw[i] * p[:, i:i + W:k] for i in range(2 * k))
    if hbits is not None:
        hs = hs & ((1 << hbits) - 1)
    vs = sum(tw[j] * hs[j:j + H:k] for j in range(2 * k))
    return (vs + (2 * k ** 4 if half is None else half)) >> (2 + 4 * _log2(k))


def tent_lin(s8, k, d=D, t=T, half=None, dec=True, enc=True, hbits=None):
    return _finish(tent_lin_mean(s8, k, d, half, dec, hbits), t, enc)


def mean_lin_mean(frames, d=D, half=None, dec=True, carry_bits=32):
    n = len(frames)
    assert n & (n - 1) == 0
    s = np.zeros(frames[0].shape, np.int64)
    for g in range(0, n, BR.GROUP):
        if g:
            s &= (1 << carry_bits) - 1
        s = s + sum((d[f] if dec else f.astype(np.int64)) for f in frames[g:g + BR.GROUP])
    return (s + (n // 2 if half is None else half)) >> _log2(n)


def mean_lin(frames, d=D, t=T, half=None, dec=True, enc=True, carry_bits=32):
    return _finish(mean_lin_mean(frames, d, half, dec, carry_bits), t, enc)


def _t_moved(v, by):
    t = T.copy()
    t[v] += by
    return t


def common_mutants(f, half):
    """[(name, function)] of a contract f(x, **kw) whose rounding constant is `half`: the mistakes every reduce can make."""
    out = [('the NONE contract', lambda x: f(x, d=D_NONE, t=T_NONE))]
    out += [('rounding constant %+d' % e, lambda x, e=e: f(x, half=half + e)) for e in (1, -1)]
    out += [('decode but no encode', lambda x: f(x, enc=False)), ('encode but no decode', lambda x: f(x, dec=False))]
    return out


def threshold_mutants(f, vs):
    return [('T[%d] %+d' % (v, e), lambda x, v=v, e=e: f(x, t=_t_moved(v, e))) for v in vs for e in (1, -1)]


def box_mutants(k):
    return common_mutants(lambda s, **kw: box_lin(s, k, **kw), k * k // 2)


def tent_mutants(k):
    f = lambda s, **kw: tent_lin(s, k, **kw)
    return common_mutants(f, 2 * k ** 4) + [('16-bit horizontal sums', lambda s: f(s, hbits=16))]


def mean_mutants(n):
    out = common_mutants(mean_lin, n // 2)
    if n > BR.GROUP:
        out.append(('16 bits between groups', lambda fr: mean_lin(fr, carry_bits=16)))
    return out


# ---- the threshold rasters ------------------------------------------------------------------------------------------------
def on_threshold():
    """For v = 1 .. 255 the four samples {v-1, v-1, v, v}: their mean (2 D[v-1] + 2 D[v] + 2) >> 2 IS T[v], by construction."""
    return [(v - 1, v - 1, v, v) for v in range(1, 256)]


_below = []


def below_threshold(reach=40):
    """{v: four samples within `reach` of v whose mean (SUM D + 2) >> 2 is T[v] - 1}: found by search over the multisets (pair
    sums, then pairs of pair sums); a v without one is left out."""
    if _below:
        return _below[0]
    found = {}
    for v in range(1, 256):
        lo, hi = max(0, v - reach), min(255, v + reach)
        vals = np.arange(lo, hi + 1)
        i, j = np.triu_indices(len(vals))
        ps = D[vals[i]] + D[vals[j]]
        order = np.argsort(ps, kind='stable')
        sp = ps[order]
        want_lo, want_hi = 4 * (T[v] - 1) - 2, 4 * (T[v] - 1) + 1       # (S + 2) >> 2 == T[v] - 1
        at = np.searchsorted(sp, want_lo - sp, side='left')
        ok = np.flatnonzero((at < len(sp)) & (sp[np.minimum(at, len(sp) - 1)] <= want_hi - sp))
        if len(ok):
            a, b = order[ok[0]], order[at[ok[0]]]
            four = (int(vals[i[a]]), int(vals[j[a]]), int(vals[i[b]]), int(vals[j[b]]))
            assert (int(D[list(four)].sum()) + 2) >> 2 == T[v] - 1
            found[v] = four
    _below.append(found)
    return found


def threshold_fours():
    """Every four-sample case: the 255 on a threshold, then those one below one."""
    return on_threshold() + [below_threshold()[v] for v in sorted(below_threshold())]


def threshold_box_raster():
    """(2 h, 2 w, 3) samples for k = 2: output pixel i holds case i of threshold_fours() as its 2 x 2 block (the channels hold the
    case rotated by 0, 1, 2 places, so that each sees every case's multiset), padded with zeros to whole rows of 32 pixels."""
    fours = threshold_fours()
    w = 32
    h = (len(fours) + w - 1) // w
    s = np.zeros((2 * h, 2 * w, 3), np.uint8)
    for i, f in enumerate(fours):
        y, x = divmod(i, w)
        for c in range(3):
            r = f[c:] + f[:c]
            s[2 * y, 2 * x, c], s[2 * y, 2 * x + 1, c], s[2 * y + 1, 2 * x, c], s[2 * y + 1, 2 * x + 1, c] = r
    return s


def threshold_frames(n):
    """n = 2: frames v-1 and v at byte v - 1 of a 255-byte row (the mean IS T[v]); n = 4: the four samples of every case of
    threshold_fours(), one per frame.  (h, 64, 3) frames (an atlas slice is at most 128 wide), h * 192 >= the cases."""
    cases = [(v - 1, v) for v in range(1, 256)] if n == 2 else threshold_fours()
    frames = [np.zeros(((len(cases) + 191) // 192, 64, 3), np.uint8) for _ in range(n)]
    for i, c in enumerate(cases):
        for k in range(n):
            frames[k].reshape(-1)[i] = c[k]
    return frames


def threshold_tent_raster():
    """(1024, 6, 3) samples for k = 2, constant along x: sample rows 4 v - 1, 4 v hold v and rows 4 v + 1, 4 v + 2 hold v - 1, so
    that output row 2 v sees (v, v, v-1, v-1) under the weights 1 3 3 1: M = (4 D[v] + 4 D[v-1] + 4) >> 3 = T[v]."""
    s = np.zeros((1024, 6, 3), np.uint8)
    for v in range(1, 256):
        s[4 * v - 1:4 * v + 1] = v
        s[4 * v + 1:4 * v + 3] = v - 1
    return s


# ---- the rounding step's critical sums ------------------------------------------------------------------------------------
# A rounding constant one off shows only where the sum is critical modulo W AND the mean crosses a threshold: random bytes do
# not get there (one byte in about 256 W).  So: `count` samples whose decoded sum is exactly count T[v] - count/2 (the mean IS
# T[v]; with the constant one less it is T[v] - 1) or one less than that (the mean is T[v] - 1; with the constant one more,
# T[v]).  count - 2 samples are drawn near v, the last two are looked up among the pair sums.
CRITICAL_VS = (20, 60, 100, 140, 180, 220)


def critical_values(count, v, below, reach=40, tries=200):
    rng = np.random.default_rng(1000 * count + 2 * v + below)
    lo, hi = max(0, v - reach), min(255, v + reach)
    vals = np.arange(lo, hi + 1)
    i, j = np.triu_indices(len(vals))
    ps = D[vals[i]] + D[vals[j]]
    target = count * int(T[v]) - count // 2 - (1 if below else 0)
    for _ in range(tries):
        rest = rng.integers(lo, hi + 1, count - 2)
        hit = np.flatnonzero(ps == target - int(D[rest].sum()))
        if len(hit):
            out = [int(a) for a in rest] + [int(vals[i[hit[0]]]), int(vals[j[hit[0]]])]
            assert int(D[out].sum()) == target
            return out
    return None


def below_threshold_k4():
    """{v: sixteen samples whose mean (SUM D + 8) >> 4 is T[v] - 1} for the v that the search over fours leaves out: at k = 4
    there is room for them."""
    missing = sorted(set(range(1, 256)) - set(below_threshold()))
    found = {v: critical_block(np.ones((4, 4), np.int64), 16 * int(T[v]) - 9, v, 9000 + v) for v in missing}
    return {v: [int(x) for x in c.reshape(-1)] for v, c in found.items() if c is not None}


def threshold_box_raster_k4():
    """(4, 4 n, 3) samples for k = 4: output pixel i holds case i of below_threshold_k4() as its 4 x 4 block."""
    cases = [c for _, c in sorted(below_threshold_k4().items())]
    s = np.zeros((4, 4 * max(1, len(cases)), 3), np.uint8)
    for i, c in enumerate(cases):
        s[:, 4 * i:4 * i + 4] = np.array(c, np.uint8).reshape(4, 4)[:, :, None]
    return s


def critical_cells(count):
    """[(v, below, values)] for the v of CRITICAL_VS that the search serves."""
    out = []
    for v in CRITICAL_VS:
        for below in (0, 1):
            c = critical_values(count, v, below)
            if c is not None:
                out.append((v, below, c))
    return out


def critical_raster(k, cells_across=4):
    """Samples for any k: per case of critical_cells(k^2) a square of 4 x 4 equal cells of k x k samples, the squares one below
    the other.  A raster of period k reduces to the same mean under the tent as under the box (t(u) + t(u + k) = 2k), so the
    squares' inner pixels sit on the same critical sums for both."""
    cells = critical_cells(k * k)
    n = cells_across * k
    s = np.zeros((n * len(cells), n, 3), np.uint8)
    for q, (v, below, c) in enumerate(cells):
        cell = np.array(c, np.uint8).reshape(k, k)
        for ch in range(3):
            s[q * n:(q + 1) * n, :, ch] = np.tile(np.roll(cell, ch, axis=1), (cells_across, cells_across))
    return s


# The tent's critical sums off the period.  A raster of period k gives the tent sums that are multiples of 4 k^2, never one
# below a multiple of W: its constant one too large cannot show there.  So: one footprint of 2k x 2k samples near v whose
# WEIGHTED sum SUM t(u) t(v) D[s] is exactly W T[v] - W/2 (the mean IS T[v]; the constant one less gives T[v] - 1) or one less
# (the mean is T[v] - 1; the constant one more gives T[v]).  The samples are drawn near v; single samples are then moved until
# what is left for the four corners (weight 1 each) is about 4 D[v], and the corners are looked up among the sums of four.
def _four_with_sum(vals, total):
    """Four of `vals` whose decoded sum is exactly `total`, or None."""
    i, j = np.triu_indices(len(vals))
    ps = D[vals[i]] + D[vals[j]]
    order = np.argsort(ps, kind='stable')
    sp = ps[order]
    at = np.minimum(np.searchsorted(sp, total - sp, side='left'), len(sp) - 1)
    ok = np.flatnonzero(sp[at] == total - sp)
    if not len(ok):
        return None
    a, b = order[ok[0]], order[at[ok[0]]]
    return [int(vals[i[a]]), int(vals[j[a]]), int(vals[i[b]]), int(vals[j[b]])]


def critical_footprint(k, v, below, reach=40, tries=50):
    """(2k, 2k) uint8 samples within `reach` of v with the weighted sum described above, or None."""
    tw = np.array(BR.tent_weights(k), np.int64)
    return critical_block(np.outer(tw, tw), 4 * k ** 4 * int(T[v]) - 2 * k ** 4 - (1 if below else 0), v, 7000 * k + 2 * v + below, reach, tries)


def critical_block(w, target, v, seed, reach=40, tries=50):
    """(n, n) uint8 samples within `reach` of v with SUM w D[s] == target, for square weights w whose corners are 1; or None."""
    rng = np.random.default_rng(seed)
    lo, hi = max(0, v - reach), min(255, v + reach)
    vals = np.arange(lo, hi + 1)
    n = w.shape[0]
    corners = [(0, 0), (0, n - 1), (n - 1, 0), (n - 1, n - 1)]
    inner = [(a, b) for a in range(n) for b in range(n) if (a, b) not in corners]
    for _ in range(tries):
        s = rng.integers(lo, hi + 1, (n, n))
        for _ in range(40 * n * n):
            left = target - int((w * D[s]).sum()) + sum(int(D[s[c]]) for c in corners)       # what the corners have to hold
            err = left - 4 * int(D[v])
            if abs(err) < 2 * int(D[min(255, v + 1)] - D[v - 1]):
                break
            a, b = inner[rng.integers(len(inner))]
            s[a, b] = vals[np.argmin(np.abs(D[vals] - (D[s[a, b]] + err / w[a, b])))]
        four = _four_with_sum(vals, left)
        if four is not None:
            for c, x in zip(corners, four):
                s[c] = x
            assert int((w * D[s]).sum()) == target
            return s.astype(np.uint8)
    return None


def critical_tent_cells(k):
    """[(v, below, footprint)] for the v of CRITICAL_VS that the search serves."""
    out = []
    for v in CRITICAL_VS:
        for below in (0, 1):
            f = critical_footprint(k, v, below)
            if f is not None:
                out.append((v, below, f))
    return out


_tent_rasters = {}


def critical_tent_raster(k):
    """(3 k cells, 3 k, 3) samples: per case of critical_tent_cells(k) a cell of 3 x 3 output pixels whose centre pixel
    (row 3 q + 1, column 1) has the case's footprint, sample rows and columns k/2 .. k/2 + 2k - 1 of the cell, in every channel;
    the rest of a cell holds v.  critical_tent_centres(k): [(row, v, below)] of the centre pixels."""
    if k not in _tent_rasters:
        cells = critical_tent_cells(k)
        s = np.zeros((3 * k * len(cells), 3 * k, 3), np.uint8)
        for q, (v, below, f) in enumerate(cells):
            s[3 * k * q:3 * k * (q + 1)] = v
            s[3 * k * q + k // 2:3 * k * q + k // 2 + 2 * k, k // 2:k // 2 + 2 * k] = f[:, :, None]
        _tent_rasters[k] = (s, [(3 * q + 1, v, below) for q, (v, below, f) in enumerate(cells)])
    return _tent_rasters[k][0]


def critical_tent_centres(k):
    critical_tent_raster(k)
    return _tent_rasters[k][1]


def critical_frames(n):
    """n frames of (1, w, 3): byte i holds case i of critical_cells(n), one value per frame."""
    cells = critical_cells(n)
    w = (len(cells) + 2) // 3
    frames = [np.zeros((1, w, 3), np.uint8) for _ in range(n)]
    for i, (v, below, c) in enumerate(cells):
        for k in range(n):
            frames[k].reshape(-1)[i] = c[k]
    return frames

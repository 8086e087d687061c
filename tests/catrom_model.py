"""The Catmull-Rom reconstruction filter's contract in numpy (include/maray_hip.h, "reconstruction filter"): what
tests/test_gpu_catrom.py and tests/test_gpu_catrom_bytes.py compare the device with, byte for byte.

Also here: the crafted rasters that reach the output clamp (uniform random bytes almost never do), and MUTANTS of the
contract -- the contract with one thing wrong, the way a kernel goes wrong.  tests/test_catrom.py checks, without a device,
that the rasters the GPU tests use tell every mutant from the contract."""
import numpy as np

import byte_rasters as BR

KS = (2, 4, 8)


def e(u, k):
    """2 D^3 CatmullRom(n / D), n = |2u + 1 - k|, D = 2k: an integer."""
    n, d = abs(2 * u + 1 - k), 2 * k
    assert n != d and n < 2 * d
    return 3 * n ** 3 - 5 * n * n * d + 2 * d ** 3 if n < d else -n ** 3 + 5 * n * n * d - 8 * n * d * d + 4 * d ** 3


def footprint(k):
    """u = -3k/2 .. 5k/2 - 1: the 4k sample offsets of a pixel, per axis."""
    return range(-(3 * k // 2), 5 * k // 2)


def weights(k):
    return [e(u, k) for u in footprint(k)]


def norm(k):
    """(W, log2 W), W = (16 k^4)^2."""
    w = (16 * k ** 4) ** 2
    shift = w.bit_length() - 1
    assert 1 << shift == w
    return w, shift


def catrom_sums(s8, k, th=None, tv=None):
    """The weighted sums before rounding, (h, w, 3) int64, separably: horizontal sums, then vertical."""
    H, W, _ = s8.shape
    t = weights(k)
    th, tv = th or t, tv or t
    pad = 3 * k // 2
    p = np.pad(s8.astype(np.int64), ((pad, pad), (pad, pad), (0, 0)), mode='edge')
    hs = sum(th[i] * p[:, i:i + W:k] for i in range(4 * k))
    return sum(tv[j] * hs[j:j + H:k] for j in range(4 * k))


def finish(sums, k):
    w, shift = norm(k)
    return np.clip((sums + w // 2) >> shift, 0, 255).astype(np.uint8)


def catrom(s8, k):
    """(k h, k w, 3) uint8 -> (h, w, 3): the contract."""
    return finish(catrom_sums(s8, k), k)


def catrom_direct(s8, k):
    """out = min(max((SUM_u SUM_v e(u) e(v) s(clamp(k px + u), clamp(k py + v), c) + W/2) >> log2 W, 0), 255): as written."""
    H, W, _ = s8.shape
    h, w = H // k, W // k
    big_w, shift = norm(k)
    out = np.zeros((h, w, 3), np.uint8)
    for py in range(h):
        for px in range(w):
            for c in range(3):
                acc = 0
                for u in footprint(k):
                    a = min(max(k * px + u, 0), W - 1)
                    for v in footprint(k):
                        b = min(max(k * py + v, 0), H - 1)
                        acc += e(u, k) * e(v, k) * int(s8[b, a, c])
                out[py, px, c] = min(max((acc + big_w // 2) >> shift, 0), 255)
    return out


# ---- the crafted rasters -----------------------------------------------------------------------------------------------
# 69 x 19 output pixels: two tiles of 64 (three of 32 at k = 8) and three tiles of rows; the chosen pixel is the first of the
# second tile of columns, in the second tile of rows of every k
LOBE_W, LOBE_H, LOBE_PX, LOBE_PY = 69, 19, 64, 9


def lobe_raster(k, w=LOBE_W, h=LOBE_H, px=LOBE_PX, py=LOBE_PY):
    """255 where e(u) e(v) > 0 in the footprint of the interior pixel (px, py), 0 elsewhere: that pixel's sum is the largest
    there is, 255 (P^2 + N^2) with P, N the sums of the positive and of the negative weights; its inverse's is the smallest,
    -255 * 2 P N."""
    assert 2 <= px < w - 2 and 2 <= py < h - 2
    s = np.zeros((k * h, k * w, 3), np.uint8)
    for u in footprint(k):
        for v in footprint(k):
            if e(u, k) * e(v, k) > 0:
                s[k * py + v, k * px + u] = 255
    return s


def lobe_inverse(k, **kw):
    return 255 - lobe_raster(k, **kw)


def impulse_raster(k, w=LOBE_W, h=LOBE_H):
    """Single samples of 255 on black: the four corners, and one sample before, at and after the boundaries between the
    kernel's tiles (columns 32 and 64, rows 8 and 16), channel by channel."""
    s = np.zeros((k * h, k * w, 3), np.uint8)
    H, W = k * h, k * w
    s[0, 0, 0] = s[0, W - 1, 1] = s[H - 1, 0, 2] = s[H - 1, W - 1, 0] = 255
    for i, d in enumerate((-1, 0, 1)):
        s[k * 4 + i, k * 32 + d, i] = 255           # column boundaries, in rows apart (no footprint holds two of them)
        s[k * 12 + i, k * 64 + d, i] = 255
        s[k * 8 + d, k * 10 + 5 * k * i, i] = 255   # row boundaries, in columns apart
        s[k * 16 + d, k * 40 + 5 * k * i, i] = 255
    return s


def gpu_rasters(k):
    """[(name, samples, output width, output height)]: the rasters of tests/test_gpu_catrom_bytes.py."""
    return [('parity', BR.parity_raster(k), BR.PARITY_W, BR.PARITY_H),
            ('lobe', lobe_raster(k), LOBE_W, LOBE_H), ('lobe inverse', lobe_inverse(k), LOBE_W, LOBE_H),
            ('impulses', impulse_raster(k), LOBE_W, LOBE_H),
            ('zeros', BR.constant(0, k * LOBE_H, k * LOBE_W), LOBE_W, LOBE_H), ('ones', BR.constant(255, k * LOBE_H, k * LOBE_W), LOBE_W, LOBE_H)]


# ---- the contract, with room for one mistake ---------------------------------------------------------------------------
def lobes_swapped(k):
    """The weights with the negative outer lobe and the positive inner one exchanged on either side."""
    t = weights(k)
    return t[k:2 * k] + t[0:k] + t[3 * k:4 * k] + t[2 * k:3 * k]


def wrap32(s, signed):
    s = np.asarray(s, np.int64) & 0xFFFFFFFF
    return np.where(s >= 1 << 31, s - (1 << 32), s) if signed else s


def catrom_banded(s8, k, band_rows, halo):
    """The contract cut into bands of band_rows output rows whose sample rows are clamped to the band plus `halo` rows (clipped
    to the image) instead of to the image: halo = 3k/2 is the contract again, k/2 the tent's halo, 0 a clamp to the band."""
    H, W, _ = s8.shape
    h = H // k
    out = []
    for o0 in range(0, h, band_rows):
        o1 = min(h, o0 + band_rows)
        lo, hi = max(0, k * o0 - halo), min(H, k * o1 + halo)
        rows = np.clip(np.arange(k * o0 - 3 * k // 2, k * o1 + 3 * k // 2), lo, hi - 1)
        out.append(_band_rows(s8[rows], k, o1 - o0))        # the band's 3k/2 + k n + 3k/2 rows, clamped the mutant's way
    return np.concatenate(out)


def _band_rows(slab, k, n):
    """Output rows of a slab that holds exactly the footprints' rows of n output rows: row j reads slab rows k j .. k j + 4k - 1."""
    W = slab.shape[1]
    t = weights(k)
    pad = 3 * k // 2
    p = np.pad(slab.astype(np.int64), ((0, 0), (pad, pad), (0, 0)), mode='edge')
    hs = sum(t[i] * p[:, i:i + W:k] for i in range(4 * k))
    return finish(sum(t[j] * hs[j:j + k * n:k] for j in range(4 * k)), k)


BAND_ROWS = (1, 3, 8)       # MARAY_FILTER_BAND_ROWS of tests/test_gpu_catrom_bytes.py::test_band_rows, on the parity raster


def band_mutants(k, band_rows):
    """The mutants that show only where a picture is cut into bands of band_rows output rows."""
    return [("the tent's halo", lambda s: catrom_banded(s, k, band_rows, k // 2)),
            ('indices clamped to the band', lambda s: catrom_banded(s, k, band_rows, 0))]


def mutants(k):
    """[(name, function samples -> picture)]: each the contract with one thing wrong, whatever the bands."""
    big_w, shift = norm(k)
    half = big_w // 2
    sw = lobes_swapped(k)
    out = [
        ('no clamp: the shifted sum wraps to a byte', lambda s: ((catrom_sums(s, k) + half) >> shift).astype(np.uint8)),
        ('clamped at 255 only', lambda s: np.minimum((catrom_sums(s, k) + half) >> shift, 255).astype(np.uint8)),
        ('clamped at 0 only', lambda s: np.maximum((catrom_sums(s, k) + half) >> shift, 0).astype(np.uint8)),
        ('horizontal lobes swapped', lambda s: finish(catrom_sums(s, k, th=sw), k)),
        ('vertical lobes swapped', lambda s: finish(catrom_sums(s, k, tv=sw), k)),
        ('W/2 left out', lambda s: np.clip(catrom_sums(s, k) >> shift, 0, 255).astype(np.uint8)),
    ]
    if k > 2:       # (at k = 2 the full sum has 25 bits: 32 are right)
        # the sum keeps its low 32 bits only, read as signed or as unsigned; rounding, shift and clamp are the contract's
        out += [
            ('32-bit signed vertical sums', lambda s: finish(wrap32(catrom_sums(s, k), True), k)),
            ('32-bit unsigned vertical sums', lambda s: finish(wrap32(catrom_sums(s, k), False), k)),
        ]
    return out

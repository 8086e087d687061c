"""Sample rasters of any bytes for the two byte kernels (maray_filter_tent<K>, maray_shutter_reduce): the helpers of
tests/test_byte_rasters.py, tests/test_gpu_filter_bytes.py and tests/test_gpu_shutter_bytes.py.

A texture lookup truncates its coordinates and returns the stored byte, so a scene that reads texture 0 at (X, Y) renders
the texture itself: the sample raster of a tent or box context, and the n frames of a shutter call, are then whatever bytes
a test chooses, and the expected picture is plain numpy on those bytes (tent, box, mean) with no oracle render.

Also here: the kinds of rasters, and MUTANTS of the two numpy contracts -- the contract with one thing wrong, the way a
kernel goes wrong (a weight, a lane's footprint, a halo row, a channel, the rounding, a clamp; a frame, a group, a carry).
A raster on which a mutant equals its contract could not show that fault on the device; tests/test_byte_rasters.py checks,
without a device, that the rasters the GPU tests use tell every mutant from its contract.
"""
import numpy as np

import maray_amd as M
from marayb import add, app, channel, encode, mul, nat, var, x, y

PITCH = 128             # the atlas' pitch: no frame of a shutter test is wider
T_MAX = 63              # slices 0 .. 63: the most frames a shutter call takes


# ---- the scenes --------------------------------------------------------------------------------------------------------
def identity_color():
    """Texture 0 at (X, Y), channel by channel.  No size occurs in it: one program for every k and every size."""
    return [app(channel(0, c), x(), y()) for c in range(3)]


def identity_scene():
    return M.Scene(encode((64, 64), identity_color()))


def atlas_color(pitch=PITCH):
    """Texture 0 at (X + t pitch, Y): slice t of an atlas (below)."""
    return [app(channel(0, c), add(x(), mul(var('t'), nat(pitch))), y()) for c in range(3)]


def atlas_scene(pitch=PITCH):
    s = M.Scene(encode((64, 64), atlas_color(pitch)))
    assert s.declare_param('t', 0.0, float(T_MAX)) == 0
    return s


def atlas(frames, pitch=PITCH, fill=0xA5):
    """n frames (h, w, 3), w <= pitch, side by side at `pitch`; what no frame covers holds `fill`."""
    h, w, _ = frames[0].shape
    assert w <= pitch and len(frames) <= T_MAX + 1
    a = np.full((h, len(frames) * pitch, 3), fill, np.uint8)
    for i, f in enumerate(frames):
        assert f.shape == (h, w, 3) and f.dtype == np.uint8
        a[:, i * pitch:i * pitch + w] = f
    return a


# ---- the rasters -------------------------------------------------------------------------------------------------------
def random_bytes(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def random_frames(seed, n, h, w):
    return list(np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8))


def constant(v, h, w):
    return np.full((h, w, 3), v, np.uint8)


def checker(h, w):
    """0 / 255 at one-sample pitch."""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)


def impulse_positions(k, n_samples):
    """Sample indices 2k + 1 apart: no footprint (2k samples) holds two of them, and since 2k + 1 = 1 modulo k, k
    consecutive ones sit at every offset modulo k, which is every footprint position 0 .. 2k - 1 (a sample at offset r
    of its pixel is position r + k/2 of that pixel's footprint and r + k/2 +- k of a neighbour's).  None within k samples of
    either end: no clamped index reads one twice."""
    return np.arange(k, n_samples - k, 2 * k + 1)


def column_impulses(h, w, k):
    """Single sample columns on black, column j in channel j modulo 3 (3 and k are coprime: 3k columns give every position
    in every channel)."""
    s = np.zeros((h, w, 3), np.uint8)
    for j, a in enumerate(impulse_positions(k, w)):
        s[:, a, j % 3] = 255
    return s


def row_impulses(h, w, k):
    """Single sample rows of white on black."""
    s = np.zeros((h, w, 3), np.uint8)
    s[impulse_positions(k, h)] = 255
    return s


def footprint_positions_hit(k, n_samples):
    """The footprint positions 0 .. 2k - 1 at which some pixel of an axis of n_samples samples sees an impulse."""
    hit = set()
    for a in impulse_positions(k, n_samples):
        for p in range(n_samples // k):
            i = int(a) - (k * p - k // 2)
            if 0 <= i < 2 * k:
                hit.add(i)
    return hit


def extreme_rasters(h, w, k):
    """(name, (k h, k w, 3) samples) of the extremes: the largest sums, and every weight on its own."""
    H, W = k * h, k * w
    return [('zeros', constant(0, H, W)), ('ones', constant(255, H, W)), ('checker', checker(H, W)),
            ('columns', column_impulses(H, W, k)), ('rows', row_impulses(H, W, k))]


# the random raster of the parity tests: 65 x 37 output pixels; with these seeds some output byte's weighted sum is exactly
# W/2 modulo W = 4 k^4 and some is W/2 - 1 (found by trying seeds 0, 1, 2, ... in turn; tests/test_byte_rasters.py checks it)
PARITY_W, PARITY_H = 65, 37
PARITY_SEED = {2: 0, 4: 0, 8: 2}


def parity_raster(k):
    return random_bytes(PARITY_SEED[k], PARITY_H * k, PARITY_W * k)


# the geometry tests' widths: 1 and 2 make every lane an edge lane; odd w at k = 2 is a row pitch of 2 modulo 4, so that all
# four shifts of a misaligned dword occur; one below, at and one above the kernel's tile of 64 pixels; two tiles and one
GEOMETRY_WS, GEOMETRY_H = (1, 2, 3, 5, 21, 63, 64, 65, 129), 19
DESTINATION_WS, DESTINATION_KS, DESTINATION_H = (1, 5, 64, 65), (2, 8), 23
STREAMS_W, STREAMS_H, STREAMS_K = 333, 120, 4
EXTREMES_W, EXTREMES_H = 65, 17


def geometry_raster(k, w):
    return random_bytes(100 * k + w, GEOMETRY_H * k, w * k)


def destination_raster(k, w):
    return random_bytes(500 * k + w, DESTINATION_H * k, w * k)


def streams_raster():
    return random_bytes(7, STREAMS_H * STREAMS_K, STREAMS_W * STREAMS_K)


# ---- the tent contract, with room for one mistake ----------------------------------------------------------------------
def tent_weights(k):
    return [2 * k - abs(2 * u + 1 - k) for u in range(-(k // 2), 3 * k // 2)]


def tent_general(s8, k, th=None, tv=None, dx=None, dy=0, half=None, chan=None, zero=()):
    """include/maray_hip.h, "reconstruction filter", by gathering: (k h, k w, 3) uint8 -> (h, w, 3).  With the defaults it is
    the contract (tests/test_filter.py::tent).  th, tv: the horizontal and vertical weights; dx: per output column, samples its
    footprint is moved by; dy: sample rows every footprint is moved by; half: the rounding constant; chan = (i, c): footprint
    position i reads channel c + 1 for channel c; zero: which of 'left', 'right', 'top', 'bottom' read 0 past the image's
    edge where the contract clamps."""
    H, W, _ = s8.shape
    h, w = H // k, W // k
    t = tent_weights(k)
    th, tv = th or t, tv or t
    half = 2 * k ** 4 if half is None else half
    s = s8.astype(np.int64)
    px, py = np.arange(w), np.arange(h)
    dxv = np.zeros(w, np.int64) if dx is None else np.asarray(dx, np.int64)
    hs = np.zeros((H, w, 3), np.int64)
    for i in range(2 * k):
        a = k * px + i - k // 2 + dxv
        v = s[:, np.clip(a, 0, W - 1), :]
        if chan is not None and chan[0] == i:
            v = v.copy()
            v[..., chan[1]] = s[:, np.clip(a, 0, W - 1), (chan[1] + 1) % 3]
        if 'left' in zero:
            v = np.where((a < 0)[None, :, None], 0, v)
        if 'right' in zero:
            v = np.where((a > W - 1)[None, :, None], 0, v)
        hs += th[i] * v
    vs = np.zeros((h, w, 3), np.int64)
    for j in range(2 * k):
        b = k * py + j - k // 2 + dy
        v = hs[np.clip(b, 0, H - 1)]
        if 'top' in zero:
            v = np.where((b < 0)[:, None, None], 0, v)
        if 'bottom' in zero:
            v = np.where((b > H - 1)[:, None, None], 0, v)
        vs += tv[j] * v
    return ((vs + half) >> (2 + 4 * (k.bit_length() - 1))).astype(np.uint8)


def tent_sums(s8, k):
    """The weighted sums before rounding, (h, w, 3) int64."""
    H, W, _ = s8.shape
    t = tent_weights(k)
    p = np.pad(s8.astype(np.int64), ((k // 2,) * 2, (k // 2,) * 2, (0, 0)), mode='edge')
    hs = sum(t[i] * p[:, i:i + W:k] for i in range(2 * k))
    return sum(t[j] * hs[j:j + H:k] for j in range(2 * k))


def _swapped(t, i):
    t = list(t)
    t[i], t[i + 1] = t[i + 1], t[i]
    return t


def tent_mutants(k, w):
    """[(name, kind, function samples -> picture)] for output width w; kind is 'sideways', 'row' or None."""
    t = tent_weights(k)
    out = []
    for i in range(2 * k - 1):
        if t[i] != t[i + 1]:
            out.append(('horizontal weights %d and %d swapped' % (i, i + 1), None, lambda s, i=i: tent_general(s, k, th=_swapped(t, i))))
            out.append(('vertical weights %d and %d swapped' % (i, i + 1), None, lambda s, i=i: tent_general(s, k, tv=_swapped(t, i))))
    for r in range(4):
        for d in (1, -1):
            dx = np.where(np.arange(w) % 4 == r, d, 0)
            out.append(('footprint of pixels %d modulo 4 moved %+d' % (r, d), None, lambda s, dx=dx: tent_general(s, k, dx=dx)))
    for d in (1, -1):
        out.append(('every footprint moved %+d sideways' % d, 'sideways', lambda s, d=d: tent_general(s, k, dx=np.full(w, d))))
        out.append(('every footprint moved %+d rows' % d, 'row', lambda s, d=d: tent_general(s, k, dy=d)))
    for i in range(2 * k):
        for c in range(3):
            out.append(('position %d reads channel %d for channel %d' % (i, (c + 1) % 3, c), None, lambda s, i=i, c=c: tent_general(s, k, chan=(i, c))))
    for d in (1, -1):
        out.append(('rounding constant %+d' % d, None, lambda s, d=d: tent_general(s, k, half=2 * k ** 4 + d)))
    for edge in ('left', 'right', 'top', 'bottom'):
        out.append(('zero past the %s edge' % edge, None, lambda s, edge=edge: tent_general(s, k, zero=(edge,))))
    return out


# ---- the shutter's contract, with room for one mistake -----------------------------------------------------------------
GROUP = 8               # frames a pass of maray_shutter_reduce takes


def mean_general(frames, half=None, twice=None, drop_first_group=False, carry_bits=16):
    """(S + n/2) >> log2 n over the frames in groups of 8, in the order given; with the defaults the contract
    (tests/test_gpu_shutter.py::mean).  half: the rounding constant; twice = i: frame i counted twice, frame i + 1 not at
    all; drop_first_group: what the first group summed is lost (n > 8); carry_bits: the bits of the sum that pass from one
    group to the next."""
    n = len(frames)
    assert n & (n - 1) == 0
    pick = list(range(n))
    if twice is not None:
        pick[twice + 1] = twice
    s = np.zeros(frames[0].shape, np.int64)
    for g in range(0, n, GROUP):
        if g:
            s &= (1 << carry_bits) - 1
        part = sum(frames[i].astype(np.int64) for i in pick[g:g + GROUP])
        s = s + (0 if (drop_first_group and g == 0 and n > GROUP) else part)
    return ((s + (n // 2 if half is None else half)) >> (n.bit_length() - 1)).astype(np.uint8)


def mean_mutants(n):
    out = [('rounding constant %+d' % d, lambda f, d=d: mean_general(f, half=n // 2 + d)) for d in (1, -1)]
    out += [('frame %d twice, frame %d dropped' % (i, i + 1), lambda f, i=i: mean_general(f, twice=i)) for i in range(n - 1)]
    if n > GROUP:
        out.append(('the first group dropped', lambda f: mean_general(f, drop_first_group=True)))
        out.append(('8 bits between groups', lambda f: mean_general(f, carry_bits=8)))
    return out


# ---- the shutter tests' frames -----------------------------------------------------------------------------------------
SHUTTER_W, SHUTTER_H = 67, 41
SHUTTER_NS = (2, 4, 8, 16, 32, 64)


def shutter_case(n, w=SHUTTER_W, h=SHUTTER_H):
    """(frames, order): n random frames, and the shuffled order their parameter rows are passed in (the contract's mean does
    not depend on it; a reduce that mixes up its groups does)."""
    frames = random_frames(1000 + n, n, h, w)
    order = [int(i) for i in np.random.default_rng(2000 + n).permutation(n)]
    return frames, order


def one_byte_frames(n, h, w):
    """n frames equal but for one byte each: frame i has byte i * (bytes - 1) / (n - 1) of a random frame inverted (the first
    byte in frame 0, the last in frame n - 1)."""
    base = random_bytes(3000 + n, h, w)
    frames = []
    for i in range(n):
        f = base.copy()
        f.reshape(-1)[i * (base.size - 1) // (n - 1)] ^= 0xFF
        frames.append(f)
    return frames


# the head-and-tail test: rasters of w x rows pixels, 3 .. 105 bytes (fewer than one 16-byte vector, a head only, a head and a
# tail), cut from the top left of these frames.  The seeds are the first with which the 105 bytes of 5 x 7 hold both critical
# sums of the rounding for their n (found by trying 0, 1, 2, ... in turn; tests/test_byte_rasters.py checks the consequence)
HEAD_TAIL_WS, HEAD_TAIL_ROWS, HEAD_TAIL_NS = (1, 5), tuple(range(1, 8)), (2, 8, 16, 64)
HEAD_TAIL_SEED = {2: 0, 8: 0, 16: 0, 64: 0}


def head_tail_case(n):
    frames = random_frames(4000 + 100 * HEAD_TAIL_SEED[n] + n, n, HEAD_TAIL_ROWS[-1], HEAD_TAIL_WS[-1])
    order = [int(i) for i in np.random.default_rng(5000 + n).permutation(n)]
    return frames, order

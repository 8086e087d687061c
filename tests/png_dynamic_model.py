"""A model of the device PNG encoder's dynamic coder (include/maray_hip.h, "device PNG encoder": MARAY_PNG_CODES_DYNAMIC) in
numpy and plain Python, no device needed: the helper of tests/test_png_dynamic_abi.py and tests/test_gpu_png_dynamic.py.

  token_counts   the tokeniser restated: the 286 literal/length counts and 30 distance counts of a band, symbol 256 included
  huffman        an unrestricted Huffman tree of counts: (cost in bits, depth)
  piece_bound    the derived bound of a band's piece in bytes
"""
import heapq

import numpy as np

SEG = 256               # pixels per segment
STEP = 64               # a run is closed at every STEP pixels of a segment
HEADER_MAX_BITS = 17 + 19 * 3 + 316 * 7      # 3 + 5 + 5 + 4, the code-length code, 286 + 30 lengths of 7 bits: no run symbols


def length_symbol(n):
    """(symbol, extra bits) of a match of n bytes, 3 .. 258 (RFC 1951, 3.2.5)."""
    if n == 258:
        return 285, 0
    l = n - 3
    if l < 8:
        return 257 + l, 0
    e = l.bit_length() - 3
    return 261 + 4 * e + ((l >> e) & 3), e


def token_counts(img):
    """(lit[286], dist[30], extra): the counts of a band's tokens -- img is the band's (rows, w, 3) uint8 -- with symbol 256
    counted once, and the sum of the matches' extra bits.  Each row is the filter byte 0 and its pixels in segments of SEG;
    a segment's first pixel is literal; in steps of STEP pixels a run of pixels equal to the pixel before them is one match of
    distance 3 over the run's bytes, closed at the step's end."""
    rows, w, _ = img.shape
    lit, dist = np.zeros(286, np.int64), np.zeros(30, np.int64)
    lit[0] += rows
    lit[256] += 1
    flat = img.astype(np.int64)
    key = (flat[:, :, 0] << 16) | (flat[:, :, 1] << 8) | flat[:, :, 2]
    eq = np.zeros((rows, w), bool)
    eq[:, 1:] = key[:, 1:] == key[:, :-1]
    eq[:, ::SEG] = False                                        # a segment's first pixel
    literal = ~eq
    for c in range(3):
        lit[:256] += np.bincount(flat[:, :, c][literal], minlength=256)
    # a match starts at an equal pixel whose predecessor is not equal, or at a step's first pixel
    x = np.arange(w)
    step_first = (x % SEG) % STEP == 0
    prev_eq = np.zeros((rows, w), bool)
    prev_eq[:, 1:] = eq[:, :-1]
    start = eq & (~prev_eq | step_first[None, :])
    # it runs on to the next pixel that does not continue it: one that is not equal, or a step's (or row's) first
    cont = (eq & ~step_first[None, :]).reshape(-1)
    breaks = np.concatenate([np.nonzero(~cont)[0], [rows * w]])
    starts = np.nonzero(start.reshape(-1))[0]
    runs = breaks[np.searchsorted(breaks, starts, side='right')] - starts
    extra = 0
    for run, n in zip(*np.unique(runs, return_counts=True)):
        assert 1 <= run <= STEP
        sym, e = length_symbol(3 * int(run))
        lit[sym] += int(n)
        extra += e * int(n)
    dist[2] = len(starts)
    return lit, dist, extra


def huffman(counts):
    """(cost, depth) of an unrestricted Huffman tree of the counts above 0: cost = sum count x length (unique), depth = the
    longest code of THIS tree (ties are broken towards the shallower subtree, which keeps the depth low).  One symbol: (0, 0)."""
    heap = [(int(c), 0) for c in counts if c > 0]
    if len(heap) < 2:
        return 0, 0
    heapq.heapify(heap)
    cost = 0
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        cost += a[0] + b[0]
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1))
    return cost, heap[0][1]


def token_bits(img):
    """T of piece_bound: the optimal cost of the band's literal/length symbols (256 included) + the extra bits + one bit per
    match; and the depth of the tree that gives it."""
    lit, dist, extra = token_counts(img)
    cost, depth = huffman(lit)
    return cost + extra + int(dist[2]), depth


def piece_bound(img):
    """ceil((2286 + T) / 8) + 5 bytes: the worst header without run symbols, the tokens at their optimal cost, the stored
    block's three bits and the padding within the rounding and the + 5, 00 00 FF FF."""
    t, _ = token_bits(img)
    return -(-(HEADER_MAX_BITS + t) // 8) + 5


def kraft(lens):
    """The Kraft sum of the lengths above 0, in units of 2^-15."""
    return sum(1 << (15 - int(l)) for l in lens if l)


def fixed_cost(lit):
    """Bits of the literal/length symbols under the fixed codes (RFC 1951, 3.2.6)."""
    fixed = np.concatenate([np.full(144, 8), np.full(112, 9), np.full(24, 7), np.full(6, 8)])
    return int((np.asarray(lit, np.int64) * fixed).sum())

"""A model of the device PNG encoder's row filters (include/maray_hip.h, "Row filters") in numpy, no device needed: the helper
of tests/test_png_filter_abi.py and tests/test_gpu_png_filter.py.

  filter_raster    the five PNG filters (bpp = 3) over whole rows: neighbours left of x = 0 and above row 0 are 0
  segment_costs    the tokeniser restated on filtered rows: per segment the bytes it occupies as a fixed-Huffman segment and
                   its token bits (tests/png_dynamic_model.py's token_counts, kept per segment)
  choose           the selection rule: per row the smallest (bytes, bits, type)
  fixed_file_size  the exact size of the fixed-code file
"""
import numpy as np

import png_dynamic_model as D

SEG, STEP = D.SEG, D.STEP
NONE, ADAPTIVE, SUB, UP, AVERAGE, PAETH = range(6)       # MARAY_PNG_FILTER_*
CONTAINER = 8 + 25 + 12 + 12                            # signature, IHDR, one IDAT's frame, IEND
ZLIB_FRAME = 2 + 5 + 4                                  # 78 01, the final empty stored block, the Adler-32


def filter_raster(img, t):
    """img (h, w, 3) uint8 with PNG filter type t (0 .. 4) on every row -> (h, w, 3) uint8.  A row's filtered bytes depend on
    the raster's rows y and y - 1 alone, so the rows of any mix of types are rows of these five."""
    x = img.astype(np.int64)
    a, b, c = np.zeros_like(x), np.zeros_like(x), np.zeros_like(x)
    a[:, 1:] = x[:, :-1]
    b[1:] = x[:-1]
    c[1:, 1:] = x[:-1, :-1]
    if t == 0:
        pred = np.zeros_like(x)
    elif t == 1:
        pred = a
    elif t == 2:
        pred = b
    elif t == 3:
        pred = (a + b) >> 1                             # the floor of the 9-bit sum's half
    else:
        p = a + b - c
        pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
        pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))      # ties: a, b, c
    return ((x - pred) & 255).astype(np.uint8)


def filter_rows(img, types):
    """The filtered raster whose row y has type types[y]."""
    all5 = [filter_raster(img, t) for t in range(5)]
    return np.stack([all5[int(t)][y] for y, t in enumerate(types)])


_MATCH_BITS = np.zeros(STEP + 1, np.int64)
for _run in range(1, STEP + 1):
    _sym, _e = D.length_symbol(3 * _run)
    _MATCH_BITS[_run] = (7 if _sym < 280 else 8) + _e + 5      # the fixed length code, the extra bits, distance code 2


def token_bits(f):
    """(h, w): the bits of the token that starts at each pixel of the filtered raster f under the fixed codes, 0 where none
    starts.  The structure is png_dynamic_model.token_counts': a segment's first pixel is literal; in steps of STEP pixels a
    run of pixels equal to the pixel before them is one match of distance 3, closed at the step's end."""
    rows, w, _ = f.shape
    flat = f.astype(np.int64)
    key = (flat[:, :, 0] << 16) | (flat[:, :, 1] << 8) | flat[:, :, 2]
    eq = np.zeros((rows, w), bool)
    eq[:, 1:] = key[:, 1:] == key[:, :-1]
    eq[:, ::SEG] = False
    bits = np.where(~eq, 24 + (flat >= 144).sum(axis=2), 0)
    x = np.arange(w)
    step_first = (x % SEG) % STEP == 0
    prev_eq = np.zeros((rows, w), bool)
    prev_eq[:, 1:] = eq[:, :-1]
    start = eq & (~prev_eq | step_first[None, :])
    cont = (eq & ~step_first[None, :]).reshape(-1)
    breaks = np.concatenate([np.nonzero(~cont)[0], [rows * w]])
    starts = np.nonzero(start.reshape(-1))[0]
    runs = breaks[np.searchsorted(breaks, starts, side='right')] - starts
    assert not len(runs) or (1 <= runs.min() and runs.max() <= STEP)
    bits.reshape(-1)[starts] = _MATCH_BITS[runs]
    return bits


def segment_costs(f):
    """(bytes, bits), each (h, segments): what each segment of the filtered raster f occupies as a fixed-Huffman segment --
    the block header's 3 bits, in a row's first segment the filter byte's 8 (every type is a literal below 144), the tokens,
    the end-of-block's 7, the stored block's 3, zeros to the byte, 00 00 FF FF -- and its bits up to the end-of-block."""
    w = f.shape[1]
    tok = np.add.reduceat(token_bits(f), np.arange(0, w, SEG), axis=1)
    bits = 3 + tok
    bits[:, 0] += 8
    return ((bits + 7 + 3 + 7) >> 3) + 4, bits


def row_costs(img):
    """(bytes, bits), each (h, 5): a row's sums over its segments under each of the five types."""
    by, bi = zip(*[segment_costs(filter_raster(img, t)) for t in range(5)])
    return np.stack([b.sum(axis=1) for b in by], axis=1), np.stack([b.sum(axis=1) for b in bi], axis=1)


def choose(img, option=ADAPTIVE):
    """The PNG filter type of every row under MARAY_PNG_FILTER_* `option`: ADAPTIVE takes the smallest (bytes, bits, type)."""
    h = img.shape[0]
    if option != ADAPTIVE:
        return np.full(h, 0 if option == NONE else option - 1, np.int64)
    by, bi = row_costs(img)
    return np.array([min(range(5), key=lambda t: (by[y, t], bi[y, t], t)) for y in range(h)], np.int64)


def fixed_stream_size(img, option=NONE):
    """Bytes of the zlib stream of the fixed-code file under `option`."""
    by, _ = row_costs(img)
    types = choose(img, option)
    return ZLIB_FRAME + int(by[np.arange(img.shape[0]), types].sum())


def fixed_file_size(img, option=NONE):
    """Bytes of the fixed-code file (one IDAT chunk: streams below 2^30 bytes)."""
    return CONTAINER + fixed_stream_size(img, option)


def filter_bytes(png):
    """The filter byte of every row of a file, read from its decompressed stream."""
    import struct
    import zlib

    import png_stream as P
    cs = P.chunks(bytes(png))
    w, h = struct.unpack('>II', cs[0][1][:8])
    raw = zlib.decompress(b''.join(d for k, d in cs if k == b'IDAT'))
    assert len(raw) == h * (3 * w + 1)
    return np.frombuffer(raw, np.uint8).reshape(h, 3 * w + 1)[:, 0].astype(np.int64)


def ramp(h=64, w=700):
    """r = (x // 3 + y) & 255, g = (x // 2) & 255, b = (3 y + x // 5) & 255."""
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(x // 3 + y) & 255, (x // 2) & 255, (3 * y + x // 5) & 255], axis=2).astype(np.uint8)


ALPHABET = np.array([0, 1, 2, 127, 128, 254, 255], np.uint8)


def alphabet_raster(seed, h, w):
    """Bytes from {0, 1, 2, 127, 128, 254, 255}: Paeth's ties (a = b, b = c, all equal), Average's odd and 9-bit sums,
    wrap-around.  Some pixels repeat their left or upper neighbour, so that ties between whole pixels occur too."""
    rng = np.random.default_rng(seed)
    img = ALPHABET[rng.integers(0, len(ALPHABET), (h, w, 3))]
    for y in range(h):
        for x in range(w):
            r = rng.integers(0, 6)
            if r == 0 and x:
                img[y, x] = img[y, x - 1]
            elif r == 1 and y:
                img[y, x] = img[y - 1, x]
            elif r == 2 and x and y:
                img[y, x] = img[y - 1, x - 1]
    return img

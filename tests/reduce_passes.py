"""Shapes at which a block of a reduce kernel takes more than one pass: the helpers of tests/test_reduce_passes.py (no device)
and tests/test_gpu_reduce_passes.py.

maray_filter_box_lin<K>, maray_filter_tent_lin<K> (linear.hip) cap their grids at LIN_MAX_BLOCKS and make a block stride over
tiles of rows by gridDim.y; maray_shutter_reduce_lin<NF> (linear.hip) and maray_shutter_reduce<NF> (shutter.hip) cap theirs at
SH_MAX_BLOCKS and make a lane stride over 16-byte vectors.  The shapes here are DERIVED from those constants, which are read
from the sources by regex (as linear_light.committed_table() reads the header): launch_filter_k's and shutter_reduce_blocks's
grid arithmetic is restated below, and a constant or a line of that arithmetic that no longer matches is an assertion failure,
never a silent default -- a change of the budgets then fails here instead of quietly taking the loops out of the tests.

The sample rasters are random bytes for the texture-identity scene and four random slices for the atlas scene of
tests/byte_rasters.py; the expected pictures are linear_light.box_lin / tent_lin / mean_lin and byte_rasters.tent_general /
mean_general.  No sample raster (and no frame) is larger than MAX_SAMPLE_BYTES.
"""
import os
import re

import numpy as np

import byte_rasters as BR
import linear_light as LL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'maray_amd', 'csrc')
MAX_SAMPLE_BYTES = 16 << 20
KS = (2, 4, 8)
RAGGED = 3              # rows of the last tile: fewer than a box group (4) and than the lowest tent tile (4 at K = 8)


# ---- the launch constants, from the sources ------------------------------------------------------------------------------
def _source(name):
    return open(os.path.join(CSRC, name)).read()


def _one(text, pattern, what):
    m = re.findall(pattern, text)
    assert len(m) == 1, '%s: %d definitions match %r' % (what, len(m), pattern)
    return m[0]


def _has(text, line, what):
    assert line in text, '%s no longer reads %r: restate it in tests/reduce_passes.py' % (what, line)


_constants = []


def constants():
    """{name: value} of the launch constants; TH is {k: rows of a tent tile}."""
    if _constants:
        return _constants[0]
    lin, sh, flt = _source('linear.hip'), _source('shutter.hip'), _source('filter.hpp')
    c = {}
    c['LIN_MAX_BLOCKS'] = int(_one(lin, r'constexpr uint32_t LIN_MAX_BLOCKS = (\d+);', 'LIN_MAX_BLOCKS'))
    c['LIN_BLOCK'] = int(_one(lin, r'constexpr int LIN_BLOCK = (\d+);', 'LIN_BLOCK'))
    th8, th = _one(lin, r'static constexpr int TH = K == 8 \? (\d+) : (\d+);', 'TentLin<K>::TH')
    c['TH'] = {2: int(th), 4: int(th), 8: int(th8)}
    c['FILTER_TILE_W'] = int(_one(flt, r'constexpr uint32_t FILTER_TILE_W = (\d+),', 'FILTER_TILE_W'))
    c['FILTER_TILE_H'] = int(_one(flt, r'constexpr uint32_t FILTER_TILE_W = \d+, FILTER_TILE_H = (\d+);', 'FILTER_TILE_H'))
    block, blocks = _one(sh, r'constexpr uint32_t SH_BLOCK = (\d+), SH_MAX_BLOCKS = (\d+);', 'SH_BLOCK, SH_MAX_BLOCKS')
    c['SH_BLOCK'], c['SH_MAX_BLOCKS'] = int(block), int(blocks)
    assert int(_one(lin, r'constexpr uint32_t SH_BLOCK = (\d+);', "linear.hip's SH_BLOCK")) == c['SH_BLOCK']
    # the arithmetic restated below, line by line
    _has(lin, 'constexpr int TW = (int)FILTER_TILE_W;', 'the tile width')
    _has(lin, 'const uint32_t gx = (a.w + FILTER_TILE_W - 1) / FILTER_TILE_W;', 'launch_filter_k')
    _has(lin, 'const uint32_t by_budget = std::max(1u, LIN_MAX_BLOCKS / gx);', 'launch_filter_k')
    _has(lin, 'const uint32_t tiles_y = (a.n_out + TentLin<K>::TH - 1) / TentLin<K>::TH;', 'launch_filter_k')
    _has(lin, 'dim3(gx, std::min(tiles_y, by_budget))', 'launch_filter_k')
    _has(lin, 'const uint32_t groups = (a.n_out + LIN_BLOCK / TW - 1) / (LIN_BLOCK / TW);', 'launch_filter_k')
    _has(lin, 'dim3(gx, std::min(groups, by_budget))', 'launch_filter_k')
    _has(lin, 'for (uint32_t ty = blockIdx.y; ty < tiles_y; ty += gridDim.y)', "the tent's tile loop")
    _has(lin, 'oy < a.n_out; oy += gridDim.y * (LIN_BLOCK / TW))', "the box's row loop")
    _has(sh, 'const size_t blocks = (bytes / 16 + SH_BLOCK - 1) / SH_BLOCK;', 'shutter_reduce_blocks')
    _has(sh, 'return (uint32_t)std::min<size_t>(std::max<size_t>(blocks, 1), SH_MAX_BLOCKS);', 'shutter_reduce_blocks')
    for text, name in ((lin, 'maray_shutter_reduce_lin'), (sh, 'maray_shutter_reduce')):
        _has(text, 'const size_t head = mis ? (16 - mis < a.bytes ? 16 - mis : a.bytes) : 0;', name)
        _has(text, 'const size_t n_vec = (a.bytes - head) / 16;', name)
        _has(text, 'const size_t stride = (size_t)gridDim.x * SH_BLOCK;', name)
        _has(text, 'for (size_t v = (size_t)blockIdx.x * SH_BLOCK + threadIdx.x; v < n_vec; v += stride)', name)
    assert c['LIN_BLOCK'] % c['FILTER_TILE_W'] == 0 and all(t % (c['LIN_BLOCK'] // c['FILTER_TILE_W']) == 0 for t in c['TH'].values())
    _constants.append(c)
    return c


# ---- launch_filter_k, restated --------------------------------------------------------------------------------------------
KERNELS = ('box', 'tent')


def unit_rows(kernel, k):
    """Output rows a block takes per trip round its loop: a tile of the tent, a group of LIN_BLOCK / TW rows of the box."""
    c = constants()
    return c['TH'][k] if kernel == 'tent' else c['LIN_BLOCK'] // c['FILTER_TILE_W']


def filter_grid(kernel, k, w, n_out):
    """(gridDim.x, gridDim.y, tiles of rows) of the pass that reduces n_out rows of w pixels."""
    c = constants()
    gx = (w + c['FILTER_TILE_W'] - 1) // c['FILTER_TILE_W']
    by_budget = max(1, c['LIN_MAX_BLOCKS'] // gx)
    u = unit_rows(kernel, k)
    tiles = (n_out + u - 1) // u
    return gx, min(tiles, by_budget), tiles


def trips(block_row, gy, tiles):
    """The tiles block row `block_row` takes, in order."""
    return list(range(block_row, tiles, gy))


def min_height(kernel, k, w):
    """The smallest output height at which block row 0 makes three trips round its loop and the picture ends on a ragged tile of
    RAGGED rows that a block reaches after a full tile.  With more than one block row the ragged tile is one more, so that block
    row 0's third trip is a full tile (what it leaves in LDS is then a whole tile's) and block row 1 ends on the ragged one; with
    one block row the single row of blocks takes two full tiles and then the ragged one."""
    c = constants()
    gx = (w + c['FILTER_TILE_W'] - 1) // c['FILTER_TILE_W']
    gy = max(1, c['LIN_MAX_BLOCKS'] // gx)
    full = 2 * gy + (1 if gy > 1 else 0)
    return unit_rows(kernel, k) * full + RAGGED


class FilterCase:
    """k x k samples per pixel, w pixels wide; the height serves both kernels (the tent's tile is a whole number of box groups,
    so the box makes at least the tent's trips and ends as ragged)."""

    def __init__(self, name, k, w, seed):
        self.name, self.k, self.w, self.seed = name, k, w, seed
        self.h = max(min_height(kernel, k, w) for kernel in KERNELS)

    @property
    def sample_shape(self):
        return (self.k * self.h, self.k * self.w, 3)

    @property
    def sample_bytes(self):
        return self.k * self.h * self.k * self.w * 3

    def raster(self):
        return BR.random_bytes(self.seed, self.k * self.h, self.k * self.w)

    def grid(self, kernel, n_out=None):
        return filter_grid(kernel, self.k, self.w, self.h if n_out is None else n_out)

    def y1_inside_the_last_full_tile(self, kernel):
        """An end of a row range inside the last full tile: the range's last tile is ragged and a block's third trip."""
        u = unit_rows(kernel, self.k)
        return (self.h // u - 1) * u + u // 2 + 1

    def __repr__(self):
        return self.name


def narrow_tall_cases():
    """gridDim.x = 1: the whole budget is block rows.  w = 3 at k = 2 is a sample pitch of 2 modulo 4."""
    return [FilterCase('tall k=%d w=%d' % (k, w), k, w, 9000 + 10 * k + w) for k in KS for w in (1, 3)]


def two_column_tile_cases():
    """A full column tile and a ragged one of one pixel: the budget per column halves."""
    return [FilterCase('two column tiles k=2 w=%d' % (constants()['FILTER_TILE_W'] + 1), 2, constants()['FILTER_TILE_W'] + 1, 9101)]


def one_block_row_cases():
    """One column tile more than half the budget: LIN_MAX_BLOCKS / gx == 1, every block loops over all its tiles."""
    c = constants()
    w = c['FILTER_TILE_W'] * (c['LIN_MAX_BLOCKS'] // 2) + 1
    return [FilterCase('one block row k=2 w=%d' % w, 2, w, 9102)]


def filter_cases():
    return narrow_tall_cases() + two_column_tile_cases() + one_block_row_cases()


def case_by_name(name):
    return {c.name: c for c in filter_cases()}[name]


CONTRACTS = {'box': LL.box_lin, 'tent': LL.tent_lin}


def cut_contract(contract, s8, k, y0, y1, halo):
    """Output rows [y0, y1) from the samples of those rows alone: cut plainly (the box, the mean), or with a halo of one output
    row on each side where the image has one (the tent: k/2 sample rows of it are read, the image's own edges clamp)."""
    h = s8.shape[0] // k
    a, b = (max(0, y0 - 1), min(h, y1 + 1)) if halo else (y0, y1)
    return contract(s8[k * a:k * b], k)[y0 - a:y1 - a]


def cut_tiles(gy, tiles):
    """The tiles a cut-independence check visits: the first trips of block rows 0 and 1, the last block row's, and the end."""
    return sorted(t for t in {0, 1, gy - 1, gy, gy + 1, 2 * gy - 1, 2 * gy, 2 * gy + 1, tiles - 2, tiles - 1} if 0 <= t < tiles)


# ---- the shutter ---------------------------------------------------------------------------------------------------------
# Frames of SHUTTER_W x h pixels.  The atlas' pitch is 128 pixels, but a frame as wide as the pitch has 384 h bytes, a multiple
# of 16 whatever h: at an aligned destination it can have no tail.  One pixel less (381 bytes a row) leaves tails at both
# misalignments, which is what the strided loop has to get right next to.
SHUTTER_W = BR.PITCH - 1
SHUTTER_MIS = (0, 9)
SHUTTER_PAST = 1024     # vectors past one pass of the grid, at least
SHUTTER_ORDER = {2: (2, 1), 16: (0, 1, 2, 3, 3, 2, 0, 0, 1, 1, 3, 2, 0, 3, 3, 1)}       # slices per frame: the groups of 8 differ
SHUTTER_SLICES = 4


def shutter_blocks(nbytes):
    c = constants()
    return min(max((nbytes // 16 + c['SH_BLOCK'] - 1) // c['SH_BLOCK'], 1), c['SH_MAX_BLOCKS'])


def shutter_split(nbytes, mis):
    """(head bytes, vectors, tail bytes, vectors a pass of the grid covers) at a destination `mis` bytes past a multiple of 16."""
    head = min(16 - mis, nbytes) if mis else 0
    n_vec = (nbytes - head) // 16
    return head, n_vec, nbytes - head - 16 * n_vec, shutter_blocks(nbytes) * constants()['SH_BLOCK']


def shutter_height_ok(h, w=SHUTTER_W, mis=SHUTTER_MIS, past=SHUTTER_PAST):
    c = constants()
    for m in mis:
        head, n_vec, tail, stride = shutter_split(3 * w * h, m)
        if not (stride == c['SH_MAX_BLOCKS'] * c['SH_BLOCK'] and n_vec >= stride + past and 1 <= tail <= 15):
            return False
    return True


def shutter_height(w=SHUTTER_W, mis=SHUTTER_MIS, past=SHUTTER_PAST):
    """The smallest height at which, at every misalignment of `mis`, the vectors exceed one pass by at least `past` and a tail
    of 1 .. 15 bytes is left."""
    h = 1
    while not shutter_height_ok(h, w, mis, past):
        h += 1
        assert 3 * w * h <= MAX_SAMPLE_BYTES, 'no such height within %d bytes' % MAX_SAMPLE_BYTES
    return h


def shutter_slices(h=None):
    """Four distinct random slices, (h, SHUTTER_W, 3) each."""
    return BR.random_frames(9200, SHUTTER_SLICES, shutter_height() if h is None else h, SHUTTER_W)


def shutter_frames(slices, n):
    return [slices[t] for t in SHUTTER_ORDER[n]]


def mean_groups(frames, lin, weights=None):
    """The shutter's contract summed group of 8 by group of 8, group g counted weights[g] times (default: once each -- then it
    is LL.mean_lin, or BR.mean_general for lin = False).  (0, 1) is a group left out, (2, 1) a group counted twice."""
    n = len(frames)
    groups = [frames[g:g + BR.GROUP] for g in range(0, n, BR.GROUP)]
    weights = (1,) * len(groups) if weights is None else weights
    assert len(weights) == len(groups)
    s = np.zeros(frames[0].shape, np.int64)
    for wt, group in zip(weights, groups):
        s += wt * sum((LL.D[f] if lin else f.astype(np.int64)) for f in group)
    m = (s + n // 2) >> (n.bit_length() - 1)
    return LL.encode(m) if lin else (m & 0xFF).astype(np.uint8)


def group_mutants(n):
    groups = (n + BR.GROUP - 1) // BR.GROUP
    out = []
    for g in range(groups):
        for wt, what in ((0, 'left out'), (2, 'counted twice')):
            if groups > 1:
                out.append(('group %d %s' % (g, what), tuple(wt if i == g else 1 for i in range(groups))))
    return out

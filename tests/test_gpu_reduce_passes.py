"""The reduce kernels where a block takes more than one pass, on the device, byte for byte: maray_filter_box_lin<K> and
maray_filter_tent_lin<K> with more tiles of rows than their grid has block rows (every block loops: a stride, per-tile values,
the barrier at the top of the tent's loop, a ragged tile after a full one), and maray_shutter_reduce<NF> /
maray_shutter_reduce_lin<NF> with more 16-byte vectors than one pass of their grid covers, with partial sums between groups of
frames and at a destination that is not 16-byte aligned.

The shapes come from tests/reduce_passes.py, which derives them from the kernels' launch constants; that they make the loops
turn, and that the numpy contracts compared with here are the contracts of the pieces, is checked without a device in
tests/test_reduce_passes.py.  The scenes are the texture-identity and atlas scenes of tests/byte_rasters.py: every sample
raster is random bytes.

Every group of cases runs in a process of its own, because the device buffers come from PyTorch, imported before the library.
Every destination lies between guard bands of 0xA5, checked after every call, and holds 0xA5 itself before the call, so that
a tile nobody wrote shows.  A child checks everything it can and prints one line per check; a line that starts with FAIL names
the check, the number of bytes that differ and where the first one lies (row, tile and the trip of its block).  A line that
starts with PRECONDITION says that a PLAIN context did not render the tall or wide texture byte for byte: a finding about the
pixel kernels at that geometry, not about the reduces.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import byte_rasters as BR
import linear_light as LL
import maray_amd as M
import reduce_passes as RP

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PAD, FILL = 256, 0xA5
FILTERS = {'box': M.FILTER_BOX, 'tent': M.FILTER_TENT}
JIT_CASE = 'tall k=2 w=3'           # the case that also runs on BACKEND_JIT, for both kernels

_CHILD = r"""
import sys
import torch
sys.path[:0] = [%(root)r, %(tests)r]
import test_gpu_reduce_passes as T
T.child(sys.argv[1])
"""


def run_child(group):
    """The child's lines.  A child that died, hung or met an error of the runtime's ends the session: nothing more is started
    on a device after a fault."""
    try:
        r = subprocess.run([sys.executable, '-c', _CHILD % {'root': ROOT, 'tests': HERE}, group], capture_output=True, text=True, timeout=600)
    except subprocess.TimeoutExpired as e:
        pytest.exit('%s: the child hung: %s' % (group, str(e.stdout)[-2000:]), returncode=3)
    lines = r.stdout.splitlines()
    if r.returncode not in (0, 1) or any(l.startswith('ERROR') for l in lines):
        pytest.exit('%s: the child ended with %d\n%s\n%s' % (group, r.returncode, '\n'.join(lines[-20:]), r.stderr[-4000:]), returncode=3)
    bad = [l for l in lines if not l.startswith('ok ')]
    assert r.returncode == 0 and lines and lines[-1] == 'ok done' and not bad, '\n'.join(bad[:40]) + '\n' + r.stderr[-4000:]
    return lines


# ---- what runs in the child ------------------------------------------------------------------------------------------------
class Checks:
    def __init__(self):
        self.failed = 0

    def ok(self, label):
        print('ok', label, flush=True)

    def fail(self, label, detail, kind='FAIL'):
        self.failed += 1
        print(kind, label + ':', detail, flush=True)


def guarded(torch, n_bytes, off):
    """A buffer of 0xA5 and the offset of a destination of n_bytes in it whose address is `off` modulo 16."""
    b8 = torch.full((n_bytes + 2 * PAD + 16,), FILL, dtype=torch.uint8, device='cuda')
    lo = PAD + (off - (b8.data_ptr() + PAD)) % 16
    assert (b8.data_ptr() + lo) % 16 == off
    return b8, lo


def first_difference(got, want):
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    return len(bad), (int(bad[0]) if len(bad) else -1)


def compare(ck, label, torch, b8, lo, want, where):
    """The guard bands of b8 and the destination at lo against `want`; where(byte index) describes a place in the picture."""
    torch.cuda.synchronize()
    g = b8.cpu().numpy()
    n = want.size
    if not ((g[:lo] == FILL).all() and (g[lo + n:] == FILL).all()):
        ck.fail(label, 'guard band written')
        return False
    count, at = first_difference(g[lo:lo + n], want)
    if count:
        unwritten = int((g[lo:lo + n] == FILL).sum())
        ck.fail(label, '%d of %d bytes differ, first at byte %d (%s); %d bytes hold the fill' % (count, n, at, where(at), unwritten))
        return False
    ck.ok(label)
    return True


def filter_where(case, kernel, y0, n_out, byte_tent=False):
    u = RP.unit_rows(kernel, case.k)
    gx, gy, tiles = case.grid(kernel, n_out)
    if byte_tent:           # maray_filter_tent<K>: a block per tile of FILTER_TILE_H rows, one trip each
        u = RP.constants()['FILTER_TILE_H']
        gy = tiles = (n_out + u - 1) // u

    def where(at):
        row, px = divmod(at // 3, case.w)
        return 'row %d of the call (image row %d), pixel %d: tile %d of %d, trip %d of block row %d of %d' % (
            row, y0 + row, px, row // u, tiles, row // u // gy, row // u % gy, gy)
    return where


def plain_precondition(ck, case, s8, tape, backend):
    """A plain context renders the texture byte for byte (through the host-raster entry point)."""
    H, W, _ = s8.shape
    ctx = M.Context(tape, textures=[s8], backend=backend)
    got, _ = ctx.render_rows(W, H, 0, H, want_f64=False)
    ctx.close()
    count, at = first_difference(got, s8)
    label = '%s: plain %d x %d on back-end %d' % (case.name, W, H, backend)
    if count:
        ck.fail(label, '%d bytes differ, first at sample row %d, sample %d' % (count, at // (3 * W), at % (3 * W) // 3), 'PRECONDITION')
        return False
    ck.ok(label)
    return True


def filter_case(ck, torch, case, tape, byte_tent=False):
    """Everything about one raster: the precondition, then per kernel the whole image at an even and an odd address, two row
    ranges, and two launches in a row into different destinations."""
    s8 = case.raster()
    k, w, h = case.k, case.w, case.h
    backends = [M.BACKEND_TAPE_SMEM] + ([M.BACKEND_JIT] if case.name == JIT_CASE and not byte_tent else [])
    plain_ok = {b: plain_precondition(ck, case, s8, tape, b) for b in backends}
    kernels = ('tent',) if byte_tent else RP.KERNELS
    for kernel in kernels:
        want = BR.tent_general(s8, k) if byte_tent else RP.CONTRACTS[kernel](s8, k)
        name = 'maray_filter_tent<%d>' % k if byte_tent else 'maray_filter_%s_lin<%d>' % (kernel, k)
        for backend in backends:
            if not plain_ok[backend]:
                continue
            tag = '%s: %s on back-end %d' % (case.name, name, backend)
            ctx = M.Context(tape, textures=[s8], backend=backend, samples=k, filter=FILTERS[kernel],
                            transfer=M.TRANSFER_NONE if byte_tent else M.TRANSFER_SRGB)
            if not ctx.kernel_name.endswith('+' + name):
                ck.fail(tag, 'the context names %s' % ctx.kernel_name)
            ranges = [(0, h, 0), (0, h, 1)]
            if backend == M.BACKEND_TAPE_SMEM:
                ranges += [(5, h, 0), (0, case.y1_inside_the_last_full_tile(kernel), 1)]
            for y0, y1, off in ranges:
                b8, lo = guarded(torch, (y1 - y0) * w * 3, off)
                ctx.render_rows_device(w, h, y0, y1, d_rgb8=b8.data_ptr() + lo)
                compare(ck, '%s rows [%d, %d) at address %d modulo 16' % (tag, y0, y1, off), torch, b8, lo, want[y0:y1],
                        filter_where(case, kernel, y0, y1 - y0, byte_tent))
            if backend == M.BACKEND_TAPE_SMEM:
                pair = [guarded(torch, h * w * 3, off) for off in (0, 1)]
                for b8, lo in pair:         # (no synchronisation in between: the second launch follows the first on the stream)
                    ctx.render_rows_device(w, h, 0, h, d_rgb8=b8.data_ptr() + lo)
                for i, (b8, lo) in enumerate(pair):
                    compare(ck, '%s launched twice in a row, launch %d' % (tag, i), torch, b8, lo, want,
                            filter_where(case, kernel, 0, h, byte_tent))
            ctx.close()


def shutter_group(ck, torch, transfer):
    """n = 2 and n = 16 frames of SHUTTER_W x h in one call each, the destination at misalignments 0 and 9."""
    lin = transfer == M.TRANSFER_SRGB
    contract = LL.mean_lin if lin else BR.mean_general
    slices = RP.shutter_slices()
    h, w = slices[0].shape[:2]
    nbytes = h * w * 3
    tape = BR.atlas_scene().lower()
    ctx = M.Context(tape, textures=[BR.atlas(slices)], backend=M.BACKEND_TAPE_SMEM, transfer=transfer)
    for t in range(len(slices)):            # the precondition: the plain render of slice t
        ctx.set_params([float(t)])
        got, _ = ctx.render_rows(w, h, 0, h, want_f64=False)
        count, at = first_difference(got, slices[t])
        label = 'shutter: plain slice %d, %d x %d' % (t, w, h)
        if count:
            ck.fail(label, '%d bytes differ, first at byte %d' % (count, at), 'PRECONDITION')
            ctx.close()
            return
        ck.ok(label)
    name = 'maray_shutter_reduce_lin' if lin else 'maray_shutter_reduce'
    for n in sorted(RP.SHUTTER_ORDER):
        want = contract(RP.shutter_frames(slices, n)).reshape(-1)
        values = [(float(t),) for t in RP.SHUTTER_ORDER[n]]
        for mis in RP.SHUTTER_MIS:
            head, n_vec, tail, stride = RP.shutter_split(nbytes, mis)

            def where(at, head=head, n_vec=n_vec, stride=stride):
                if at < head:
                    return 'the head'
                v = (at - head) // 16
                return 'the tail' if v >= n_vec else 'vector %d of %d: trip %d of lane %d of %d' % (v, n_vec, v // stride, v % stride, stride)
            tag = '%s n = %d at misalignment %d' % (name, n, mis)
            b8, lo = guarded(torch, nbytes, mis)
            ctx.render_rows_shutter_device(w, h, 0, h, values, b8.data_ptr() + lo)
            torch.cuda.synchronize()
            g = b8.cpu().numpy()
            if not ((g[:lo] == FILL).all() and (g[lo + nbytes:] == FILL).all()):
                ck.fail(tag, 'guard band written')
                continue
            got = g[lo:lo + nbytes]
            for part, a, b in (('first 64 bytes', 0, 64), ('last 64 bytes', nbytes - 64, nbytes), ('whole picture', 0, nbytes)):
                count, at = first_difference(got[a:b], want[a:b])
                if count:
                    ck.fail('%s, %s' % (tag, part), '%d of %d bytes differ, first at byte %d (%s); %d hold the fill' % (
                        count, b - a, a + at, where(a + at), int((got[a:b] == FILL).sum())))
                else:
                    ck.ok('%s, %s' % (tag, part))
    ctx.close()


GROUPS = ['tall k=2', 'tall k=4', 'tall k=8', 'two column tiles', 'one block row', 'byte tent', 'shutter none', 'shutter srgb']


def child(group):
    import torch
    ck = Checks()
    try:
        if group.startswith('shutter'):
            shutter_group(ck, torch, M.TRANSFER_SRGB if group.endswith('srgb') else M.TRANSFER_NONE)
        else:
            tape = BR.identity_scene().lower()
            if group == 'byte tent':
                cases = [c for c in RP.narrow_tall_cases() if c.k in (2, 8)]
            else:
                cases = [c for c in RP.filter_cases() if c.name.startswith(group)]
            assert cases, group
            for case in cases:
                filter_case(ck, torch, case, tape, byte_tent=group == 'byte tent')
    except M.MarayError as e:          # nothing more runs on the device after an error of the runtime's
        print('ERROR %s: %s' % (group, e), flush=True)
        sys.exit(1)
    if ck.failed:
        sys.exit(1)
    print('ok done', flush=True)


# ---- the tests -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', RP.KS)
def test_narrow_and_tall_every_block_row_takes_three_tiles(k):
    """gridDim.x = 1, 2048 block rows, 4098 tiles of the tent (8195 groups of the box at k = 2 and 4): w = 1 and 3, box and tent
    in linear light against box_lin and tent_lin; the whole image at an even and an odd address, rows [5, h), rows that end
    inside the last full tile, two launches in a row.  k = 2, w = 3 also on the specialised back-end."""
    lines = run_child('tall k=%d' % k)
    assert sum('maray_filter_box_lin<%d>' % k in l for l in lines) >= 12 and sum('maray_filter_tent_lin<%d>' % k in l for l in lines) >= 12
    assert (k == 2) == any('on back-end %d' % M.BACKEND_JIT in l for l in lines)


def test_two_column_tiles_the_second_ragged():
    """w = 65: 2 x 1024 blocks, the second column tile one pixel wide."""
    assert sum('_lin<2>' in l for l in run_child('two column tiles')) == 12


def test_one_block_row_every_block_loops_over_all_its_tiles():
    """w = 65,537: 1025 column tiles, LIN_MAX_BLOCKS / gx == 1: 3 tiles of the tent and 5 groups of the box per block."""
    assert sum('_lin<2>' in l for l in run_child('one block row')) == 12


def test_control_the_byte_tent_on_the_tall_rasters():
    """transfer = NONE: maray_filter_tent<K>, one tile per block and no loop, on the same tall rasters (k = 2 and 8) against
    byte_rasters.tent_general: a control for the tests above, and the byte kernel at a grid of 4098 tiles."""
    lines = run_child('byte tent')
    assert sum('maray_filter_tent<2>' in l for l in lines) == 12 and sum('maray_filter_tent<8>' in l for l in lines) == 12


@pytest.mark.parametrize('transfer', ['none', 'srgb'])
def test_shutter_past_one_pass_with_partial_sums_and_a_misaligned_destination(transfer):
    """Frames of 127 x 22,061 pixels (8 MiB and 1,039 vectors more): n = 2 and n = 16 (partial sums between the two groups, the
    groups of different slices) at destination misalignments 0 and 9, against mean_general (NONE) and mean_lin (SRGB); the first
    and the last 64 bytes are compared on their own, so that a head or a tail that is wrong is named as one."""
    lines = run_child('shutter ' + transfer)
    assert sum('maray_shutter_reduce' in l for l in lines) == 12

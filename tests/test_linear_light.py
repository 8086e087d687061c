"""The transfer option (include/maray_hip.h, "transfer") as far as it can be checked without a device: the table, the struct
words, the argument errors that come before a device is looked for, the CLI flag -- and that the numpy contracts of
tests/linear_light.py are the byte contracts with a decode and an encode, and that the rasters tests/test_gpu_linear_bytes.py
uses tell every mutant of a contract from the contract."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import byte_rasters as BR
import linear_light as LL
import maray_amd as M
from test_filter import tent
from test_gpu_shutter import mean
from test_gpu_supersample import box

E_ARG = -1
KS = [2, 4, 8]
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ---- the table -----------------------------------------------------------------------------------------------------------
def test_transfer_table_is_the_committed_table_and_the_formula():
    d, t = M.transfer_table()
    assert d.dtype == np.uint16 and np.array_equal(d, LL.D) and np.array_equal(t, LL.T)
    assert np.array_equal(LL.D, LL.formula_table())
    lin = lambda c: c / 12.92 if c <= 0.04045 else ((c + 0.055) / 1.055) ** 2.4
    assert [math.floor(65535 * lin(v / 255) + 0.5) for v in range(256)] == list(LL.D)
    assert list(LL.D[:4]) == [0, 20, 40, 60] and LL.D[255] == 65535
    steps = np.diff(LL.D)
    assert steps.min() == 19 and steps.max() == 583
    d0, t0 = M.transfer_table(M.TRANSFER_NONE)
    assert np.array_equal(d0, np.arange(256)) and np.array_equal(t0, np.arange(256))
    with pytest.raises(M.MarayError) as e:
        M.transfer_table(2)
    assert e.value.code == E_ARG


def test_encode_inverts_decode_and_a_bin_holds_one_threshold():
    assert np.array_equal(LL.encode(LL.D), np.arange(256))
    assert (np.diff(LL.T[1:]) >= 19).all()
    assert len(set(int(t) >> 4 for t in LL.T[1:])) == 255
    # the 4096-entry table plus one compare the kernels use is E: the count up to the bin's end, less one below a threshold in the bin
    m = np.arange(65536)
    cnt = LL.encode(16 * (m >> 4) + 15).astype(np.int64)
    off = np.where((LL.T[cnt] >> 4) == (m >> 4), LL.T[cnt] & 15, 0)
    assert np.array_equal(cnt - ((m & 15) < off), LL.encode(m))
    assert np.array_equal(LL.encode(m, LL.T_NONE), np.minimum(m, 255))


# ---- the struct words ----------------------------------------------------------------------------------------------------
def test_struct_layout():
    assert M.CtxOpts.transfer.offset == 16 and C.sizeof(M.CtxOpts) == 32
    assert M.GenOpts.transfer.offset == 28 and C.sizeof(M.GenOpts) == 32
    assert (M.TRANSFER_NONE, M.TRANSFER_SRGB) == (0, 1)


# ---- argument errors before any device -----------------------------------------------------------------------------------
def test_unknown_transfer_is_an_argument_error_before_any_device(tmp_path):
    scene = BR.identity_scene()
    with pytest.raises(M.MarayError) as e:
        M.gen_to_image(scene, size=(4, 4), textures=[BR.constant(1, 4, 4)], transfer=2)
    assert e.value.code == E_ARG and 'transfer' in str(e.value)
    with pytest.raises(M.MarayError) as e:
        M.gen(scene, str(tmp_path / 'x.png'), textures=[BR.constant(1, 4, 4)], transfer=2)
    assert e.value.code == E_ARG and 'transfer' in str(e.value)
    assert not (tmp_path / 'x.png').exists()
    ms = C.c_float()
    assert M.lib().maray_hip_time_filter_ex(0, 8, 8, 2, M.FILTER_BOX, M.TRANSFER_NONE, 1, C.byref(ms)) == E_ARG
    assert M.lib().maray_hip_time_filter_ex(0, 8, 8, 2, M.FILTER_TENT, 2, 1, C.byref(ms)) == E_ARG
    assert M.lib().maray_hip_time_shutter_reduce_ex(0, 64, 2, 2, 1, C.byref(ms)) == E_ARG


def test_cli_accepts_linear_and_rejects_a_value():
    exe = os.path.join(ROOT, 'maray_amd', 'maray')
    r = subprocess.run([exe, '--linear=x', '-i', 'a', '-o', 'b'], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and 'Usage' in r.stderr
    # accepted: the run gets as far as the input file, which does not exist
    r = subprocess.run([exe, '--linear', '-s', '2', '-i', os.path.join(HERE, 'no_such.maray'), '-o', 'b'], capture_output=True, text=True, timeout=60)
    assert r.returncode != 2 and 'Usage' not in r.stderr and 'no_such.maray' in r.stderr
    assert '--linear' in subprocess.run([exe, '--help'], capture_output=True, text=True, timeout=60).stderr


# ---- the contracts are the byte contracts with a decode and an encode -----------------------------------------------------
@pytest.mark.parametrize('k', KS)
def test_with_identity_tables_the_contracts_are_the_byte_contracts(k):
    s = BR.parity_raster(k)
    none = dict(d=LL.D_NONE, t=LL.T_NONE)
    assert np.array_equal(LL.tent_lin(s, k, **none), tent(s, k)) and np.array_equal(LL.tent_lin(s, k, **none), BR.tent_general(s, k))
    assert np.array_equal(LL.box_lin(s, k, **none), box(s, k))
    for d in (1, -1):
        assert np.array_equal(LL.tent_lin(s, k, half=2 * k ** 4 + d, **none), BR.tent_general(s, k, half=2 * k ** 4 + d))
    for n in (2, 16, 64):
        frames, _ = BR.shutter_case(n)
        assert np.array_equal(LL.mean_lin(frames, **none), mean(frames))
        assert np.array_equal(LL.mean_lin(frames, carry_bits=8, **none), BR.mean_general(frames, carry_bits=8))


def test_known_answers():
    """Half the light of white is 188, not 128; a constant comes out unchanged."""
    for k in KS:
        c = BR.checker(8 * k, 8 * k)
        inner = (slice(1, -1), slice(1, -1))         # (at the image's edge the tent's clamp counts a sample twice)
        assert (LL.box_lin(c, k) == 188).all() and (LL.tent_lin(c, k)[inner] == 188).all()
        assert (box(c, k) == 128).all() and (tent(c, k)[inner] == 128).all()
        for v in (0, 1, 17, 128, 254, 255):
            assert (LL.box_lin(BR.constant(v, 4 * k, 4 * k), k) == v).all() and (LL.tent_lin(BR.constant(v, 4 * k, 4 * k), k) == v).all()
    for n in BR.SHUTTER_NS:
        frames = [BR.constant(255 * (i & 1), 3, 5) for i in range(n)]
        assert (LL.mean_lin(frames) == 188).all() and (mean(frames) == 128).all()
    assert LL.encode((int(LL.D[0]) + int(LL.D[255]) + 1) >> 1) == 188


# ---- the rasters are sharp ------------------------------------------------------------------------------------------------
def test_threshold_cases():
    """{v-1, v-1, v, v} lands on T[v] for every v; the search finds four samples one below T[v] for all but at most 11 of the
    255 thresholds (as run: v = 1 .. 4 and 249 .. 255, where D steps too evenly or the window is cut)."""
    for v, four in zip(range(1, 256), LL.on_threshold()):
        assert (int(LL.D[list(four)].sum()) + 2) >> 2 == LL.T[v]
    below = LL.below_threshold()
    missing = sorted(set(range(1, 256)) - set(below))
    assert len(missing) <= 11, missing
    for v, four in below.items():
        assert (int(LL.D[list(four)].sum()) + 2) >> 2 == LL.T[v] - 1 and all(abs(a - v) <= 40 for a in four)


def test_k4_blocks_add_thresholds_the_fours_leave_out():
    """At k = 4 sixteen samples have room for a mean one below T[v] where four have not: as run, v = 3, 4 and 249 .. 253 of
    the eleven left out (v = 1: 16 T - 9 = 151 is no sum of the table's first entries, 0 20 40 60 80 99 119 139).  A threshold
    moved down by one shows on those pixels."""
    k4 = LL.below_threshold_k4()
    assert set(k4) <= set(range(1, 256)) - set(LL.below_threshold()) and len(k4) >= 5
    s = LL.threshold_box_raster_k4()
    assert np.array_equal(LL.box_lin(s, 4)[0, :, 0], [v - 1 for v in sorted(k4)])
    for v in k4:
        assert (int(LL.D[k4[v]].sum()) + 8) >> 4 == LL.T[v] - 1
    for name, f in LL.threshold_mutants(lambda x, **kw: LL.box_lin(x, 4, **kw), sorted(k4)):
        if name.endswith('-1'):
            assert not np.array_equal(f(s), LL.box_lin(s, 4)), name


def test_threshold_rasters_tell_every_moved_threshold():
    s = LL.threshold_box_raster()
    want = LL.box_lin(s, 2)
    below = LL.below_threshold()
    for name, f in LL.threshold_mutants(lambda x, **kw: LL.box_lin(x, 2, **kw), range(1, 256)):
        v, e = int(name[2:name.index(']')]), int(name.split()[-1])
        if e == 1 or v in below:        # a threshold moved down shows on a pixel one below it
            assert not np.array_equal(f(s), want), name
    for n in (2, 4):
        frames = LL.threshold_frames(n)
        want = LL.mean_lin(frames)
        for name, f in LL.threshold_mutants(LL.mean_lin, range(1, 256)):
            v, e = int(name[2:name.index(']')]), int(name.split()[-1])
            if e == 1 or (n == 4 and v in below):
                assert not np.array_equal(f(frames), want), (n, name)
    s = LL.threshold_tent_raster()
    m = LL.tent_lin_mean(s, 2)
    assert all((m[2 * v] == LL.T[v]).all() for v in range(1, 256))
    want = LL.tent_lin(s, 2)
    for name, f in LL.threshold_mutants(lambda x, **kw: LL.tent_lin(x, 2, **kw), range(1, 256)):
        if name.endswith('+1'):
            assert not np.array_equal(f(s), want), name


@pytest.mark.parametrize('k', KS)
def test_parity_and_extreme_rasters_kill_the_filter_mutants(k):
    """Random bytes kill all but the rounding constants (a critical sum that also crosses a threshold: one byte in about
    256 W).  The critical raster (cells of period k) kills both of the box's; under the tent its sums are multiples of 4 k^2,
    never one below a multiple of W, so the tent's two die on the footprints of critical_tent_raster, whose weighted sums are
    W T[v] - W/2 and one less."""
    s, crit, crit_tent = BR.parity_raster(k), LL.critical_raster(k), LL.critical_tent_raster(k)
    assert len(LL.critical_cells(k * k)) >= 4 and {b for _, b, _ in LL.critical_cells(k * k)} == {0, 1}
    centres = LL.critical_tent_centres(k)
    assert {(v, b) for _, v, b in centres} == {(v, b) for v in LL.CRITICAL_VS for b in (0, 1)}
    m, W = LL.tent_lin_mean(crit_tent, k), 4 * k ** 4
    for row, v, below in centres:
        assert (m[row, 1] == LL.T[v] - below).all()
        assert (LL.tent_lin_mean(crit_tent, k, half=W // 2 + (1 if below else -1))[row, 1] == LL.T[v] - (0 if below else 1)).all()
    for mutants, f, sharp in ((LL.box_mutants(k), LL.box_lin, crit), (LL.tent_mutants(k), LL.tent_lin, crit_tent)):
        left = [name for name, g in mutants if np.array_equal(g(s), f(s, k))]
        assert set(left) <= {'rounding constant +1', 'rounding constant -1'}, (k, left)
        for name, g in mutants:
            if name.startswith('rounding'):
                assert not np.array_equal(g(sharp), f(sharp, k)), (k, name)
    # 16-bit horizontal sums: the all-255 raster of the extremes holds the largest
    ones = BR.constant(255, k * BR.EXTREMES_H, k * BR.EXTREMES_W)
    assert not np.array_equal(LL.tent_lin(ones, k, hbits=16), LL.tent_lin(ones, k))
    assert (LL.tent_lin(ones, k) == 255).all() and LL.tent_lin_mean(ones, k).max() == 65535


@pytest.mark.parametrize('n', BR.SHUTTER_NS)
def test_shutter_frames_kill_the_mean_mutants(n):
    frames, order = BR.shutter_case(n)
    passed = [frames[i] for i in order]
    want = LL.mean_lin(frames)
    assert np.array_equal(LL.mean_lin(passed), want)
    crit = LL.critical_frames(n)
    assert len(LL.critical_cells(n)) >= 2 and {b for _, b, _ in LL.critical_cells(n)} == {0, 1}
    for name, f in LL.mean_mutants(n):
        if name.startswith('rounding'):         # (random bytes: one in about 256 n sits on such a sum and a threshold)
            assert not np.array_equal(f(crit), LL.mean_lin(crit)), name
        else:
            assert not np.array_equal(f(passed), want), name


@pytest.mark.parametrize('n', BR.HEAD_TAIL_NS)
def test_head_and_tail_frames_kill_the_mean_mutants_at_their_largest_size(n):
    frames, order = BR.head_tail_case(n)
    passed = [frames[i] for i in order]
    want = LL.mean_lin(passed)
    for name, f in LL.mean_mutants(n):
        if not name.startswith('rounding'):         # (105 bytes need not hold a critical sum of 65536 n)
            assert not np.array_equal(f(passed), want), name

"""The tent reconstruction filter without a device (include/maray_hip.h, "reconstruction filter"): the numpy restatement of
the contract that tests/test_gpu_filter.py compares the device with, checked against the contract's formula written as a
double loop; the options structs' layout; the CLI's usage errors; the façade's argument check."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import maray_amd as M
import scenes
from marayb import encode

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
E_ARG = -1


def tent(s8, k):
    """(k h, k w, 3) uint8 -> (h, w, 3): the contract, separably (horizontal sums, then vertical)."""
    H, W, _ = s8.shape
    t = [2 * k - abs(2 * u + 1 - k) for u in range(-(k // 2), 3 * k // 2)]
    p = np.pad(s8.astype(np.uint32), ((k // 2,) * 2, (k // 2,) * 2, (0, 0)), mode='edge')
    hs = sum(t[i] * p[:, i:i + W:k] for i in range(2 * k))
    vs = sum(t[j] * hs[j:j + H:k] for j in range(2 * k))
    return ((vs + 2 * k ** 4) >> (2 + 4 * (k.bit_length() - 1))).astype(np.uint8)


def tent_direct(s8, k):
    """out(px, py, c) = (SUM_u SUM_v t(u) t(v) s(clamp(k px + u), clamp(k py + v), c) + W/2) >> log2 W, W = 4 k^4: as written."""
    H, W, _ = s8.shape
    h, w = H // k, W // k
    big_w = 4 * k ** 4
    shift = big_w.bit_length() - 1
    assert 1 << shift == big_w
    out = np.zeros((h, w, 3), np.uint8)
    for py in range(h):
        for px in range(w):
            for c in range(3):
                acc = 0
                for u in range(-(k // 2), 3 * k // 2):
                    a = min(max(k * px + u, 0), W - 1)
                    for v in range(-(k // 2), 3 * k // 2):
                        b = min(max(k * py + v, 0), H - 1)
                        acc += (2 * k - abs(2 * u + 1 - k)) * (2 * k - abs(2 * v + 1 - k)) * int(s8[b, a, c])
                out[py, px, c] = (acc + big_w // 2) >> shift
    return out


@pytest.mark.parametrize('k', [2, 4, 8])
def test_weights_are_the_contracts(k):
    t = [2 * k - abs(2 * u + 1 - k) for u in range(-(k // 2), 3 * k // 2)]
    assert t == list(range(1, 2 * k, 2)) + list(range(2 * k - 1, 0, -2))
    assert sum(t) == 2 * k * k and 4 * k ** 4 == {2: 64, 4: 1024, 8: 16384}[k]


@pytest.mark.parametrize('k', [2, 4, 8])
def test_a_constant_image_comes_out_unchanged(k):
    for v in (0, 1, 127, 128, 254, 255):
        s8 = np.full((5 * k, 7 * k, 3), v, np.uint8)
        assert (tent(s8, k) == v).all(), v
    s8 = np.empty((3 * k, 4 * k, 3), np.uint8)
    s8[...] = (255, 0, 77)
    assert (tent(s8, k) == np.array([255, 0, 77], np.uint8)).all()


@pytest.mark.parametrize('k', [2, 4, 8])
def test_random_bytes_equal_the_double_loop(k):
    """7 x 5 output pixels: every pixel of the first and last column and row clamps."""
    rng = np.random.default_rng(100 + k)
    s8 = rng.integers(0, 256, (5 * k, 7 * k, 3), dtype=np.uint8)
    s8[0, 0] = 255
    s8[-1, -1] = (0, 255, 0)
    got = tent(s8, k)
    assert got.shape == (5, 7, 3)
    assert np.array_equal(got, tent_direct(s8, k))


def test_every_sample_weighs_the_same():
    """Per axis the weights a sample gets from all pixels sum to 2k (two footprints overlap on it); the k/2 samples at either
    end also stand in for the clamped indices past the edge, so the total over a row is the pixels' count times 2 k^2."""
    for k in (2, 4, 8):
        t = [2 * k - abs(2 * u + 1 - k) for u in range(-(k // 2), 3 * k // 2)]
        n = 6 * k
        total = np.zeros(n, np.int64)
        for p in range(6):
            for i, u in enumerate(range(-(k // 2), 3 * k // 2)):
                total[min(max(k * p + u, 0), n - 1)] += t[i]
        assert (total[k // 2:n - k // 2] == 2 * k).all()                 # interior samples: 2k per axis
        assert total.sum() == 6 * 2 * k * k


def test_options_structs_keep_their_size():
    assert C.sizeof(M.api.CtxOpts) == 32 and M.api.CtxOpts.filter.offset == 12
    assert C.sizeof(M.api.GenOpts) == 32 and M.api.GenOpts.filter.offset == 20
    assert (M.FILTER_BOX, M.FILTER_TENT) == (0, 1)


def _cli(*args):
    return subprocess.run([os.path.join(ROOT, 'maray_amd', 'maray')] + list(args), capture_output=True, text=True, timeout=300,
                          env=dict(os.environ, HIP_VISIBLE_DEVICES='-1', ROCR_VISIBLE_DEVICES='-1'))


def test_cli_filter_options(tmp_path):
    path = os.path.join(HERE, 'golden', 'chess.maray')
    out = tmp_path / 'o.png'
    for bad in (['--filter', 'tent'], ['--filter', 'tent', '-s', '1'], ['--filter', 'mitchell', '-s', '4'], ['--filter', 'TENT', '-s', '4'],
                ['-s', '4', '--filter']):
        r = _cli('-i', path, '-o', str(out), *bad)
        assert r.returncode == 2 and 'no HIP device' not in r.stderr, (bad, r.stderr)
        assert 'Usage' in r.stderr, (bad, r.stderr)
        assert not out.exists()
    h = _cli('--help')
    assert h.returncode == 0 and '--filter <' in h.stderr
    # a well-formed command line gets as far as the device
    for good in (['-s', '4', '--filter', 'tent'], ['--filter', 'tent', '-s', '2'], ['--filter', 'box'], ['-s', '8', '--filter', 'box']):
        ok = _cli('-i', path, '-o', str(out), *good)
        assert ok.returncode == 1 and 'no HIP device' in ok.stderr and 'usage' not in ok.stderr.lower(), (good, ok.stderr)


def test_facade_refuses_tent_without_samples_before_any_device():
    """Code -1 here means the arguments were checked first: on a machine without a device anything later is code -8."""
    s = M.Scene(encode((16, 8), scenes.all_ops(16, 8)))
    for k in (0, 1):
        with pytest.raises(M.MarayError) as e:
            M.gen_to_image(s, samples=k, filter=M.FILTER_TENT)
        assert e.value.code == E_ARG, k
    with pytest.raises(M.MarayError) as e:
        M.gen_to_image(s, samples=4, filter=2)
    assert e.value.code == E_ARG
    with pytest.raises(M.MarayError) as e:
        M.gen_to_image(s, samples=3, filter=M.FILTER_TENT)
    assert e.value.code == E_ARG

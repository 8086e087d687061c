"""The shutter's scene layer and command line (include/maray_hip.h, "shutter"): spans, the n x P matrix of frame values,
argument errors.  Needs no GPU."""
import math
import os
import subprocess

import numpy as np
import pytest

import maray_amd as M
import params as PR
from marayb import add, encode, nat, var, x, y

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
E_ARG = -1
FRAMES = (1, 2, 4, 8, 16, 32, 64)
CENTRES = [0.0, -0.0, 0.1, -37.5, 1e300, math.inf, math.nan]
SPANS = [0.0, 0.5, 1.0 / 3.0, 80.0]


def scene_with(n_params):
    s = M.Scene(encode((8, 8), [add(x(), var('p0')), y(), nat(1)]))
    for k in range(n_params):
        assert s.declare_param('p%d' % k) == k
    return s


def want_values(centres, spans, n):
    """The contract's formula, in Python's f64: c_i exact, one multiply, one add; span 0 copies the centre."""
    out = np.zeros((n, len(centres)), np.float64)
    for i in range(n):
        c = float(2 * i + 1 - n) / float(2 * n)
        for p, (v, s) in enumerate(zip(centres, spans)):
            out[i, p] = v + s * c if s > 0 else v
    return out


@pytest.mark.parametrize('n', FRAMES)
def test_shutter_values_equal_the_formula_bit_for_bit(n):
    cases = [(v, s) for v in CENTRES for s in SPANS if s == 0.0 or math.isfinite(v)]
    scene = scene_with(len(cases))
    for k, (v, s) in enumerate(cases):
        scene.set_param(k, v)
        scene.set_param_span(k, s)
        assert scene.param_span(k) == s
    got = scene.shutter_values(n)
    assert got.shape == (n, len(cases)) and got.dtype == np.float64
    want = want_values([v for v, _ in cases], [s for _, s in cases], n)
    assert PR.same_f64(got, want)
    assert np.array_equal(got.view(np.uint64)[~np.isnan(want)], want.view(np.uint64)[~np.isnan(want)])
    # span 0: the value itself in every frame, the sign of a zero and NaN included
    for k, (v, s) in enumerate(cases):
        if s == 0.0:
            col = got[:, k]
            assert all(math.isnan(c) for c in col) if v != v else all(c == v and math.copysign(1.0, c) == math.copysign(1.0, v) for c in col)
    # the frames are centred on the value and cover less than the span
    k = cases.index((0.1, 80.0))
    assert n == 1 and got[0, k] == 0.1 or (got[0, k] < 0.1 < got[-1, k] and got[-1, k] - got[0, k] < 80.0)


def test_negative_zero_with_span_zero_stays_negative_zero():
    scene = scene_with(2)
    scene.set_param(0, -0.0)
    scene.set_param(1, 3.0)
    scene.set_param_span(1, 80.0)
    for n in FRAMES:
        got = scene.shutter_values(n)
        assert all(v == 0.0 and math.copysign(1.0, v) < 0 for v in got[:, 0]), n


def test_spans_start_at_zero_and_are_not_part_of_the_programs_name():
    scene = scene_with(1)
    assert scene.param_span(0) == 0.0
    key = scene.lower().jit_code_key
    scene.set_param_span('p0', 12.5)
    assert scene.param_span(0) == 12.5 and scene.lower().jit_code_key == key
    assert scene.param_info(0)[1:3] == (-math.inf, math.inf)


def test_argument_errors():
    scene = scene_with(2)
    for n in (0, 3, 128):
        with pytest.raises(M.MarayError) as e:
            scene.shutter_values(n)
        assert e.value.code == E_ARG, n
    for span in (-1.0, -0.0 - 1e-300, math.nan, math.inf, -math.inf):
        with pytest.raises(M.MarayError) as e:
            scene.set_param_span(0, span)
        assert e.value.code == E_ARG, span
    assert scene.param_span(0) == 0.0
    with pytest.raises(M.MarayError) as e:
        scene.set_param_span(2, 1.0)
    assert e.value.code == E_ARG
    with pytest.raises(M.MarayError) as e:
        scene.param_span(2)
    assert e.value.code == E_ARG
    with pytest.raises(KeyError):
        scene.set_param_span('nobody', 1.0)


def test_gen_opts_keep_their_size():
    import ctypes as C
    assert C.sizeof(M.api.GenOpts) == 32 and M.api.GenOpts.shutter.offset == 16


def _cli(*args):
    return subprocess.run([os.path.join(ROOT, 'maray_amd', 'maray')] + list(args), capture_output=True, text=True, timeout=300,
                          env=dict(os.environ, HIP_VISIBLE_DEVICES='-1', ROCR_VISIBLE_DEVICES='-1'))


def test_cli_shutter_options(tmp_path):
    spec = PR.SCENES['slide'](64, 32)
    path = tmp_path / 'slide.maray'
    path.write_bytes(encode((64, 32), spec['color']))
    out = tmp_path / 'o.png'
    for bad in (['--shutter', 't=80', '--shutter-samples', '3'], ['--shutter-samples', '3'], ['--shutter-samples', '128'], ['--shutter', 't'],
                ['--shutter', 't=-1'], ['--shutter', 't=inf'], ['--shutter', 't=1:2']):
        r = _cli('-i', str(path), '-o', str(out), *bad)
        assert r.returncode == 2 and 'no HIP device' not in r.stderr, (bad, r.stderr)
        assert not out.exists()
    h = _cli('--help')
    assert h.returncode == 0 and '--shutter <' in h.stderr and '--shutter-samples' in h.stderr
    # a well-formed command line gets as far as the device
    ok = _cli('-i', str(path), '-o', str(out), '-p', 't=20:-512:512', '-p', 'u=-15', '--shutter', 't=80', '--shutter', 'u=40', '--shutter-samples', '4')
    assert ok.returncode == 1 and 'no HIP device' in ok.stderr and 'usage' not in ok.stderr.lower(), ok.stderr
    ok = _cli('-i', str(path), '-o', str(tmp_path / 'f%02d.png'), '--animate', 't=0:100:3', '--shutter', 't=16')
    assert ok.returncode == 1 and 'no HIP device' in ok.stderr and 'usage' not in ok.stderr.lower(), ok.stderr

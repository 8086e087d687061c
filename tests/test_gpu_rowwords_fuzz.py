"""Row words on the device, on random soups (tests/rowwords_fuzz_scenes.py): for each of twenty seeded soups the
fourth table of guard words and the flagged rectangles' row words against the numpy model (tests/rowwords_scenes.py) bit for bit,
and every raster of four launches -- RGB8 byte for byte, f64 planes bit for bit -- against the oracle's and against a context
created with MARAY_JIT_ROW_WORDS=0.  tests/test_rowwords_fuzz.py holds the condition that keeps these cases from being empty:
each has a flagged rectangle with a covered, an emptied and a mixed row.

Every test body runs in a child process with a time limit of its own; nothing follows a failure inside one.  A child prints one
line per case, `rowwords-fuzz: ...`; the test prints them again."""
import os
import subprocess
import sys

import pytest

import cover_fuzz_scenes as F
import rowwords_fuzz_scenes as RF

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

_CHILD = r"""
import sys
sys.path[:0] = [%(root)r, %(tests)r]
import test_gpu_rowwords_fuzz as T
T.child(%(kind)r)
print('child ok')
"""


def child(kind):
    import test_gpu_cover_fuzz as CF
    import test_gpu_rowwords as TR
    for case in [c for c in RF.CASES if c[0] == kind]:
        tape, color, _, _, _ = F.lowered(case)
        w, h, y0, y1 = case[2]
        want8, want64 = CF.oracle(color, None, None, case[2])
        m = TR.four_renders(tape, want8, w=w, h=h, y0=y0, y1=y1, want64=want64)
        full = RF.full_rectangles(tape, m)
        assert full, case
        print('rowwords-fuzz: %s seed %d %dx%d rows %d-%d: %d of %d rectangles flagged, %d with a covered, an emptied and a mixed row' %
              (case[0], case[1], w, h, y0, y1, int(m['flagged'].sum()), len(m['flagged']), len(full)))


@pytest.mark.parametrize('kind', F.KINDS)
def test_soups_words_and_rasters(kind):
    """Five soups of a kind: four launches with the knob on (the second takes the scan; the third and the fourth run
    maray_jit_pixels_rw), three with it off, the words after the fourth."""
    code = _CHILD % dict(root=ROOT, tests=HERE, kind=kind)
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith('child ok'), (out.stdout[-2000:], out.stderr[-4000:])
    lines = [ln for ln in out.stdout.split('\n') if ln.startswith('rowwords-fuzz:')]
    print('\n'.join(lines))
    assert len(lines) == 5

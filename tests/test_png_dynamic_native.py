"""Host code of the dynamic coder (png_device.cpp: the code lengths, the canonical codes, the header writer, the piece closer)
under AddressSanitizer and UBSan in a stand-alone program -- CPU build only, no device, nothing loaded into Python
(tests/native/png_dynamic_asan.cpp plays the device's part by emitting the tokens on the CPU).  The program's files are
inflated here by tests/png_stream.py and compared with the rasters it wrote beside them."""
import glob
import os
import re
import subprocess

import numpy as np

import png_stream as P
from conftest import ROOT


def test_dynamic_pieces_under_asan_ubsan(tmp_path):
    csrc = os.path.join(ROOT, 'maray_amd', 'csrc')
    rocm = os.environ.get('ROCM', '/opt/rocm')
    exe = str(tmp_path / 'png_dynamic_asan')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-D__HIP_PLATFORM_AMD__', '-I' + csrc, '-I' + os.path.join(ROOT, 'include'), '-I' + os.path.join(rocm, 'include'),
                           os.path.join(ROOT, 'tests', 'native', 'png_dynamic_asan.cpp'), os.path.join(csrc, 'png_device.cpp'),
                           os.path.join(csrc, 'png.cpp'), '-o', exe, '-lz', '-lpthread', '-L' + os.path.join(rocm, 'lib'), '-lamdhip64',
                           '-Wl,-rpath,' + os.path.join(rocm, 'lib')])
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=1', UBSAN_OPTIONS='print_stacktrace=1')
    files = tmp_path / 'files'
    files.mkdir()
    out = subprocess.run([exe, str(files)], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    assert 'all ok' in out.stdout
    pngs = sorted(glob.glob(str(files / '*.png')))
    assert len(pngs) >= 40
    for path in pngs:
        w, h = map(int, re.search(r'_(\d+)x(\d+)\.png$', path).groups())
        want = np.fromfile(path[:-4] + '.rgb', np.uint8).reshape(h, w, 3)
        assert np.array_equal(P.decode(open(path, 'rb').read()), want), path

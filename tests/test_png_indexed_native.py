"""Host code of the indexed-colour files (png_container.hpp's container with PLTE, png_indexed.hpp's depth rule and row
geometry, png_indexed.cpp's assembly) under AddressSanitizer and UBSan in a stand-alone program -- CPU build only, no device,
nothing loaded into Python (tests/native/png_indexed_asan.cpp plays the device's part with stored blocks)."""
import os
import subprocess

from conftest import ROOT


def test_the_indexed_container_and_assembly_under_asan_ubsan(tmp_path):
    csrc = os.path.join(ROOT, 'maray_amd', 'csrc')
    rocm = os.environ.get('ROCM', '/opt/rocm')
    exe = str(tmp_path / 'png_indexed_asan')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-D__HIP_PLATFORM_AMD__', '-I' + csrc, '-I' + os.path.join(ROOT, 'include'), '-I' + os.path.join(rocm, 'include'),
                           os.path.join(ROOT, 'tests', 'native', 'png_indexed_asan.cpp'), os.path.join(csrc, 'png_indexed.cpp'),
                           os.path.join(csrc, 'png_device.cpp'), os.path.join(csrc, 'png.cpp'), '-o', exe, '-lz', '-lpthread',
                           '-L' + os.path.join(rocm, 'lib'), '-lamdhip64', '-Wl,-rpath,' + os.path.join(rocm, 'lib')])
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=1', UBSAN_OPTIONS='print_stacktrace=1')
    out = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    assert 'all ok' in out.stdout

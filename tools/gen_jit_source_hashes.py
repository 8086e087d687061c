#!/usr/bin/env python3
"""tools/gen_jit_source_hashes.py — writes tests/golden/jit_source_hashes.json: SHA-256 of the kernel sources the generator
(maray_amd/csrc/jit_source.cpp, jit_emit.hpp) makes of a fixed set of scenes: the PIXEL source, the ROW source and the
supersampling sources for k = 2, 4, 8 of every scene of gen_tape_hashes.scenes_to_hash() and of a 1,000-triangle soup (the only
one with more than 12 guard words: one word per lane), and the same under each generator knob on a subset that the knob changes.
tests/test_jit_source_stability.py compares: a change to the generator that is meant to keep its output (a refactor) must leave
every hash alone -- same text, same compiler options, same kernels.  A change that is MEANT to alter kernels regenerates the
file (and says what it measured)."""
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')]
import maray_amd as M  # noqa: E402
from gen_tape_hashes import scenes_to_hash  # noqa: E402

SOUP_1000 = 'polygon soup 1000 triangles'
# each knob was checked to change at least one source of this subset (the generator reads a knob when it makes a source)
KNOB_SCENES = ('chess x4 y4 guarded', 'textured 512', 'polygon soup 5', 'curved soup 5', SOUP_1000)
KNOBS = ('MARAY_JIT_REDUCE=0', 'MARAY_JIT_FUSE_CMP=0', 'MARAY_JIT_TEXEL_ONCE=0', 'MARAY_JIT_WIDE_APP=0', 'MARAY_JIT_MIN_REGION=12',
         'MARAY_JIT_GUARD_W=256', 'MARAY_JIT_GUARD_W=128', 'MARAY_JIT_GUARD_H=8', 'MARAY_JIT_ROW_GUARDS=0')


def tapes():
    import fuzz_scenes
    from marayb import encode
    for name, s, kw in scenes_to_hash():
        yield name, s.lower(**kw)
    yield SOUP_1000, M.Scene(encode((1024, 256), fuzz_scenes.polygon_soup(21, 1000, 1024, 256, mixed=False))).lower()


def source_hashes(tape):
    """{kind: hash} of the five sources of a tape under the environment as it is."""
    L = M.lib()
    L.maray_jit_source.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    L.maray_jit_source_rows.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)]
    L.maray_jit_source_samples.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]
    p = C.byref(tape.program)
    calls = [('pixels', lambda src: L.maray_jit_source(p, src)), ('rows', lambda src: L.maray_jit_source_rows(p, src, C.byref(C.c_uint32())))]
    calls += [('samples %d' % k, lambda src, k=k: L.maray_jit_source_samples(p, k, src)) for k in (2, 4, 8)]
    out = {}
    for kind, call in calls:
        src = C.c_void_p()
        assert call(C.byref(src)) == 0, L.maray_last_error()
        out[kind] = hashlib.sha256(C.string_at(src)).hexdigest()[:24]
        L.maray_free(src)
    return out


def all_hashes():
    """{'default' | 'KNOB=value': {scene: {kind: hash}}}; the environment is left as it was found."""
    saved = {k: os.environ.pop(k) for k in list(os.environ) if k.startswith('MARAY_JIT_')}
    try:
        ts = dict(tapes())
        res = {'default': {name: source_hashes(t) for name, t in ts.items()}}
        for knob in KNOBS:
            var, val = knob.split('=')
            os.environ[var] = val
            try:
                res[knob] = {name: source_hashes(ts[name]) for name in KNOB_SCENES}
            finally:
                del os.environ[var]
        return res
    finally:
        os.environ.update(saved)


if __name__ == '__main__':
    out = os.path.join(ROOT, 'tests', 'golden', 'jit_source_hashes.json')
    json.dump(all_hashes(), open(out, 'w'), indent=1, sort_keys=True)
    print('wrote', out)

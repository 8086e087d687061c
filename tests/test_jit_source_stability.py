"""The generator's output on a fixed set of scenes, hash by hash (tests/golden/jit_source_hashes.json,
tools/gen_jit_source_hashes.py): the text of the PIXEL, ROW and supersampling kernels, under the default settings and under each
generator knob.  A kernel's source, the compiler's options and the launch are all there is to its speed and its results: a change
to the generator that is not meant to change the kernels (a refactor of jit_source.cpp or jit_emit.hpp) must leave these alone."""
import json
import os
import sys

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tools'))


def test_the_sources_of_the_fixed_scenes_are_what_they_were():
    import gen_jit_source_hashes
    want = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'jit_source_hashes.json')))
    got = gen_jit_source_hashes.all_hashes()
    assert sorted(got) == sorted(want)
    for setting in want:
        assert sorted(got[setting]) == sorted(want[setting]), setting
    changed = [(setting, scene, kind) for setting in want for scene in want[setting] for kind in want[setting][scene]
               if got[setting][scene].get(kind) != want[setting][scene][kind]]
    assert not changed, ('generated sources changed (regenerate with tools/gen_jit_source_hashes.py if that was meant, and measure the '
                         'kernels again): %s' % changed)

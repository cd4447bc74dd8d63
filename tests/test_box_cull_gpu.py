"""The box cull (csrc/bmo_lane.hpp box_cull, DESIGN.md §3 "box cull") on the GPU: the engine against the oracle — which knows no cull — at
zero tolerance on BASELINE bundles, a retrace, a sweep whose second configuration moves a lens (the boxes must move with it), the
directed mini scenes of tests/box_scenes.py, and one wave whose lanes disagree on the cull.  Every GPU step runs in a child process of
its own under a time limit (tests/box_gpu_step.py), a few seconds each.  These tests are the ones that read the blob's box table on the
device (the emulator of tests/test_box_cull.py has no blob and derives each box on the spot, by the same shape_box)."""
import os
import subprocess
import sys

import pytest

import box_scenes as bx

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
BASELINE = [("c2s", 4096), ("c5", 4096), ("c3", 1024), ("c4", 1024)]


_stopped = None  # the step that ended in a fault, an abort or at its time limit: nothing more is started on the GPU after it


def _step(*args, limit=120, wide=False):
    """One GPU step: tests/box_gpu_step.py <args> as a fresh process under `timeout`; its output is shown when it fails.  After a step
    that ended in a time limit (124, 137), an abort (134) or a segmentation fault (139), or by any other signal, no further step is
    started: the remaining tests of this file fail without touching the GPU."""
    global _stopped
    assert _stopped is None, "not started: an earlier GPU step of this file ended abnormally (%s)" % _stopped
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.join(HERE, "box_gpu_step.py")] + [str(a) for a in args]
    env = dict(os.environ, BOX_EMU_BUILD_DIR=bx.emu_dir())  # (one host build of the emulator for all steps)
    if wide:  # the Ray kernel's build for large launches at any size: the variant of the plain-shapes level that runs the box test
        env["BMO_WIDE_MIN_WAVES"] = "0"
        env["BMO_DEBUG"] = "1"  # (the step log on stderr names the kernel build of every launch)
    p = subprocess.run(cmd, capture_output=True, text=True, env=env)
    if p.returncode in (124, 134, 137, 139) or p.returncode < 0 or "illegal memory access" in p.stderr:
        _stopped = "%s: exit %d" % (" ".join(cmd[4:]), p.returncode)
    assert p.returncode == 0, "%s: exit %d\n%s\n%s" % (" ".join(cmd[4:]), p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    if wide:  # not vacuous: some launch of the step did run that variant
        assert "kernel build: 4 waves per SIMD, in-loop splitters" in p.stderr, p.stderr[-2000:]
    return p.stdout


@pytest.mark.parametrize("name,n", BASELINE)
def test_engine_equals_oracle_on_baseline_bundles(name, n):
    assert "equal" in _step("baseline", name, n)


def test_engine_equals_oracle_on_the_headline_bundle_in_the_kernel_of_large_launches():
    assert "equal" in _step("baseline", "c2s", 4096, wide=True)


def test_engine_retrace_equals_oracle():
    assert "equal" in _step("retrace")


def test_sweep_boxes_move_with_the_lens():
    assert "equal" in _step("sweep")


@pytest.mark.parametrize("name", list(bx.DIRECTED))
def test_engine_equals_oracle_on_directed_scenes(name):
    # (the asphere takes its scene to the kernels of the extended-shape level: every variant of those runs the box test, none is "wide")
    assert "equal" in _step("directed", name, wide=name != "asphere_and_sphereless_lens_without_boxes")

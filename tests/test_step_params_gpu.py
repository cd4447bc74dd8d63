"""The step kernels read their launch parameters where they use them (csrc/bmo_engine.hip `step_params_again`): at the head of every
bounce level and again behind the marches the fields of StepParams come from the kernel-argument segment by scalar loads instead of being
held — spilled into vector-register lanes — for the whole kernel.  These cases take every field that is read that way through the engine at the
smallest sizes that still reach the path, each against the oracle at zero tolerance (tests/parity.py):

  chunk of the level   `cur` at level 0, `inner[b - 1]` from level 1 on, `inner[b]` for the in-place write, `nxt` for the compaction: fuse depths
  `pend`               the splitter chain (a kept reflected child, a second split while one waits, kept children compacted at the end of a loop)
  `nodes.*`, `ctr`     every case (node tables of ended beams, children, the slot allocation)
  `r_max`              the header of every record that goes on
  `old`                the retrace kernels;  `sweep` (the same bytes of the arguments) a sweep
  `wave_last`          cases with and without the segment log
  `lane_shift`         fewer records per wave than lanes (the knob is read once per process: a child process)

and two launches in a row on one stream whose parameters differ.

The change these cases came with alters no result, so they hold for the engine before it too (all but the debug line that names the kernel
build): they are parity cases aimed at the parameter fields, not a before / after test."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import bmo_amd as bmo
import scenes
from parity import compare
from test_retrace import RETRACE_CASES, retrace_pair
from test_splitter_chain import _bundle as chain_bundle, _chain
from test_sweep_gpu import _perturbed_snapshots, _sweep_vs_separate

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAIN_R_MAX = 50


def _trace(scene, bundle, r_max=100):
    eng = bmo.Engine(scene, 0)
    try:
        return eng.trace(bundle, r_max)
    finally:
        eng.close()


@pytest.fixture(scope="module")
def disc(oracle):
    """config 2's scene under SURVEY 8(d)'s collimated disc (the bench's `c2s`), 2 048 rays = 32 waves, and the oracle's solution"""
    system, _ = scenes.c2_scene()
    bundle = scenes.c2_survey_bundle(2048)
    scene = bmo.CompiledScene(system, bundle.lambdas)
    return scene, bundle, oracle.trace(scene, bundle, 100, threads=16)


@pytest.fixture(scope="module")
def chain(oracle):
    """test_splitter_chain's scene (a lens, four thin splitters in a row, a detector) under 96 rays = 1.5 waves"""
    bundle = chain_bundle("ray", 96)
    scene = bmo.CompiledScene(_chain(4), bundle.lambdas)
    ref = oracle.trace(scene, bundle, CHAIN_R_MAX, threads=8)
    assert ref.n_nodes >= 9 * bundle.n  # the transmitted beam meets the next splitter: at least 1 + 2 x 4 beams per ray
    return scene, bundle, ref


def _child(mode, **env):
    """This file as a child process (knobs the engine reads once per process: `BMO_DEBUG`, `BMO_THIN_WAVES`); the child compares with the oracle itself."""
    path = os.pathsep.join([ROOT, os.path.join(ROOT, "oracle")] + ([os.environ["PYTHONPATH"]] if os.environ.get("PYTHONPATH") else []))
    env = dict(os.environ, BMO_DEBUG="1", PYTHONPATH=path, **env)
    for name in ("BMO_FUSE", "BMO_WIDE_MIN_WAVES"):
        env.pop(name, None)
    r = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), mode], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stderr


def test_disc_through_the_wide_and_the_narrow_build():
    """The 4-waves-per-SIMD and the 3-waves-per-SIMD build of the Ray kernels (`BMO_WIDE_MIN_WAVES`, read per launch), one solve each; the
    engine's debug line says which build every launch ran, so the two solves are known to have run different kernels."""
    err = _child("wide-narrow")
    wide, narrow = err.split("== BMO_WIDE_MIN_WAVES=1\n")[1].split("== BMO_WIDE_MIN_WAVES=1000000000\n")
    assert "kernel build: 4 waves per SIMD" in wide and "kernel build: default" not in wide, wide[-2000:]
    assert "kernel build: default waves per SIMD" in narrow and "kernel build: 4 waves" not in narrow, narrow[-2000:]


def test_fuse_depths_address_every_chunk_of_a_launch(disc, monkeypatch):
    """`BMO_FUSE` = 1, 2, 3 and unset: a launch reads level 0 from `cur` and level b from `inner[b - 1]`, writes in place into `inner[b]` and
    compacts into `nxt`.  A launch advances a beam by at most its fuse depth, so a solve takes at least deepest / depth launches; the
    number of launches differs, the solution does not."""
    scene, bundle, ref = disc
    deepest = int(ref.node_nseg.max())
    steps = {}
    for fuse in ("1", "2", "3", None):
        if fuse is None:
            monkeypatch.delenv("BMO_FUSE", raising=False)
        else:
            monkeypatch.setenv("BMO_FUSE", fuse)
        got = _trace(scene, bundle)
        compare(got, ref, 0.0, "disc, BMO_FUSE=%s" % fuse)
        steps[fuse] = got.n_steps
        assert got.n_steps >= math.ceil(deepest / (32 if fuse is None else int(fuse))), (fuse, got.n_steps, deepest)
    assert steps["1"] > steps[None], steps


def test_segment_log_off(disc):
    """`record_segments = 0` (nobody reads the in-place levels: no `wave_last`): beam tree, statuses, counts and detector rows as with the log."""
    scene, bundle, ref = disc
    eng = bmo.Engine(scene, 0)
    try:
        dev = eng.upload(bundle)
        res = eng.trace_device(dev, 100, record_segments=False)
        assert eng.result_size(res) == (ref.n_intersect_calls, ref.n_records, ref.n_nodes, int(ref.det_count.sum()))
        got = eng.result_view(res)
        eng.free_result(res)
        eng.free_batch(dev)
    finally:
        eng.close()
    for name in ("node_root", "node_parent", "node_first_child", "node_nseg", "node_status", "det_count", "det_offset", "det_node"):
        assert np.array_equal(getattr(got, name), getattr(ref, name)), name
    assert np.array_equal(got.det_data.view(np.int64), ref.det_data.view(np.int64))
    assert got.n_records == 0 and got.rec.size == 0


def test_splitter_chain_in_one_and_a_half_waves(chain):
    """In-loop splits, a kept reflected child (`pend`), a second split while one child waits, idle lanes in the second wave."""
    scene, bundle, ref = chain
    compare(_trace(scene, bundle, CHAIN_R_MAX), ref, 0.0, "splitter chain, 96 rays")


def test_second_launch_reads_its_own_parameters(chain, monkeypatch):
    """`BMO_FUSE=4` ends the first launch in the middle of the chain: the launches that follow on the same stream have other chunks, another
    counter slot (`parity`), another node count (`nodes0`) — a launch that read its predecessor's parameters would not give the oracle's tree."""
    scene, bundle, ref = chain
    monkeypatch.setenv("BMO_FUSE", "4")
    got = _trace(scene, bundle, CHAIN_R_MAX)
    assert got.n_steps >= 2, got.n_steps
    compare(got, ref, 0.0, "splitter chain, BMO_FUSE=4")


def test_gaussian_splitter_chain(oracle, monkeypatch):
    """`step_kernel_gauss` through what the two cases above take `step_kernel` through, 96 GaussianBeamlets = 1.5 waves: in-loop splits, a kept
    reflected child (`gkeep`), a second split while one waits (pushed to `nxt`), a lane that takes its kept child up, kept children compacted
    at the end of a loop; then a launch that ends in the middle of the chain (the beamlet kernels take their fuse depth from `BMO_FUSE_GAUSS`);
    then one retrace after the second splitter was tilted: children re-walk their stored beamlets and keep the stored waist."""
    system = _chain(4)
    bundle = chain_bundle("gauss", 96)
    scene0 = bmo.CompiledScene(system, bundle.lambdas)
    ref0, sol = oracle.trace(scene0, bundle, CHAIN_R_MAX, threads=8, keep=True)
    assert ref0.n_nodes >= 9 * bundle.n
    for name in ("BMO_FUSE", "BMO_FUSE_GAUSS"):
        monkeypatch.delenv(name, raising=False)
    compare(_trace(scene0, bundle, CHAIN_R_MAX), ref0, 0.0, "splitter chain, 96 beamlets")
    monkeypatch.setenv("BMO_FUSE", "4")
    monkeypatch.setenv("BMO_FUSE_GAUSS", "4")
    got = _trace(scene0, bundle, CHAIN_R_MAX)
    assert got.n_steps >= 2, got.n_steps
    compare(got, ref0, 0.0, "splitter chain, 96 beamlets, fuse depth 4")
    monkeypatch.delenv("BMO_FUSE")
    monkeypatch.delenv("BMO_FUSE_GAUSS")
    bmo.xrotate3d(system.objects_tree[2], math.radians(0.7))
    scene1 = bmo.CompiledScene(system, bundle.lambdas)
    ref1 = oracle.trace(scene1, bundle, CHAIN_R_MAX, threads=8, prev=sol)
    g0, h0 = bmo.system._engine_solve(scene0, bundle, CHAIN_R_MAX, None)
    try:
        g1, h1 = bmo.system._engine_solve(scene1, bundle, CHAIN_R_MAX, h0)
        try:
            compare(g1, ref1, 0.0, "splitter chain, 96 beamlets, retrace")
        finally:
            h1.free()
    finally:
        h0.free()


def test_fewer_records_per_wave_than_lanes():
    """`BMO_THIN_WAVES=8` spreads the 96 records over six waves of 16 (`lane_shift` = 4: the upper lanes idle).  The knob is read once per
    process, so the solve runs in a child process that compares with the oracle itself."""
    err = _child("thin-waves", BMO_THIN_WAVES="8")
    assert "launching m=96, 16 records per wave" in err, err[-2000:]


@pytest.mark.parametrize("case", RETRACE_CASES)
def test_retrace_after_a_move(oracle, case):
    """The retrace kernels (`old`: the previous solution's tables) after a kinematic move, 192 rays = 3 waves."""
    scene0, scene1, bundle = retrace_pair("ray", case, 192)
    a0, sol = oracle.trace(scene0, bundle, 20, threads=8, keep=True)
    a1 = oracle.trace(scene1, bundle, 20, threads=8, prev=sol)
    g0, h0 = bmo.system._engine_solve(scene0, bundle, 20, None)
    try:
        compare(g0, a0, 0.0, case + ", first solve")
        g1, h1 = bmo.system._engine_solve(scene1, bundle, 20, h0)
        try:
            compare(g1, a1, 0.0, case + ", retrace")
        finally:
            h1.free()
    finally:
        h0.free()


def test_sweep_of_three_configurations(oracle):
    """3 configurations x 64 rays in one sweep launch (`sweep`, in the room `old` has in the other kernels' arguments)."""
    system, _ = scenes.c2_scene()
    bundle = scenes.c2_bundle(64)
    snaps = _perturbed_snapshots(system, bundle.lambdas, 3, 11)
    _sweep_vs_separate(snaps, [bundle] * 3, 100, label="c2 sweep", oracle=oracle, oracle_every=1)


def test_gaussian_beamlets(oracle):
    system, _ = scenes.c2_scene()
    bundle = scenes.c3_bundle(256)
    scene = bmo.CompiledScene(system, bundle.lambdas)
    compare(_trace(scene, bundle), oracle.trace(scene, bundle, 100, threads=16), 0.0, "c3, 256 beamlets")


def test_polarized_rays(oracle):
    system, _ = scenes.c4_scene()
    bundle = scenes.c4_bundle(256)
    scene = bmo.CompiledScene(system, bundle.lambdas)
    compare(_trace(scene, bundle), oracle.trace(scene, bundle, 100, threads=16), 0.0, "c4, 256 PolarizedRays")


if __name__ == "__main__":  # the child processes of _child
    import pyoracle

    if sys.argv[1:] == ["thin-waves"]:
        b = chain_bundle("ray", 96)
        s = bmo.CompiledScene(_chain(4), b.lambdas)
        compare(_trace(s, b, CHAIN_R_MAX), pyoracle.trace(s, b, CHAIN_R_MAX, threads=8), 0.0, "splitter chain, BMO_THIN_WAVES=8")
    elif sys.argv[1:] == ["wide-narrow"]:
        b = scenes.c2_survey_bundle(2048)
        s = bmo.CompiledScene(scenes.c2_scene()[0], b.lambdas)
        want = pyoracle.trace(s, b, 100, threads=16)
        for wide_min in ("1", "1000000000"):
            os.environ["BMO_WIDE_MIN_WAVES"] = wide_min
            print("== BMO_WIDE_MIN_WAVES=" + wide_min, file=sys.stderr, flush=True)
            compare(_trace(s, b), want, 0.0, "disc, BMO_WIDE_MIN_WAVES=" + wide_min)
    else:
        raise SystemExit("unknown mode %r" % sys.argv[1:])

"""The box cull (csrc/bmo_lane.hpp box_cull, DESIGN.md §3 "box cull") is result-preserving — CPU part.

The emulator is built twice, with BMO_BOX_CULL on and off (both with BMO_EMU_STATS).  Both builds must equal the oracle — which knows no
cull at all — and each other at zero tolerance, `calls` and detector hit counts included, on the BASELINE bundles, on random scenes, on
a retrace and on directed mini scenes that aim at the cull's edge cases.  The switch-on build must cull something on every BASELINE
bundle (so the comparison is not vacuous) and the switch-off build nothing.  Containment: every intersection point the oracle reports
on a shape lies inside that shape's box before its margin, to 1e-9 m.

The emulator builds its SceneView from the description, not from a blob: its tracing_step derives each candidate's box on the spot with
shape_box, the function the scene builder fills the blob's table with.  The table itself, its offset and its place in a sweep's
configurations are read here only through bmo_emu_box_table (test_box_table_rules, the directed scenes) and on the device by
tests/test_box_cull_gpu.py."""
import numpy as np
import pytest

import bmo_amd as bmo
import box_scenes as bx
import scenes
from parity import compare
from test_fuzz import R_MAX as FUZZ_R_MAX, _case, _limit, _retrace_case

R_MAX = 100  # the benchmark's


def _both_equal_oracle(oracle, scene, bundle, r_max, label, max_beams=0):
    """(marches started, candidates culled) of the switch-on build, after the three comparisons and the containment check."""
    on, started, culled = bx.emu_trace(1, scene, bundle, r_max, max_beams=max_beams)
    off, started0, culled0 = bx.emu_trace(0, scene, bundle, r_max, max_beams=max_beams)
    ref = oracle.trace(scene, bundle, r_max, threads=8)
    compare(on, ref, 0.0, label + ": box cull on vs oracle")
    compare(off, ref, 0.0, label + ": box cull off vs oracle")
    compare(on, off, 0.0, label + ": on vs off")
    assert np.array_equal(on.det_count, ref.det_count) and on.n_intersect_calls == off.n_intersect_calls == ref.n_intersect_calls
    assert culled0 == 0 and started0 == started + culled, (label, started, culled, started0, culled0)
    bx.hits_inside_boxes(scene, ref)
    return started, culled


BASELINE = {
    "c2s": (scenes.c2_scene, scenes.c2_survey_bundle, 2048),
    "c2v": (scenes.c2_scene, scenes.c2_vignetted_bundle, 2048),
    "c2": (scenes.c2_scene, scenes.c2_bundle, 2048),
    "c5": (scenes.c5_scene, scenes.c5_bundle, 2048),
    "c3": (scenes.c2_scene, scenes.c3_bundle, 512),
    "c4": (scenes.c4_scene, scenes.c4_bundle, 512),
}


@pytest.mark.parametrize("name", list(BASELINE))
def test_baseline_bundles(oracle, name):
    scene_fn, bundle_fn, n = BASELINE[name]
    bundle = bundle_fn(n)
    scene = bmo.CompiledScene(scene_fn()[0], bundle.lambdas)
    started, culled = _both_equal_oracle(oracle, scene, bundle, R_MAX, name)
    print("%s: %d marches started, %d candidates culled by their box" % (name, started, culled))
    if name in ("c2s", "c2v", "c2", "c5"):
        assert culled > 0, name


# 35 scenes of tests/test_fuzz.py's generator: Ray, PolarizedRay and GaussianBeamlet bundles (119: a runaway beam tree, which that file skips)
FUZZ = [(seed, "ray") for seed in range(101, 127) if seed != 119] + [(seed, "pol") for seed in range(201, 206)] + [(seed, "gauss") for seed in range(301, 306)]


@pytest.mark.parametrize("seed,kind", FUZZ)
def test_random_scenes(oracle, seed, kind):
    scene, bundle = _case(seed, kind, 128 if kind == "ray" else 64)
    _both_equal_oracle(oracle, scene, bundle, FUZZ_R_MAX, "fuzz %d %s" % (seed, kind), max_beams=_limit(bundle.n))


def test_retrace(oracle):
    scene0, scene1, bundle = _retrace_case(401, "ray", 96)
    on0 = bx.emu_trace(1, scene0, bundle, FUZZ_R_MAX)[0]
    on1 = bx.emu_trace(1, scene1, bundle, FUZZ_R_MAX, prev=on0)[0]
    off0 = bx.emu_trace(0, scene0, bundle, FUZZ_R_MAX)[0]
    off1 = bx.emu_trace(0, scene1, bundle, FUZZ_R_MAX, prev=off0)[0]
    a0, sol = oracle.trace(scene0, bundle, FUZZ_R_MAX, threads=4, keep=True)
    a1 = oracle.trace(scene1, bundle, FUZZ_R_MAX, threads=4, prev=sol)
    compare(on0, a0, 0.0, "first solve, box cull on")
    compare(on1, a1, 0.0, "retrace, box cull on")
    compare(off1, a1, 0.0, "retrace, box cull off")
    compare(on1, off1, 0.0, "retrace, on vs off")
    bx.hits_inside_boxes(scene1, a1)


@pytest.mark.parametrize("name", list(bx.DIRECTED))
def test_directed_scenes(oracle, name):
    scene, bundle = bx.DIRECTED[name]()
    assert bundle.n <= 64
    started, culled = _both_equal_oracle(oracle, scene, bundle, bx.R_MAX, name)
    print("%s: %d marches started, %d candidates culled by their box" % (name, started, culled))
    if name in ("rim_graze_inside_the_margin", "rim_fan_lanes_disagree", "plate_splitter_behind_culled_lenses"):
        assert culled > 0, name  # (what these scenes are built for)


def test_face_plane_rays_hit_the_lens(oracle):
    """The rays that start on the front face plane of the first lens's box do hit that lens (the scene is what its name says)."""
    for zeros in (1, 2):
        scene, bundle = bx.face_plane_case(zeros)
        ref = oracle.trace(scene, bundle, bx.R_MAX, threads=4)
        first = np.asarray(ref.rec_obj)[np.asarray(ref.node_first_rec)[:6]]
        assert (first == 0).all(), first
        assert int((np.asarray(bundle.planes)[3:6] == 0.0).all(axis=1).sum()) == zeros


def test_box_table_rules():
    """No box for meshes, inexact shapes and shapes without a sphere; a union's box is the hull of its children's; the margin is the
    bounding sphere's r * 1e-6 + 1 um with r half the diagonal."""
    scene, _ = bx.no_box_case()
    table, raw = bx.box_table(scene)
    d = scene.desc
    for s in range(d.n_shapes):
        sh = scene._shapes[s]
        if table[s, 0] > table[s, 3]:
            assert (table[s, :3] > table[s, 3:]).all() and (raw[s, :3] > raw[s, 3:]).all()
            continue
        assert not (sh.flags & 1) and sh.bs_radius >= 0 and sh.kind != 0
        r = 0.5 * np.linalg.norm(raw[s, 3:] - raw[s, :3])
        m = r * 1e-6 + 1e-6
        assert np.allclose(table[s, :3], raw[s, :3] - m, rtol=0, atol=1e-15) and np.allclose(table[s, 3:], raw[s, 3:] + m, rtol=0, atol=1e-15)
        if sh.kind == 5:  # UNION
            kids = [d.children[sh.child_begin + c] for c in range(sh.child_count)]
            assert np.array_equal(raw[s, :3], raw[kids, :3].min(axis=0)) and np.array_equal(raw[s, 3:], raw[kids, 3:].max(axis=0))
        c = np.array(sh.bs_center[:])  # the bounding sphere's centre lies in the box
        assert (raw[s, :3] <= c).all() and (c <= raw[s, 3:]).all()
    mesh = bmo.Mirror(bmo.CircularFlatMesh(5e-3, 12))
    sc = bmo.CompiledScene(bmo.System([mesh]), [bx.LAM])
    t, _ = bx.box_table(sc)
    assert (t[:, 0] > t[:, 3]).all()

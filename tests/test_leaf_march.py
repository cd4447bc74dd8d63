"""Outside marches of a single plain shape in tracing_step's specialised march loop (csrc/bmo_lane.hpp, BMO_LEAF_MARCH).

The loop that round 5 gave the union marches also takes the lanes that march a shape which is no union (leaf classes 1 - 5): the
shape is its own "child", the `others_lb` compare is vacuous.  A trip that ends the march (hit, recede, `lim` prune, iteration limit)
is not committed; the generic trip repeats it from the same state.

CPU: the host emulator built twice, both with every kernel's fast path forced on (BMO_MARCH_FASTPATH=2) and with BMO_EMU_STATS, once
with BMO_LEAF_MARCH=1 and once with 0 (the parent's loop: unions only).  Both must equal the oracle and each other bit for bit, make
the same number of SDF evaluations, and the on build's counter of committed single-shape trips must grow — otherwise the test proves
nothing.  The mini scenes below take the loop through each of its exits.
GPU: the grazing mini scene, the hinted-shape waterfall, and config 2's disc and ragged bundles through the 3- and the 4-waves build of
the step kernels, for the three beam kinds, against the oracle at tolerance 0.
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import bmo_amd as bmo
import parity
import scenes
from bmo_amd import abi
from parity import compare, emu_trace
from test_fuzz import _case, _engine_first, _limit, R_MAX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_SRC = os.path.join(ROOT, "tests", "emu", "emu.cpp")
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-shared", "-DBMO_MARCH_FASTPATH=2", "-DBMO_EMU_STATS",
         "-fno-gnu-unique"]  # (the counters are inline variables: as GNU unique symbols the two libraries would share one set)
mm = 1e-3
FLAG_INEXACT = 1


def _load(path):
    lib = C.CDLL(path)
    lib.bmo_emu_trace.argtypes = [C.POINTER(abi.SceneDesc), C.POINTER(abi.RayBatch), C.POINTER(abi.TraceOpts), C.POINTER(C.c_void_p),
                                  C.POINTER(abi.ResultView)]
    lib.bmo_emu_free.argtypes = [C.c_void_p]
    lib.bmo_emu_retrace.argtypes = [C.POINTER(abi.SceneDesc), C.POINTER(abi.RayBatch), C.POINTER(abi.TraceOpts), C.POINTER(abi.ResultView),
                                    C.POINTER(C.c_void_p), C.POINTER(abi.ResultView)]
    return lib


@pytest.fixture(scope="module")
def emus(tmp_path_factory):
    d = tmp_path_factory.mktemp("emu_leaf_march")
    libs = {}
    for mode, leaf in (("on", "1"), ("off", "0")):
        so = str(d / ("libemu_%s.so" % mode))
        subprocess.check_call(["g++"] + FLAGS + ["-DBMO_LEAF_MARCH=" + leaf, "-o", so, EMU_SRC])
        libs[mode] = _load(so)
    return libs


def _trace(lib, scene, bundle, r_max, **kw):
    saved = parity._emu
    parity._emu = lib
    try:
        return emu_trace(scene, bundle, r_max, **kw)
    finally:
        parity._emu = saved


def _counter(lib, name):
    return C.c_long.in_dll(lib, "_ZN3bmo%d%sE" % (len(name), name)).value


class _Counts:
    """What a block of traces added to an emulator's counters."""

    NAMES = ("g_emu_sdf_any", "g_emu_sdf_leaf", "g_emu_leaf_outside", "g_emu_leaf_loop", "g_emu_leaf_loop_back", "g_emu_union_loop")

    def __init__(self, lib):
        self.lib = lib
        self.t0 = {n: _counter(lib, n) for n in self.NAMES}

    def __getitem__(self, name):
        return _counter(self.lib, "g_emu_" + name) - self.t0["g_emu_" + name]

    def frozen(self):
        return {n[6:]: self[n[6:]] for n in self.NAMES}


def _on_off_oracle(oracle, emus, scene, bundle, r_max, label, **kw):
    """Trace with both builds and the oracle, require equal bits and equal evaluation counts; returns the on build's counts."""
    con, coff = _Counts(emus["on"]), _Counts(emus["off"])
    on = _trace(emus["on"], scene, bundle, r_max, **kw)
    off = _trace(emus["off"], scene, bundle, r_max, **kw)
    ref = oracle.trace(scene, bundle, r_max, threads=4)
    compare(on, ref, 0.0, label + " loop on")
    compare(off, ref, 0.0, label + " loop off")
    compare(on, off, 0.0, label + " on vs off")
    assert coff["leaf_loop"] == 0
    assert con["sdf_any"] == coff["sdf_any"] and con["sdf_leaf"] == coff["sdf_leaf"], (label, "evaluation counts differ")
    assert con["union_loop"] == coff["union_loop"], label
    # every trip is either committed in the loop or made by the generic branch
    assert con["leaf_loop"] + con["leaf_outside"] == coff["leaf_outside"], label
    return con.frozen(), on


# ---------------------------------------------------------------------------------------------------------------- configs, random scenes
BUNDLES = {
    "c2s": lambda: (scenes.c2_scene()[0], scenes.c2_survey_bundle(2048)),
    "c2v": lambda: (scenes.c2_scene()[0], scenes.c2_vignetted_bundle(2048)),
    "c2": lambda: (scenes.c2_scene()[0], scenes.c2_bundle(1024)),
    "c5": lambda: (scenes.c5_scene()[0], scenes.c5_bundle(1024)),
}


@pytest.mark.parametrize("name", sorted(BUNDLES))
def test_leaf_march_equals_oracle_on_configs(oracle, emus, name):
    system, bundle = BUNDLES[name]()
    scene = bmo.CompiledScene(system, bundle.lambdas)
    con, _ = _on_off_oracle(oracle, emus, scene, bundle, 20, name)
    assert con["leaf_loop"] > 0, "the single-shape loop was never taken"


def test_leaf_march_equals_off_on_retrace(oracle, emus):
    system, bundle = BUNDLES["c2s"]()
    scene = bmo.CompiledScene(system, bundle.lambdas)
    first = _trace(emus["on"], scene, bundle, 20)
    con = _Counts(emus["on"])
    on = _trace(emus["on"], scene, bundle, 20, prev=first)
    off = _trace(emus["off"], scene, bundle, 20, prev=first)
    assert con["leaf_loop"] > 0
    compare(on, off, 0.0, "c2s retrace on vs off")


# (the random-scene list of test_march_fastpath.py; seed 119 draws a runaway beam tree: test_fuzz.py skips it)
CASES = [(seed, "ray") for seed in range(101, 125) if seed != 119] + [(seed, "pol") for seed in range(201, 207)] + [(seed, "gauss") for seed in range(301, 307)]


@pytest.mark.parametrize("seed,kind", CASES)
def test_leaf_march_equals_oracle_on_random_scenes(oracle, emus, seed, kind):
    scene, bundle = _case(seed, kind, 128 if kind == "ray" else 64)
    on = _engine_first(lambda: _trace(emus["on"], scene, bundle, R_MAX, max_beams=_limit(bundle.n)))
    ref = oracle.trace(scene, bundle, R_MAX, threads=4)
    compare(on, ref, 0.0, "fuzz %d %s loop on" % (seed, kind))
    off = _trace(emus["off"], scene, bundle, R_MAX, max_beams=_limit(bundle.n))
    compare(on, off, 0.0, "fuzz %d %s on vs off" % (seed, kind))


# ---------------------------------------------------------------------------------------------------------------- grazing exit
ROD_R, ROD_H = 2 * mm, 40 * mm


def _rod_scene():
    """A glass rod along y (one CylinderSDF: a plain shape of leaf class 1) whose index is so close to 1 that a ray inside leaves through the
    barrel at 20 mrad and more instead of being reflected (critical grazing angle sqrt(2e-4) = 14 mrad)."""
    rod = bmo.Lens(bmo.CylinderSDF(ROD_R, ROD_H), lambda lam: 1.0001)
    return bmo.System([rod])


def _rays(pos, dirs, lam=1.064e-6):
    dirs = np.asarray(dirs, dtype=np.float64)
    dirs = dirs / np.sqrt((dirs * dirs).sum(axis=1))[:, None]
    return bmo.RayBundle.rays(np.asarray(pos, dtype=np.float64), dirs, lam)


def _grazing_rays(n, graze):
    """n rays that enter the rod's end face; those of `graze` (a mask) run radially outwards at 20 - 25 mrad to the axis and leave through
    the barrel 7 - 40 mm further on: the march back to the wall from the eps_ins step shrinks its distance by sin(angle) per trip.  The
    others run along the axis and leave through the far face."""
    k = np.arange(n)
    phi = k * (2 * math.pi / (1 + math.sqrt(5)))
    x0 = np.where(graze, (1.2 + 0.5 * ((k * 7) % 16) / 15.0) * mm, 0.8 * mm * np.sqrt((k + 0.5) / n))
    th = np.where(graze, 20e-3 + 5e-3 * ((k * 5) % 64) / 63.0, 0.0)
    pos = np.stack([x0 * np.cos(phi), np.full(n, -50 * mm), x0 * np.sin(phi)], axis=1)
    dirs = np.stack([np.sin(th) * np.cos(phi), np.cos(th), np.sin(th) * np.sin(phi)], axis=1)
    return _rays(pos, dirs)


def _one_in_64(n):
    return (np.arange(n) % 64) == 37


def test_grazing_exit_through_a_barrel(oracle, emus):
    system = _rod_scene()
    # the reference's cost of ONE such ray (the emulator counts one sdf_any call per evaluation of the reference)
    one = _grazing_rays(1, np.ones(1, dtype=bool))
    scene = bmo.CompiledScene(system, one.lambdas)
    coff = _Counts(emus["off"])
    _trace(emus["off"], scene, one, 20)
    assert coff.frozen()["sdf_any"] > 300
    for label, bundle in (("all of 64 graze", _grazing_rays(64, np.ones(64, dtype=bool))), ("one of 64 grazes", _grazing_rays(64, _one_in_64(64)))):
        scene = bmo.CompiledScene(system, bundle.lambdas)
        con, on = _on_off_oracle(oracle, emus, scene, bundle, 20, label)
        n_graze = 64 if label.startswith("all") else 1
        assert con["leaf_loop_back"] > 300 * n_graze, (label, con["leaf_loop_back"])
        assert on.n_records == 3 * 64  # every ray crosses the rod: in through the end face, out through the barrel or the far face


# ---------------------------------------------------------------------------------------------------------------- one scene per exit
def _window(d=10 * mm, t=2 * mm, n=1.5):
    return bmo.Lens(bmo.PlanoSurfaceSDF(t, d), lambda lam, n=n: n)


def _axial_disc(n, diameter, y=-20 * mm, jitter=2e-3):
    return scenes.disc_bundle(n, center=[0, y, 0], direction=[0, 1, 0], diameter=diameter, e1=[1, 0, 0], jitter=jitter)


def test_back_march_on_a_single_plain_shape(oracle, emus):
    """Rays through a window: inside it the march steps eps_ins ahead and comes back along -dir (ST_BACK) on the one plain shape."""
    bundle = _axial_disc(64, 6 * mm)
    scene = bmo.CompiledScene(bmo.System([_window()]), bundle.lambdas)
    con, on = _on_off_oracle(oracle, emus, scene, bundle, 20, "window")
    assert con["leaf_loop_back"] > 0 and con["leaf_loop"] > con["leaf_loop_back"]
    assert on.n_records == 3 * 64  # to the window, through it, on to infinity


def test_unculled_miss_runs_into_the_iteration_limit(oracle, emus):
    """No bounding spheres (cull=False): a ray that passes 3 mm over the window's face, parallel to it, is neither culled nor found receding
    and marches until march_iters ends it: one evaluation for the start classification, march_iters of the march.  The loop commits
    every trip of the march but the last (whose iteration count ends it) for as long as the distance is finite: behind the window it
    roughly doubles per trip, so from 3 mm its square overflows after some 520 trips and the generic trip makes the rest."""
    n = 16
    pos = np.stack([np.full(n, -20 * mm), np.full(n, 5 * mm), (np.arange(n) - 7.5) * 0.3 * mm], axis=1)
    bundle = _rays(pos, np.tile([1.0, 0.0, 0.0], (n, 1)))
    for iters in (1000, 37):
        scene = bmo.CompiledScene(bmo.System([_window()]), bundle.lambdas, cull=False, consts=dict(march_iters=iters))
        con, on = _on_off_oracle(oracle, emus, scene, bundle, 20, "unculled miss, %d iterations" % iters)
        assert on.n_records == n  # nobody hits
        assert con["sdf_any"] == n * (iters + 1), (iters, con["sdf_any"])
        if iters == 37:
            assert con["leaf_loop"] == n * (iters - 1), con["leaf_loop"]
        else:
            assert n * 500 <= con["leaf_loop"] < n * (iters - 1), con["leaf_loop"]


def _lim_scene():
    """A small window and, behind it, a wide one tilted by 70 degrees: the march to the wide one starts in front of both and gains only
    cos(70 deg) = 0.34 of the remaining way per trip, so its running t passes the first hit's (`lim`) on its third or fourth trip."""
    near, far = _window(10 * mm), _window(60 * mm)
    bmo.xrotate3d(far, math.radians(70))
    bmo.translate3d(far, [0, 12 * mm, 0])
    return bmo.System([near, far])


def test_second_plain_shape_is_pruned_by_lim(oracle, emus):
    bundle = _axial_disc(64, 2 * mm)
    scene = bmo.CompiledScene(_lim_scene(), bundle.lambdas)
    con, on = _on_off_oracle(oracle, emus, scene, bundle, 20, "lim prune")
    assert con["leaf_loop"] > 0
    assert on.n_records == 5 * 64
    # the same two with the first-order flag: no prune, every march to the second shape runs on to its hit (exact = false in the loop too)
    scene_i = bmo.CompiledScene(_lim_scene(), bundle.lambdas)
    for i in range(scene_i.desc.n_shapes):
        scene_i._shapes[i].flags |= FLAG_INEXACT
    con_i, on_i = _on_off_oracle(oracle, emus, scene_i, bundle, 20, "inexact plain shapes")
    compare(on_i, on, 0.0, "inexact against exact")
    assert con_i["sdf_any"] > con["sdf_any"] and con_i["leaf_loop"] > con["leaf_loop"], (con_i["sdf_any"], con["sdf_any"], con_i["leaf_loop"], con["leaf_loop"])


def test_receding_exit(oracle, emus):
    """Rays that pass a squat cylinder inside its bounding sphere, 0.3 - 1.5 mm beside its barrel: once behind it and outside the sphere
    the distance grows and the march ends as receding."""
    n = 32
    stub = bmo.Lens(bmo.CylinderSDF(5 * mm, 5 * mm), lambda lam: 1.5)
    k = np.arange(n)
    phi = k * (2 * math.pi / n)
    r = (5.3 + 1.2 * (k % 5) / 4.0) * mm
    pos = np.stack([r * np.cos(phi), np.full(n, -20 * mm), r * np.sin(phi)], axis=1)
    bundle = _rays(pos, np.tile([0.0, 1.0, 0.0], (n, 1)))
    scene = bmo.CompiledScene(bmo.System([stub]), bundle.lambdas)
    con, on = _on_off_oracle(oracle, emus, scene, bundle, 20, "receding")
    assert on.n_records == n and con["leaf_loop"] > 0
    assert con["sdf_any"] < n * 100  # (none of them ran to the iteration limit)


def _side_by_side():
    """Three plain shapes of three kinds next to each other along x; ray i goes through shape i % 3, so inside them neighbouring lanes
    carry different hinted shapes (trace_one's slot -1: the waterfall over `usid` makes three passes per wave)."""
    a = _window(5 * mm, 2 * mm)
    b = bmo.Lens(bmo.CylinderSDF(2.5 * mm, 1.5 * mm), lambda lam: 1.6)
    c = bmo.Lens(bmo.BoxSDF(5 * mm, 2.5 * mm, 5 * mm), lambda lam: 1.7)
    bmo.translate3d(a, [-6 * mm, 0, 0])
    bmo.translate3d(c, [6 * mm, 0.5 * mm, 0])
    return bmo.System([a, b, c])


def _side_by_side_rays(n):
    b = _axial_disc(n, 3 * mm, jitter=5e-3)
    P = b.planes.copy()
    P[0] += ((np.arange(n) % 3) - 1) * 6 * mm
    return bmo.RayBundle.rays(P[0:3].T.copy(), P[3:6].T.copy(), 1.064e-6)


def test_hinted_shapes_differ_between_neighbouring_lanes(oracle, emus):
    bundle = _side_by_side_rays(96)
    scene = bmo.CompiledScene(_side_by_side(), bundle.lambdas)
    con, on = _on_off_oracle(oracle, emus, scene, bundle, 20, "side by side")
    assert con["leaf_loop_back"] > 0
    assert on.n_records == 3 * 96
    hit = on.rec_shape[on.node_first_rec[:96]]
    assert np.array_equal(hit, np.arange(96) % 3), "ray i must hit shape i % 3"


# ---------------------------------------------------------------------------------------------------------------- GPU
def _engine_equals(oracle, scene, bundle, r_max, label, wide=(None,), monkeypatch=None):
    ref = oracle.trace(scene, bundle, r_max, threads=16)
    eng = bmo.Engine(scene, 0)
    try:
        dev = eng.upload(bundle)
        try:
            for wide_min in wide:
                if wide_min is not None:
                    monkeypatch.setenv("BMO_WIDE_MIN_WAVES", wide_min)
                res = eng.trace_device(dev, r_max)
                try:
                    compare(eng.result_view(res), ref, 0.0, "%s, BMO_WIDE_MIN_WAVES=%s" % (label, wide_min))
                finally:
                    eng.free_result(res)
        finally:
            eng.free_batch(dev)
    finally:
        eng.close()
    return ref


@pytest.mark.gpu
def test_gpu_grazing_exit(oracle):
    """256 rays on the rod: a wave in which every lane grazes, then waves in which one lane of 64 does and the others wait for it."""
    system = _rod_scene()
    for label, graze in (("all graze", np.ones(256, dtype=bool)), ("one of 64 grazes", _one_in_64(256))):
        bundle = _grazing_rays(256, graze)
        scene = bmo.CompiledScene(system, bundle.lambdas)
        ref = _engine_equals(oracle, scene, bundle, 20, "rod, " + label)
        assert ref.n_records == 3 * 256


@pytest.mark.gpu
def test_gpu_hinted_shapes_differ_between_neighbouring_lanes(oracle):
    bundle = _side_by_side_rays(256)
    scene = bmo.CompiledScene(_side_by_side(), bundle.lambdas)
    ref = _engine_equals(oracle, scene, bundle, 20, "side by side")
    assert ref.n_records == 3 * 256


def _ragged_case(n):
    """config 2's scene under the ragged bundle (as in test_scheduling.py)"""
    system, _ = scenes.c2_scene()
    b = scenes.c2_vignetted_bundle(n)
    return bmo.CompiledScene(system, b.lambdas), b


def _disc_case(n):
    """config 2's scene under SURVEY 8(d)'s collimated disc (as in test_scheduling.py)"""
    system, _ = scenes.c2_scene()
    b = scenes.c2_survey_bundle(n)
    return bmo.CompiledScene(system, b.lambdas), b


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["ragged", "disc"])
def test_gpu_config_2_through_both_wave_builds(oracle, monkeypatch, case):
    """8 192 rays through the step kernels compiled for 4 waves per SIMD (BMO_WIDE_MIN_WAVES=0) and for 3 (10^9)."""
    scene, b = (_ragged_case if case == "ragged" else _disc_case)(8192)
    _engine_equals(oracle, scene, b, 100, case, wide=("0", "1000000000"), monkeypatch=monkeypatch)


def _kind_bundle(kind, n):
    geo = dict(center=[0, 0, -0.77 * mm], direction=[0, 0, 1], diameter=0.8 * 2.288 * mm)
    if kind == "ray":
        return scenes.c2_survey_bundle(n)
    if kind == "pol":
        return scenes.polarized_bundle(n, e1=[1, 0, 0], **geo)
    return scenes.gaussian_bundle(n, w0=50e-6, support=(1.0, 0.0, 0.0), **geo)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ray", "pol", "gauss"])
def test_gpu_config_2_for_each_beam_kind(oracle, monkeypatch, kind):
    """The Ray, PolarizedRay and GaussianBeamlet kernels share tracing_step: 1 024 beams of each on config 2's scene, both wave builds."""
    system, _ = scenes.c2_scene()
    b = _kind_bundle(kind, 1024)
    scene = bmo.CompiledScene(system, b.lambdas)
    _engine_equals(oracle, scene, b, 100, "config 2, " + kind, wide=("0", "1000000000"), monkeypatch=monkeypatch)

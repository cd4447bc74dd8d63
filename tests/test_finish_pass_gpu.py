"""The finish pass of a solve (csrc/bmo_trace_host.inc.hpp `count_and_gather_hits`): behind the last launch the segment count and the
detector tables come from counts per tile of 256 canonical nodes, one scan over detectors x tiles of them and a gather that ranks a
tile's hits in LDS.  Every case here asks for the oracle's solution: node tables in canonical order, segments, detector rows, `det_node`,
`det_offset`, `det_count`, `n_records`, the call count (parity.compare at zero tolerance).  The cases are the smallest that reach each
way the counts can go wrong: the edges of the 256-node tiling, trees with children behind each of the three orderings (the engine's
`node order:` debug line says which one ran), three rows per hit, tiles and detectors without hits, a PSFDetector, solves without the
log, a retrace, a sweep, and two solves of one batch in a row (the second sorts its tiles by the first one's times)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bmo_amd as bmo
import scenes
from parity import compare
from scenes import mm
from test_psf_readout import airy_setup
from test_retrace import RETRACE_CASES, retrace_pair
from test_splitter_chain import _bundle as chain_bundle, _chain
from test_sweep_gpu import _perturbed_snapshots, _sweep_vs_separate

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAIN_R_MAX = 50
TILE = 256  # canonical nodes per workgroup of hit_count_kernel / hit_gather_kernel


def _trace(scene, bundle, r_max=100):
    eng = bmo.Engine(scene, 0)
    try:
        return eng.trace(bundle, r_max)
    finally:
        eng.close()


def _lens_and_detector():
    """one lens, one Spotdetector behind it: no splitter, every beam is a root"""
    lens = bmo.SphericalLens(120 * mm, -120 * mm, 4 * mm, 25.4 * mm, 1.5)
    bmo.translate3d(lens, [0, 10 * mm, 0])
    det = bmo.Spotdetector(40 * mm)
    bmo.translate3d(det, [0, 40 * mm, 0])
    return bmo.System([lens, det])


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_tile_edges_roots_only(oracle, n):
    """Roots only, at the edges of the 256-node tiling: config 4's three singlets (no detector: the segment count alone, summed per tile)
    and a lens in front of a Spotdetector (every node has a hit: a tile's count, its first row, the rank within the tile)."""
    bundle = scenes.c4_bundle(n)
    scene = bmo.CompiledScene(scenes.c4_scene()[0], bundle.lambdas)
    got = _trace(scene, bundle)
    assert got.n_nodes == n and got.n_detectors == 0
    compare(got, oracle.trace(scene, bundle, 100, threads=4), 0.0, "c4, %d rays, oracle" % n)
    bundle = chain_bundle("ray", n)
    scene = bmo.CompiledScene(_lens_and_detector(), bundle.lambdas)
    got = _trace(scene, bundle)
    assert got.n_nodes == n and got.det_count.tolist() == [n] and np.array_equal(got.det_node, np.arange(n))
    compare(got, oracle.trace(scene, bundle, 100, threads=4), 0.0, "lens + detector, %d rays, oracle" % n)


def test_two_detectors_hits_on_children(oracle):
    """Config 2 under the survey bundle, 2 048 rays = 32 waves: the splitter's children carry the hits, both detectors have rows, the heap ordering."""
    bundle = scenes.c2_survey_bundle(2048)
    scene = bmo.CompiledScene(scenes.c2_scene()[0], bundle.lambdas)
    got = _trace(scene, bundle)
    assert got.n_nodes > bundle.n and (got.det_count > 0).all() and got.det_node.max() >= bundle.n
    compare(got, oracle.trace(scene, bundle, 100, threads=16), 0.0, "c2 survey bundle, oracle")


@pytest.mark.parametrize("kind,nsub", [("ray", 1), ("gauss", 3)])
def test_splitter_chain_heap_ordering(oracle, kind, nsub):
    """Four splitters in a row under 96 beams: trees four levels deep; GaussianBeamlets have three rows per hit (nsub = 3)."""
    bundle = chain_bundle(kind, 96)
    scene = bmo.CompiledScene(_chain(4), bundle.lambdas)
    got = _trace(scene, bundle, CHAIN_R_MAX)
    assert got.n_nodes >= 9 * bundle.n and got.det_count.sum() % nsub == 0 and got.det_count.sum() >= nsub * bundle.n
    compare(got, oracle.trace(scene, bundle, CHAIN_R_MAX, threads=8), 0.0, "splitter chain, %s, oracle" % kind)


def _child(mode, **env):
    """This file as a child process (BMO_DEBUG and the ordering hooks are read by the engine as the child sets them); the child compares itself."""
    path = os.pathsep.join([ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")] + ([os.environ["PYTHONPATH"]] if os.environ.get("PYTHONPATH") else []))
    base = {k: v for k, v in os.environ.items() if k not in ("BMO_LPT", "BMO_FORCE_SORT_ORDER", "BMO_FORCE_DEEP_ORDER")}
    env = dict(base, BMO_DEBUG="1", PYTHONPATH=path, **env)
    r = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), mode], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stderr


def _node_orders(err):
    return [line.split("node order: ")[1] for line in err.splitlines() if "node order: " in line]


@pytest.mark.parametrize("hook", ["BMO_FORCE_SORT_ORDER", "BMO_FORCE_DEEP_ORDER"])
def test_splitter_chain_behind_the_other_orderings(hook):
    """The same chain with the canonical order made by the packed-key sort and level by level (the child compares itself with the
    oracle); the debug line says that the hook took effect."""
    path = {"BMO_FORCE_SORT_ORDER": "packed keys", "BMO_FORCE_DEEP_ORDER": "level by level"}[hook]
    assert _node_orders(_child("chain", **{hook: "1"})) == [path]


def test_splitter_chain_heap_index_without_a_hook():
    """A fresh process with neither hook set orders the chain's four-level trees by heap index."""
    assert _node_orders(_child("chain")) == ["heap index"]


def _two_detector_scene():
    """a Spotdetector off to the side that nothing reaches (detector 0), a lens, a Spotdetector on the axis (detector 1)"""
    aside = bmo.Spotdetector(10 * mm)
    bmo.translate3d(aside, [200 * mm, 40 * mm, 0])
    lens = bmo.SphericalLens(120 * mm, -120 * mm, 4 * mm, 25.4 * mm, 1.5)
    bmo.translate3d(lens, [0, 10 * mm, 0])
    det = bmo.Spotdetector(40 * mm)
    bmo.translate3d(det, [0, 40 * mm, 0])
    return bmo.System([aside, lens, det])


def test_no_hits_at_all(oracle):
    """Every ray leaves config 2's scene backwards: all counts 0, all offsets equal."""
    bundle = scenes.disc_bundle(600, center=[0, 0, -0.77 * mm], direction=[0, 0, -1], diameter=1 * mm, e1=[1, 0, 0])
    scene = bmo.CompiledScene(scenes.c2_scene()[0], bundle.lambdas)
    got = _trace(scene, bundle)
    assert got.n_nodes == 600 and got.det_count.tolist() == [0, 0] and got.det_offset.tolist() == [0, 0] and got.det_node.size == 0
    compare(got, oracle.trace(scene, bundle, 100, threads=4), 0.0, "no hits, oracle")


def test_all_hits_on_the_second_detector(oracle):
    bundle = chain_bundle("ray", 600)
    scene = bmo.CompiledScene(_two_detector_scene(), bundle.lambdas)
    got = _trace(scene, bundle)
    assert got.det_count.tolist() == [0, 600] and got.det_offset.tolist() == [0, 0]
    compare(got, oracle.trace(scene, bundle, 100, threads=4), 0.0, "second detector only, oracle")


def test_tiles_without_hits_between_tiles_with_one(oracle):
    """Only every 300th root looks at the detector, the others away from it: tiles with one hit, tiles with none between them and at the end."""
    n = 2100
    b = chain_bundle("ray", n)
    planes = b.planes.copy()
    away = np.arange(n) % 300 != 0
    planes[3:6, away] *= -1.0
    bundle = bmo.RayBundle(b.kind, planes)
    scene = bmo.CompiledScene(_two_detector_scene(), bundle.lambdas)
    got = _trace(scene, bundle)
    want = np.arange(0, n, 300)
    assert got.det_count.tolist() == [0, want.size] and np.array_equal(got.det_node, want)
    tiles = set((want // TILE).tolist())
    assert any(t not in tiles and t - 1 in tiles and t + 1 in tiles for t in range(n // TILE)) and (n - 1) // TILE not in tiles
    compare(got, oracle.trace(scene, bundle, 100, threads=4), 0.0, "every 300th, oracle")


def test_psf_detector_rows(oracle):
    """The Airy scene of the read-out tests under 512 rays: a PSFDetector keeps all nine columns of a row."""
    system, _, _, lam, D = airy_setup(num_rays=8)
    bundle = scenes.disc_bundle(512, center=[0, -10e-3, 0], direction=[0, 1, 0], diameter=D, lam=lam, e1=[1, 0, 0], jitter=0.0)
    scene = bmo.CompiledScene(system, bundle.lambdas)
    got = _trace(scene, bundle)
    assert got.det_count.tolist() == [512] and np.isfinite(got.det_data).all() and (np.abs(got.det_data) > 0).any(axis=0).sum() >= 8
    compare(got, oracle.trace(scene, bundle, 100, threads=4), 0.0, "airy scene, oracle")


def test_without_the_segment_log(oracle):
    """record_segments = 0: nodes, counts and detector rows as with the log; the segment count is still that of the beams."""
    bundle = scenes.c2_survey_bundle(2048)
    scene = bmo.CompiledScene(scenes.c2_scene()[0], bundle.lambdas)
    sizes = []

    def solve():
        eng = bmo.Engine(scene, 0)
        try:
            dev = eng.upload(bundle)
            res = eng.trace_device(dev, 100, record_segments=False)
            sizes.append(eng.result_size(res))
            view = eng.result_view(res)
            eng.free_result(res)
            eng.free_batch(dev)
            return view
        finally:
            eng.close()

    got = solve()
    ref = oracle.trace(scene, bundle, 100, threads=16)
    assert sizes[0] == (ref.n_intersect_calls, ref.n_records, ref.n_nodes, int(ref.det_count.sum()))
    for name in ("node_root", "node_parent", "node_first_child", "node_nseg", "node_status", "det_count", "det_offset", "det_node"):
        assert np.array_equal(getattr(got, name), getattr(ref, name)), name
    assert np.array_equal(got.det_data.view(np.int64), ref.det_data.view(np.int64))


def test_retrace(oracle):
    """A retrace after the splitter was tilted (192 rays): first solve and retrace."""
    case = RETRACE_CASES[0]
    scene0, scene1, bundle = retrace_pair("ray", case, 192)
    first = []

    def solve():
        g0, h0 = bmo.system._engine_solve(scene0, bundle, 20, None)
        try:
            first.append(g0)
            g1, h1 = bmo.system._engine_solve(scene1, bundle, 20, h0)
            h1.free()
            return g1
        finally:
            h0.free()

    got = solve()
    a0, sol = oracle.trace(scene0, bundle, 20, threads=8, keep=True)
    compare(first[0], a0, 0.0, case + ", first solve, oracle")
    compare(got, oracle.trace(scene1, bundle, 20, threads=8, prev=sol), 0.0, case + ", retrace, oracle")


def test_sweep(oracle):
    """4 configurations x 64 rays in one sweep: each configuration's slice against its separate solve and against the oracle."""
    system, _ = scenes.c2_scene()
    bundle = scenes.c2_bundle(64)
    snaps = _perturbed_snapshots(system, bundle.lambdas, 4, 11)
    got = _sweep_vs_separate(snaps, [bundle] * 4, 100, label="c2 sweep", oracle=oracle, oracle_every=1)
    assert got.n_roots == 4 * 64 and got.det_count.sum() > 0


def test_two_solves_of_one_batch():
    """4 096 rays = 64 tiles of the step kernel through config 2, two solves of the resident batch: the first equals the oracle's solution
    and the second equals the first (the child compares), the first has no tile costs, the second sorts its tiles by the first one's."""
    err = _child("twice")
    order = [line.split("tile order: ")[1] for line in err.splitlines() if "tile order: " in line]
    assert len(order) == 2 and order[0].startswith("as laid out") and order[1].startswith("by the cost"), order


if __name__ == "__main__":  # the child processes of _child
    if sys.argv[1:] == ["chain"]:
        import pyoracle

        b = chain_bundle("ray", 96)
        s = bmo.CompiledScene(_chain(4), b.lambdas)
        compare(_trace(s, b, CHAIN_R_MAX), pyoracle.trace(s, b, CHAIN_R_MAX, threads=8), 0.0, "splitter chain, oracle")
    elif sys.argv[1:] == ["twice"]:
        import pyoracle

        b = scenes.c2_survey_bundle(4096)
        s = bmo.CompiledScene(scenes.c2_scene()[0], b.lambdas)
        eng = bmo.Engine(s, 0)
        dev = eng.upload(b)
        views = []

        for _ in range(2):
            res = eng.trace_device(dev, 100)
            views.append(eng.result_view(res))
            eng.free_result(res)
        compare(views[0], pyoracle.trace(s, b, 100, threads=16), 0.0, "two solves of one batch, first against the oracle")
        for v in views[1:]:
            compare(views[0], v, 0.0, "two solves of one batch, first against a later one")
        eng.free_batch(dev)
        eng.close()
    else:
        raise SystemExit("unknown mode %r" % sys.argv[1:])

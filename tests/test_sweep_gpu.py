"""Sweeps on the GPU: every configuration's slice of one bmo_trace_sweep equals, bit for bit, a separate bmo_trace of that configuration."""
import math

import numpy as np
import pytest

import bmo_amd as bmo
from bmo_amd.system import _engine_solve
from parity import compare
from test_fuzz import cavity_case, random_bundle, random_system
from test_photodetector import michelson
from test_splitter_chain import _bundle as chain_bundle, _chain
from tests import mesh_scenes as ms

pytestmark = pytest.mark.gpu
mm = 1e-3


class _Slice:
    """Configuration c's part of a sweep TraceResult, renumbered as a solve of that configuration alone (detector rows included)."""

    def __init__(self, res, c, n0, n1, root0, n_roots):
        sl = bmo.system._ResultSlice(res, n0, n1, bmo.system._first_rec(res, n0), bmo.system._first_rec(res, n1), root0)
        self.__dict__.update(sl.__dict__)
        self.n_roots = n_roots
        counts, offsets, nodes, data = [], [], [], []
        for slot in range(res.n_detectors):
            dn = res.detector_nodes(slot)
            keep = (dn >= n0) & (dn < n1)
            offsets.append(sum(counts))
            counts.append(int(keep.sum()))
            nodes.append(dn[keep] - n0)
            data.append(res.detector_hits(slot)[keep])
        self.det_count, self.det_offset = np.array(counts, dtype=np.int64), np.array(offsets, dtype=np.int64)
        self.det_node = np.concatenate(nodes).astype(np.int32) if nodes else np.zeros(0, np.int32)
        self.det_data = np.concatenate(data) if data else np.zeros((0, 9))
        self.n_intersect_calls = None


def _sweep_vs_separate(scenes, bundles, r_max=100, record_segments=True, label="", oracle=None, oracle_every=0):
    """One bmo_trace_sweep over (scenes[c], bundles[c]) against a separate bmo_trace per configuration, at rtol = 0."""
    kind = next(b.kind for b in bundles if b is not None and b.n)
    planes = np.concatenate([b.planes for b in bundles if b.n], axis=1)
    cfg = np.concatenate([np.full(b.n, c, dtype=np.int32) for c, b in enumerate(bundles)])
    res, h, lib = bmo.sweep_trace(scenes, bmo.RayBundle(kind, planes), cfg, r_max, 0, record_segments)
    try:
        starts = np.concatenate([[0], np.cumsum([b.n for b in bundles])])
        node_start = np.searchsorted(res.node_root, starts)
        calls = 0
        for c, (scene, bundle) in enumerate(zip(scenes, bundles)):
            sl = _Slice(res, c, int(node_start[c]), int(node_start[c + 1]), int(starts[c]), bundle.n)
            if bundle.n == 0:
                assert sl.n_nodes == 0
                continue
            eng = bmo.Engine(scene, 0)
            try:
                if record_segments:
                    one = eng.trace(bundle, r_max)
                else:
                    b = eng.upload(bundle)
                    hr = eng.trace_device(b, r_max, record_segments=False)
                    one = eng.result_view(hr)
                    eng.free_result(hr)
                    eng.free_batch(b)
            finally:
                eng.close()
            calls += one.n_intersect_calls
            sl.n_intersect_calls = one.n_intersect_calls
            compare(sl, one, 0.0, "%s config %d" % (label, c))
            if oracle is not None and oracle_every and c % oracle_every == 0:
                ref = oracle.trace(scene, bundle, r_max, threads=16)
                sl.n_intersect_calls = ref.n_intersect_calls
                compare(sl, ref, 0.0, "%s config %d vs oracle" % (label, c))
        assert res.n_intersect_calls == calls, (label, res.n_intersect_calls, calls)
    finally:
        lib.bmo_result_free(h)
    return res


def _perturbed_snapshots(system, lambdas, k, seed, scale=1.0):
    rng = np.random.Generator(np.random.PCG64(seed))
    objs = list(system.objects())

    def configure(c):
        for o in objs:
            bmo.translate3d(o, list(rng.uniform(-0.3, 0.3, 3) * mm * scale))
            bmo.zrotate3d(o, math.radians(float(rng.uniform(-0.5, 0.5)) * scale))
            bmo.xrotate3d(o, math.radians(float(rng.uniform(-0.5, 0.5)) * scale))

    return bmo.sweep_snapshots(system, lambdas, k, configure)[0]


# ------------------------------------------------------------------------------------------------ the reference's Michelson KAT in one call
def test_michelson_kat_as_one_sweep():
    """runtests.jl:2092-2121 with 200 mirror positions in one solve_sweep: the KAT's tolerances, and every configuration's field equal, bit for
    bit, to a fresh single-configuration solve + bmo_photodetector_field."""
    n_steps = 200
    system, m1, m2, bs, pd, l_0, pd_size = michelson()
    lam, P_0 = 635e-9, 5e-3
    beam = bmo.GaussianBeamlet([0, -l_0, 0], [0, 1.0, 0], lam, 1e-4, P0=P_0)
    lambdas = bmo.linalg.linrange(-lam, lam, n_steps)

    def configure(c):
        bmo.translate_to3d(m2, np.array([0, l_0, 0]) + np.array([0, lambdas[c], 0]))

    sol = bmo.solve_sweep(system, beam, n_steps, configure)
    try:
        assert beam.children == [] and len(beam.chief.rays) == 1  # the beams are read, not solved
        fields = sol.photodetector_field(pd)
        pwr = sol.optical_power(pd, fields)
        path = np.array([sol.beams(c)[0].children[0].children[1].length() for c in range(n_steps)])
        path_ana = 2 * lambdas + 4 * l_0
        pwr_ana = P_0 * (0.5 * np.cos(2 * math.pi * (2 * lambdas / lam) + math.pi) + 0.5)
        assert np.all(np.abs(pwr_ana - pwr) <= 5e-6)
        assert np.allclose(path_ana, path, rtol=1.5e-8, atol=0)
        slot = sol._slot(pd)
        bundle = bmo.RayBundle.from_beams([beam])
        for c in range(n_steps):
            scene = sol.scenes[c]
            res, one = _engine_solve(scene, bundle, 100, None)
            try:
                f = np.zeros_like(pd.field)
                one.photodetector_field(slot, sol._poses[c][slot][0], sol._poses[c][slot][1], pd.x, pd.y, f)
            finally:
                one.free()
            same = (f.view(np.int64) == fields[c].view(np.int64)).all()
            assert same, (c, np.abs(f - fields[c]).max())
            # and the same optical power the single-configuration detector reports
            pd.field = f
            assert pd.optical_power() == pwr[c]
    finally:
        sol.close()


# ------------------------------------------------------------------------------------------------ random systems, all three beam kinds
@pytest.mark.parametrize("kind", ["ray", "pol", "gauss"])
@pytest.mark.parametrize("seed", [101, 202, 303])
def test_random_systems_sweep_equals_separate_solves(oracle, kind, seed):
    system, rng = random_system(seed, with_detectors=(kind != "gauss"))
    bundle = random_bundle(rng, kind, 300)
    k = 5 + seed % 5  # 5 - 9 configurations
    scenes = _perturbed_snapshots(system, bundle.lambdas, k, seed)
    _sweep_vs_separate(scenes, [bundle] * k, 30, label="fuzz %d %s" % (seed, kind), oracle=oracle if seed == 101 else None, oracle_every=3)


# ------------------------------------------------------------------------------------------------ regrouping across launches
@pytest.mark.parametrize("kind", ["ray", "gauss"])
def test_deep_trees_with_ragged_configurations(kind):
    """cavity_case trees (r_max 100, far more than 32 fused levels), a different mirror tilt per configuration (different numbers of surviving
    beams), 1 / 63 / 64 / 65 / 0 roots per configuration and one configuration whose roots all miss."""
    scene0, bundle = cavity_case(kind, 200)
    system = bmo.System(scene0.leaf_objects)
    b_mirror = scene0.leaf_objects[2]
    tilts = [0.0, 0.002, -0.004, 0.006, 0.0, 0.01]

    def configure(c):
        bmo.xrotate3d(b_mirror, math.radians(tilts[c]))

    scenes = bmo.sweep_snapshots(system, bundle.lambdas, len(tilts), configure)[0]
    counts = [1, 63, 64, 65, 0, 40]
    bundles = []
    off = 0
    for c, n in enumerate(counts):
        sub = bmo.RayBundle(bundle.kind, bundle.planes[:, off:off + n].copy())
        off += n
        if c == 5:  # every root of this configuration misses: turned round, away from the cavity
            sub.planes[3:6] *= -1
            if sub.planes.shape[0] >= 25:  # GaussianBeamlet: the waist and divergence rays too
                sub.planes[9:12] *= -1
                sub.planes[15:18] *= -1
        bundles.append(sub)
    res = _sweep_vs_separate(scenes, bundles, 100, label="cavity " + kind)
    assert res.n_steps > 1


@pytest.mark.parametrize("kind", ["ray", "pol", "gauss"])
def test_splitter_chain_sweep(kind):
    system = _chain(4)
    bundle = chain_bundle(kind, 130)
    scenes = _perturbed_snapshots(system, bundle.lambdas, 5, 77, scale=2.0)
    sizes = [130, 65, 1, 64, 63]
    _sweep_vs_separate(scenes, [bmo.RayBundle(bundle.kind, bundle.planes[:, :n].copy()) for n in sizes], 100, label="chain " + kind)


# ------------------------------------------------------------------------------------------------ meshes (BVH level)
@pytest.mark.parametrize("name", ["H", "M"])
@pytest.mark.parametrize("kind", ["ray", "gauss"])
def test_mesh_scenes_sweep(name, kind):
    if name == "H":
        system, parts = ms.housing_scene(3)
        mover = parts["housing"]
    else:
        system, parts = ms.mirror_scene(20, 60)
        mover = parts["mirror"]
    bundle = ms.bundle_of(kind, name, 256)

    def configure(c):
        bmo.translate3d(mover, [0.05 * mm * c, 0.1 * mm * c, 0])
        bmo.xrotate3d(mover, math.radians(0.2 * c))

    scenes = bmo.sweep_snapshots(system, bundle.lambdas, 3, configure)[0]
    assert any(v[0] > 0 for v in bmo.mesh_bvh_stats(scenes[0]).values())  # BVH level (EXT = 3)
    _sweep_vs_separate(scenes, [bundle] * 3, 100, label="mesh %s %s" % (name, kind))


@pytest.mark.parametrize("kind", ["ray", "gauss"])
def test_light_trap_sweep(oracle, kind):
    """The light trap of tests/mesh_scenes.py (four BVH meshes, rays in all directions) with the ball moved and turned differently in each
    configuration — each configuration has its own tree over the ball — under ragged slices of the permuted bundle; every configuration against the oracle too."""
    system, parts = ms.light_trap_scene()
    bundle = ms.light_trap_bundle(kind, 130)
    moves = [([0.0, 0.0, 0.0], 0.0), ([0.05 * mm, 0.1 * mm, 0.0], 0.3), ([-0.2 * mm, 0.0, 0.15 * mm], -7.0)]

    def configure(c):
        bmo.translate3d(parts["ball"], moves[c][0])
        bmo.zrotate3d(parts["ball"], math.radians(moves[c][1]))

    scenes = bmo.sweep_snapshots(system, bundle.lambdas, 3, configure)[0]
    assert sum(v[0] > 0 for v in bmo.mesh_bvh_stats(scenes[0]).values()) == 4
    ball = scenes[0].shape_id(parts["ball"].shape)
    assert len({bmo.mesh_bvh_stats(s)[ball] for s in scenes}) == 3  # three different trees over the ball
    sizes = [130, 65, 1]
    _sweep_vs_separate(scenes, [bmo.RayBundle(bundle.kind, bundle.planes[:, :n].copy()) for n in sizes], 20, label="light trap " + kind,
                       oracle=oracle, oracle_every=1)


# ------------------------------------------------------------------------------------------------ detector-only sweeps
def test_detector_only_sweep_spot_hits():
    system, rng = random_system(404, with_detectors=True)
    bundle = random_bundle(rng, "ray", 2000)
    scenes = _perturbed_snapshots(system, bundle.lambdas, 6, 404)
    _sweep_vs_separate(scenes, [bundle] * 6, 30, record_segments=False, label="detector only")


def test_solve_sweep_spot_hits_match_the_reference_loop():
    """solve_sweep's spot_hits(det, c) against the reference's loop of fresh solve_system calls (Spotdetector rows)."""
    system, rng = random_system(505, with_detectors=True)
    spots = [o for o in system.objects() if isinstance(o, bmo.Spotdetector)]
    lens = list(system.objects())[0]
    rays = [bmo.Beam(bmo.Ray([x * mm, -20 * mm, 0.3 * mm], [0, 1.0, 0], 1.064e-6)) for x in np.linspace(-2, 2, 9)]

    def configure(c):
        bmo.translate_to3d(lens, [0.1 * mm * c, lens.position()[1], lens.position()[2]])

    y0 = lens.position()[1]
    sol = bmo.solve_sweep(system, rays, 4, configure)
    try:
        for c in range(4):
            bmo.translate_to3d(lens, [0.1 * mm * c, y0, lens.position()[2]])
            for d in spots:
                d.data = np.zeros((0, 2))
            fresh = [bmo.Beam(bmo.Ray(b.rays[0].pos, b.rays[0].dir, 1.064e-6)) for b in rays]
            bmo.solve_system(system, fresh)
            bmo.release(fresh)
            for d in spots:
                assert np.array_equal(sol.spot_hits(d, c), d.data), c
            got = sol.beams(c)
            for a, b in zip(got, fresh):
                assert len(a.rays) == len(b.rays) and a.status == b.status
                assert all(np.array_equal(r.pos, q.pos) and np.array_equal(r.dir, q.dir) for r, q in zip(a.rays, b.rays))
    finally:
        sol.close()

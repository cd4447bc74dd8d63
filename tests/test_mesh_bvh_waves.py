"""Mesh BVH under incoherent waves (DESIGN.md §3 "mesh BVH"), CPU part: the inputs of tests/test_mesh_bvh_waves_gpu.py are what that file
needs them to be, so that it cannot pass vacuously — every wave of 64 rays mixes the seven ray families, all direction signs, hits and
misses; the light trap keeps its rays bouncing between all its meshes — and the two CPU references agree on them: the oracle's first
record against the library's host query (brute force, and through the BVH), the lane code's host build against the oracle on the trap."""
import functools

import numpy as np
import pytest

import bmo_amd as bmo

from tests import mesh_scenes as ms
from tests.parity import compare, emu_trace

N = ms.DIRECTED_N
R_MAX = 5
TRAP_N = 4097
TRAP_R_MAX = 20


def first_records(res):
    """(hit mask, t) of every root's first segment, in bundle order."""
    assert res.n_nodes == res.n_roots and np.array_equal(res.node_root, np.arange(res.n_roots))
    r = res.node_first_rec
    return res.rec_obj[r] >= 0, res.rec[7, r]


@functools.lru_cache(maxsize=None)
def _measured(name):
    import pyoracle

    v, f, bundle, fam = ms.directed_case(name)
    slow = ms.one_mesh_scene(v, f, mesh_bvh=False)
    fast = ms.one_mesh_scene(v, f)
    assert bmo.mesh_bvh_stats(fast)[0][0] > 0 and bmo.mesh_bvh_stats(slow)[0][0] == 0
    pos, dir = bundle.planes[0:3].T, bundle.planes[3:6].T
    t0, f0 = bmo.mesh_nearest_host(slow, 0, pos, dir)
    t1, f1 = bmo.mesh_nearest_host(fast, 0, pos, dir)
    hit, t = first_records(pyoracle.trace(fast, bundle, R_MAX, threads=16))
    return dict(t0=t0, f0=f0, t1=t1, f1=f1, hit=hit, t=t)


def _waves(x):
    """The full waves of a per-ray array: (n_waves, 64)."""
    w = len(x) // ms.WAVE
    return x[:w * ms.WAVE].reshape(w, ms.WAVE)


@pytest.mark.parametrize("name", list(ms.MESHES))
def test_every_wave_holds_all_families_and_direction_signs(name):
    _, _, bundle, fam = ms.directed_case(name)
    assert bundle.n == N and len(_waves(fam)) == N // 64
    assert np.array_equal(fam[:7 * (N // 7)], np.arange(7 * (N // 7)) % 7)  # ray i comes from family i mod 7
    for k in range(7):
        assert (_waves(fam) == k).any(axis=1).all(), k
    for axis in range(3):
        d = _waves(bundle.planes[3 + axis])
        assert ((d > 0).any(axis=1) & (d < 0).any(axis=1)).all(), axis


@pytest.mark.parametrize("name", list(ms.MESHES))
def test_waves_mix_hits_and_misses(name):
    hit = _measured(name)["f0"] >= 0
    mixed = (_waves(hit).any(axis=1) & (~_waves(hit)).any(axis=1)).mean()
    print(f"\n{name}: hit fraction {hit.mean():.3f} ({hit.sum()} hits), waves with a hit and a miss {mixed:.3f}")
    if name == "slivers":  # (most slivers are thinner than kϵ allows: |Det| < kϵ for every ray)
        assert mixed >= 0.1
        assert hit.sum() >= 20
    else:
        assert mixed >= 0.99
        assert 0.5 < hit.mean() < 1.0


@pytest.mark.parametrize("name", list(ms.MESHES))
def test_oracle_host_brute_force_and_host_bvh_agree(oracle, name):
    m = _measured(name)
    bits = lambda x: x.view(np.int64)  # noqa: E731
    assert np.array_equal(m["hit"], m["f0"] >= 0)
    bad = np.flatnonzero(m["hit"] & (bits(m["t"]) != bits(m["t0"])))
    assert bad.size == 0, (name, "oracle / host brute force", bad[:5], m["t"][bad[:5]], m["t0"][bad[:5]])
    bad = np.flatnonzero((bits(m["t1"]) != bits(m["t0"])) | (m["f1"] != m["f0"]))
    assert bad.size == 0, (name, "host BVH / host brute force", bad[:5], m["t1"][bad[:5]], m["t0"][bad[:5]], m["f1"][bad[:5]], m["f0"][bad[:5]])


def test_bad_lanes_take_every_lane_position():
    _, _, bundle, _ = ms.directed_case("sphere")
    b, bad = ms.bad_lane_bundle(bundle)
    idx = np.flatnonzero(bad)
    assert np.array_equal(idx, np.arange(0, N, 97)) and idx[64] == 6208
    assert set(idx % 64) == set(range(64)) and idx[0] % 64 == 0 and idx[64] % 64 == 0  # lane 0: the lane readfirstlane picks
    finite = np.isfinite(b.planes[0:6]).all(axis=0)
    assert np.array_equal(finite[~bad], np.ones(N - len(idx), dtype=bool))
    # five of the six rows are not finite; the sixth starts 1e30 away
    assert np.array_equal(finite[idx], (np.arange(len(idx)) % 6) == 5) and (b.planes[0, idx[5::6]] == 1e30).all()
    same = (b.planes[:, ~bad].view(np.int64) == bundle.planes[:, ~bad].view(np.int64)).all()
    assert same  # the good rays are the same doubles as without bad lanes


def test_light_trap_keeps_rays_between_all_its_meshes(oracle):
    system, parts = ms.light_trap_scene()
    bundle = ms.light_trap_bundle("ray", TRAP_N)
    scene = bmo.CompiledScene(system, bundle.lambdas)
    st = bmo.mesh_bvh_stats(scene)
    sid = {k: scene.shape_id(parts[k].shape) for k in ("ball", "flat63", "flat64", "shell", "shell2")}
    assert st[sid["flat63"]][0] == 0 and all(st[sid[k]][0] > 0 for k in ("ball", "flat64", "shell", "shell2")), st
    ref = oracle.trace(scene, bundle, TRAP_R_MAX, threads=16)
    counts = [int((ref.rec_obj == i).sum()) for i in range(5)]
    print(f"\nlight trap: records per object {counts}, segments per beam {ref.node_nseg.min()} .. {ref.node_nseg.max()}")
    assert [o for o in scene.leaf_objects] == parts["objects"]
    assert all(c >= 1000 for c in counts[:4]), counts
    assert counts[4] == 0, counts  # a coincident later copy loses every tie
    assert ref.node_nseg.min() >= 10
    head = bmo.RayBundle(bundle.kind, bundle.planes[:, :257].copy())
    compare(emu_trace(scene, head, TRAP_R_MAX), oracle.trace(scene, head, TRAP_R_MAX, threads=16), 0.0, "light trap, lane code on the host")

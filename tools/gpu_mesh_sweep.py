"""Random scenes with tessellated meshes (BVH kernels) against the oracle, bit for bit: python tools/gpu_mesh_sweep.py [--scenes 40] [--n 2048]

Each scene: one to three icosphere / spherical-cap meshes (80 - 7 080 faces; IntersectableObject, Mirror or a cap Mirror) at random
places and sizes, optionally with the config-2 lens train, and a Ray, PolarizedRay or GaussianBeamlet bundle aimed at them; fresh solve,
then a retrace after a random move of one mesh.  Prints one line per scene and the number of mismatches."""
import argparse
import math
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import bmo_amd as bmo  # noqa: E402
import pyoracle  # noqa: E402
from tests import mesh_scenes as ms  # noqa: E402
from tests import scenes  # noqa: E402
from tests.parity import compare  # noqa: E402

mm = 1e-3


def random_scene(rng):
    objs, meshes = [], []
    if rng.uniform() < 0.4:
        objs += list(bmo.System(scenes.miniscope_objects()).objects())  # (no beam splitter: with mirrors around it the beam tree can run away)
    for _ in range(rng.integers(1, 4)):
        if rng.uniform() < 0.5:
            v, f = ms.icosphere(int(rng.integers(1, 5)), rng.uniform(5, 40) * mm, rng.uniform(-20, 40, 3) * mm)
        else:
            v, f = ms.spherical_cap(rng.uniform(30, 200) * mm, rng.uniform(5, 25) * mm, int(rng.integers(4, 30)), int(rng.integers(8, 120)))
            v = v - [0, v[0][1], 0] + rng.uniform(-10, 60, 3) * mm
        m = bmo.Mesh(v, f)
        o = bmo.IntersectableObject(m) if rng.uniform() < 0.4 else bmo.Mirror(m)
        bmo.xrotate3d(o, rng.uniform(-0.5, 0.5))
        objs.append(o)
        meshes.append(o)
    return bmo.System(objs), meshes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=40)
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--seed", type=int, default=20251016)
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    bad = 0
    for i in range(a.scenes):
        system, meshes = random_scene(rng)
        kind = ["ray", "pol", "gauss"][i % 3]
        c, d = [0, 0, -0.77 * mm], rng.normal(size=3) * 0.3 + [0, 0.3, 1]
        d = d / np.linalg.norm(d)
        if kind == "ray":
            b = scenes.disc_bundle(a.n, center=c, direction=list(d), diameter=4 * mm, lam=1.064e-6, cone=0.5, seed=int(rng.integers(1 << 30)))
        elif kind == "pol":
            b = scenes.polarized_bundle(a.n, center=c, direction=list(d), diameter=4 * mm, seed=int(rng.integers(1 << 30)))
        else:
            b = scenes.gaussian_bundle(a.n, center=c, direction=list(d), diameter=4 * mm, w0=50e-6, cone=0.3, seed=int(rng.integers(1 << 30)))
        s0 = bmo.CompiledScene(system, b.lambdas)
        nb = sum(1 for st in bmo.mesh_bvh_stats(s0).values() if st[0] > 0)
        ok = True
        try:
            a0, sol = pyoracle.trace(s0, b, 20, threads=16, keep=True)
            g0, gs0 = bmo.system._engine_solve(s0, b, 20, None)
            compare(g0, a0, 0.0, "fresh")
            bmo.translate3d(meshes[int(rng.integers(len(meshes)))], list(rng.normal(size=3) * 0.5 * mm))
            s1 = bmo.CompiledScene(system, b.lambdas)
            a1 = pyoracle.trace(s1, b, 20, threads=16, prev=sol)
            g1, gs1 = bmo.system._engine_solve(s1, b, 20, gs0)
            compare(g1, a1, 0.0, "retrace")
            gs0.free()
            gs1.free()
            line = f"records {a0.n_records} / {a1.n_records}"
        except AssertionError as e:
            ok = False
            line = f"MISMATCH {str(e)[:200]}"
        bad += not ok
        print(f"scene {i:3d} {kind:5s} meshes {len(meshes)} (BVH {nb}) faces {s0.desc.n_tris:6d}: {line}", flush=True)
    print(f"{a.scenes} scenes, {bad} mismatches")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

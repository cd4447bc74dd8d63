"""Mesh BVH against brute force on the scenes H and M (tests/mesh_scenes.py): python tools/mesh_bench.py [--n 1048576] [--reps 5]

BVH and brute-force (mesh_bvh=False) solves alternate in one process after a warm-up of each; prints ms per solve (host wall time of
bmo_trace), kernel ms and scene build ms (bmo_scene_create), and checks that the two outputs are identical.  Then H with a 327 680-face
housing (BVH only: brute force would take seconds per solve) for the scaling of the BVH with the face count."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import bmo_amd as bmo  # noqa: E402
from bmo_amd import abi  # noqa: E402
from tests import mesh_scenes as ms  # noqa: E402
from tests.parity import compare  # noqa: E402

R_MAX = 20


def build_ms(scene, reps=3):
    lib = abi.load_engine()
    best = 1e30
    for _ in range(reps):
        h = C.c_void_p()
        t = time.perf_counter()
        abi.check(lib, lib.bmo_scene_create(C.byref(scene.desc), C.byref(h)), "bmo_scene_create")
        best = min(best, (time.perf_counter() - t) * 1e3)
        lib.bmo_scene_destroy(h)
    return best


def solve(eng, bundle):
    t = time.perf_counter()
    r = eng.trace(bundle, R_MAX)
    return r, (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-big", action="store_true")
    a = ap.parse_args()
    for name, make in (("H", ms.housing_scene), ("M", ms.mirror_scene)):
        system, _ = make()
        bundle = ms.bundle_of("ray", name, a.n)
        sc = {"bvh": bmo.CompiledScene(system, bundle.lambdas), "brute": bmo.CompiledScene(system, bundle.lambdas, mesh_bvh=False)}
        stats = {k: bmo.mesh_bvh_stats(s) for k, s in sc.items()}
        eng = {k: bmo.Engine(s, 0) for k, s in sc.items()}
        first = {k: solve(e, bundle)[0] for k, e in eng.items()}  # warm-up (and the outputs compared)
        compare(first["bvh"], first["brute"], 0.0, f"{name} BVH against brute force")
        wall = {k: [] for k in eng}
        kern = {k: [] for k in eng}
        for _ in range(a.reps):
            for k, e in eng.items():
                r, ms_ = solve(e, bundle)
                wall[k].append(ms_)
                kern[k].append(r.kernel_ms)
        print(f"{name}: {a.n} rays, outputs identical (records {first['bvh'].n_records}, intersect calls {first['bvh'].n_intersect_calls}); "
              f"BVH stats {[v for v in stats['bvh'].values() if v[0]]}")
        for k in eng:
            print(f"  {k:5s}  solve {np.median(wall[k]):9.2f} ms (min {min(wall[k]):9.2f})  kernel {np.median(kern[k]):9.2f} ms  "
                  f"build {build_ms(sc[k]):7.2f} ms")
        print(f"  speed-up: solve x{np.median(wall['brute']) / np.median(wall['bvh']):.1f}, kernel x{np.median(kern['brute']) / np.median(kern['bvh']):.1f}")
        for e in eng.values():
            e.close()
    if a.no_big:
        return
    res = {}
    for level in (5, 7):
        system, _ = ms.housing_scene(level)
        bundle = ms.bundle_of("ray", "H", a.n)
        s = bmo.CompiledScene(system, bundle.lambdas)
        e = bmo.Engine(s, 0)
        solve(e, bundle)
        ks = [solve(e, bundle)[0].kernel_ms for _ in range(a.reps)]
        res[level] = (20 * 4 ** level, float(np.median(ks)), build_ms(s, 1))
        e.close()
    for level, (nf, k, b) in res.items():
        print(f"H with a {nf}-face housing (BVH): kernel {k:.2f} ms, build {b:.1f} ms")
    print(f"327 680 faces against 20 480: kernel x{res[7][1] / res[5][1]:.2f}")


if __name__ == "__main__":
    main()

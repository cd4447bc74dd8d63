"""Sweeps against loops of single solves: python tools/sweep_bench.py [--ks 101,1024,8192] [--reps 3] [--json OUT]

1. The reference's Michelson scan (test/runtests.jl:2092-2121: move mirror 2, solve one GaussianBeamlet, read the Photodetector's power) with K
   positions: a loop of K fresh solve_system + optical_power calls against ONE solve_sweep + optical_power.  Wall times end to end (every
   engine call returns after its device work: the loop's per-step latency is what it measures), the host snapshot time of the sweep
   separately, and the trace and read-out kernel times the engine reports.
2. Config 2 (tests/scenes.py c2_scene) with 1 024 rays x 64 configurations (lens 1 moved by 10 um per configuration) against 64 separate
   Engine.trace calls.
Every sweep result is checked against the loop (powers and hit counts)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bmo_amd as bmo  # noqa: E402
from test_photodetector import michelson  # noqa: E402
from tests import scenes  # noqa: E402


def timing(lib, h):
    """bmo_result_timing: (step-kernel ms, total ms, launches)."""
    import ctypes as C
    ms, tot, nl = C.c_double(), C.c_double(), C.c_int32()
    lib.bmo_result_timing(h, C.byref(ms), C.byref(tot), C.byref(nl))
    return ms.value, tot.value, nl.value


def michelson_case(K, reps):
    system, m1, m2, bs, pd, l_0, pd_size = michelson()
    lam, P_0 = 635e-9, 5e-3
    beam = bmo.GaussianBeamlet([0, -l_0, 0], [0, 1.0, 0], lam, 1e-4, P0=P_0)
    steps = bmo.linalg.linrange(-lam, lam, K)

    def configure(c):
        bmo.translate_to3d(m2, np.array([0, l_0, 0]) + np.array([0, steps[c], 0]))

    out = dict(case="michelson", K=K)
    loop_t, sweep_t, snap_t, kern_t, read_t = [], [], [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        p_loop = np.zeros(K)
        for c in range(K):
            configure(c)
            pd.empty()
            b = bmo.GaussianBeamlet([0, -l_0, 0], [0, 1.0, 0], lam, 1e-4, P0=P_0)
            bmo.solve_system(system, b)
            p_loop[c] = pd.optical_power()
            bmo.release(b)
        loop_t.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        snaps = bmo.sweep_snapshots(system, [lam], K, configure)
        t1 = time.perf_counter()
        sol = bmo.solve_sweep(system, beam, K, configure)
        fields = sol.photodetector_field(pd)
        p_sweep = sol.optical_power(pd, fields)
        t2 = time.perf_counter()
        ms, tot, nl = timing(sol.lib, sol._handle)
        kern_t.append(ms)
        read_t.append(sol.readout_ms)
        sol.close()
        snap_t.append(t1 - t0)
        sweep_t.append(t2 - t1)
        del snaps
        assert np.array_equal(p_loop, p_sweep), np.abs(p_loop - p_sweep).max()
    out.update(loop_ms=1e3 * min(loop_t), sweep_ms=1e3 * min(sweep_t), snapshot_ms=1e3 * min(snap_t), sweep_trace_kernel_ms=min(kern_t),
               sweep_readout_kernel_ms=min(read_t), launches=nl)
    out["speedup"] = out["loop_ms"] / out["sweep_ms"]
    return out


def c2_case(n_rays, K, reps):
    system, parts = scenes.c2_scene()
    bundle = scenes.c2_bundle(n_rays)
    lens = list(system.objects())[0]
    y0 = np.array(lens.position(), dtype=np.float64)

    def configure(c):
        bmo.translate_to3d(lens, list(y0 + np.array([10e-6 * c, 0, 0])))

    snaps = bmo.sweep_snapshots(system, bundle.lambdas, K, configure)[0]
    tiled = bmo.RayBundle(bundle.kind, np.tile(bundle.planes, (1, K)))
    cfg = np.repeat(np.arange(K, dtype=np.int32), bundle.n)
    loop_t, sweep_t, kern_loop, kern_sweep = [], [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        ks, hits = 0.0, []
        for c in range(K):
            eng = bmo.Engine(snaps[c], 0)
            r = eng.trace(bundle, 100)
            ks += r.kernel_ms
            hits.append(int(r.det_count.sum()))
            eng.close()
        loop_t.append(time.perf_counter() - t0)
        kern_loop.append(ks)
        t0 = time.perf_counter()
        res, h, lib = bmo.sweep_trace(snaps, tiled, cfg, 100)
        sweep_t.append(time.perf_counter() - t0)
        ms, tot, nl = timing(lib, h)
        kern_sweep.append(ms)
        lib.bmo_result_free(h)
        assert int(res.det_count.sum()) == sum(hits)
    return dict(case="c2", rays=n_rays, K=K, loop_ms=1e3 * min(loop_t), sweep_ms=1e3 * min(sweep_t), loop_kernel_ms=min(kern_loop),
                sweep_kernel_ms=min(kern_sweep), speedup=min(loop_t) / min(sweep_t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="101,1024,8192")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--c2", type=int, default=64, help="configurations of the config-2 case (0: skip)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    rows = []
    for K in [int(k) for k in a.ks.split(",") if k]:
        r = michelson_case(K, a.reps if K < 8192 else 1)
        rows.append(r)
        print("michelson K=%5d  loop %9.1f ms  sweep %8.1f ms (x%.1f)  snapshots %7.1f ms  trace kernels %6.2f ms in %d launches  read-out %6.2f ms"
              % (K, r["loop_ms"], r["sweep_ms"], r["speedup"], r["snapshot_ms"], r["sweep_trace_kernel_ms"], r["launches"], r["sweep_readout_kernel_ms"]),
              flush=True)
    if a.c2:
        r = c2_case(1024, a.c2, a.reps)
        rows.append(r)
        print("c2 1024 rays x %d  loop %8.1f ms (kernels %.2f ms)  sweep %7.1f ms (kernels %.2f ms)  x%.1f"
              % (a.c2, r["loop_ms"], r["loop_kernel_ms"], r["sweep_ms"], r["sweep_kernel_ms"], r["speedup"]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

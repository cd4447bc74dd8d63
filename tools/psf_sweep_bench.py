"""PSF read-out of a sweep: the batched bmo_psf_intensity_sweep against loops of single bmo_psf_intensity calls.
python tools/psf_sweep_bench.py [--reps 5] [--json OUT]

Workloads: the Airy KAT scene (tests/test_psf_readout.py airy_setup) with the PSFDetector moved through focus, solved once as a sweep;
K = 64 and K = 1 024 configurations of 1 024 rays at n = 64, and K = 64 configurations of 65 536 rays at n = 100.  Three read-outs of
every configuration's PSF, alternating within one process:
  host loop   : per configuration, its rows from the host view, PSFDetector.sample_axes' window, bmo_psf_intensity on the host rows;
  device loop : the same with the rows' device pointer (bmo_result_device_hits + the configuration's first row), no upload;
  batched     : SweepSolution.psf_intensity (the same windows, then one bmo_psf_intensity_sweep).
Each loop gets its configurations' row ranges precomputed (slices of the host view), so the wall times compare read-outs only.  Wall
time is end to end per read-out of all K configurations (median of --reps rounds after one warm-up round); kernel time is the engine's
event time summed over the loop's calls, or that of the batched call.  All three must agree bit for bit.  "host windows alone" times the
K windows by themselves: host work that every variant contains."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bmo_amd as bmo  # noqa: E402
from bmo_amd import abi  # noqa: E402
from test_psf_readout import airy_setup  # noqa: E402


def case(K, rays, n, reps):
    system, cs, psfd, lam, D = airy_setup(num_rays=rays)
    p0 = np.array(psfd.position(), dtype=np.float64)
    dys = bmo.linalg.linrange(-1e-3, 1e-3, K)

    def configure(c):
        bmo.translate_to3d(psfd, list(p0 + np.array([0, dys[c], 0])))

    sol = bmo.solve_sweep(system, cs, K, configure)
    try:
        slot = sol._slot(psfd)
        poses = [sol._poses[c][slot] for c in range(K)]
        cfg = sol.res.node_root[sol.res.detector_nodes(slot)] // sol.n_roots
        start = np.searchsorted(cfg, np.arange(K + 1))
        rows = sol.res.detector_hits(slot)
        ptr, cnt = C.POINTER(C.c_double)(), C.c_int64()
        abi.check(sol.lib, sol.lib.bmo_result_device_hits(sol._handle, slot, C.byref(ptr), C.byref(cnt)), "bmo_result_device_hits")
        base = C.cast(ptr, C.c_void_p).value

        def loop(on_device):
            I, ks = np.zeros((K, n, n)), 0.0
            for c in range(K):
                r = rows[start[c]:start[c + 1]]
                pos, ori = poses[c]
                xs, zs = bmo.components.psf_sample_axes(r, pos, ori, n=n)
                if on_device:
                    I[c], _, ms = abi.psf_intensity(None, pos, ori[:, 0], ori[:, 2], xs, zs, hits_device_ptr=base + 72 * int(start[c]),
                                                    n_hits=len(r))
                else:
                    I[c], _, ms = abi.psf_intensity(r, pos, ori[:, 0], ori[:, 2], xs, zs)
                ks += ms
            return I, ks

        def batched():
            _, _, I = sol.psf_intensity(psfd, n=n)
            return I, sol.readout_ms

        def windows():  # the host part every variant contains: PSFDetector.sample_axes' window of each configuration
            for c in range(K):
                bmo.components.psf_sample_axes(rows[start[c]:start[c + 1]], poses[c][0], poses[c][1], n=n)
            return None, 0.0

        variants = (("host_loop", lambda: loop(False)), ("device_loop", lambda: loop(True)), ("batched", batched), ("windows", windows))
        wall = {k: [] for k, _ in variants}
        kern = {k: [] for k, _ in variants}
        ref = None
        for rep in range(reps + 1):  # the first round warms up (code objects, allocator) and is not counted
            for name, fn in variants:
                t0 = time.perf_counter()
                I, ks = fn()
                dt = time.perf_counter() - t0
                if ref is None:
                    ref = I
                assert I is None or np.array_equal(I, ref), name
                if rep:
                    wall[name].append(1e3 * dt)
                    kern[name].append(ks)
        out = dict(K=K, rays=rays, n=n, rows=int(len(rows)))
        for name, _ in variants:
            out[name + "_ms"] = float(np.median(wall[name]))
            out[name + "_kernel_ms"] = float(np.median(kern[name]))
        out["speedup_vs_host_loop"] = out["host_loop_ms"] / out["batched_ms"]
        out["speedup_vs_device_loop"] = out["device_loop_ms"] / out["batched_ms"]
        out["kernel_ratio_vs_loop"] = out["host_loop_kernel_ms"] / out["batched_kernel_ms"]
        return out
    finally:
        sol.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    rows = []
    for K, rays, n in ((64, 1024, 64), (1024, 1024, 64), (64, 1 << 16, 100)):
        r = case(K, rays, n, a.reps)
        rows.append(r)
        print("K=%5d rays=%6d n=%3d | wall ms: host loop %9.2f  device loop %9.2f  batched %8.2f  (x%.1f, x%.1f), host windows alone %7.2f "
              "| kernel ms: loop %8.3f  device loop %8.3f  batched %8.3f (x%.2f)"
              % (K, rays, n, r["host_loop_ms"], r["device_loop_ms"], r["batched_ms"], r["speedup_vs_host_loop"], r["speedup_vs_device_loop"],
                 r["windows_ms"], r["host_loop_kernel_ms"], r["device_loop_kernel_ms"], r["batched_kernel_ms"], r["kernel_ratio_vs_loop"]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

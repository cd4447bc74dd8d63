"""Zernike read-out: bmo_psf_zernike_sweep on resident rows against the copy path, a device-to-device copy and bmo_psf_stats.
python tools/psf_zernike_bench.py [--reps 5] [--skip-sweep] [--rays N] [--orders 2,4,6]

One process, the variants alternating within a round, medians of --reps rounds after one warm-up round, [min .. max] for kernel times.

Single results: the Airy KAT scene (tests/test_psf_readout.py airy_setup's lens and detector) on a disc bundle of 2^20 rays with the
segment log and of 2^22 rays detector-only (record_segments = 0); the PSFDetector is slot 0.  Per order 2, 4, 6:
  (a) copy   : bmo_result_copy_hits of the 72-byte rows into pinned host memory, then the fit in numpy (basis, normal equations, solve);
  (b) device : bmo_psf_zernike_sweep on the resident rows: wall time and the engine's kernel_ms (four passes and their reduces);
  (c) d2d    : a device-to-device copy of a buffer of exactly the size of the slot's rows through torch, timed with events;
  (d) stats  : bmo_psf_stats_sweep on the same rows (the same plumbing, three passes).
(a) and (b) must agree to the tolerance of a float64 numpy evaluation (printed, not asserted).

Sweep: K = 1 024 configurations x 1 024 rows: SweepSolution.psf_zernike against SweepSolution.psf_stats.
--rays N runs one detector-only workload of N rays only (for profiler runs)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bmo_amd as bmo  # noqa: E402
from bmo_amd import abi  # noqa: E402
import scenes  # noqa: E402
from test_psf_readout import airy_setup  # noqa: E402

mm = 1e-3


def med(v):
    return float(np.median(v))


def spread(v):
    return "%8.3f [%7.3f .. %7.3f]" % (med(v), min(v), max(v))


def numpy_fit(rows, origin, e1, e2, order):
    """The fit of include/bmo.h "Zernike read-out" in numpy (pairwise sums, LAPACK solve)."""
    d = rows[:, 0:3] - origin[None, :]
    x, z, w = d @ e1, d @ e2, rows[:, 7]
    s = w.sum()
    p = (origin + ((w * x).sum() / s) * e1) + ((w * z).sum() / s) * e2
    W = rows[:, 6] + ((p[None, :] - rows[:, 0:3]) * rows[:, 3:6]).sum(axis=1)
    u, v = rows[:, 3:6] @ e1, rows[:, 3:6] @ e2
    u0, v0 = (w * u).sum() / s, (w * v).sum() / s
    rho = np.sqrt(((u - u0) ** 2 + (v - v0) ** 2).max())
    Z = bmo.components.zernike_basis((u - u0) / rho, (v - v0) / rho, order)
    D = W - (w * W).sum() / s
    return np.linalg.solve((Z * w[None, :]) @ Z.T, (Z * w[None, :]) @ D)


def workload(name, n_rays, record, reps, orders):
    system, cs, psfd, lam, D = airy_setup(num_rays=1)
    bundle = scenes.disc_bundle(n_rays, center=[0, -10 * mm, 0], direction=[0, 1, 0], diameter=D, lam=lam)
    scene = bmo.CompiledScene(system, bundle.lambdas)
    eng = bmo.Engine(scene, 0)
    dev = eng.upload(bundle)
    res = eng.trace_device(dev, 100, record_segments=record)
    try:
        slot = 0
        ptr, n = eng.result_device_hits(res, slot)
        pos, ori = np.asarray(psfd.position(), dtype=np.float64), np.asarray(psfd.orientation(), dtype=np.float64)
        e1, e2 = ori[:, 0].copy(), ori[:, 2].copy()
        print("== %s: %d rays, %s, slot %d holds %d rows (%.1f MB resident)" % (name, n_rays, "segment log" if record else "detector-only", slot, n, n * 72 / 1e6),
              flush=True)
        pinned = torch.empty((n, 9), dtype=torch.float64, pin_memory=True)
        host = pinned.numpy()
        src = torch.empty(n * 72, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)

        def d2d():
            e0, e1_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(src)
            e1_.record()
            e1_.synchronize()
            return e0.elapsed_time(e1_)

        for order in orders:
            t_a, t_copy, t_b, k_b, t_c, k_d = [], [], [], [], [], []
            for rep in range(reps + 1):  # the first round warms up and is not counted
                t0 = time.perf_counter()
                eng.result_copy_hits(res, slot, host.ctypes.data, n)
                t1 = time.perf_counter()
                ref = numpy_fit(host, pos, e1, e2, order)
                t2 = time.perf_counter()
                coef, info, _, ms = abi.psf_zernike_sweep(res, slot, 1, pos, e1, e2, order=order)
                t3 = time.perf_counter()
                c = d2d()
                _, ms_d = abi.psf_stats_sweep(res, slot, 1, pos, e1, e2)
                if rep:
                    t_a.append(1e3 * (t2 - t0))
                    t_copy.append(1e3 * (t1 - t0))
                    t_b.append(1e3 * (t3 - t2))
                    k_b.append(ms)
                    t_c.append(c)
                    k_d.append(ms_d)
            coef, info = coef[0], info[0]
            big = np.abs(coef).max()
            print("order %d (J = %d): STATUS %d  RHO %.6g  FIT_RMS %.4e m  largest |c| %.4e m  largest difference to numpy %.1e of it"
                  % (order, len(coef), info[abi.ZERN_STATUS], info[abi.ZERN_RHO], info[abi.ZERN_FIT_RMS], big, np.abs(coef - ref).max() / big))
            print("   (a) copy + numpy fit       wall ms %9.2f  (copy alone %8.2f)" % (med(t_a), med(t_copy)))
            print("   (b) resident read-out      wall ms %9.2f   kernel ms %s (four passes)" % (med(t_b), spread(k_b)))
            print("   (c) d2d copy of rows       event ms %s   kernel / d2d = %.2f;  end to end (a) / (b) = %.1f"
                  % (spread(t_c), med(k_b) / med(t_c), med(t_a) / med(t_b)))
            print("   (d) psf_stats, same rows   kernel ms %s   zernike / stats = %.2f" % (spread(k_d), med(k_b) / med(k_d)), flush=True)
    finally:
        eng.free_result(res)
        eng.free_batch(dev)
        eng.close()


def sweep(K, rays, reps, orders):
    system, cs, psfd, lam, D = airy_setup(num_rays=rays)
    p0 = np.array(psfd.position(), dtype=np.float64)
    dys = bmo.linalg.linrange(-1e-3, 1e-3, K)
    sol = bmo.solve_sweep(system, cs, K, lambda c: bmo.translate_to3d(psfd, list(p0 + np.array([0, dys[c], 0]))))
    try:
        print("== sweep: K = %d configurations x %d rays" % (K, rays))
        for order in orders:
            wall, kern, kst = [], [], []
            for rep in range(reps + 1):
                t0 = time.perf_counter()
                coef, info = sol.psf_zernike(psfd, order=order)
                dt = time.perf_counter() - t0
                ms = sol.readout_ms
                sol.psf_stats(psfd)
                if rep:
                    wall.append(1e3 * dt)
                    kern.append(ms)
                    kst.append(sol.readout_ms)
            j = (2 * 4) // 2  # Z_2^0
            print("   order %d: wall ms %9.2f   kernel ms %s   psf_stats kernel ms %s   solved %d of %d, defocus %.3e .. %.3e m"
                  % (order, med(wall), spread(kern), spread(kst), int((info[:, abi.ZERN_STATUS] == 0).sum()), K, coef[:, j].min(), coef[:, j].max()), flush=True)
    finally:
        sol.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-sweep", action="store_true")
    ap.add_argument("--rays", type=int, default=0)
    ap.add_argument("--orders", default="2,4,6")
    a = ap.parse_args()
    orders = [int(o) for o in a.orders.split(",")]
    print("library: %s" % os.path.basename(abi.ENGINE_PATH))
    if a.rays:
        workload("airy %d" % a.rays, a.rays, False, a.reps, orders)
        return
    workload("airy 2^20", 1 << 20, True, a.reps, orders)
    workload("airy 2^22", 1 << 22, False, a.reps, orders)
    if not a.skip_sweep:
        sweep(1024, 1024, a.reps, orders)


if __name__ == "__main__":
    main()

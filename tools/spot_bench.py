"""Spotdetector read-out: the image and the statistics computed on the device from the resident rows, against the copy path.
python tools/spot_bench.py [--reps 5] [--skip-sweep] [--ab-only]

Workloads: the config-2 scene (tests/scenes.py) on c2_survey_bundle(2^20) with the segment log, and on 2^22 rays detector-only
(record_segments = 0); detector slot 0.  Images: 256 x 256 on the detector face ("uniform"), 128 x 128 on the face ("uniform128": the
largest image that is accumulated in LDS) and 16 x 16 on a window 1000 x the spot's geometric radius around its centroid ("focused":
nearly all hits in <= 4 bins).  Per workload three timed paths, alternating within one process after one warm-up round:
  (a) copy   : bmo_result_copy_hit_columns of 2 columns into pinned host memory, then the numpy rule (tests/spot_ref.py bin_rule), or
               numpy mean / central moments for the statistics;
  (b) device : bmo_spot_image_sweep / bmo_spot_stats_sweep on the resident rows: wall time and the engine's kernel_ms;
  (c) d2d    : a device-to-device copy of a buffer of exactly the size of the slot's rows (72 B per row) through torch, timed with
               events: the streaming yardstick for kernel_ms.
Every figure is the median of --reps rounds, with [min .. max] for the kernel times (the run-to-run spread an A/B must beat).
(a) and (b) must agree exactly (images) or to the derived tolerance of a float64 numpy evaluation (statistics: printed, not asserted).
Sweep: K = 1 024 configurations x 1 024 rays of a through-focus scan, one spot_stats call against the loop over spot_hits(det, c) + numpy.
--ab-only prints the image kernel times alone (for a library built with another SPOT_AGG_ITERS, chosen with BMO_ENGINE_LIB)."""
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
import spot_ref as sr  # noqa: E402

mm = 1e-3


def med(v):
    return float(np.median(v))


def spread(v):
    return "%8.3f [%7.3f .. %7.3f]" % (med(v), min(v), max(v))


def numpy_stats(rows):
    x, z = rows[:, 0], rows[:, 1]
    cx, cz = x.mean(), z.mean()
    dx, dz = x - cx, z - cz
    mxx, mzz, mxz = (dx * dx).mean(), (dz * dz).mean(), (dx * dz).mean()
    return np.array([len(x), cx, cz, x.min(), x.max(), z.min(), z.max(), mxx, mzz, mxz, np.sqrt(mxx + mzz), np.sqrt((dx * dx + dz * dz).max())])


def workload(name, n_rays, record, reps, ab_only):
    system, parts = scenes.c2_scene()
    bundle = scenes.c2_survey_bundle(n_rays)
    scene = bmo.CompiledScene(system, bundle.lambdas)
    eng = bmo.Engine(scene, 0)
    dev = eng.upload(bundle)
    res = eng.trace_device(dev, 100, record_segments=record)
    try:
        slot = 0
        ptr, n = eng.result_device_hits(res, slot)
        hw = scene.detectors[slot].hw
        print("== %s: %d rays, %s, slot %d holds %d rows (%.1f MB resident, 16 B of every 72 used)"
              % (name, n_rays, "segment log" if record else "detector-only", slot, n, n * 72 / 1e6), flush=True)
        pinned = torch.empty((n, 2), dtype=torch.float64, pin_memory=True)
        host = pinned.numpy()
        src = torch.empty(n * 72, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        st0 = abi.spot_stats_sweep(res, slot, 1)[0][0]
        r = 1000 * st0[sr.GEO_R]
        images = (("uniform", 256, 256, (-hw, hw, -hw, hw)), ("uniform128", 128, 128, (-hw, hw, -hw, hw)),
                  ("focused", 16, 16, (st0[sr.CX] - r, st0[sr.CX] + r, st0[sr.CZ] - r, st0[sr.CZ] + r)))

        def copy_rows():
            eng.result_copy_hit_columns(res, slot, 2, host.ctypes.data, n)
            return host

        def d2d():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(src)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)

        for label, nx, nz, window in images:
            t_a, t_copy, t_b, k_b, t_c = [], [], [], [], []
            for rep in range(reps + 1):  # the first round warms up and is not counted
                if not ab_only:
                    t0 = time.perf_counter()
                    rows = copy_rows()
                    t1 = time.perf_counter()
                    want, want_out = sr.bin_rule(rows, window, nx, nz)
                    t2 = time.perf_counter()
                t3 = time.perf_counter()
                img, outside, ms = abi.spot_image_sweep(res, slot, 1, window, nx, nz)
                t4 = time.perf_counter()
                c = d2d()
                if not ab_only:
                    assert np.array_equal(img[0], want) and outside[0] == want_out, label
                if rep:
                    if not ab_only:
                        t_a.append(1e3 * (t2 - t0))
                        t_copy.append(1e3 * (t1 - t0))
                    t_b.append(1e3 * (t4 - t3))
                    k_b.append(ms)
                    t_c.append(c)
            top = np.sort(img[0].reshape(-1))[::-1]
            print("image %-10s %3d x %3d  top-4 bins hold %5.1f %% of %d inside" % (label, nx, nz, 100.0 * top[:4].sum() / max(1, top.sum()), top.sum()))
            if not ab_only:
                print("   (a) copy + numpy rule  wall ms %9.2f  (copy alone %8.2f)" % (med(t_a), med(t_copy)))
            print("   (b) resident read-out  wall ms %9.2f   kernel ms %s" % (med(t_b), spread(k_b)))
            print("   (c) d2d copy of rows   event ms %s   kernel / d2d = %.2f" % (spread(t_c), med(k_b) / med(t_c)), flush=True)
            if not ab_only:
                print("   end to end (a) / (b) = %.1f" % (med(t_a) / med(t_b)))
        if ab_only:
            return
        t_a, t_b, k_b, t_c = [], [], [], []
        for rep in range(reps + 1):
            t0 = time.perf_counter()
            ref = numpy_stats(copy_rows())
            t1 = time.perf_counter()
            st, ms = abi.spot_stats_sweep(res, slot, 1)
            t2 = time.perf_counter()
            c = d2d()
            if rep:
                t_a.append(1e3 * (t1 - t0))
                t_b.append(1e3 * (t2 - t1))
                k_b.append(ms)
                t_c.append(c)
        rel = np.abs(st[0] - ref) / np.maximum(np.abs(ref), 1e-300)
        print("statistics: N %d  RMS_R %.6e  GEO_R %.6e   max relative difference to numpy %.2e" % (st[0][sr.N], st[0][sr.RMS_R], st[0][sr.GEO_R], rel.max()))
        print("   (a) copy + numpy moments wall ms %9.2f" % med(t_a))
        print("   (b) resident read-out    wall ms %9.2f   kernel ms %s (two passes over the rows)" % (med(t_b), spread(k_b)))
        print("   (c) d2d copy of rows     event ms %s   kernel / d2d = %.2f;  end to end (a) / (b) = %.1f"
              % (spread(t_c), med(k_b) / med(t_c), med(t_a) / med(t_b)), flush=True)
    finally:
        eng.free_result(res)
        eng.free_batch(dev)
        eng.close()


def sweep(K, rays, reps):
    lens = bmo.SphericalLens(100 * mm, float("inf"), 1 * mm, 25.4 * mm, lambda lam_: 1.5)
    sd = bmo.Spotdetector(4 * mm)
    system = bmo.System([lens, sd])
    cs = bmo.UniformDiscSource([0, -10 * mm, 0], [0, 1, 0], 10 * mm, 1e-6, num_rays=rays)
    ys = bmo.linalg.linrange(185 * mm, 215 * mm, K)
    sol = bmo.solve_sweep(system, cs, K, lambda c: bmo.translate_to3d(sd, [0, ys[c], 0]))
    try:
        t_loop, t_dev, k_dev = [], [], []
        for rep in range(reps + 1):
            t0 = time.perf_counter()
            ref = np.array([numpy_stats(sol.spot_hits(sd, c)) for c in range(K)])
            t1 = time.perf_counter()
            st = sol.spot_stats(sd)
            t2 = time.perf_counter()
            if rep:
                t_loop.append(1e3 * (t1 - t0))
                t_dev.append(1e3 * (t2 - t1))
                k_dev.append(sol.readout_ms)
        best = int(st[:, sr.RMS_R].argmin())
        print("== sweep: K = %d configurations x %d rays, through focus; smallest RMS_R %.4e m at y = %.3f mm (numpy loop agrees to %.1e relative)"
              % (K, rays, st[best, sr.RMS_R], ys[best] / mm, np.abs(st[:, sr.RMS_R] / ref[:, sr.RMS_R] - 1).max()))
        print("   loop over spot_hits(det, c) + numpy  wall ms %10.2f" % med(t_loop))
        print("   one spot_stats call                  wall ms %10.2f   kernel ms %s   loop / call = %.0f"
              % (med(t_dev), spread(k_dev), med(t_loop) / med(t_dev)), flush=True)
    finally:
        sol.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-sweep", action="store_true")
    ap.add_argument("--ab-only", action="store_true")
    a = ap.parse_args()
    print("library: %s" % os.path.basename(abi.ENGINE_PATH))
    workload("c2 survey 2^20", 1 << 20, True, a.reps, a.ab_only)
    workload("c2 survey 2^22", 1 << 22, False, a.reps, a.ab_only)
    if not (a.skip_sweep or a.ab_only):
        sweep(1024, 1024, 3)


if __name__ == "__main__":
    main()

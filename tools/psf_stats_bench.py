"""Wavefront read-out: bmo_psf_stats on resident rows against the copy path, and the device window of a sweep's PSF read-out.
python tools/psf_stats_bench.py [--reps 5] [--skip-sweep]

One process, the variants alternating within a round, medians of --reps rounds after one warm-up round, [min .. max] for kernel times.

Single results: the Airy KAT scene (tests/test_psf_readout.py airy_setup's lens and detector) on a disc bundle of 2^20 rays with the
segment log and of 2^22 rays detector-only (record_segments = 0); the PSFDetector is slot 0.
  (a) copy   : bmo_result_copy_hits of the 72-byte rows into pinned host memory, then the three passes in numpy;
  (b) device : bmo_psf_stats_sweep on the resident rows: wall time and the engine's kernel_ms (three accumulate passes and their reduces);
  (c) d2d    : a device-to-device copy of a buffer of exactly the size of the slot's rows through torch, timed with events: the streaming
               yardstick for kernel_ms (the same yardstick as tools/spot_bench.py).
(a) and (b) must agree to the tolerance of a float64 numpy evaluation (printed, not asserted).

Sweep: the K = 1 024 x 1 024-row, n = 64 case of tools/psf_sweep_bench.py: SweepSolution.psf_intensity with window="host" and with
window="device", against the loop of single bmo_psf_intensity calls on device rows (windows by psf_sample_axes on host rows)."""
import argparse
import ctypes as C
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


def numpy_stats(rows, origin, e1, e2):
    """The three passes of include/bmo.h "Wavefront read-out" in numpy (pairwise sums)."""
    d = rows[:, 0:3] - origin[None, :]
    x, z, w, k = d @ e1, d @ e2, rows[:, 7], rows[:, 8]
    s = w.sum()
    cx, cz = (w * x).sum() / s, (w * z).sum() / s
    p = (origin + cx * e1) + cz * e2
    W = rows[:, 6] + ((p[None, :] - rows[:, 0:3]) * rows[:, 3:6]).sum(axis=1)
    m = (w * W).sum() / s
    ph = k * W
    re, im = (w * np.cos(ph)).sum(), (w * np.sin(ph)).sum()
    dW = W - m
    return np.array([len(rows), s, cx, cz, x.min(), x.max(), z.min(), z.max(), np.abs(x - cx).max(), np.abs(z - cz).max(), cx, cz, m,
                     np.sqrt((w * dW * dW).sum() / s), dW.min(), dW.max(), re, im, (re * re + im * im) / (s * s), k.min(), k.max()])


def workload(name, n_rays, record, reps):
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

        t_a, t_copy, t_b, k_b, t_c = [], [], [], [], []
        for rep in range(reps + 1):  # the first round warms up and is not counted
            t0 = time.perf_counter()
            eng.result_copy_hits(res, slot, host.ctypes.data, n)
            t1 = time.perf_counter()
            ref = numpy_stats(host, pos, e1, e2)
            t2 = time.perf_counter()
            st, ms = abi.psf_stats_sweep(res, slot, 1, pos, e1, e2)
            t3 = time.perf_counter()
            c = d2d()
            if rep:
                t_a.append(1e3 * (t2 - t0))
                t_copy.append(1e3 * (t1 - t0))
                t_b.append(1e3 * (t3 - t2))
                k_b.append(ms)
                t_c.append(c)
        st = st[0]
        print("statistics: N %d  W_RMS %.6e m  PV %.6e m  STREHL %.6f  Marechal %.6f" % (st[abi.PSF_N], st[abi.PSF_W_RMS], st[abi.PSF_W_HI] - st[abi.PSF_W_LO],
                                                                                         st[abi.PSF_STREHL], bmo.components.psf_marechal(st)))
        cols = [abi.PSF_S, abi.PSF_CX, abi.PSF_HWX, abi.PSF_W_MEAN, abi.PSF_W_RMS, abi.PSF_STREHL]
        print("   relative difference to numpy: " + "  ".join("%s %.1e" % (nm, abs(st[c] - ref[c]) / max(abs(ref[c]), 1e-300))
                                                              for nm, c in zip(("S", "CX", "HWX", "W_MEAN", "W_RMS", "STREHL"), cols)))
        print("   (a) copy + numpy passes  wall ms %9.2f  (copy alone %8.2f)" % (med(t_a), med(t_copy)))
        print("   (b) resident read-out    wall ms %9.2f   kernel ms %s (three passes)" % (med(t_b), spread(k_b)))
        print("   (c) d2d copy of rows     event ms %s   kernel / d2d = %.2f;  end to end (a) / (b) = %.1f"
              % (spread(t_c), med(k_b) / med(t_c), med(t_a) / med(t_b)), flush=True)
    finally:
        eng.free_result(res)
        eng.free_batch(dev)
        eng.close()


def sweep(K, rays, n, reps):
    system, cs, psfd, lam, D = airy_setup(num_rays=rays)
    p0 = np.array(psfd.position(), dtype=np.float64)
    dys = bmo.linalg.linrange(-1e-3, 1e-3, K)
    sol = bmo.solve_sweep(system, cs, K, lambda c: bmo.translate_to3d(psfd, list(p0 + np.array([0, dys[c], 0]))))
    try:
        slot = sol._slot(psfd)
        poses = [sol._poses[c][slot] for c in range(K)]
        cfg = sol.res.node_root[sol.res.detector_nodes(slot)] // sol.n_roots
        start = np.searchsorted(cfg, np.arange(K + 1))
        rows = sol.res.detector_hits(slot)
        ptr, cnt = C.POINTER(C.c_double)(), C.c_int64()
        abi.check(sol.lib, sol.lib.bmo_result_device_hits(sol._handle, slot, C.byref(ptr), C.byref(cnt)), "bmo_result_device_hits")
        base = C.cast(ptr, C.c_void_p).value

        def loop():
            I, ks = np.zeros((K, n, n)), 0.0
            for c in range(K):
                r = rows[start[c]:start[c + 1]]
                pos, ori = poses[c]
                xs, zs = bmo.components.psf_sample_axes(r, pos, ori, n=n)
                I[c], _, ms = abi.psf_intensity(None, pos, ori[:, 0], ori[:, 2], xs, zs, hits_device_ptr=base + 72 * int(start[c]), n_hits=len(r))
                ks += ms
            return I, ks

        def batched(window):
            _, _, I = sol.psf_intensity(psfd, n=n, window=window)
            return I, sol.readout_ms

        def stats_alone():
            sol.psf_stats(psfd)
            return None, sol.readout_ms

        variants = (("loop", loop), ("host", lambda: batched("host")), ("device", lambda: batched("device")), ("stats", stats_alone))
        wall = {k: [] for k, _ in variants}
        kern = {k: [] for k, _ in variants}
        got = {}
        for rep in range(reps + 1):
            for name, fn in variants:
                t0 = time.perf_counter()
                I, ks = fn()
                dt = time.perf_counter() - t0
                got[name] = I
                if rep:
                    wall[name].append(1e3 * dt)
                    kern[name].append(ks)
        assert np.array_equal(got["loop"], got["host"])
        rel = np.abs(got["device"] - got["host"]).max() / got["host"].max()
        print("== sweep: K = %d configurations x %d rays, n = %d; device-window image differs from the host-window one by %.1e of the peak" % (K, rays, n, rel))
        print("   loop of single calls (device rows)   wall ms %9.2f   kernel ms %s" % (med(wall["loop"]), spread(kern["loop"])))
        print("   batched, window=\"host\"               wall ms %9.2f   kernel ms %s   loop / call = %.2f"
              % (med(wall["host"]), spread(kern["host"]), med(wall["loop"]) / med(wall["host"])))
        print("   batched, window=\"device\"             wall ms %9.2f   kernel ms %s   loop / call = %.2f"
              % (med(wall["device"]), spread(kern["device"]), med(wall["loop"]) / med(wall["device"])))
        print("   psf_stats alone (K rows of 21)       wall ms %9.2f   kernel ms %s" % (med(wall["stats"]), spread(kern["stats"])), flush=True)
    finally:
        sol.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-sweep", action="store_true")
    a = ap.parse_args()
    print("library: %s" % os.path.basename(abi.ENGINE_PATH))
    workload("airy 2^20", 1 << 20, True, a.reps)
    workload("airy 2^22", 1 << 22, False, a.reps)
    if not a.skip_sweep:
        sweep(1024, 1024, 64, a.reps)


if __name__ == "__main__":
    main()

"""OPD map read-out: bmo_psf_opd_map on resident rows against bmo_psf_zernike, a device-to-device copy of the rows and the copy path.
python tools/psf_opd_bench.py [--reps 5] [--rays N] [--bins 32,128,1024] [--order 4] [--ab-only] [--profile]

One process, the variants alternating within a round, medians of --reps rounds after one warm-up round, [min .. max] for kernel times.

The Airy KAT scene (tests/test_psf_readout.py airy_setup's lens and detector) on a disc bundle of 2^20 rays, detector-only; the
PSFDetector is slot 0.  Per bin count n:
  (a) copy    : bmo_result_copy_hits of the 72-byte rows into pinned host memory, then the map in numpy (np.add.at of float sums);
  (b) map     : bmo_psf_opd_map on the resident rows with the coefficients, reference point and pupil of a fit at --order with piston
                and tilt kept out (remove = "tilt"): wall time and the engine's kernel_ms (passes A, B, E, M and the finish);
  (c) zernike : bmo_psf_zernike_sweep at the same order on the same rows, kernel_ms (four passes);
  (d) d2d     : a device-to-device copy of a buffer of the size of the row table through torch, timed with events.
(a) and (b) must agree to the tolerance of a float64 numpy evaluation (printed, not asserted).

A/B of the wave-aggregated add: the same map (b) on a device copy of the rows in the solve's own coherence order, and on the same rows
shuffled (seeded).  --ab-only prints these two kernel times alone, for a library built with another BMO_OPD_AGG_ITERS and chosen with
BMO_ENGINE_LIB (-DBMO_OPD_AGG_ITERS=0: plain per-lane atomics); alternate the two libraries run by run.
--profile runs every map once more after the timed rounds and nothing else worth a trace: for a rocprofv3 --kernel-trace --stats run, which
gives pass M (psf_opd_bin_kernel) against psf_zernike_residual_kernel, the same reads and term evaluation without the binning."""
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


def numpy_map(rows, origin, e1, e2, order, coef, ref, pupil, n):
    """The map of include/bmo.h "OPD map read-out" in plain numpy: float sums per bin."""
    p = (origin + ref[0] * e1) + ref[1] * e2
    W = rows[:, 6] + ((p[None, :] - rows[:, 0:3]) * rows[:, 3:6]).sum(axis=1)
    w = rows[:, 7]
    x, y = (rows[:, 3:6] @ e1 - pupil[0]) / pupil[2], (rows[:, 3:6] @ e2 - pupil[1]) / pupil[2]
    E = (W - (w * W).sum() / w.sum()) - np.tensordot(coef, bmo.components.zernike_basis(x, y, order), axes=1)
    inside = (x >= -1) & (x <= 1) & (y >= -1) & (y <= 1)
    key = (np.minimum(np.floor((x + 1.0) * (n / 2.0)), n - 1) + n * np.minimum(np.floor((y + 1.0) * (n / 2.0)), n - 1)).astype(np.int64)[inside]
    num, den = np.zeros(n * n), np.zeros(n * n)
    np.add.at(num, key, (w * E)[inside])
    np.add.at(den, key, w[inside])
    with np.errstate(all="ignore"):
        return (num / den).reshape(n, n).T


def run(n_rays, reps, order, bins, ab_only, profile):
    system, cs, psfd, lam, D = airy_setup(num_rays=1)
    bundle = scenes.disc_bundle(n_rays, center=[0, -10 * mm, 0], direction=[0, 1, 0], diameter=D, lam=lam)
    scene = bmo.CompiledScene(system, bundle.lambdas)
    eng = bmo.Engine(scene, 0)
    dev = eng.upload(bundle)
    res = eng.trace_device(dev, 100, record_segments=False)
    try:
        slot = 0
        ptr, n = eng.result_device_hits(res, slot)
        pos, ori = np.asarray(psfd.position(), dtype=np.float64), np.asarray(psfd.orientation(), dtype=np.float64)
        e1, e2 = ori[:, 0].copy(), ori[:, 2].copy()
        print("== airy: %d rays, detector-only, slot %d holds %d rows (%.1f MB resident), order %d" % (n_rays, slot, n, n * 72 / 1e6, order), flush=True)
        pinned = torch.empty((n, 9), dtype=torch.float64, pin_memory=True)
        host = pinned.numpy()
        eng.result_copy_hits(res, slot, host.ctypes.data, n)
        ordered = torch.from_numpy(host).to("cuda")
        shuffled = torch.from_numpy(host[np.random.default_rng(1).permutation(n)]).to("cuda")
        src = torch.empty(n * 72, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        torch.cuda.synchronize()

        def d2d():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            dst.copy_(src)
            b.record()
            b.synchronize()
            return a.elapsed_time(b)

        coef, zi, _, _ = abi.psf_zernike_sweep(res, slot, 1, pos, e1, e2, order=order)
        cf = coef[0].copy()
        cf[3:] = 0.0
        ref, pupil = zi[0, [abi.ZERN_X_REF, abi.ZERN_Z_REF]], zi[0, [abi.ZERN_U0, abi.ZERN_V0, abi.ZERN_RHO]]
        kw = dict(order=order, coef=cf, ref=ref, pupil=pupil)
        for nb in bins:
            t_a, t_copy, t_b, k_b, k_z, t_d, k_o, k_s = [], [], [], [], [], [], [], []
            for rep in range(reps + 1):  # the first round warms up and is not counted
                if not ab_only:
                    t0 = time.perf_counter()
                    eng.result_copy_hits(res, slot, host.ctypes.data, n)
                    t1 = time.perf_counter()
                    want = numpy_map(host, pos, e1, e2, order, cf, ref, pupil, nb)
                    t2 = time.perf_counter()
                    opd, weight, count, info, _, ms = abi.psf_opd_map_sweep(res, slot, 1, pos, e1, e2, n=nb, **kw)
                    t3 = time.perf_counter()
                    ms_z = abi.psf_zernike_sweep(res, slot, 1, pos, e1, e2, order=order)[3]
                    c = d2d()
                ms_o = abi.psf_opd_map(None, pos, e1, e2, n=nb, hits_device_ptr=ordered.data_ptr(), n_hits=n, **kw)[5]
                ms_s = abi.psf_opd_map(None, pos, e1, e2, n=nb, hits_device_ptr=shuffled.data_ptr(), n_hits=n, **kw)[5]
                if rep:
                    k_o.append(ms_o)
                    k_s.append(ms_s)
                    if not ab_only:
                        t_a.append(1e3 * (t2 - t0))
                        t_copy.append(1e3 * (t1 - t0))
                        t_b.append(1e3 * (t3 - t2))
                        k_b.append(ms)
                        k_z.append(ms_z)
                        t_d.append(c)
            if not ab_only:
                opd, info = opd[0], info[0]
                both = np.isfinite(opd) & np.isfinite(want)
                print("n = %d: STATUS %d  %d of %d bins filled  N_OUTSIDE %d  map %.4e .. %.4e m  largest difference to numpy %.1e of the range"
                      % (nb, info[abi.OPD_STATUS], info[abi.OPD_N_FILLED], nb * nb, info[abi.OPD_N_OUTSIDE], info[abi.OPD_MAP_LO], info[abi.OPD_MAP_HI],
                         np.abs(opd - want)[both].max() / (info[abi.OPD_MAP_HI] - info[abi.OPD_MAP_LO])))
                print("   (a) copy + numpy map       wall ms %9.2f  (copy alone %8.2f)" % (med(t_a), med(t_copy)))
                print("   (b) resident map           wall ms %9.2f   kernel ms %s (A, B, E, M, finish)" % (med(t_b), spread(k_b)))
                print("   (c) psf_zernike, same rows kernel ms %s   map / zernike = %.2f" % (spread(k_z), med(k_b) / med(k_z)))
                print("   (d) d2d copy of rows       event ms %s   map / d2d = %.2f;  end to end (a) / (b) = %.1f" % (spread(t_d), med(k_b) / med(t_d), med(t_a) / med(t_b)))
            print("   A/B n = %4d   ordered rows kernel ms %s   shuffled rows kernel ms %s" % (nb, spread(k_o), spread(k_s)), flush=True)
        if profile:
            for nb in bins:
                abi.psf_opd_map_sweep(res, slot, 1, pos, e1, e2, n=nb, **kw)
                abi.psf_opd_map(None, pos, e1, e2, n=nb, hits_device_ptr=shuffled.data_ptr(), n_hits=n, **kw)
            abi.psf_zernike_sweep(res, slot, 1, pos, e1, e2, order=order)
    finally:
        eng.free_result(res)
        eng.free_batch(dev)
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--bins", default="32,128,1024")
    ap.add_argument("--order", type=int, default=4)
    ap.add_argument("--ab-only", action="store_true")
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    print("library: %s" % os.path.basename(abi.ENGINE_PATH))
    run(a.rays, a.reps, a.order, [int(b) for b in a.bins.split(",")], a.ab_only, a.profile)


if __name__ == "__main__":
    main()

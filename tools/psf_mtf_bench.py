"""MTF read-out: bmo_psf_geo_otf on resident rows against copying the rows out and transforming them in numpy, and bmo_psf_otf against
bmo_psf_through_focus alone.
python tools/psf_mtf_bench.py [--reps 5] [--rays 1048576] [--n 64] [--freqs 64] [--planes 1,16,64] [--stack-planes 1,16]

One process, the variants alternating within a round, medians of --reps rounds after one warm-up round, [min .. max] for kernel times.

The Airy KAT scene (tests/test_psf_readout.py airy_setup's lens and detector) on a disc bundle of 2^20 rays, detector-only
(record_segments = 0); the PSFDetector is slot 0.  64 frequencies from 0 to 1.2 cutoffs along x, M planes from -0.5 mm to +0.5 mm along the
detector's local y, the phase counted from each plane's centroid (bmo_psf_focus_stats).  The bundle carries scenes.disc_bundle's direction
jitter like the other read-out benches, so its geometric MTF at these frequencies is near zero: this measures cost, which does not depend on
the values; tests/test_mtf_ref.py holds the values of the unjittered scene.
Geometric, per M:
  (a) copy   : bmo_result_copy_hits of the 72-byte rows into pinned host memory, then the transform of ONE plane in numpy (propagation,
               np.exp of rows x frequencies), measured once, and M times that as the cost of the stack;
  (b) device : bmo_psf_geo_otf on the resident rows: wall time and the engine's kernel_ms; ps per (row, plane, frequency) pair;
  (c) psf    : bmo_psf_intensity at n = 64 on the same rows, the yardstick of a sincos per pair: ps per (row, point) pair;
  (d) d2d    : a device-to-device copy of a buffer of the size of the rows through torch, timed with events: the streaming yardstick.
(a) and (b) must agree to the tolerance of a float64 numpy evaluation (printed, not asserted).
Diffraction, per M of --stack-planes at n x n samples on mtf_window's grid:
  (e) bmo_psf_through_focus alone, (f) bmo_psf_otf (the same stack, transformed where it lies; only otf, mtf and sums come back)."""
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
cp = bmo.components


def med(v):
    return float(np.median(v))


def spread(v):
    return "%9.3f [%8.3f .. %8.3f]" % (med(v), min(v), max(v))


def numpy_plane(rows, pos, e1, e2, axis, off, center, freqs):
    """T [nf] of one plane in numpy: the propagation of include/bmo.h and np.exp over rows x frequencies, in blocks that stay in cache."""
    nrm = np.cross(e1, e2)
    om = pos + off * axis
    s = ((om - rows[:, 0:3]) @ nrm) / (rows[:, 3:6] @ nrm)
    q = rows[:, 0:3] + s[:, None] * rows[:, 3:6] - om
    x, z, w = q @ e1 - center[0], q @ e2 - center[1], rows[:, 7]
    T = np.zeros(len(freqs), dtype=np.complex128)
    for b in range(0, len(rows), 1 << 16):
        sl = slice(b, b + (1 << 16))
        T += w[sl] @ np.exp(-2j * np.pi * (x[sl, None] * freqs[None, :, 0] + z[sl, None] * freqs[None, :, 1]))
    return T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--freqs", type=int, default=64)
    ap.add_argument("--planes", default="1,16,64")
    ap.add_argument("--stack-planes", default="1,16")
    a = ap.parse_args()
    print("library: %s" % os.path.basename(abi.ENGINE_PATH))
    system, cs, psfd, lam, D = airy_setup(num_rays=1)
    bundle = scenes.disc_bundle(a.rays, center=[0, -10 * mm, 0], direction=[0, 1, 0], diameter=D, lam=lam)
    scene = bmo.CompiledScene(system, bundle.lambdas)
    eng = bmo.Engine(scene, 0)
    dev = eng.upload(bundle)
    res = eng.trace_device(dev, 100, record_segments=False)
    try:
        ptr, H = eng.result_device_hits(res, 0)
        pos, ori = np.asarray(psfd.position(), dtype=np.float64), np.asarray(psfd.orientation(), dtype=np.float64)
        e1, e2, axis = ori[:, 0].copy(), ori[:, 2].copy(), ori[:, 1].copy()
        kw = dict(hits_device_ptr=ptr, n_hits=H)
        st0, _ = abi.psf_stats(None, pos, e1, e2, **kw)
        rho = abi.psf_zernike(None, pos, e1, e2, order=0, **kw)[1][abi.ZERN_RHO]
        f_c = cp.mtf_cutoff(st0[abi.PSF_K_MAX], rho)
        freqs = cp.mtf_frequencies(1.2 * f_c, a.freqs, 0.0)
        xs, zs = cp.psf_axes_from_stats(st0, n=a.n)
        print("== %d rays, detector-only, slot 0 holds %d rows (%.1f MB resident); cutoff %.0f cycles/m, %d frequencies up to 1.2 cutoffs"
              % (a.rays, H, H * 72 / 1e6, f_c, a.freqs), flush=True)
        pinned = torch.empty((H, 9), dtype=torch.float64, pin_memory=True)
        host = pinned.numpy()
        src = torch.empty(H * 72, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)

        def d2d():
            e0, e1_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(src)
            e1_.record()
            e1_.synchronize()
            return e0.elapsed_time(e1_)

        for M in [int(v) for v in a.planes.split(",")]:
            off = np.linspace(-0.5 * mm, 0.5 * mm, M) if M > 1 else np.array([0.0])
            cen = abi.psf_focus_stats(None, pos, e1, e2, axis, off, **kw)[0][:, [abi.FOCUS_CX, abi.FOCUS_CZ]]
            t_copy, t_b, k_b, k_c, t_d = [], [], [], [], []
            for rep in range(a.reps + 1):  # the first round warms up and is not counted
                t0 = time.perf_counter()
                eng.result_copy_hits(res, 0, host.ctypes.data, H)
                t1 = time.perf_counter()
                mtf, otf, sums, ms = abi.psf_geo_otf(None, pos, e1, e2, axis, off, freqs, centers=cen, **kw)
                t2 = time.perf_counter()
                ms_c = abi.psf_intensity(None, pos, e1, e2, xs, zs, **kw)[2]
                ms_d = d2d()
                if rep:
                    t_copy.append(1e3 * (t1 - t0)), t_b.append(1e3 * (t2 - t1)), k_b.append(ms), k_c.append(ms_c), t_d.append(ms_d)
            t0 = time.perf_counter()
            ref = numpy_plane(host, pos, e1, e2, axis, off[M // 2], cen[M // 2], freqs)
            t_np = 1e3 * (time.perf_counter() - t0)
            rel = np.abs(otf[M // 2] - ref).max() / sums[M // 2]
            pairs = H * M * a.freqs
            print("-- M = %d planes x %d frequencies: %d pairs; device differs from numpy by %.1e of S (plane %d); MTF at 0.6 cutoffs %.4f"
                  % (M, a.freqs, pairs, rel, M // 2, mtf[M // 2, a.freqs // 2]))
            print("   (a) copy %8.2f ms + numpy %9.1f ms per plane (one plane measured): %10.1f ms for the stack" % (med(t_copy), t_np, med(t_copy) + M * t_np))
            print("   (b) bmo_psf_geo_otf     wall ms %9.2f   kernel ms %s   %7.2f ps per pair   (a) / (b) = %.0f"
                  % (med(t_b), spread(k_b), 1e9 * med(k_b) / pairs, (med(t_copy) + M * t_np) / med(t_b)))
            print("   (c) bmo_psf_intensity n = %d            kernel ms %s   %7.2f ps per pair" % (a.n, spread(k_c), 1e9 * med(k_c) / (H * a.n * a.n)))
            print("   (d) d2d copy of the rows                       ms %s" % spread(t_d), flush=True)

        hw, n_rule = cp.mtf_window(st0[abi.PSF_K_MAX], rho, H, 1.2 * f_c)
        gx = bmo.linalg.linrange(-hw, hw, a.n)
        cp.mtf_check_pitch(gx, gx, freqs)
        print("== diffraction: n = %d on a window of half-width %.1f um (mtf_window: n >= %d)" % (a.n, 1e6 * hw, n_rule))
        for M in [int(v) for v in a.stack_planes.split(",")]:
            off = np.linspace(-0.5 * mm, 0.5 * mm, M) if M > 1 else np.array([0.0])
            st = abi.psf_focus_stats(None, pos, e1, e2, axis, off, **kw)[0]
            d = off[:, None] * axis[None, :] + st[:, abi.FOCUS_CX:abi.FOCUS_CX + 1] * e1[None, :] + st[:, abi.FOCUS_CZ:abi.FOCUS_CZ + 1] * e2[None, :]
            w_e, k_e, w_f, k_f = [], [], [], []
            for rep in range(a.reps + 1):
                t0 = time.perf_counter()
                I, _, ms_e = abi.psf_through_focus(None, pos, e1, e2, d, gx, gx, **kw)
                t1 = time.perf_counter()
                mtf, otf, sums, _, ms_f = abi.psf_otf(None, pos, e1, e2, d, gx, gx, freqs, **kw)
                t2 = time.perf_counter()
                if rep:
                    w_e.append(1e3 * (t1 - t0)), k_e.append(ms_e), w_f.append(1e3 * (t2 - t1)), k_f.append(ms_f)
            s = np.hypot(freqs[:, 0], freqs[:, 1]) / f_c
            err = np.abs(mtf[M // 2] - cp.mtf_diffraction_limit(s))
            print("-- M = %d planes; plane %d: |MTF - limit| %.4f up to the cutoff, %.1e beyond" % (M, M // 2, err[s <= 1].max(), err[s > 1].max()))
            print("   (e) bmo_psf_through_focus   wall ms %9.2f   kernel ms %s" % (med(w_e), spread(k_e)))
            print("   (f) bmo_psf_otf             wall ms %9.2f   kernel ms %s   (f) - (e) = %.3f ms of kernels"
                  % (med(w_f), spread(k_f), med(k_f) - med(k_e)), flush=True)
    finally:
        eng.free_result(res)
        eng.free_batch(dev)
        eng.close()


if __name__ == "__main__":
    main()

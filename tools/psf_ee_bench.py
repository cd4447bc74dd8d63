"""Encircled-energy read-out: bmo_psf_geo_ee on resident rows against bmo_psf_geo_otf on the same planes and against copying the rows out
and counting in numpy, bmo_psf_ee against bmo_psf_through_focus alone, and bmo_spot_ee against bmo_spot_image and numpy.
python tools/psf_ee_bench.py [--reps 5] [--rays 1048576] [--n 64] [--radii 64] [--planes 1,16,64] [--stack-planes 1,16] [--skip-spot] [--skip-sweep]

One process, the variants alternating within a round, medians of --reps rounds after one warm-up round, [min .. max] for kernel times.

PSF rows: the Airy KAT scene (tests/test_psf_readout.py airy_setup's lens and detector) on a disc bundle of 2^20 rays, detector-only
(record_segments = 0); the PSFDetector is slot 0.  64 radii from 0 to the largest radius of the in-focus plane, M planes from -0.5 mm to
+0.5 mm along the detector's local y, about each plane's centroid (bmo_psf_focus_stats).
Geometric, per M:
  (a) copy   : bmo_result_copy_hits of the 72-byte rows into pinned host memory, then ONE plane in numpy (propagation, r2, a compare and a
               masked sum per radius), measured once, and M times that as the cost of the stack;
  (b) device : bmo_psf_geo_ee on the resident rows: wall time and the engine's kernel_ms; ps per (row, plane, radius) pair;
  (c) otf    : bmo_psf_geo_otf with as many frequencies on the same planes: the walk with a sincospi in place of the compare;
  (d) d2d    : a device-to-device copy of a buffer of the size of the rows through torch, timed with events: the streaming yardstick.
(a) and (b) must agree in every count (printed, not asserted).
Diffraction, per M of --stack-planes at n x n samples on mtf_window's grid at the cutoff:
  (e) bmo_psf_through_focus alone, (f) bmo_psf_ee (the same stack, summed where it lies; only ee, energy, sums and the centres come back);
  the distance of the in-focus curve from components.ee_diffraction_limit (a property of the sampling and of the bundle's jitter).
Spot rows: the config-2 scene (tests/scenes.py) on 2^20 and 2^22 rays detector-only, slot 0; 64 and 4 096 radii about the centroid:
  (g) bmo_spot_ee_sweep on the resident rows, (h) bmo_spot_image_sweep at 128 x 128 (the LDS path) on the same rows, (d) the copy yardstick,
  (i) bmo_result_copy_hit_columns of 2 columns + numpy (r2, sort, searchsorted).
Sweep: K = 1 024 configurations x 1 024 rays of a through-focus scan, one spot_encircled_energy call against the loop over spot_hits + numpy."""
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
from test_psf_readout import airy_setup  # noqa: E402

mm = 1e-3
cp = bmo.components


def med(v):
    return float(np.median(v))


def spread(v):
    return "%9.3f [%8.3f .. %8.3f]" % (med(v), min(v), max(v))


def d2d_timer(n_bytes):
    src = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)

    def d2d():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    return d2d


def numpy_plane(rows, pos, e1, e2, axis, off, center, radii):
    """(count, energy) [nr] of one plane in numpy: the propagation of include/bmo.h, r2, and a compare and a masked sum per radius."""
    nrm = np.cross(e1, e2)
    om = pos + off * axis
    s = ((om - rows[:, 0:3]) @ nrm) / (rows[:, 3:6] @ nrm)
    q = rows[:, 0:3] + s[:, None] * rows[:, 3:6] - om
    ax, az, w = q @ e1 - center[0], q @ e2 - center[1], rows[:, 7]
    r2 = ax * ax + az * az
    inside = [r2 <= R * R for R in radii]
    return np.array([m.sum() for m in inside]), np.array([w[m].sum() for m in inside])


def numpy_spot(rows, center, radii):
    ax, az = rows[:, 0] - center[0], rows[:, 1] - center[1]
    r2 = np.sort(ax * ax + az * az)
    return np.searchsorted(r2, radii * radii, side="right")


def psf_part(a):
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
        fs0 = abi.psf_focus_stats(None, pos, e1, e2, axis, [0.0], **kw)[0][0]
        radii = cp.ee_radii(fs0[abi.FOCUS_MAX_R], a.radii)
        freqs = cp.mtf_frequencies(1.2 * f_c, a.radii, 0.0)
        print("== %d rays, detector-only, slot 0 holds %d rows (%.1f MB resident); %d radii up to %.1f um (the in-focus plane's largest radius)"
              % (a.rays, H, H * 72 / 1e6, a.radii, 1e6 * radii[-1]), flush=True)
        pinned = torch.empty((H, 9), dtype=torch.float64, pin_memory=True)
        host = pinned.numpy()
        d2d = d2d_timer(H * 72)
        for M in [int(v) for v in a.planes.split(",")]:
            off = np.linspace(-0.5 * mm, 0.5 * mm, M) if M > 1 else np.array([0.0])
            cen = abi.psf_focus_stats(None, pos, e1, e2, axis, off, **kw)[0][:, [abi.FOCUS_CX, abi.FOCUS_CZ]]
            t_copy, t_b, k_b, k_c, t_d = [], [], [], [], []
            for rep in range(a.reps + 1):  # the first round warms up and is not counted
                t0 = time.perf_counter()
                eng.result_copy_hits(res, 0, host.ctypes.data, H)
                t1 = time.perf_counter()
                ee, energy, count, sums, ms = abi.psf_geo_ee(None, pos, e1, e2, axis, off, radii, centers=cen, **kw)
                t2 = time.perf_counter()
                ms_c = abi.psf_geo_otf(None, pos, e1, e2, axis, off, freqs, centers=cen, **kw)[3]
                ms_d = d2d()
                if rep:
                    t_copy.append(1e3 * (t1 - t0)), t_b.append(1e3 * (t2 - t1)), k_b.append(ms), k_c.append(ms_c), t_d.append(ms_d)
            t0 = time.perf_counter()
            ref_n, ref_e = numpy_plane(host, pos, e1, e2, axis, off[M // 2], cen[M // 2], radii)
            t_np = 1e3 * (time.perf_counter() - t0)
            pairs = H * M * a.radii
            print("-- M = %d planes x %d radii: %d pairs; plane %d: %d counts differ from numpy's, energy by %.1e of S; EE at half the largest radius %.4f"
                  % (M, a.radii, pairs, M // 2, int((count[M // 2] != ref_n).sum()), np.abs(energy[M // 2] - ref_e).max() / sums[M // 2], ee[M // 2, a.radii // 2]))
            print("   (a) copy %8.2f ms + numpy %9.1f ms per plane (one plane measured): %10.1f ms for the stack" % (med(t_copy), t_np, med(t_copy) + M * t_np))
            print("   (b) bmo_psf_geo_ee      wall ms %9.2f   kernel ms %s   %7.2f ps per pair   (a) / (b) = %.0f"
                  % (med(t_b), spread(k_b), 1e9 * med(k_b) / pairs, (med(t_copy) + M * t_np) / med(t_b)))
            print("   (c) bmo_psf_geo_otf, %d frequencies     kernel ms %s   %7.2f ps per pair   (b) / (c) = %.2f"
                  % (a.radii, spread(k_c), 1e9 * med(k_c) / pairs, med(k_b) / med(k_c)))
            print("   (d) d2d copy of the rows                       ms %s" % spread(t_d), flush=True)

        hw, n_rule = cp.mtf_window(st0[abi.PSF_K_MAX], rho, H, f_c)
        gx = bmo.linalg.linrange(-hw, hw, a.n)
        airy = 1.22 * np.pi / (st0[abi.PSF_K_MAX] * rho)
        rr_ = cp.ee_radii(min(4 * airy, 0.9 * hw), a.radii)
        print("== diffraction: n = %d on a window of half-width %.1f um (mtf_window at the cutoff: n >= %d); %d radii up to %.1f um (Airy radius %.2f um)"
              % (a.n, 1e6 * hw, n_rule, a.radii, 1e6 * rr_[-1], 1e6 * airy))
        for M in [int(v) for v in a.stack_planes.split(",")]:
            off = np.linspace(-0.5 * mm, 0.5 * mm, M) if M > 1 else np.array([0.0])
            st = abi.psf_focus_stats(None, pos, e1, e2, axis, off, **kw)[0]
            d = off[:, None] * axis[None, :] + st[:, abi.FOCUS_CX:abi.FOCUS_CX + 1] * e1[None, :] + st[:, abi.FOCUS_CZ:abi.FOCUS_CZ + 1] * e2[None, :]
            w_e, k_e, w_f, k_f = [], [], [], []
            for rep in range(a.reps + 1):
                t0 = time.perf_counter()
                I, _, ms_e = abi.psf_through_focus(None, pos, e1, e2, d, gx, gx, **kw)
                t1 = time.perf_counter()
                ee, energy, sums, cen, _, ms_f = abi.psf_ee(None, pos, e1, e2, d, gx, gx, rr_, **kw)
                t2 = time.perf_counter()
                if rep:
                    w_e.append(1e3 * (t1 - t0)), k_e.append(ms_e), w_f.append(1e3 * (t2 - t1)), k_f.append(ms_f)
            lim = cp.ee_diffraction_limit(st0[abi.PSF_K_MAX] * rho * rr_)
            m0 = int(np.argmin(np.abs(off)))
            print("-- M = %d planes; plane %d (offset %.3f mm): |EE - limit| at most %.4f (at r = %.2f um); centroid (%.2e, %.2e) m of the grid"
                  % (M, m0, off[m0] / mm, np.abs(ee[m0] - lim).max(), 1e6 * rr_[int(np.abs(ee[m0] - lim).argmax())], cen[m0, 0], cen[m0, 1]))
            print("   (e) bmo_psf_through_focus   wall ms %9.2f   kernel ms %s" % (med(w_e), spread(k_e)))
            print("   (f) bmo_psf_ee              wall ms %9.2f   kernel ms %s   (f) - (e) = %.3f ms of kernels"
                  % (med(w_f), spread(k_f), med(k_f) - med(k_e)), flush=True)
    finally:
        eng.free_result(res)
        eng.free_batch(dev)
        eng.close()


def spot_part(n_rays, reps):
    system, parts = scenes.c2_scene()
    bundle = scenes.c2_survey_bundle(n_rays)
    scene = bmo.CompiledScene(system, bundle.lambdas)
    eng = bmo.Engine(scene, 0)
    dev = eng.upload(bundle)
    res = eng.trace_device(dev, 100, record_segments=False)
    try:
        slot = 0
        ptr, n = eng.result_device_hits(res, slot)
        hw = scene.detectors[slot].hw
        print("== spot: c2 survey, %d rays detector-only, slot %d holds %d rows (%.1f MB resident, 16 B of every 72 used)" % (n_rays, slot, n, n * 72 / 1e6), flush=True)
        pinned = torch.empty((n, 2), dtype=torch.float64, pin_memory=True)
        host = pinned.numpy()
        d2d = d2d_timer(n * 72)
        st0 = abi.spot_stats_sweep(res, slot, 1)[0][0]
        center = st0[[sr.CX, sr.CZ]]
        for nr in (64, 4096):
            radii = cp.ee_radii(st0[sr.GEO_R], nr)
            t_a, t_copy, t_g, k_g, k_h, t_d = [], [], [], [], [], []
            for rep in range(reps + 1):
                t0 = time.perf_counter()
                eng.result_copy_hit_columns(res, slot, 2, host.ctypes.data, n)
                t1 = time.perf_counter()
                want = numpy_spot(host, center, radii)
                t2 = time.perf_counter()
                inside, _, ms = abi.spot_ee_sweep(res, slot, 1, center, radii)
                t3 = time.perf_counter()
                ms_h = abi.spot_image_sweep(res, slot, 1, (-hw, hw, -hw, hw), 128, 128)[2]
                ms_d = d2d()
                if rep:
                    t_a.append(1e3 * (t2 - t0)), t_copy.append(1e3 * (t1 - t0)), t_g.append(1e3 * (t3 - t2)), k_g.append(ms), k_h.append(ms_h), t_d.append(ms_d)
            print("-- %d radii up to the geometric radius %.3e m: %d counts differ from numpy's; half the rows inside r = %.3e m"
                  % (nr, radii[-1], int((inside[0] != want).sum()), cp.ee_radius_at(radii, inside[0] / n, 0.5)))
            print("   (g) bmo_spot_ee_sweep       wall ms %9.2f   kernel ms %s   kernel / d2d = %.2f" % (med(t_g), spread(k_g), med(k_g) / med(t_d)))
            print("   (h) bmo_spot_image 128 x 128                kernel ms %s   (g) / (h) = %.2f" % (spread(k_h), med(k_g) / med(k_h)))
            print("   (d) d2d copy of the rows                         ms %s" % spread(t_d))
            print("   (i) copy + numpy            wall ms %9.2f  (copy alone %8.2f)   (i) / (g) = %.1f" % (med(t_a), med(t_copy), med(t_a) / med(t_g)), flush=True)
    finally:
        eng.free_result(res)
        eng.free_batch(dev)
        eng.close()


def sweep_part(K, rays, reps):
    lens = bmo.SphericalLens(100 * mm, float("inf"), 1 * mm, 25.4 * mm, lambda lam_: 1.5)
    sd = bmo.Spotdetector(4 * mm)
    system = bmo.System([lens, sd])
    cs = bmo.UniformDiscSource([0, -10 * mm, 0], [0, 1, 0], 10 * mm, 1e-6, num_rays=rays)
    ys = bmo.linalg.linrange(185 * mm, 215 * mm, K)
    sol = bmo.solve_sweep(system, cs, K, lambda c: bmo.translate_to3d(sd, [0, ys[c], 0]))
    radii = cp.ee_radii(0.5 * mm, 64)
    try:
        t_loop, t_dev, k_dev = [], [], []
        for rep in range(reps + 1):
            t0 = time.perf_counter()
            ref = []
            for c in range(K):
                rows = sol.spot_hits(sd, c)
                ref.append(numpy_spot(rows, rows.mean(axis=0), radii))
            t1 = time.perf_counter()
            frac, inside, n_rows, cen = sol.spot_encircled_energy(sd, radii)
            t2 = time.perf_counter()
            if rep:
                t_loop.append(1e3 * (t1 - t0)), t_dev.append(1e3 * (t2 - t1)), k_dev.append(sol.readout_ms)
        r80 = cp.ee_radius_at(radii, frac, 0.8)
        best = int(np.nanargmin(r80))
        print("== sweep: K = %d configurations x %d rays, through focus; smallest 80 %% radius %.4e m at y = %.3f mm; %d of %d counts differ from the numpy loop's"
              % (K, rays, r80[best], ys[best] / mm, int((inside != np.array(ref)).sum()), inside.size))
        print("   (the loop centres on numpy's mean, the call on bmo_spot_stats' centroid: a row within rounding of an edge may differ)")
        print("   loop over spot_hits(det, c) + numpy         wall ms %10.2f" % med(t_loop))
        print("   one spot_encircled_energy call (stats + ee) wall ms %10.2f   kernel ms %s   loop / call = %.0f"
              % (med(t_dev), spread(k_dev), med(t_loop) / med(t_dev)), flush=True)
    finally:
        sol.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--radii", type=int, default=64)
    ap.add_argument("--planes", default="1,16,64")
    ap.add_argument("--stack-planes", default="1,16")
    ap.add_argument("--skip-psf", action="store_true")
    ap.add_argument("--skip-spot", action="store_true")
    ap.add_argument("--skip-sweep", action="store_true")
    a = ap.parse_args()
    print("library: %s" % os.path.basename(abi.ENGINE_PATH))
    if not a.skip_psf:
        psf_part(a)
    if not a.skip_spot:
        spot_part(1 << 20, a.reps)
        spot_part(1 << 22, a.reps)
    if not a.skip_sweep:
        sweep_part(1024, 1024, 3)


if __name__ == "__main__":
    main()

"""Through-focus read-out: bmo_psf_through_focus against a loop of bmo_psf_intensity calls with shifted origins, and bmo_psf_focus_stats
against a loop of bmo_psf_stats calls, all on resident rows.
python tools/psf_focus_bench.py [--reps 5] [--rays 1048576] [--n 64] [--planes 1,4,16,64]

One process, the variants alternating within a round, medians of --reps rounds after one warm-up round, [min .. max] for kernel times.

The Airy KAT scene (tests/test_psf_readout.py airy_setup's lens and detector) on a disc bundle of 2^20 rays, detector-only
(record_segments = 0); the PSFDetector is slot 0.  M planes from -0.5 mm to +0.5 mm along the detector's local y, the n x n window that of
the rows where they lie (psf_axes_from_stats), common to the stack.
  (a) loop  : M bmo_psf_intensity calls on the resident rows, the origin shifted by d_m: what there was before the stack;
  (b) stack : one bmo_psf_through_focus call;
  (c) stats : bmo_psf_focus_stats for the same M against M bmo_psf_stats calls at the shifted origins (a comparison of cost only: the
              wavefront statistics do not propagate the rows).
(a) and (b) must agree to rounding (the largest difference over the peak is printed, not asserted).  BMO_ENGINE_LIB chooses another build
of the engine (the A/B of planes per chunk: -DBMO_PSF_FOCUS_MP=8 against 16)."""
import argparse
import os
import sys
import time

import numpy as np

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
    return "%9.3f [%8.3f .. %8.3f]" % (med(v), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--planes", default="1,4,16,64")
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
        st0, _ = abi.psf_stats(None, pos, e1, e2, hits_device_ptr=ptr, n_hits=H)
        xs, zs = bmo.components.psf_axes_from_stats(st0, n=a.n)
        print("== %d rays, detector-only, slot 0 holds %d rows (%.1f MB resident); n = %d: %d pairs per plane" % (a.rays, H, H * 72 / 1e6, a.n, H * a.n * a.n),
              flush=True)
        kw = dict(hits_device_ptr=ptr, n_hits=H)
        for M in [int(v) for v in a.planes.split(",")]:
            off = np.linspace(-0.5 * mm, 0.5 * mm, M) if M > 1 else np.array([0.25 * mm])
            d = off[:, None] * axis[None, :]

            def loop():
                I, ks = np.zeros((M, a.n, a.n)), 0.0
                for m in range(M):
                    I[m], _, ms = abi.psf_intensity(None, pos + d[m], e1, e2, xs, zs, **kw)
                    ks += ms
                return I, ks

            def stack():
                I, _, ms = abi.psf_through_focus(None, pos, e1, e2, d, xs, zs, **kw)
                return I, ms

            def stats_loop():
                st, ks = np.zeros((M, abi.PSF_STAT_N)), 0.0
                for m in range(M):
                    st[m], ms = abi.psf_stats(None, pos + d[m], e1, e2, **kw)
                    ks += ms
                return st, ks

            def stats_stack():
                return abi.psf_focus_stats(None, pos, e1, e2, axis, off, **kw)

            variants = (("loop", loop), ("stack", stack), ("stats_loop", stats_loop), ("stats", stats_stack))
            wall, kern, got = {k: [] for k, _ in variants}, {k: [] for k, _ in variants}, {}
            for rep in range(a.reps + 1):  # the first round warms up and is not counted
                for name, fn in variants:
                    t0 = time.perf_counter()
                    got[name], ks = fn()
                    dt = time.perf_counter() - t0
                    if rep:
                        wall[name].append(1e3 * dt)
                        kern[name].append(ks)
            rel = np.abs(got["loop"] - got["stack"]).max() / got["loop"].max()
            print("-- M = %d planes; stack differs from the loop by %.1e of the peak" % (M, rel))
            print("   (a) loop of M bmo_psf_intensity    wall ms %10.2f   kernel ms %s" % (med(wall["loop"]), spread(kern["loop"])))
            print("   (b) bmo_psf_through_focus          wall ms %10.2f   kernel ms %s   (a) / (b) = %.2f"
                  % (med(wall["stack"]), spread(kern["stack"]), med(kern["loop"]) / med(kern["stack"])))
            print("   (c) loop of M bmo_psf_stats        wall ms %10.2f   kernel ms %s" % (med(wall["stats_loop"]), spread(kern["stats_loop"])))
            print("       bmo_psf_focus_stats            wall ms %10.2f   kernel ms %s   loop / call = %.2f"
                  % (med(wall["stats"]), spread(kern["stats"]), med(kern["stats_loop"]) / med(kern["stats"])), flush=True)
    finally:
        eng.free_result(res)
        eng.free_batch(dev)
        eng.close()


if __name__ == "__main__":
    main()

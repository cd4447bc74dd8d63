"""Through-focus and MTF read-out of sweeps: the batched entries of include/bmo_sweep_readout.h against a loop of single calls on the
same resident rows.
python tools/psf_focus_sweep_bench.py [--reps 5] [--shapes 64x1024,1024x1024,8x65536] [--n 64] [--planes 9] [--freqs 16]

The Airy KAT scene (tests/test_psf_readout.py airy_setup) swept through focus: K configurations, the PSFDetector moved along y from
-0.5 mm to +0.5 mm about the focus, detector-only (record_segments = 0).  Per shape K x rays and per read-out
  stats  bmo_psf_focus_stats     M planes
  stack  bmo_psf_through_focus   M planes, n x n samples
  geo    bmo_psf_geo_otf         M planes, nf frequencies
  otf    bmo_psf_otf             M planes, n x n samples, nf frequencies
  (a) loop    : K single calls on device pointers into the resident rows (bmo_result_device_hits plus the configuration's first row)
  (b) batched : the one _sweep call
(a) and (b) alternate in one process; medians of --reps rounds after one warm-up round, [min .. max]; kernel ms is the entries' kernel_ms
(summed over the loop), wall ms is time.perf_counter around the Python calls.  Every plane, axis and frequency is the same in (a) and (b);
whether all outputs agree bit for bit is printed, not asserted.  The yardstick is the loop (a) on the same build."""
import argparse
import ctypes as C
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

mm = 1e-3
cp = bmo.components


def spread(v):
    return "%9.3f [%9.3f .. %9.3f]" % (float(np.median(v)), min(v), max(v))


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if np.iscomplexobj(a):
        return same(a.real, b.real) and same(a.imag, b.imag)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def shape_part(a, K, rays):
    system, cs, psfd, lam, D = airy_setup(num_rays=rays)
    y0 = psfd.position()[1]

    def configure(c):
        bmo.translate_to3d(psfd, [0.0, y0 + (c / max(K - 1, 1) - 0.5) * 1.0 * mm, 0.0])

    t0 = time.perf_counter()
    sol = bmo.solve_sweep(system, cs, K, configure, record_segments=False)
    t_solve = time.perf_counter() - t0
    try:
        slot = sol._slot(psfd)
        p, cnt = C.POINTER(C.c_double)(), C.c_int64()
        abi.check(sol.lib, sol.lib.bmo_result_device_hits(sol._handle, slot, C.byref(p), C.byref(cnt)), "bmo_result_device_hits")
        ptr, H = C.cast(p, C.c_void_p).value or 0, cnt.value
        cfg = sol.res.node_root[sol.res.detector_nodes(slot)] // max(1, sol.n_roots)
        count = np.bincount(cfg, minlength=K)
        begin = np.concatenate([[0], np.cumsum(count)[:-1]])
        pos = np.ascontiguousarray([sol._poses[c][slot][0] for c in range(K)], dtype=np.float64)
        ori = np.ascontiguousarray([sol._poses[c][slot][1] for c in range(K)], dtype=np.float64)
        e1s, e2s, ys = (np.ascontiguousarray(ori[:, :, q]) for q in (0, 2, 1))
        M, n, nf = a.planes, a.n, a.freqs
        off = np.tile(np.linspace(-0.3 * mm, 0.3 * mm, M), (K, 1))
        disp = off[:, :, None] * ys[:, None, :]
        xs = zs = np.tile(np.linspace(-60e-6, 60e-6, n), (K, 1))
        freqs = cp.mtf_frequencies(1e5, nf, 30.0)
        print("== K = %d x %d rays: %d resident rows (%d .. %d per configuration), solve %.0f ms; M = %d planes, n = %d, nf = %d"
              % (K, rays, H, count.min(), count.max(), 1e3 * t_solve, M, n, nf), flush=True)

        def rows(c):
            return dict(device=0, hits_device_ptr=ptr + 72 * int(begin[c]), n_hits=int(count[c]))

        h = sol._handle
        readouts = {
            "stats": (lambda c: abi.psf_focus_stats(None, pos[c], e1s[c], e2s[c], ys[c], off[c], **rows(c)),
                      lambda: abi.psf_focus_stats_sweep(h, slot, K, pos, e1s, e2s, ys, off), 1),
            "stack": (lambda c: abi.psf_through_focus(None, pos[c], e1s[c], e2s[c], disp[c], xs[c], zs[c], **rows(c)),
                      lambda: abi.psf_through_focus_sweep(h, slot, K, pos, e1s, e2s, disp, xs, zs), 1),
            "geo": (lambda c: abi.psf_geo_otf(None, pos[c], e1s[c], e2s[c], ys[c], off[c], freqs, **rows(c)),
                    lambda: abi.psf_geo_otf_sweep(h, slot, K, pos, e1s, e2s, ys, off, freqs), 3),
            "otf": (lambda c: abi.psf_otf(None, pos[c], e1s[c], e2s[c], disp[c], xs[c], zs[c], freqs, **rows(c)),
                    lambda: abi.psf_otf_sweep(h, slot, K, pos, e1s, e2s, disp, xs, zs, freqs), 3),
        }
        for name, (single, batched, n_out) in readouts.items():
            k_a, k_b, w_a, w_b, agree = [], [], [], [], True
            for rep in range(a.reps + 1):  # the first round warms up and is not counted
                t0 = time.perf_counter()
                loop = [single(c) for c in range(K)]
                t1 = time.perf_counter()
                one = batched()
                t2 = time.perf_counter()
                if rep == 0:
                    agree = all(same(one[q][c], loop[c][q]) for c in range(K) for q in range(n_out))
                    continue
                k_a.append(sum(r[-1] for r in loop))
                k_b.append(one[-1])
                w_a.append(1e3 * (t1 - t0))
                w_b.append(1e3 * (t2 - t1))
            print("  %-5s kernel ms  (a) loop %s   (b) batched %s   a/b %6.2f   b - a %+9.3f (spread of a %.3f)"
                  % (name, spread(k_a), spread(k_b), np.median(k_a) / np.median(k_b), np.median(k_b) - np.median(k_a), max(k_a) - min(k_a)))
            print("  %-5s wall ms    (a) loop %s   (b) batched %s   a/b %6.2f   bit for bit: %s"
                  % (name, spread(w_a), spread(w_b), np.median(w_a) / np.median(w_b), agree), flush=True)
    finally:
        sol.close()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--shapes", default="64x1024,1024x1024,8x65536")
    p.add_argument("--n", type=int, default=64)
    p.add_argument("--planes", type=int, default=9)
    p.add_argument("--freqs", type=int, default=16)
    a = p.parse_args()
    for shape in a.shapes.split(","):
        K, rays = (int(v) for v in shape.split("x"))
        shape_part(a, K, rays)


if __name__ == "__main__":
    main()

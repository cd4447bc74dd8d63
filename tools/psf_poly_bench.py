"""Polychromatic read-out: the band split (discovery and stable partition) and the polychromatic stack of resident rows, against the
monochromatic stack of the same rows at the same n and M.
python tools/psf_poly_bench.py [--reps 5] [--rays 1048576] [--n 64] [--planes 1,16]

One process, the variants alternating within a round, medians of --reps rounds after one warm-up round, [min .. max] for kernel times.

The Airy KAT scene (tests/test_psf_readout.py airy_setup's lens, whose index does not depend on the wavelength, and detector) on a disc
bundle of 2^20 rays of three wavelengths (486, 546.1 and 656.3 nm) interleaved ray by ray, detector-only (record_segments = 0); the
PSFDetector is slot 0.  Every wave of the split's kernels therefore holds all three keys: the worst case of the ballot loops.
  (a) split/listed   : bmo_psf_bands_create with the three wave numbers given: the partition alone (count, scan, scatter);
  (b) split/discover : bmo_psf_bands_create with ks = NULL: the discovery pass and the partition; (b) - (a) is the discovery pass;
  (c) mono           : bmo_psf_through_focus of all rows, the coherent sum: what there was before;
  (d) poly           : bmo_psf_poly_through_focus on the handle: three band stacks and three combine launches;
  (e) poly + bands   : the same with out_band_intensity (a copy of every band's stack to the host).
(d) does the work of (c) on the same number of (row, point) pairs, in three calls of a third of the rows each; the split is paid once per
handle, whatever is read from it afterwards."""
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
LAMS = (486e-9, 546.1e-9, 656.3e-9)


def med(v):
    return float(np.median(v))


def spread(v):
    return "%9.3f [%8.3f .. %8.3f]" % (med(v), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--planes", default="1,16")
    a = ap.parse_args()
    print("library: %s" % os.path.basename(abi.ENGINE_PATH))
    system, cs, psfd, lam, D = airy_setup(num_rays=1)
    bundle = scenes.disc_bundle(a.rays, center=[0, -10 * mm, 0], direction=[0, 1, 0], diameter=D, lam=lam)
    bundle.planes[6] = np.asarray(LAMS)[np.arange(a.rays) % len(LAMS)]
    ks = [2 * 3.141592653589793 / l for l in LAMS]
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
        kw = dict(hits_device_ptr=ptr, n_hits=H)
        print("== %d rays of %d wavelengths interleaved, detector-only, slot 0 holds %d rows (%.1f MB resident); n = %d"
              % (a.rays, len(LAMS), H, H * 72 / 1e6, a.n), flush=True)

        def split(keys):
            b, ms = abi.psf_bands(None, ks=keys, want_ms=True, **kw)
            counts = b.counts.tolist()
            b.close()
            return counts, ms

        variants = (("listed", lambda: split(ks)), ("discover", lambda: split(None)))
        wall, kern, got = {k: [] for k, _ in variants}, {k: [] for k, _ in variants}, {}
        for rep in range(a.reps + 1):  # the first round warms up and is not counted
            for name, fn in variants:
                t0 = time.perf_counter()
                got[name], t = fn()
                dt = time.perf_counter() - t0
                if rep:
                    wall[name].append(1e3 * dt)
                    kern[name].append(t)
        assert sorted(got["listed"]) == sorted(got["discover"]) and sum(got["listed"]) == H
        print("-- the split: bands of %s rows" % got["listed"])
        print("   (a) bmo_psf_bands_create, ks listed    wall ms %10.2f   kernel ms %s" % (med(wall["listed"]), spread(kern["listed"])))
        print("   (b) bmo_psf_bands_create, discovery    wall ms %10.2f   kernel ms %s   discovery pass = (b) - (a) = %.3f ms"
              % (med(wall["discover"]), spread(kern["discover"]), med(kern["discover"]) - med(kern["listed"])), flush=True)
        split_ms = med(kern["discover"])

        bands = abi.psf_bands(None, ks=ks, **kw)
        try:
            S = np.array([abi.psf_focus_stats(None, pos, e1, e2, axis, [0.0], device=bands.device, hits_device_ptr=bands.rows(b)[0], n_hits=bands.rows(b)[1])[0][0, abi.FOCUS_S]
                          for b in range(len(bands))])
            coeffs = bmo.components.poly_coefficients(None, S)
            for M in [int(v) for v in a.planes.split(",")]:
                off = np.linspace(-0.5 * mm, 0.5 * mm, M) if M > 1 else np.array([0.25 * mm])
                d = off[:, None] * axis[None, :]

                def mono():
                    I, _, ms = abi.psf_through_focus(None, pos, e1, e2, d, xs, zs, **kw)
                    return I, ms

                def poly():
                    I, _, ms = abi.psf_poly_through_focus(bands, pos, e1, e2, d, xs, zs, coeffs)
                    return I, ms

                def poly_bands():
                    I, _, ms = abi.psf_poly_through_focus(bands, pos, e1, e2, d, xs, zs, coeffs, want_bands=True)
                    return I, ms

                variants = (("mono", mono), ("poly", poly), ("poly_bands", poly_bands))
                wall, kern, got = {k: [] for k, _ in variants}, {k: [] for k, _ in variants}, {}
                for rep in range(a.reps + 1):
                    for name, fn in variants:
                        t0 = time.perf_counter()
                        got[name], t = fn()
                        dt = time.perf_counter() - t0
                        if rep:
                            wall[name].append(1e3 * dt)
                            kern[name].append(t)
                assert np.array_equal(got["poly"], got["poly_bands"])
                print("-- M = %d planes, %d (row, point) pairs per plane" % (M, H * a.n * a.n))
                print("   (c) bmo_psf_through_focus, all rows    wall ms %10.2f   kernel ms %s" % (med(wall["mono"]), spread(kern["mono"])))
                print("   (d) bmo_psf_poly_through_focus         wall ms %10.2f   kernel ms %s   (d) / (c) = %.3f"
                      % (med(wall["poly"]), spread(kern["poly"]), med(kern["poly"]) / med(kern["mono"])))
                print("   (e) the same with out_band_intensity   wall ms %10.2f   kernel ms %s" % (med(wall["poly_bands"]), spread(kern["poly_bands"])))
                print("       the split (b) is %.2f %% of one monochromatic stack (c)" % (100 * split_ms / med(kern["mono"])), flush=True)
        finally:
            bands.close()
    finally:
        eng.free_result(res)
        eng.free_batch(dev)
        eng.close()


if __name__ == "__main__":
    main()

"""The polychromatic read-out restated in numpy (include/bmo.h "Polychromatic read-out"): the defining property of the band split, the
discovery of the bands, and the left-to-right combination of the bands' images.  Everything here is exact: the split copies rows, the
counts are integers, and the combination is the same two IEEE operations per band in the same order."""
import numpy as np

WAVELENGTHS = (486e-9, 546.1e-9, 656.3e-9)  # F, e and C lines


def wave_number(lam):
    """k as the engine writes it into column 8 (bmo_lane.hpp): 2 * 3.141592653589793 / lambda."""
    return 2 * 3.141592653589793 / lam


def band_split(rows, ks):
    """([rows of band b, in order, for every k_b of ks], unmatched): band b is rows[rows[:, 8] == k_b], a plain FP64 compare (a NaN equals
    nothing); unmatched counts the rows of no band."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 9)
    bands = [rows[rows[:, 8] == k] for k in ks]
    return bands, len(rows) - sum(len(b) for b in bands)


def discover(rows):
    """(ks ascending, counts, unmatched) of the discovery form: the distinct keys that are not NaN; only NaN rows are unmatched."""
    k = np.asarray(rows, dtype=np.float64).reshape(-1, 9)[:, 8]
    nan = np.isnan(k)
    ks, counts = np.unique(k[~nan], return_counts=True)
    return ks, counts.astype(np.int64), int(nan.sum())


def combine(coeffs, images):
    """acc = coeffs[0] * I_0, then acc = acc + coeffs[b] * I_b for b = 1 .. B - 1: one multiply and one add per band, in band order."""
    acc = np.float64(coeffs[0]) * np.asarray(images[0], dtype=np.float64)
    for b in range(1, len(coeffs)):
        acc = acc + np.float64(coeffs[b]) * np.asarray(images[b], dtype=np.float64)
    return acc


def synthetic_rows(band_of_row, ks, seed=20251003):
    """[H, 9] rows of seeded normal numbers whose column 8 is ks[band_of_row[h]] (ks may hold NaN): what the split needs of a row is its key."""
    band_of_row = np.asarray(band_of_row, dtype=np.int64)
    rows = np.random.Generator(np.random.PCG64(seed)).standard_normal((len(band_of_row), 9))
    rows[:, 8] = np.asarray(ks, dtype=np.float64)[band_of_row] if len(band_of_row) else 0.0
    return rows


def recolour(rows, lams=WAVELENGTHS, seed=7):
    """A copy of traced PSF rows with column 8 rewritten to the wave numbers of `lams`, assigned row by row by a seeded generator."""
    rows = np.array(rows, dtype=np.float64)
    pick = np.random.Generator(np.random.PCG64(seed)).integers(0, len(lams), len(rows))
    rows[:, 8] = np.array([wave_number(l) for l in lams])[pick]
    return rows


def bits(a):
    """The IEEE patterns of a real or complex array (a complex number as its two doubles), for bit-for-bit comparisons."""
    a = np.asarray(a)
    a = np.ascontiguousarray(a, dtype=np.complex128 if np.iscomplexobj(a) else np.float64)
    return a.view(np.float64).view(np.uint64)

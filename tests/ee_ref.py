"""Helpers of the encircled-energy read-out tests (not a test file): 40-digit evaluations written from the formulas of include/bmo.h
"Encircled-energy read-out" alone, and the error bounds of the engine's arithmetic, derived here and not fitted.

A point at (ax, az) from the centre has one key, and it is inside the half-size R iff key <= threshold:

    circle:  key = ax^2 + az^2,          threshold R^2          square:  key = max(|ax|, |az|),   threshold R

(the square's rule |ax| <= R and |az| <= R is the same statement).  The edge is closed.

1. geo_ee_exact: every row propagated exactly to the plane through o_m = origin + offsets[m] axis (mtf_ref.local_xz_exact), its (x, z) there
   less the centre (cx_m, cz_m) given as doubles, the exact key, the set of rows inside each exact threshold, the sum of their proj rounded
   once at the end, and S = sum proj.

2. image_ee_exact: the same for an image of doubles I[i, j] sampled at (xs[i], zs[j]) about one centre.

3. A compare has no error bound: a point whose exact key is closer to a threshold than the engine's key can be from the exact one may fall
   on either side.  undecided(keys, thresholds, D) lists those points; the tests choose radii for which there is none (radii_between puts a
   radius in the middle of a gap between neighbouring exact keys) and assert so, and that the nearest key is at least 1e3 D away, before
   they compare anything.  u = 2^-53.  D, the distance in key units within which the engine's compare is not decided:

   Geometric.  The engine's x and z of a row and plane are within E_row = u kappa^2 (12 L + 36 R) of the exact ones (focus_ref, "The
   statistics").  ax^ = fl(x^ - cx) adds u |ax^|: with A the largest exact |ax| or |az| of the plane and A' = A + E_row,
       e_a = E_row + u A' (1 + u)           bounds |ax^ - ax| and |az^ - az|.
     square:  max(|ax^|, |az^|) is within e_a of max(|ax|, |az|), and the threshold R is the double itself:       D = e_a.
     circle:  |ax^ ax^ - ax ax| <= 2 A e_a + e_a^2, the same for az: 4 A e_a + 2 e_a^2;
              the two squares round by u each of themselves: u (ax^^2 + az^^2) <= 2 u A'^2;
              their sum rounds by u of itself: 2 u A'^2 (1 + u);
              the threshold fl(R R) is within u R^2 of the exact R^2:
                                                                 D = 4 A e_a + 2 e_a^2 + 4 u A'^2 (1 + u) + u R^2.
   Image.  xs[i], zs[j] and the centre are doubles the exact evaluator takes as they are, so only the last three apply: E_row = 0,
       e_a = u A (1 + u);   square: D = e_a;   circle: D = 4 A e_a + 2 e_a^2 + 4 u A^2 (1 + u) + u R^2.
   D is applied with a factor (1 + 1e-9), which covers the second-order terms dropped above (they are below 1e-15 of the first-order ones).

4. The bounds, once no point is undecided (the engine and the exact evaluator then sum over the same set).  gamma_k = k u / (1 - k u).
     count:   equal.
     energy:  a sum of the H' <= H proj inside in some order, each passing at most H - 1 additions (a row outside adds +0.0, exactly
              nothing):  gamma_{H-1} sum |proj inside| + u |exact| for the rounding of the exact value to a double   (energy_bound)
     sums:    gamma_{H-1} S.
     ee:      fl(energy^ / S^): the quotient u, S^ within gamma_{H-1}:
              energy_bound / S + (gamma_{H-1} + 2 u) ee (1 + 1e-9)                                                    (ee_bound)
     image:   two nested sequential sums of n terms each: gamma_{2n} in place of gamma_{H-1}, for energy, sums and ee alike.
"""
import numpy as np

import focus_ref as fr
import mtf_ref as mr

U = fr.U
CIRCLE, SQUARE = 0, 1

# planted mistakes of the exact evaluators (tests/test_ee_ref.py shows that each misses a known answer by far more than a bound)
MISTAKES = ("r_for_r2", "open_edge", "n_for_s", "square_one_axis", "center_ignored")


def _mpf(mp, v):
    return mp.mpf(float(v))  # a double is a dyadic rational: mpf(float) is exact


def _key(mp, ax, az, shape, mistake):
    if shape == CIRCLE:
        return ax * ax + az * az
    return abs(ax) if mistake == "square_one_axis" else max(abs(ax), abs(az))


def thresholds_exact(radii, shape, mistake=None):
    """[mpf per radius]: R^2 (circle) or R (square) of the doubles `radii`, exact; call it inside mp.workdps(40)."""
    import mpmath as mp

    r = [_mpf(mp, v) for v in np.asarray(radii, dtype=np.float64).reshape(-1)]
    return [v * v for v in r] if shape == CIRCLE and mistake != "r_for_r2" else r


def _inside(key, thr, mistake):
    return key < thr if mistake == "open_edge" else key <= thr


def _sums(mp, keys, weights, thr, mistake):
    """(count, energy rounded once, sum |w| inside) of the points with `keys` and `weights` inside each threshold."""
    count, energy, mass = [], [], []
    for t in thr:
        sel = [w for k, w in zip(keys, weights) if _inside(k, t, mistake)]
        count.append(len(sel))
        energy.append(float(len(sel)) if mistake == "n_for_s" else float(mp.fsum(sel)))
        mass.append(float(mp.fsum(abs(w) for w in sel)))
    return count, energy, mass


def geo_ee_exact(hits, origin, e1, e2, axis, offsets, radii, centers=None, shape=CIRCLE, mistake=None, xz=None):
    """The exact geometric encircled energy: a dict of
         keys [M][H] mpf (exact keys), thr [nr] mpf (exact thresholds), count [M, nr] int, energy [M, nr] (each rounded once),
         mass [M, nr] (sum |proj| inside), S (sum proj), ee [M, nr] (energy / S at 40 digits), A [M] (the largest |ax| or |az| of a plane).
    xz: mtf_ref.local_xz_exact of the same rows, pose, axis and offsets, where a test evaluates them more than once."""
    import mpmath as mp

    assert mistake is None or mistake in MISTAKES
    h = np.asarray(hits, dtype=np.float64).reshape(-1, 9)
    off = np.asarray(offsets, dtype=np.float64).reshape(-1)
    r = np.asarray(radii, dtype=np.float64).reshape(-1)
    cen = np.zeros((len(off), 2)) if centers is None or mistake == "center_ignored" else np.asarray(centers, dtype=np.float64).reshape(len(off), 2)
    out = dict(keys=[], count=np.zeros((len(off), len(r)), dtype=np.int64), energy=np.zeros((len(off), len(r))), mass=np.zeros((len(off), len(r))),
               ee=np.zeros((len(off), len(r))), A=[])
    with mp.workdps(40):
        w = [_mpf(mp, v) for v in h[:, 7]]
        s_exact = mp.fsum(w)
        out["S"] = float(s_exact)
        out["thr"] = thresholds_exact(r, shape, mistake)
        for m, plane in enumerate(mr.local_xz_exact(h, origin, e1, e2, axis, off) if xz is None else xz):
            cx, cz = _mpf(mp, cen[m, 0]), _mpf(mp, cen[m, 1])
            axz = [(x - cx, z - cz) for x, z in plane]
            keys = [_key(mp, a, b, shape, mistake) for a, b in axz]
            out["keys"].append(keys)
            out["A"].append(float(max([max(abs(a), abs(b)) for a, b in axz] or [0])))
            out["count"][m], out["energy"][m], out["mass"][m] = _sums(mp, keys, w, out["thr"], mistake)
            with np.errstate(invalid="ignore", divide="ignore"):
                out["ee"][m] = [float(mp.mpf(e) / s_exact) if s_exact != 0 else np.nan for e in out["energy"][m]]
    return out


def image_ee_exact(I, xs, zs, center, radii, shape=CIRCLE, mistake=None):
    """The same for the image I[i, j] of doubles at (xs[i], zs[j]) about center = (cx, cz): keys is a flat list in the order [i * n + j],
    S the sum of the image, A one number; centroid = (cx, cz) of the image's intensity centroid as floats of 40-digit values."""
    import mpmath as mp

    assert mistake is None or mistake in MISTAKES
    img = np.asarray(I, dtype=np.float64)
    assert img.shape == (len(xs), len(zs))
    r = np.asarray(radii, dtype=np.float64).reshape(-1)
    c = (0.0, 0.0) if mistake == "center_ignored" else center
    with mp.workdps(40):
        x, z = [_mpf(mp, v) for v in xs], [_mpf(mp, v) for v in zs]
        cx, cz = _mpf(mp, c[0]), _mpf(mp, c[1])
        w = [_mpf(mp, img[i, j]) for i in range(len(x)) for j in range(len(z))]
        axz = [(x[i] - cx, z[j] - cz) for i in range(len(x)) for j in range(len(z))]
        keys = [_key(mp, a, b, shape, mistake) for a, b in axz]
        thr = thresholds_exact(r, shape, mistake)
        count, energy, mass = _sums(mp, keys, w, thr, mistake)
        s_exact = mp.fsum(w)
        ee = [float(mp.mpf(e) / s_exact) if s_exact != 0 else np.nan for e in energy]
        centroid = (np.nan, np.nan)
        if s_exact != 0:
            centroid = (float(mp.fsum(w[i * len(z) + j] * x[i] for i in range(len(x)) for j in range(len(z))) / s_exact),
                        float(mp.fsum(w[i * len(z) + j] * z[j] for i in range(len(x)) for j in range(len(z))) / s_exact))
        return dict(keys=keys, thr=thr, count=np.array(count, dtype=np.int64), energy=np.array(energy), mass=np.array(mass), S=float(s_exact), ee=np.array(ee),
                    A=float(max([max(abs(a), abs(b)) for a, b in axz] or [0])), centroid=centroid,
                    mx=float(mp.fsum(abs(w[i * len(z) + j] * x[i]) for i in range(len(x)) for j in range(len(z)))),
                    mz=float(mp.fsum(abs(w[i * len(z) + j] * z[j]) for i in range(len(x)) for j in range(len(z)))))


# ------------------------------------------------------------------------------------------------ the compares
def d_key(A, radius, shape, e_row=0.0):
    """D of the module docstring for one plane (A: its largest |ax| or |az|; e_row: focus_ref's E_row, 0 for an image) and one radius."""
    a1 = A + e_row
    e_a = e_row + U * a1 * (1 + U)
    if shape == SQUARE:
        return e_a
    return 4 * A * e_a + 2 * e_a * e_a + 4 * U * a1 * a1 * (1 + U) + U * float(radius) ** 2


def gaps(keys, thr):
    """[float per threshold]: the distance from each exact threshold to the nearest exact key (inf without keys)."""
    return [float(min([abs(k - t) for k in keys] or [float("inf")])) for t in thr]


def undecided(keys, thr, D):
    """[(point, radius), ...]: the points whose exact key lies within D (one number, or one per threshold) of an exact threshold."""
    d = np.broadcast_to(np.asarray(D, dtype=np.float64), (len(thr),))
    return [(p, q) for q, t in enumerate(thr) for p, k in enumerate(keys) if abs(k - t) <= d[q] * (1 + 1e-9)]


def radii_between(keys, quantiles, shape, reach=8):
    """One radius (a double) per quantile, in the middle of a gap between neighbouring exact radii: of the sorted distinct radii of the points (the
    root of a circle's key, a square's key itself) the gap at the quantile's place or one of the `reach` gaps either side, whichever is
    widest.  Call it with the keys of every plane the radii are to serve, pooled."""
    import mpmath as mp

    with mp.workdps(40):
        r = sorted(set(mp.sqrt(k) if shape == CIRCLE else k for k in keys))  # distinct radii: the samples of an image share many
        assert len(r) >= 2
        out = []
        for q in quantiles:
            i = min(max(int(float(q) * (len(r) - 1)), 0), len(r) - 2)
            lo, hi = max(i - reach, 0), min(i + reach, len(r) - 2)
            j = max(range(lo, hi + 1), key=lambda t: r[t + 1] - r[t])
            out.append(float((r[j] + r[j + 1]) / 2))
    return np.array(out)


# ------------------------------------------------------------------------------------------------ the bounds
def energy_bound(n_terms, mass, exact):
    """|energy - exact| for a sum whose terms pass at most n_terms additions (H - 1 for rows, 2 n for an image)."""
    return fr.gamma(max(n_terms, 1)) * mass + U * abs(exact)


def ee_bound(n_terms, mass, exact_energy, s, ee):
    return (energy_bound(n_terms, mass, exact_energy) / s + (fr.gamma(max(n_terms, 1)) + 2 * U) * abs(ee)) * (1 + 1e-9)


def centroid_bound(n, moment_mass, s, c):
    """|c^ - c| of an image's intensity centroid c^ = fl((sum_j sum_i fl(I x)) / S^), n samples a side: the products round by u and pass
    2 n additions (gamma_{2n+1} of moment_mass = sum |I x|), S^ is within gamma_{2n}, the quotient rounds by u; u |c| for the exact value
    given as a double."""
    return (fr.gamma(2 * n + 1) * moment_mass / s + (fr.gamma(2 * n) + U) * abs(c)) * (1 + 1e-9) + U * abs(c)


# ------------------------------------------------------------------------------------------------ scenes with known answers
def fibonacci_disc_rows(H, a, center=(0.0, 0.0), proj=0.5):
    """[H, 9] rows that hit the plane y = 0 on a Fibonacci disc of radius a about `center` (local x, z = world x, z with the frame
    e1 = (1, 0, 0), e2 = (0, 0, 1), origin 0), all along +y with the weight `proj`: a uniformly weighted disc."""
    i = np.arange(H, dtype=np.float64)
    rad, phi = a * np.sqrt((i + 0.5) / H), i * (np.pi * (3.0 - np.sqrt(5.0)))
    rows = np.zeros((H, 9))
    rows[:, 0], rows[:, 2] = center[0] + rad * np.cos(phi), center[1] + rad * np.sin(phi)
    rows[:, 4], rows[:, 7], rows[:, 8] = 1.0, proj, 2 * np.pi / 1e-6
    return rows


FLAT_FRAME = (np.zeros(3), np.array([1.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.0]))  # nrm = e1 x e2 = (0, -1, 0)
FLAT_AXIS = np.array([0.0, 1.0, 0.0])

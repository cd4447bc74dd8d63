"""Encircled-energy read-out on the GPU: bmo_psf_geo_ee against the 40-digit evaluation of the propagated rows, bmo_psf_ee against the 40-digit
sums of the image the same call returned, bmo_spot_ee against numpy's evaluation of the same FP64 expressions, the bit-for-bit identities they
promise, and the Python layer.  A compare has no error bound, so every comparing test first shows on the exact evaluator that no point lies
within the decision distance D of a threshold (tests/ee_ref.py derives D and the bounds; nothing is fitted)."""
import numpy as np
import pytest

import bmo_amd as bmo
from bmo_amd import abi
import ee_ref as er
import focus_ref as fr
import mtf_ref as mr
import spot_ref as sr
from test_focus_gpu import MP, _axes, _oblique, _solve

pytestmark = pytest.mark.gpu

mm = 1e-3
H_ALL = 5000
QUANTILES = (0.1, 0.3, 0.5, 0.75, 0.95)
SHAPES = (("circle", er.CIRCLE), ("square", er.SQUARE))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.fixture(scope="module")
def case():
    """tilted_psf_case at 5000 rays solved once; a test of fewer rows takes the first of them."""
    ns, per = sr.spot_splits(H_ALL)
    assert ns == 3 and (H_ALL - 2 * per) % 256 != 0  # three splits, the third ends in a ragged tile
    rows, pose, o = _solve(H_ALL)
    assert np.all(np.abs(pose[1]) > 1e-3) and np.all(np.abs(pose[2]) > 1e-3) and (rows[:, 3:6] != 0).all()
    return rows, pose, o


def _axis(pose):
    return np.cross(pose[1], pose[2]) + 0.05 * pose[1] - 0.03 * pose[2]  # oblique to the planes, no zero component


def geo_inputs(rows, pose, axis, offsets, centers, quantiles=QUANTILES):
    """What a comparing test of the geometric kind needs of the exact evaluator, computed once: the propagated rows, the focus statistics'
    scales, and per shape the radii that radii_between puts between the pooled exact keys of the planes."""
    import mpmath as mp

    with mp.workdps(40):
        xz = mr.local_xz_exact(rows, *pose, axis, offsets)
    e_rows = [mr.e_row(ex) for ex in fr.focus_stats_exact(rows, *pose, axis, offsets)]
    radii = {}
    for name, shape in SHAPES:
        keys = er.geo_ee_exact(rows, *pose, axis, offsets, [], centers=centers, shape=shape, xz=xz)["keys"]
        radii[name] = er.radii_between([k for plane in keys for k in plane], quantiles, shape)
    return xz, e_rows, radii


def check_decided(ex, radii, shape, e_rows, what):
    """The condition on the inputs: on the exact evaluator no point is within D of a threshold, and the nearest is at least 1e3 D away."""
    for m, keys in enumerate(ex["keys"]):
        D = [er.d_key(ex["A"][m], R, shape, e_rows[m] if e_rows else 0.0) for R in radii]
        gap = er.gaps(keys, ex["thr"])
        print("%s plane %d: D %s, nearest key at %s" % (what, m, ["%.2e" % d for d in D], ["%.2e" % g for g in gap]))
        assert er.undecided(keys, ex["thr"], D) == [], (what, m)
        assert all(g >= 1e3 * d for g, d in zip(gap, D)), (what, m)


def check_geo(rows, pose, axis, offsets, centers, radii, name, shape, got, planes, xz=None, e_rows=None):
    """Planes `planes` of got = (ee, energy, count, sums) against the exact evaluator: count equal, energy, ee and sums inside the bounds."""
    ee, energy, count, sums = got
    off, cen = np.asarray(offsets)[planes], None if centers is None else np.asarray(centers)[planes]
    ex = er.geo_ee_exact(rows, *pose, axis, off, radii, centers=cen, shape=shape, xz=None if xz is None else [xz[m] for m in planes])
    if e_rows is None:
        e_rows = [mr.e_row(s) for s in fr.focus_stats_exact(rows, *pose, axis, off)]
    else:
        e_rows = [e_rows[m] for m in planes]
    check_decided(ex, radii, shape, e_rows, name)
    H = len(rows)
    for a, m in enumerate(planes):
        assert abs(sums[m] - ex["S"]) <= fr.gamma(max(H - 1, 1)) * ex["S"]
        assert np.array_equal(count[m], ex["count"][a]), (name, m, count[m], ex["count"][a])
        for q in range(len(radii)):
            be = er.energy_bound(H - 1, ex["mass"][a, q], ex["energy"][a, q])
            bq = er.ee_bound(H - 1, ex["mass"][a, q], ex["energy"][a, q], ex["S"], ex["ee"][a, q]) + fr.U * ex["ee"][a, q]
            print("%s H = %d plane %d R = %.4e: count %d, energy error %.2e bound %.2e, ee %.6f error %.2e bound %.2e"
                  % (name, H, m, radii[q], count[m, q], abs(energy[m, q] - ex["energy"][a, q]), be, ee[m, q], abs(ee[m, q] - ex["ee"][a, q]), bq))
            assert abs(energy[m, q] - ex["energy"][a, q]) <= be, (name, m, q)
            assert abs(ee[m, q] - ex["ee"][a, q]) <= bq < 3 * (H + 2) * fr.U, (name, m, q)  # the bound has teeth: two gamma_{H-1} and a few u
    return ex


def test_geometric_against_the_exact_sets():
    """H = 600, three planes along an oblique axis, five radii between the pooled exact keys, both shapes, about each plane's centroid."""
    rows, pose, o = _solve(600)
    axis, offsets = _axis(pose), np.array([-0.4 * mm, 0.07 * mm, 0.5 * mm])
    st, _ = abi.psf_focus_stats(rows, *pose, axis, offsets)
    centers = st[:, [fr.CX, fr.CZ]]
    xz, e_rows, radii = geo_inputs(rows, pose, axis, offsets, centers)
    for name, shape in SHAPES:
        got = abi.psf_geo_ee(rows, *pose, axis, offsets, radii[name], centers=centers, shape=name)
        assert got[0].shape == got[1].shape == got[2].shape == (3, 5) and got[3].shape == (3,) and got[4] > 0
        ex = check_geo(rows, pose, axis, offsets, centers, radii[name], name, shape, got[:4], [0, 1, 2], xz, e_rows)
        assert np.array_equal(_bits(got[3]), _bits(st[:, fr.S]))
        assert np.abs(got[0][0] - got[0][1]).max() > 1e-3 and 0 < ex["count"].min() and ex["count"].max() < 600  # the planes differ by far more than a bound
        assert np.array_equal(_bits(abi.psf_geo_ee(rows, *pose, axis, offsets, radii[name], centers=centers, shape=name, want_count=False)[1]), _bits(got[1]))
    # without centres the energy is counted about each plane's origin
    bare = abi.psf_geo_ee(rows, *pose, axis, offsets, radii["circle"])
    assert np.abs(bare[0] - abi.psf_geo_ee(rows, *pose, axis, offsets, radii["circle"], centers=centers)[0]).max() > 1e-3
    assert np.array_equal(_bits(bare[0]), _bits(abi.psf_geo_ee(rows, *pose, axis, offsets, radii["circle"], centers=np.zeros((3, 2)))[0]))


@pytest.mark.parametrize("H", [0, 1, 256, 257])
def test_geometric_edge_row_counts(case, H):
    """No rows, one row, exactly one tile, one tile and a row; about each plane's origin."""
    rows, pose, o = case
    rows, axis, offsets = rows[:H], _axis(pose), np.array([0.0, 0.3 * mm])
    if H == 0:
        ee, energy, count, sums, _ = abi.psf_geo_ee(rows, *pose, axis, offsets, [1e-4, 0.0, 1.0])
        assert ee.shape == (2, 3) and np.isnan(ee).all() and not energy.any() and not count.any() and not sums.any()
        return
    for name, shape in SHAPES:
        keys = er.geo_ee_exact(rows, *pose, axis, offsets, [], shape=shape)["keys"]
        pooled = sorted(float(k) ** (0.5 if shape == er.CIRCLE else 1.0) for plane in keys for k in plane)
        radii = np.array([0.5 * pooled[0], 2 * pooled[-1]]) if H == 1 else er.radii_between([k for plane in keys for k in plane], (0.2, 0.6, 0.9), shape)
        got = abi.psf_geo_ee(rows, *pose, axis, offsets, radii, shape=name)
        check_geo(rows, pose, axis, offsets, None, radii, name, shape, got[:4], [0, 1])
        if H == 1:
            assert got[0].tolist() == [[0.0, 1.0]] * 2 and got[2].tolist() == [[0, 1]] * 2 and got[1][0, 1] == rows[0, 7] == got[3][0]


def test_geometric_three_splits_the_third_ragged(case):
    """H = 5000: splits of 1792, 1792 and 1416 rows; nine planes (a second, partial chunk), the first and the last of them against the
    exact sets; S equals the focus statistics' bit for bit."""
    rows, pose, o = case
    axis, offsets = _axis(pose), np.linspace(-0.5 * mm, 0.5 * mm, 9)
    st, _ = abi.psf_focus_stats(rows, *pose, axis, offsets)
    centers = st[:, [fr.CX, fr.CZ]]
    planes = [0, 8]
    xz, e_rows, radii = geo_inputs(rows, pose, axis, offsets[planes], centers[planes], quantiles=(0.1, 0.5, 0.95))
    xz9, e9 = [xz[0]] + [None] * 7 + [xz[1]], [e_rows[0]] + [None] * 7 + [e_rows[1]]
    for name, shape in SHAPES:
        got = abi.psf_geo_ee(rows, *pose, axis, offsets, radii[name], centers=centers, shape=name)
        check_geo(rows, pose, axis, offsets, centers, radii[name], name, shape, got[:4], planes, xz9, e9)
        assert np.array_equal(_bits(got[3]), _bits(st[:, fr.S]))


@pytest.mark.parametrize("nr,M", [(1, 1), (255, 1), (257, 1), (51, 5), (1, 257)])
def test_geometric_pair_blocks(case, nr, M):
    """n_radii * M = 1, 255, 257: a partial block of pairs and a second one, by radii and by planes.  Every pair of a sample bit for bit what
    a call for it alone returns (the order of a pair's sum does not depend on the pairs asked for along with it)."""
    rows, pose, o = case
    rows, axis = rows[:300], _axis(pose)
    offsets = np.linspace(-0.5 * mm, 0.5 * mm, M) if M > 1 else np.array([0.2 * mm])
    st, _ = abi.psf_focus_stats(rows, *pose, axis, offsets)
    centers = st[:, [fr.CX, fr.CZ]]
    radii = st[:, fr.MAX_R].max() * (0.03 + 1.1 * ((np.arange(nr) * 7) % nr + 0.5) / nr)  # scrambled, the largest holds every row
    assert nr * M in (1, 255, 257)
    for name, shape in SHAPES:
        ee, energy, count, sums, _ = abi.psf_geo_ee(rows, *pose, axis, offsets, radii, centers=centers, shape=name)
        assert ee.shape == (M, nr) and np.isfinite(ee).all() and count.max() <= 300 and (nr == 1 or (count.max() == 300 and count.min() < 150))
        for m in sorted({0, M // 2, M - 1}):
            for q in sorted({0, nr // 3, nr - 2 if nr > 1 else 0, nr - 1}):
                one = abi.psf_geo_ee(rows, *pose, axis, offsets[m:m + 1], radii[q:q + 1], centers=centers[m:m + 1], shape=name)
                for a, b in zip(one[:4], (ee[m, q:q + 1], energy[m, q:q + 1], count[m, q:q + 1], sums[m:m + 1])):
                    assert np.array_equal(np.ravel(a).view(np.uint64), np.ravel(b).view(np.uint64)), (name, m, q)


@pytest.mark.parametrize("record", [True, False])
def test_geometric_subsets_and_resident_rows_bit_for_bit(record):
    """A subset of planes and radii in scrambled order equals the full call; resident rows equal host rows, after a solve with the segment
    log and after a detector-only one."""
    rows, pose, o, (eng, dev, res, bundle) = _solve(2100, record=record, keep=True)
    sol = bmo.system.EngineSolution(eng.lib, res, bundle.n, bundle.kind)
    try:
        axis, offsets = _axis(pose), np.linspace(-0.5 * mm, 0.5 * mm, 11)
        st, _ = abi.psf_focus_stats(rows, *pose, axis, offsets)
        cen = st[:, [fr.CX, fr.CZ]]
        radii = st[:, fr.MAX_R].min() * np.array([0.9, 0.1, 0.35, 0.6, 0.2])
        for name, _ in SHAPES:
            full = abi.psf_geo_ee(rows, *pose, axis, offsets, radii, centers=cen, shape=name)
            assert np.array_equal(_bits(full[3]), _bits(st[:, fr.S])) and 0 < full[2].min() and full[2].max() < 2100
            ps, rs = [9, 0, 4], [3, 1]
            part = abi.psf_geo_ee(rows, *pose, axis, offsets[ps], radii[rs], centers=cen[ps], shape=name)
            for a, b in zip(part[:4], (full[0][np.ix_(ps, rs)], full[1][np.ix_(ps, rs)], full[2][np.ix_(ps, rs)], full[3][ps])):
                assert np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))
            ptr, cnt, d = sol._psf_resident_rows(0)
            assert cnt == 2100
            resident = abi.psf_geo_ee(None, *pose, axis, offsets, radii, centers=cen, shape=name, device=d, hits_device_ptr=ptr, n_hits=cnt)
            for a, b in zip(resident[:4], full[:4]):
                assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    finally:
        sol.handle = None  # the engine frees the result
        eng.free_result(res)
        eng.free_batch(dev)
        eng.close()


def test_geometric_row_parallel_to_the_planes_reads_nan(case):
    rows, pose, o = case
    flat = rows[:300].copy()
    flat[7, 3:6] = [1.0, 0.0, 0.0]
    frame = (pose[0], np.array([1.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.0]))  # nrm = (0, -1, 0): row 7 runs in the plane
    radii = [5e-4, 1e-3, 1.0]
    ee, energy, count, sums, _ = abi.psf_geo_ee(flat, *frame, [0.0, 1.0, 0.0], [0.0, 1e-4], radii)
    assert np.isnan(ee).all() and np.isnan(energy).all() and np.isnan(sums).all()
    rest = abi.psf_geo_ee(np.delete(flat, 7, axis=0), *frame, [0.0, 1.0, 0.0], [0.0, 1e-4], radii)
    assert np.isfinite(rest[0]).all() and np.array_equal(count, rest[2]) and (count[:, 2] == 299).all()  # the plain count: the row in the plane is outside
    nanproj = flat.copy()
    nanproj[7] = rows[7]
    nanproj[9, 7] = np.nan
    ee, energy, count, sums, _ = abi.psf_geo_ee(nanproj, *frame, [0.0, 1.0, 0.0], [0.0, 1e-4], radii)
    assert np.isnan(ee).all() and np.isnan(energy).all() and np.isnan(sums).all() and (count[:, 2] == 300).all()


def test_geometric_closed_edge_exactly():
    """Rows along +y on the plane y = 0 keep their (x, z) exactly.  (3, 4) units lies ON the circle of 5 units and ON the square of 4 units;
    its neighbours stand one ulp either side in x or in z.  The weights are powers of two, so the energy names the rows inside."""
    B = 2.0 ** -10
    up, dn = (lambda v: float(np.nextafter(v, np.inf))), (lambda v: float(np.nextafter(v, -np.inf)))
    pts = [(3 * B, 4 * B), (up(3 * B), 4 * B), (3 * B, up(4 * B)), (dn(3 * B), 4 * B), (3 * B, dn(4 * B))]
    rows = np.zeros((5, 9))
    for q, (r, (x, z)) in enumerate(zip(rows, pts)):
        r[:] = [x, 0.0, z, 0.0, 1.0, 0.0, 1.0, 2.0 ** q, 2 * np.pi / 1e-6]
    frame = (np.zeros(3), np.array([1.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.0]))
    x, z = rows[:, 0], rows[:, 2]
    for name, R, inside in (("circle", 5 * B, x * x + z * z <= (5 * B) * (5 * B)), ("square", 4 * B, (np.abs(x) <= 4 * B) & (np.abs(z) <= 4 * B))):
        ee, energy, count, sums, _ = abi.psf_geo_ee(rows, *frame, [0.0, 1.0, 0.0], [0.0], [R], shape=name)
        assert inside[0] and not inside[2] and (name == "square" or not inside[1])  # the row on the edge counts, the outer neighbours do not
        assert energy[0, 0] == rows[inside, 7].sum() and count[0, 0] == inside.sum() and sums[0] == 31.0 and ee[0, 0] == energy[0, 0] / 31.0, name
        assert int(energy[0, 0]) & 1 == 1 and int(energy[0, 0]) & 4 == 0
    assert abi.psf_geo_ee(rows, *frame, [0.0, 1.0, 0.0], [0.0], [dn(5 * B)], shape="circle")[2][0, 0] < 5


# ------------------------------------------------------------------------------------------------ diffraction
@pytest.mark.parametrize("n,M", [(5, 1), (17, 1), (5, MP + 1), (17, MP + 1)])
def test_diffraction_sums_of_the_stack(case, n, M):
    """The image equals bmo_psf_through_focus bit for bit; the energies against the exact sums of that image about given centres; the
    intensity centroid and its round trip; a radius that covers the window reads the plane's sum.  n = 5: one partial block of points;
    n = 17: a second one; M = MP + 1 crosses the chunk of the stack."""
    rows, pose, o = case
    rows = rows[:600]
    xs, zs = _axes(rows, pose, o, n)
    d = _oblique(pose, M)
    px, pz = xs[1] - xs[0], zs[1] - zs[0]
    cen = np.stack([xs.mean() + px * (0.137 + 0.05 * np.arange(M)), zs.mean() - pz * (0.211 + 0.03 * np.arange(M))], axis=1)
    cover = 2 * (xs[-1] - xs[0] + zs[-1] - zs[0])  # a circle and a square that hold every sample about any centre inside the window
    I0 = abi.psf_through_focus(rows, *pose, d, xs, zs)[0]
    planes = sorted({0, M - 1, M // 2})
    for name, shape in SHAPES:
        keys = [k for m in planes for k in er.image_ee_exact(I0[m], xs, zs, cen[m], [], shape=shape)["keys"]]
        radii = np.append(er.radii_between(keys, (0.1, 0.4, 0.7), shape, reach=2), cover)
        ee, energy, sums, cout, I, ms = abi.psf_ee(rows, *pose, d, xs, zs, radii, centers=cen, shape=name, want_intensity=True)
        assert ee.shape == energy.shape == (M, 4) and sums.shape == (M,) and I.shape == (M, n, n) and ms > 0
        assert np.array_equal(_bits(I), _bits(I0)) and np.array_equal(_bits(cout), _bits(cen))
        assert np.array_equal(_bits(energy[:, 3]), _bits(sums)) and (ee[:, 3] == 1.0).all() and (ee[:, :3] < 1.0).all()
        for m in planes:
            ex = er.image_ee_exact(I[m], xs, zs, cen[m], radii, shape=shape)
            check_decided(dict(keys=[ex["keys"]], A=[ex["A"]], thr=ex["thr"]), radii, shape, None, "%s n = %d plane %d" % (name, n, m))
            assert abs(sums[m] - ex["S"]) <= fr.gamma(2 * n) * ex["S"]
            for q in range(4):
                be = er.energy_bound(2 * n, ex["mass"][q], ex["energy"][q])
                bq = er.ee_bound(2 * n, ex["mass"][q], ex["energy"][q], ex["S"], ex["ee"][q]) + fr.U * ex["ee"][q]
                assert abs(energy[m, q] - ex["energy"][q]) <= be < 1e-13 * ex["S"], (name, m, q)
                assert abs(ee[m, q] - ex["ee"][q]) <= bq, (name, m, q)
        # the intensity centroid, and its round trip
        auto = abi.psf_ee(rows, *pose, d, xs, zs, radii, shape=name)
        for m in planes:
            ex = er.image_ee_exact(I[m], xs, zs, (0.0, 0.0), [], shape=shape)
            for c, want, mass in ((auto[3][m, 0], ex["centroid"][0], ex["mx"]), (auto[3][m, 1], ex["centroid"][1], ex["mz"])):
                assert abs(c - want) <= er.centroid_bound(n, mass, ex["S"], want) < 1e-12 * (xs[-1] - xs[0]), (name, m)
        assert np.array_equal(_bits(auto[2]), _bits(sums)) and xs[0] < auto[3][:, 0].min() and auto[3][:, 0].max() < xs[-1]
        back = abi.psf_ee(rows, *pose, d, xs, zs, radii, centers=auto[3], shape=name)
        for a, b in zip(back[:4], auto[:4]):
            assert np.array_equal(_bits(a), _bits(b)), name
    none = abi.psf_ee(rows[:0], *pose, d, xs, zs, [1e-5, 1.0], want_intensity=True)
    assert np.isnan(none[0]).all() and not none[1].any() and not none[2].any() and np.isnan(none[3]).all() and not none[4].any()
    assert np.array_equal(abi.psf_ee(rows[:0], *pose, d, xs, zs, [1e-5], centers=cen)[3], cen)


# ------------------------------------------------------------------------------------------------ spot
def _spot_numpy(rows, center, radii, shape):
    """The counts by the header's FP64 expressions in elementwise numpy (IEEE, one rounding per operation, no contraction)."""
    ax, az = rows[:, 0] - center[0], rows[:, 1] - center[1]
    if shape == "circle":
        r2 = ax * ax + az * az
        return np.array([int((r2 <= R * R).sum()) for R in radii], dtype=np.int64)
    return np.array([int(((np.abs(ax) <= R) & (np.abs(az) <= R)).sum()) for R in radii], dtype=np.int64)


def _spot_rows(H, cols=2, seed=3):
    rng = np.random.default_rng(seed)
    r = rng.standard_normal((H, cols))
    r[:, 0], r[:, 1] = 2e-4 + 1e-4 * r[:, 0], -1e-4 + 2e-4 * r[:, 1]
    if H > 2:
        r[1, 0] = r[2, 1] = np.nan  # outside every radius, by x or by z alone
    return r


SPOT_CENTER = (2.1e-4, -0.8e-4)


def _spot_radii(rows):
    """Scrambled, with a duplicate, zero, a radius that holds every row, and radii ON a row: its |ax| and the root of nothing (R * R is
    compared, so only the square's edge can be met by construction)."""
    r = [3e-4, 0.0, 1e-4, 5e-5, 1e-4, 1.0, 2e-4, 1.7e-4]
    if _edge_row(rows) is not None:
        r.append(abs(rows[_edge_row(rows), 0] - SPOT_CENTER[0]))
    return np.array(r)


def _edge_row(rows):
    """The first row that is nearer the centre in z than in x: it lies ON the edge of the square of half-size |ax|."""
    near = np.nonzero(np.abs(rows[:, 1] - SPOT_CENTER[1]) < np.abs(rows[:, 0] - SPOT_CENTER[0]))[0]
    return int(near[0]) if len(near) else None


@pytest.mark.parametrize("H", [0, 1, 256, 257, 5000])
def test_spot_counts_equal_numpy(H):
    rows = _spot_rows(H)
    radii = _spot_radii(rows)
    for name, _ in SHAPES:
        inside, ms = abi.spot_ee(rows, SPOT_CENTER, radii, shape=name)
        want = _spot_numpy(rows, SPOT_CENTER, radii, name)
        assert inside.dtype == np.int64 and np.array_equal(inside, want), (name, inside, want)
        nan_rows = 2 if H > 2 else 0
        assert inside[1] == 0 and inside[5] == H - nan_rows and inside[2] == inside[4] and ms >= 0
        if H == 5000:
            assert 0 < inside[3] < inside[2] < inside[6] < inside[0] < H and sr.spot_splits(H)[0] == 3
            wide = np.hstack([rows, np.full((H, 3), 7.0)])  # five columns: the stride is the caller's
            assert np.array_equal(abi.spot_ee(wide, SPOT_CENTER, radii, shape=name)[0], want)
            if name == "square":  # the row the last radius was taken from lies ON the square's edge in x, and counts
                assert want[-1] == _spot_numpy(np.delete(rows, _edge_row(rows), axis=0), SPOT_CENTER, radii, name)[-1] + 1


@pytest.mark.parametrize("nr", [1, 4096])
def test_spot_radius_counts(nr):
    rows = _spot_rows(5000)
    radii = 8e-4 * ((np.arange(nr) * 1237) % nr) / nr  # scrambled
    if nr > 1:
        radii[7] = radii[100]
    for name, _ in SHAPES:
        inside, _ = abi.spot_ee(rows, SPOT_CENTER, radii, shape=name)
        assert np.array_equal(inside, _spot_numpy(rows, SPOT_CENTER, radii, name)), name
    with pytest.raises(RuntimeError, match=r"bmo_spot_ee failed \(-6\)"):
        abi.spot_ee(rows, SPOT_CENTER, np.linspace(0.0, 1e-3, 4097))


def _ragged_sweep():
    """A 4 mm detector in a 15 mm collimated beam, moved sideways: the row counts differ and configuration 3 records no hit."""
    cs = bmo.UniformDiscSource([0, -10 * mm, 0], [0, 1, 0], 15 * mm, 1e-6, num_rays=2000, e1=[1, 0, 0])
    sd = bmo.Spotdetector(4 * mm)
    bmo.translate3d(sd, [0, 50 * mm, 0])
    xoff = [0.0, 3 * mm, 5.5 * mm, 30 * mm, 1 * mm]
    return cs, sd, bmo.System([sd]), xoff, (lambda c: bmo.translate_to3d(sd, [xoff[c], 50 * mm, 0]))


def test_spot_sweep_equals_the_single_calls():
    """K = 5 ragged configurations, one of them empty: every curve equals the single call on that configuration's rows and numpy; the
    centroid centres come from one spot_stats call."""
    cs, sd, system, xoff, configure = _ragged_sweep()
    sol = bmo.solve_sweep(system, cs, len(xoff), configure)
    try:
        K = len(xoff)
        rows = [sol.spot_hits(sd, c) for c in range(K)]
        counts = [len(r) for r in rows]
        assert counts[3] == 0 and len(set(counts)) == K and min(counts[:3] + counts[4:]) > 0, counts
        radii = np.array([1.5 * mm, 0.2 * mm, 3 * mm, 0.7 * mm, 0.2 * mm])
        given = np.array([[0.1 * mm, -0.2 * mm], [0.5 * mm, 0.0], [-1 * mm, 0.3 * mm], [0.0, 0.0], [0.0, 1 * mm]])
        for name, _ in SHAPES:
            for center in (given, (0.2 * mm, -0.1 * mm), None):
                frac, inside, n_rows, cen = sol.spot_encircled_energy(sd, radii, center=center, shape=name)
                assert inside.shape == frac.shape == (K, 5) and n_rows.tolist() == counts and cen.shape == (K, 2) and sol.readout_ms > 0
                if center is None:
                    st = sol.spot_stats(sd)
                    assert np.array_equal(_bits(cen[[0, 1, 2, 4]]), _bits(st[[0, 1, 2, 4], 1:3])) and not cen[3].any()
                for c in range(K):
                    one, _ = abi.spot_ee(rows[c], cen[c], radii, shape=name)
                    assert np.array_equal(inside[c], one) and np.array_equal(one, _spot_numpy(rows[c], cen[c], radii, name)), (name, c)
                assert not inside[3].any() and np.isnan(frac[3]).all() and np.array_equal(frac[0], inside[0] / counts[0])
                assert (inside[[0, 1, 2, 4], 2] > 0).all() and inside[0, 1] < inside[0, 3] < inside[0, 0]
    finally:
        sol.close()


def test_spot_detector_solution_and_sweep_agree():
    """Spotdetector.encircled_energy on the copied rows, EngineSolution.spot_encircled_energy on the resident ones (with the segment log and
    detector-only) and SweepSolution.spot_encircled_energy read the same curve."""
    cs, sd, system, xoff, configure = _ragged_sweep()
    sol = bmo.solve_sweep(system, cs, len(xoff), configure)
    radii = bmo.components.ee_radii(2.5 * mm, 9)[::-1]
    try:
        swept = {name: sol.spot_encircled_energy(sd, radii, shape=name) for name, _ in SHAPES}
    finally:
        sol.close()
    for c in (1, 3):
        configure(c)
        sd.empty()
        bmo.solve_system(system, cs)
        bundle = bmo.RayBundle.from_beams(cs.beams)
        scene = bmo.CompiledScene(system, bundle.lambdas)
        for name, _ in SHAPES:
            frac, inside, n_rows = sd.encircled_energy(radii, shape=name)
            assert n_rows == swept[name][2][c] and np.array_equal(inside, swept[name][1][c]) and np.array_equal(_bits(frac), _bits(swept[name][0][c])), (name, c)
            _, esol = bmo.system._engine_solve(scene, bundle, 100, None)
            try:
                got = esol.spot_encircled_energy(0, radii, shape=name)
                assert got[2] == n_rows and np.array_equal(got[1], inside) and np.array_equal(_bits(got[0]), _bits(frac)) and (esol.readout_ms > 0 or n_rows == 0)
                if n_rows:
                    ptr, cnt = esol_rows(esol, 0)
                    assert cnt == n_rows and np.array_equal(abi.spot_ee(None, (0.0, 0.1 * mm), radii, shape=name, rows_device_ptr=ptr, n_rows=cnt)[0],
                                                            abi.spot_ee(sd.data, (0.0, 0.1 * mm), radii, shape=name)[0])
            finally:
                esol.free()
        bmo.release(cs)


def esol_rows(esol, slot):
    """(device pointer, count) of the resident rows of `slot` (bmo_result_device_hits)."""
    import ctypes as C

    p, cnt = C.POINTER(C.c_double)(), C.c_int64()
    abi.check(esol.lib, esol.lib.bmo_result_device_hits(esol.handle, slot, C.byref(p), C.byref(cnt)), "bmo_result_device_hits")
    return C.cast(p, C.c_void_p).value, cnt.value


def test_spot_detector_only_sweep_reads_the_same():
    """record_segments = 0: the resident rows read the same counts as after a solve with the segment log."""
    cs, sd, system, xoff, configure = _ragged_sweep()
    K = len(xoff)
    bundle = bmo.RayBundle.from_beams(cs.beams)
    scenes_, poses, grids = bmo.system.sweep_snapshots(system, bundle.lambdas, K, configure)
    tiled = bmo.RayBundle(bundle.kind, np.tile(bundle.planes, (1, K)))
    cfg = np.repeat(np.arange(K, dtype=np.int32), bundle.n)
    got = []
    for record in (True, False):
        _, h, lib = bmo.system.sweep_trace(scenes_, tiled, cfg, record_segments=record, view=False)
        try:
            got.append(abi.spot_ee_sweep(h, 0, K, (0.1 * mm, 0.0), [1 * mm, 0.3 * mm, 2 * mm], shape="square")[:2])
        finally:
            lib.bmo_result_free(h)
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]) and got[0][1][3] == 0 and got[0][0].sum() > 0


# ------------------------------------------------------------------------------------------------ the Python layer
def test_detector_and_solution_read_the_same_curves():
    """PSFDetector.encircled_energy on the copied rows and EngineSolution.psf_encircled_energy on the resident ones, both kinds, bit for
    bit; the window of the diffraction kind comes from mtf_window at the cutoff on both paths."""
    rows, pose, o, (eng, dev, res, bundle) = _solve(600, record=False, keep=True)
    sol = bmo.system.EngineSolution(eng.lib, res, bundle.n, bundle.kind)
    psfd = bmo.PSFDetector(10 * mm)
    psfd.data, psfd.position, psfd.orientation = rows, (lambda: pose[0]), (lambda: o)
    offsets = [-0.2 * mm, 0.0, 0.2 * mm]
    radii = bmo.components.ee_radii(2e-5, 6)
    try:
        for kw in (dict(kind="geometric"), dict(kind="geometric", shape="square", follow=None, axis=_axis(pose)), dict(kind="diffraction"),
                   dict(kind="diffraction", shape="square", n=24, half_width=1.5e-4, follow=None)):
            got, want = sol.psf_encircled_energy(0, pose[0], o, radii, offsets=offsets, **kw), psfd.encircled_energy(radii, offsets=offsets, **kw)
            assert got[0].shape == got[1].shape == (3, 6) and got[2].shape == (3,) and got[3].shape == (3, 2) and got[4].shape == (3, 12) and sol.readout_ms > 0
            for a, b in zip(got, want):
                assert np.array_equal(_bits(a), _bits(b)), kw
            assert np.isfinite(got[0]).all() and (np.diff(got[0], axis=1) >= 0).all() and (got[0] <= 1.0).all() and got[0].max() > 0
        st = got[4]
        geo = psfd.encircled_energy(radii, offsets=offsets)
        direct = abi.psf_geo_ee(rows, *pose, o[:, 1], offsets, radii, centers=st[:, [fr.CX, fr.CZ]])
        assert np.array_equal(_bits(geo[0]), _bits(direct[0])) and np.array_equal(_bits(geo[3]), _bits(st[:, [fr.CX, fr.CZ]]))
        with pytest.raises(ValueError, match="window"):
            psfd.encircled_energy([2e-4], kind="diffraction", n=8, half_width=1e-4)
        with pytest.raises(ValueError, match="window"):
            sol.psf_encircled_energy(0, pose[0], o, [2e-4], kind="diffraction", n=8, half_width=1e-4)
    finally:
        sol.handle = None  # the engine frees the result
        eng.free_result(res)
        eng.free_batch(dev)
        eng.close()


def test_resident_rows_are_refused_where_they_are_not_psf_rows():
    """EngineSolution.psf_encircled_energy asks the library for the rows (bmo_result_psf_rows): a slot of another detector kind is
    BMO_ERR_INVALID, a GaussianBeamlet solution BMO_ERR_UNSUPPORTED; spot_encircled_energy likewise through bmo_spot_ee_sweep."""
    import scenes

    psfd, spot = bmo.PSFDetector(5 * mm), bmo.Spotdetector(5 * mm)
    bmo.translate3d(psfd, [-5 * mm, 50 * mm, 0])
    bmo.translate3d(spot, [5 * mm, 50 * mm, 0])
    bundle = scenes.disc_bundle(64, center=[0, 0, 0], direction=[0, 1, 0], diameter=18 * mm, lam=1e-6, jitter=0.0)
    sc = bmo.CompiledScene(bmo.System([psfd, spot]), bundle.lambdas)
    _, sol = bmo.system._engine_solve(sc, bundle, 100, None)
    try:
        kinds = {type(dd): slot for slot, dd in enumerate(sc.detectors)}
        pos, ori = np.asarray(psfd.position(), dtype=np.float64), np.asarray(psfd.orientation(), dtype=np.float64)
        out = sol.psf_encircled_energy(kinds[bmo.PSFDetector], pos, ori, [0.0, 1.0], kind="geometric")
        assert out[0].shape == (1, 2) and abs(out[0][0, 1] - 1.0) <= 2 * fr.gamma(64)  # every row inside: energy and S add the 64 proj in two orders
        frac, inside, n_rows = sol.spot_encircled_energy(kinds[bmo.Spotdetector], [1.0])
        assert n_rows > 0 and inside.tolist() == [n_rows] and frac.tolist() == [1.0]
        for slot in (kinds[bmo.Spotdetector], -1, 2):
            for kind in ("geometric", "diffraction"):
                with pytest.raises(RuntimeError, match=r"bmo_result_psf_rows failed \(-1\)"):
                    sol.psf_encircled_energy(slot, pos, ori, [1e-5], kind=kind, n=4, half_width=1e-4)
        for slot in (kinds[bmo.PSFDetector], -1, 2):
            with pytest.raises(RuntimeError, match=r"bmo_spot_ee_sweep failed \(-1\)"):
                sol.spot_encircled_energy(slot, [1e-5], center=(0.0, 0.0))
        with pytest.raises(RuntimeError, match=r"bmo_spot_ee_sweep failed \(-1\).*n_configs"):
            abi.spot_ee_sweep(sol.handle, kinds[bmo.Spotdetector], 2, np.zeros((2, 2)), [1e-5])
    finally:
        sol.free()
    system3, _ = scenes.c2_scene()
    b3 = scenes.c3_bundle(64)
    _, sol3 = bmo.system._engine_solve(bmo.CompiledScene(system3, b3.lambdas), b3, 100, None)
    try:
        with pytest.raises(RuntimeError, match=r"bmo_result_psf_rows failed \(-4\).*GaussianBeamlet"):
            sol3.psf_encircled_energy(0, np.zeros(3), np.eye(3), [1e-5], kind="geometric")
        with pytest.raises(RuntimeError, match=r"bmo_spot_ee_sweep failed \(-4\).*GaussianBeamlet"):
            sol3.spot_encircled_energy(0, [1e-5], center=(0.0, 0.0))
    finally:
        sol3.free()

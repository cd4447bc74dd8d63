"""SDF marches under incoherent waves, CPU part.  tests/test_sdf_waves_gpu.py holds the step kernels to the oracle on
waves whose lanes disagree; here the oracle's solution of its inputs (never the engine's) shows that they are what that file assumes,
so that it cannot pass vacuously: every wave of 64 roots holds every ray family, many first-hit shapes, hits and misses, entering and
leaving starts, short and long beams, splitting roots.  The host build of the lane code equals the oracle on the head of every bundle,
and the two premises of the result-preserving shortcuts that no test held so far — every exact sdf is 1-Lipschitz (union child skip,
running-t prune) and bounded below by the distance to its bounding sphere where that bound is tight — are checked for every leaf kind
of shapes.py and for the lens shapes the builders make of them."""
import functools
import math

import numpy as np
import pytest

import bmo_amd as bmo
from bmo_amd import shapes as sh

from tests import wave_scenes as ws
from tests.parity import compare
from test_leaf_march import _trace, emus  # noqa: F401  (the fixture: the emulator with BMO_MARCH_FASTPATH=2, BMO_LEAF_MARCH on and off)

mm = 1e-3
SCENE_NAMES = list(ws.SCENES)
KIND_CASES = [(name, "ray", ws.N_RAYS) for name in SCENE_NAMES] + [(name, kind, 1024) for name in ("c2", "train") for kind in ("pol", "gauss")]


@functools.lru_cache(maxsize=None)
def solved(name, kind="ray", n=ws.N_RAYS):
    """(compiled scene, parts, bundle, family per ray, the oracle's solution) of a scene under its mixed bundle."""
    import pyoracle

    system, parts, bundle, fam = ws.case(name, kind, n)
    scene = bmo.CompiledScene(system, bundle.lambdas)
    return scene, parts, bundle, fam, pyoracle.trace(scene, bundle, ws.R_MAX, threads=8)


def _waves(x):
    w = len(x) // ws.WAVE
    return x[:w * ws.WAVE].reshape(w, ws.WAVE)


def first_hits(scene, res):
    """Per root, in bundle order: object and shape of the first intersection (-1: none), whether the shape is an SDF, and
    dot(dir, normal) there (> 0: the ray leaves the shape it was in)."""
    root_node = np.searchsorted(res.node_root, np.arange(res.n_roots), side="left")
    assert np.array_equal(res.node_root[root_node], np.arange(res.n_roots)) and (res.node_parent[root_node] < 0).all()
    r = res.node_first_rec[root_node]
    shape = res.rec_shape[r]
    is_sdf = np.array([ws._is_sdf(scene, int(s)) for s in shape])
    dot = (res.rec[3:6, r] * res.rec[8:11, r]).sum(axis=0)
    return dict(obj=res.rec_obj[r], shape=shape, sdf=is_sdf, dot=np.where(shape >= 0, dot, np.nan), nseg=res.node_nseg[root_node],
                n_nodes=np.bincount(res.node_root, minlength=res.n_roots))


def _distinct_per_wave(ids, valid):
    return np.array([len(set(w[v].tolist())) for w, v in zip(_waves(ids), _waves(valid))])


MIN_SHAPES = {"c2": 6, "c5": 12, "train": 5}


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_every_wave_holds_every_family_many_shapes_hits_and_misses(oracle, name):
    scene, parts, bundle, fam, ref = solved(name)
    assert bundle.n == ws.N_RAYS and ref.n_roots == ws.N_RAYS and len(_waves(fam)) == 48
    assert np.array_equal(fam, ws.PATTERN[np.arange(bundle.n) % 32])
    for f in range(len(ws.FAMILIES)):
        assert (_waves(fam) == f).any(axis=1).all(), ws.FAMILIES[f]
    fh = first_hits(scene, ref)
    hit = fh["shape"] >= 0
    assert (_waves(hit).any(axis=1) & (~_waves(hit)).any(axis=1)).all()
    if name == "cell":
        n_mirrors = 101
        distinct = _distinct_per_wave(fh["obj"], hit & (fh["obj"] < n_mirrors))
        print(f"\n{name}: distinct first-hit mirrors per wave {distinct.min()} .. {distinct.max()}")
        assert distinct.min() >= 8
        assert (ref.rec_obj >= 64).sum() > 0 and (fh["obj"] >= 64).sum() > 0  # the second candidate chunk
    else:
        distinct = _distinct_per_wave(fh["shape"], hit)
        print(f"\n{name}: distinct first-hit shapes per wave {distinct.min()} .. {distinct.max()} of {scene.desc.n_shapes}")
        assert distinct.min() >= MIN_SHAPES[name]


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_starts_on_surfaces_and_in_glass_enter_and_leave(oracle, name):
    """An on-surface start that the reference classifies as entering marches inside and first hits the far side of its own shape from
    within (dot(dir, normal) > 0 on an SDF shape); one that leaves has no intersection at t = 0: a later hit from outside, or none."""
    scene, parts, bundle, fam, ref = solved(name)
    fh = first_hits(scene, ref)
    from_within = (fh["shape"] >= 0) & fh["sdf"] & (fh["dot"] > 0)
    on = fam == ws.SURFACE
    entering, leaving = int((on & from_within).sum()), int((on & ~from_within).sum())
    glass = int(((fam == ws.GLASS) & from_within).sum())
    print(f"\n{name}: on-surface starts entering {entering}, leaving {leaving}; in-glass first hits with a leaving normal {glass}")
    assert entering >= 50 and leaving >= 50
    assert glass >= 100


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_waves_mix_bounce_counts_and_splitting_roots(oracle, name):
    scene, parts, bundle, fam, ref = solved(name)
    fh = first_hits(scene, ref)
    spread = _waves(fh["nseg"]).max(axis=1) - _waves(fh["nseg"]).min(axis=1)
    splits = (_waves(fh["n_nodes"]) > 1).any(axis=1)
    print(f"\n{name}: nseg spread per wave {spread.min()} .. {spread.max()}, waves with a splitting root {splits.sum()} of {len(splits)}")
    if name in ("c2", "c5"):
        assert spread.min() >= 5
    assert splits.mean() >= 0.5  # (every scene has a splitter)


@pytest.mark.parametrize("name", ["train", "cell"])
def test_plate_splitter_coating_and_substrate_are_first_hits(oracle, name):
    scene, parts, bundle, fam, ref = solved(name)
    plate = parts["plate_bs"] if name == "train" else next(o for o in scene.leaf_objects if isinstance(o, bmo.RectangularPlateBeamsplitter))
    fh = first_hits(scene, ref)
    coating = int((fh["shape"] == scene.shape_id(plate.coating.shape)).sum())
    substrate = int((fh["shape"] == scene.shape_id(plate.substrate.shape)).sum())
    print(f"\n{name}: first hits on the plate's coating {coating}, on its substrate {substrate}")
    assert coating > 0 and substrate > 0


def test_generic_train_is_left_to_the_generic_trip():
    """The train's lens shapes are the kinds tracing_step's specialised loop does not take (csrc/bmo_lane.hpp leaf_class 0)."""
    system, parts = ws.generic_train()
    assert isinstance(parts["meniscus"].shape, sh.MeniscusLensSDF)
    kinds = {name: {type(s).__name__ for s in getattr(parts[name].shape, "sdfs", [parts[name].shape])} for name in ("asphere", "asphere2", "cylinder", "acylinder")}
    assert any("Aspherical" in k for k in kinds["asphere"]) and sum("Aspherical" in k for k in kinds["asphere2"]) >= 1, kinds
    assert any("Cylinder" in k for k in kinds["cylinder"]), kinds
    assert isinstance(parts["plate_bs"], bmo.RectangularPlateBeamsplitter) and isinstance(parts["cube_bs"], bmo.CubeBeamsplitter)


def test_bad_lanes_take_every_lane_position():
    _, _, bundle, _ = ws.case("c2")
    b, bad = ws.bad_lanes(bundle)
    idx = np.flatnonzero(bad)
    assert np.array_equal(idx, np.arange(0, bundle.n, ws.BAD_STRIDE)) and idx[0] % 64 == 0
    assert len(set((idx % 64).tolist())) == len(idx)  # 32 bad rays in 32 different lane positions, lane 0 among them
    finite = np.isfinite(b.planes[0:6]).all(axis=0)
    assert finite[~bad].all() and np.array_equal(finite[idx], (np.arange(len(idx)) % 6) == 5) and (b.planes[0, idx[5::6]] == 1e30).all()
    assert (b.planes[:, ~bad].view(np.int64) == bundle.planes[:, ~bad].view(np.int64)).all()


def test_by_root_follows_a_permutation_of_the_roots(oracle):
    """by_root of a solve of permuted roots is the permutation of by_root of the solve, bit for bit (oracle on both sides)."""
    scene, parts, bundle, fam, ref = solved("c2")
    order = np.random.default_rng(5).permutation(512)
    a = ws.by_root(oracle.trace(scene, ws.head(bundle, 512), ws.R_MAX, threads=8))
    b = ws.by_root(oracle.trace(scene, ws.permuted(ws.head(bundle, 512), order), ws.R_MAX, threads=8))
    assert ws.roots_differing(b, a, zip(range(512), order)) == []
    assert sum(len(r["nseg"]) > 1 for r in a) > 10  # roots with children among them
    assert len(ws.roots_differing(b, a, zip(range(512), range(512)))) > 400  # (and the comparison can fail)


@pytest.mark.parametrize("name,kind,n", KIND_CASES)
def test_lane_code_equals_oracle_on_mixed_bundles(oracle, emus, name, kind, n):  # noqa: F811
    system, parts, bundle, fam = ws.case(name, kind, n)
    part = ws.head(bundle, 256)
    scene = bmo.CompiledScene(system, part.lambdas)
    ref = oracle.trace(scene, part, ws.R_MAX, threads=8)
    on = _trace(emus["on"], scene, part, ws.R_MAX)
    off = _trace(emus["off"], scene, part, ws.R_MAX)
    compare(on, ref, 0.0, f"{name} {kind}, loop on")
    compare(off, ref, 0.0, f"{name} {kind}, loop off")


def test_retrace_probe_holds_and_misses_in_most_waves(oracle):
    """After the first doublet of config 2 moved by 0.05 mm and 0.3 deg the stored path of some roots of a wave still holds (their
    trees are those of the first solve) and that of others does not."""
    bundle = ws.case("c2")[2]
    system = ws.fresh_system("c2")  # (the cached case's system stays as it is)
    scene0 = bmo.CompiledScene(system, bundle.lambdas)
    a0, sol0 = oracle.trace(scene0, bundle, ws.R_MAX, threads=8, keep=True)
    try:
        ws.move_first_doublet(system)
        scene1 = bmo.CompiledScene(system, bundle.lambdas)
        a1 = oracle.trace(scene1, bundle, ws.R_MAX, threads=8, prev=sol0)
    finally:
        sol0.free()
    n = bundle.n
    broke = np.zeros(n, dtype=bool)
    broke[[i for i, _ in ws.roots_differing(ws.by_root(a0), ws.by_root(a1), zip(range(n), range(n)))]] = True
    both = _waves(broke).any(axis=1) & (~_waves(broke)).any(axis=1)
    print(f"\nretrace: {broke.sum()} of {n} roots changed, waves with both outcomes {both.sum()} of {len(both)}")
    assert both.mean() >= 0.5


# ---------------------------------------------------------------------------------------------------------------- premises
def _leaf_factories():
    """One or more posed instances per exact leaf class of shapes.py, by class name."""
    return {
        "PlanoSurfaceSDF": [lambda: sh.PlanoSurfaceSDF(2 * mm, 8 * mm)],
        "SphereSDF": [lambda: sh.SphereSDF(3 * mm)],
        "ConcaveSphericalSurfaceSDF": [lambda: sh.ConcaveSphericalSurfaceSDF(10 * mm, 8 * mm)],
        "ConvexSphericalSurfaceSDF": [lambda: sh.ConvexSphericalSurfaceSDF(10 * mm, 8 * mm), lambda: sh.ConvexSphericalSurfaceSDF(4.1 * mm, 8 * mm)],
        "BoxSDF": [lambda: sh.BoxSDF(3 * mm, 4 * mm, 5 * mm)],
        "CylinderSDF": [lambda: sh.CylinderSDF(2 * mm, 3 * mm)],
        "CutSphereSDF": [lambda: sh.CutSphereSDF(5 * mm, 2 * mm), lambda: sh.CutSphereSDF(5 * mm, -2 * mm)],
        "RingSDF": [lambda: sh.RingSDF(4 * mm, 1 * mm, 2 * mm)],
        "RightAnglePrismSDF": [lambda: sh.RightAnglePrismSDF(6 * mm, 4 * mm)],
        "TestPointSDF": [lambda: sh.TestPointSDF()],
        "ConvexCylinderSDF": [lambda: sh.ConvexCylinderSDF(30 * mm, 20 * mm, 22 * mm)],
        "ConcaveCylinderSDF": [lambda: sh.ConcaveCylinderSDF(30 * mm, 20 * mm, 22 * mm)],
        "UnionSDF": [lambda: sh.BiConvexLensSDF(20 * mm, 30 * mm, 4 * mm, 10 * mm), lambda: sh.PlanoConcaveLensSDF(15 * mm, 3 * mm, 10 * mm, 12 * mm),
                     lambda: sh.BiConcaveLensSDF(15 * mm, 20 * mm, 3 * mm, 10 * mm, 12 * mm)],
        "MeniscusLensSDF": [lambda: bmo.SphericalLens(30 * mm, 60 * mm, 2.5 * mm, 25.4 * mm, 1.6).shape,
                            lambda: bmo.SphericalLens(-60 * mm, -30 * mm, 2.5 * mm, 25.4 * mm, 1.6).shape],
    }


def _builder_shapes():
    """The unions and lenses the builders of components.py make of the leaves: plano-convex, thin lens, ring lens (a mechanical
    diameter), doublet halves, meniscus, plano-concave, bi-concave, a cylinder lens."""
    nb = lambda lam: 1.5  # noqa: E731
    doublet = bmo.SphericalDoubletLens(60 * mm, -40 * mm, -120 * mm, 6 * mm, 2.5 * mm, 25.4 * mm, 1.5, 1.7)
    ring = bmo.Lens(bmo.SphericalSurface(38.184 * mm, 2 * 1.840 * mm, 2 * 2.380 * mm), bmo.SphericalSurface(3.467 * mm, 2 * 2.060 * mm, 2 * 2.380 * mm), 0.5 * mm, nb)
    out = {
        "plano-convex": bmo.SphericalLens(math.inf, -40 * mm, 5 * mm, 25.4 * mm, 1.7).shape,
        "thin lens": bmo.ThinLens(50 * mm, 80 * mm, 25.4 * mm, 1.5).shape,
        "ring lens": ring.shape,
        "doublet front": doublet.front.shape, "doublet back": doublet.back.shape,
        "meniscus": bmo.SphericalLens(30 * mm, 60 * mm, 2.5 * mm, 25.4 * mm, 1.6).shape,
        "plano-concave": bmo.SphericalLens(math.inf, 40 * mm, 3 * mm, 25.4 * mm, 1.5).shape,
        "bi-concave": bmo.SphericalLens(-50 * mm, 40 * mm, 3 * mm, 25.4 * mm, 1.5).shape,
        "cylinder lens": bmo.Lens(bmo.CylindricalSurface(40 * mm, 20 * mm, 22 * mm), 5 * mm, nb).shape,
        "concave cylinder lens": bmo.Lens(bmo.CylindricalSurface(-40 * mm, 20 * mm, 22 * mm), 5 * mm, nb).shape,
    }
    return out


def _exact_leaf_classes():
    def subclasses(c):
        for s in c.__subclasses__():
            yield s
            yield from subclasses(s)

    return sorted({c.__name__ for c in subclasses(sh.AbstractSDF) if c.__module__ == sh.__name__ and not c.__name__.startswith("_")
                   and not (getattr(c, "flags", 0) & sh.FLAG_INEXACT)})


def test_every_exact_leaf_kind_is_covered():
    """The list is taken by introspection: a leaf kind added to shapes.py fails here until it is given a factory or flagged inexact."""
    assert _exact_leaf_classes() == sorted(_leaf_factories())
    for name, makers in _leaf_factories().items():
        for make in makers:
            assert type(make()).__name__ == name


@functools.lru_cache(maxsize=None)
def _posed_shapes():
    out = []
    for name, makers in _leaf_factories().items():
        for k, make in enumerate(makers):
            out.append((f"{name} #{k}", make()))
    out += list(_builder_shapes().items())
    posed = []
    for i, (label, s) in enumerate(out):
        bmo.xrotate3d(s, 0.3 + 0.07 * i)
        bmo.zrotate3d(s, -0.7 + 0.05 * i)
        bmo.translate3d(s, [1 * mm * (i % 5), -2 * mm, 3 * mm])
        sc = bmo.CompiledScene(bmo.System([bmo.IntersectableObject(s)]), [1e-6])
        rec = sc._shapes[sc.shape_id(s)]
        assert not (rec.flags & sh.FLAG_INEXACT), label
        posed.append((label, s, sc))
    return posed


def _sdf_n(oracle, sc, s, pts):
    return np.array([oracle.sdf(sc, s, p) for p in pts])


def _surface_points(oracle, sc, s, c, R, rng, m):
    """m points close to the shape's surface (faces, edges and rims among them): random points in the bounding sphere walked down the
    sdf along a random direction's best step (sphere tracing towards the surface from outside, bisection from inside)."""
    pts = []
    if type(s).__name__ == "TestPointSDF":  # (a point has no inside: the pairs lie around the point itself)
        return np.tile(np.asarray(s.pos, dtype=np.float64), (m, 1))
    while len(pts) < m:
        a = c + ws._random_units(rng, 1)[0] * R * rng.uniform(0.0, 1.5)
        b = c + ws._random_units(rng, 1)[0] * R * rng.uniform(0.0, 1.5)
        fa, fb = oracle.sdf(sc, s, a), oracle.sdf(sc, s, b)
        if not (np.isfinite(fa) and np.isfinite(fb)) or (fa > 0) == (fb > 0):
            continue
        for _ in range(40):  # bisect the segment for the sign change: a point of the surface
            mid = 0.5 * (a + b)
            fm = oracle.sdf(sc, s, mid)
            if (fm > 0) == (fa > 0):
                a, fa = mid, fm
            else:
                b = mid
        pts.append(0.5 * (a + b))
    return np.array(pts)


def test_exact_sdfs_are_1_lipschitz(oracle):
    """|sdf(p) - sdf(q)| <= |p - q| (1 + 1e-9) + 1e-12: the allowance sdf_any adds to `acc` per trip (csrc/bmo_lane.hpp) and the premise
    of the running-t prune.  2 000 pairs per posed shape within two bounding radii, separations 1e-4 .. 1e-1 of the radius; half of
    them straddle the surface at a random place (faces, edges, rims: the pair is centred on a surface point)."""
    rng = np.random.default_rng(11)
    worst = {}
    for label, s, sc in _posed_shapes():
        rec = sc._shapes[sc.shape_id(s)]
        c, R = np.array(rec.bs_center[:]), max(rec.bs_radius, 1 * mm)
        m = 1000
        sep = R * 10.0 ** rng.uniform(-4, -1, 2 * m)
        u = ws._random_units(rng, 2 * m)
        far = c + ws._random_units(rng, m) * (2 * R * rng.uniform(0, 1, (m, 1)) ** (1 / 3))
        near = _surface_points(oracle, sc, s, c, R, rng, 100)[rng.integers(0, 100, m)]
        mid = np.concatenate([far, near])
        p, q = mid + 0.5 * sep[:, None] * u, mid - 0.5 * sep[:, None] * u
        fp, fq = _sdf_n(oracle, sc, s, p), _sdf_n(oracle, sc, s, q)
        dist = np.linalg.norm(p - q, axis=1)
        slack = np.abs(fp - fq) - (dist * (1 + 1e-9) + 1e-12)
        worst[label] = float((np.abs(fp - fq) / dist).max())
        straddle = ((fp[m:] > 0) != (fq[m:] > 0)).mean()
        assert straddle > 0.5 or label.startswith("TestPointSDF"), (label, straddle)
        bad = np.flatnonzero(~(slack <= 0))
        assert bad.size == 0, (label, p[bad[:3]], q[bad[:3]], fp[bad[:3]], fq[bad[:3]], dist[bad[:3]])
    print("\nlargest difference quotient per shape: " + ", ".join(f"{k} {v:.6f}" for k, v in worst.items()))


def test_sdf_is_bounded_by_the_distance_to_its_bounding_sphere(oracle):
    """sdf(p) >= |p - c| - R outside the sphere (the premise of the miss cull and of the receding exit), for every exact leaf kind and
    builder shape.  The points lie on rays from the centre through the surface points farthest from it — box and prism corners, rims
    of caps, cylinder ends, where the sphere touches the solid and the bound is tight — and in random directions."""
    rng = np.random.default_rng(12)
    tightest = {}
    for label, s, sc in _posed_shapes():
        rec = sc._shapes[sc.shape_id(s)]
        c, R = np.array(rec.bs_center[:]), rec.bs_radius
        assert R > 0
        if type(s).__name__ == "TestPointSDF":
            dirs = ws._random_units(rng, 300)
        else:
            surf = _surface_points(oracle, sc, s, c, R, rng, 300)
            r = np.linalg.norm(surf - c, axis=1)
            far = surf[np.argsort(r)[-60:]]  # the surface points nearest the sphere
            assert (r <= R).all(), (label, r.max(), R)
            dirs = np.concatenate([ws._unit(far - c), ws._unit(far - c + 0.02 * R * rng.normal(size=far.shape)), ws._random_units(rng, 180)])
        scale = 1 + 10.0 ** rng.uniform(-6, 0.5, len(dirs))
        p = c + dirs * (R * scale)[:, None]
        v = _sdf_n(oracle, sc, s, p)
        lb = np.linalg.norm(p - c, axis=1) - R
        bad = np.flatnonzero(~(v >= lb))
        assert bad.size == 0, (label, p[bad[:3]], v[bad[:3]], lb[bad[:3]])
        tightest[label] = float((v - lb).min() / R)
    print("\nsmallest (sdf - bound) / R per shape: " + ", ".join(f"{k} {v:.2e}" for k, v in tightest.items()))

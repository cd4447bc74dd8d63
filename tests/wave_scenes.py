"""Scenes and bundles of the SDF wave tests (DESIGN.md §2 "SDF marches under incoherent waves"; tests/test_sdf_waves.py on the CPU,
tests/test_sdf_waves_gpu.py on the GPU).

The step kernels read the scene through wave-uniform indices (csrc/bmo_lane.hpp, file header): the union child evaluated first, the
specialised march loop's child, the hinted and the winning shape of the waterfalls come from the wave's first active lane, the candidate
slots from a scalar mask, while the nearest-hit prune, the start classification and the retrace probe use each lane's own state.  The
host build of the lane code runs one lane at a time and sees none of that.  The bundles here make the lanes of every wave of 64
consecutive roots disagree about all of it: eight families of rays, dealt lane by lane in a fixed pattern of 32, so that every full
wave holds every family.  A bundle's numbering is the device's root order under BMO_ROOT_ORDER=none.
"""
import functools
import math

import numpy as np

import bmo_amd as bmo
from bmo_amd import shapes as sh

from tests import scenes

mm = 1e-3
WAVE = 64
LAM = 1.064e-6
R_MAX = 30
N_RAYS = 3072  # 48 waves: the smallest size at which every family fills every wave with its share of the pattern

FAMILIES = ("forward", "backward", "around", "surface", "glass", "side", "nearmiss", "graze")
FORWARD, BACKWARD, AROUND, SURFACE, GLASS, SIDE, NEARMISS, GRAZE = range(8)
# shares of a pattern of 32 lanes (two patterns per wave).  Near misses are kept few: each costs the oracle march_iters evaluations.
_SHARE = {FORWARD: 5, BACKWARD: 4, AROUND: 7, SURFACE: 5, GLASS: 4, SIDE: 4, NEARMISS: 1, GRAZE: 2}
_GROUPED = [f for f in range(8) for _ in range(_SHARE[f])]
PATTERN = np.array([_GROUPED[(13 * i) % 32] for i in range(32)])  # 13 is coprime with 32: neighbours come from different families
assert len(_GROUPED) == 32 and sorted(PATTERN.tolist()) == _GROUPED

BAD_STRIDE = 97  # as tests/mesh_scenes.py: coprime with 64, the bad lane takes every lane position, lane 0 included


def _unit(x):
    x = np.asarray(x, dtype=np.float64)
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def _random_units(rng, m):
    return _unit(rng.normal(size=(m, 3)))


def _perpendicular(rng, a):
    """One random unit vector perpendicular to each row of a (unit rows)."""
    while True:
        r = rng.normal(size=a.shape)
        r = r - (r * a).sum(axis=1, keepdims=True) * a
        if (np.linalg.norm(r, axis=1) > 1e-3).all():
            return _unit(r)


# ------------------------------------------------------------------ scenes
def _c2_coherent(kind, n):
    geo = dict(center=[0, 0, -0.77 * mm], direction=[0, 0, 1], diameter=0.3 * mm)
    if kind == "ray":
        return scenes.c2_bundle(n)
    if kind == "pol":
        return scenes.polarized_bundle(n, e1=[1, 0, 0], jitter=0.25, **geo)
    return scenes.gaussian_bundle(n, w0=50e-6, support=(1.0, 0.0, 0.0), cone=0.1, **geo)


def _c5_coherent(kind, n):
    assert kind == "ray"
    return scenes.c5_bundle(n)


TRAIN_D = 25.4 * mm
TRAIN_SEEDS = {"asphere": 7101, "asphere2": 7102, "cylinder": 7103, "acylinder": 7104, "plate_bs": 7105, "cube_bs": 7106}


def generic_train():
    """One train along +y of the leaf classes the specialised march loop leaves to the generic trip (leaf_class 0: meniscus, even
    asphere on one and on two sides, cylinder lens, acylinder) with a plate splitter (coating and substrate candidates) and a cube
    splitter, drawn by tests/test_fuzz.py's _make from pinned seeds, small tilts and decentres like random_system's; a Spotdetector
    behind the train and one beside it for the reflected arms."""
    from tests.test_fuzz import _make

    meniscus = bmo.SphericalLens(30 * mm, 60 * mm, 2.5 * mm, TRAIN_D, 1.6)
    assert isinstance(meniscus.shape, bmo.MeniscusLensSDF)
    parts = {"meniscus": (meniscus, 2.5 * mm)}
    for name, seed in TRAIN_SEEDS.items():
        parts[name] = _make(np.random.Generator(np.random.PCG64(seed)), name)
    rng = np.random.Generator(np.random.PCG64(7100))
    objs, y = [], 0.0
    for name in ("meniscus", "asphere", "plate_bs", "cylinder", "asphere2", "cube_bs", "acylinder"):
        o, length = parts[name]
        bmo.xrotate3d(o, math.radians(float(rng.uniform(-3, 3))))
        bmo.zrotate3d(o, math.radians(float(rng.uniform(-3, 3))))
        bmo.translate3d(o, [float(rng.uniform(-1, 1) * mm), y, float(rng.uniform(-1, 1) * mm)])
        objs.append(o)
        y += length + float(rng.uniform(4, 10) * mm)
    end = bmo.Spotdetector(40 * mm)
    bmo.translate3d(end, [0, y + 10 * mm, 0])
    side = bmo.Spotdetector(80 * mm)
    bmo.xrotate3d(side, math.radians(90))
    bmo.translate3d(side, [0, y / 2, -70 * mm])
    named = {name: parts[name][0] for name in parts}
    return bmo.System(objs + [end, side]), dict(named, end=end, side=side)


def _train_coherent(kind, n):
    geo = dict(center=[0.3 * mm, -20 * mm, -0.2 * mm], direction=[0.01, 1.0, -0.005])
    if kind == "ray":
        return scenes.disc_bundle(n, diameter=0.6 * TRAIN_D, lam=LAM, cone=0.04, seed=7110, **geo)
    if kind == "pol":
        return scenes.polarized_bundle(n, diameter=0.6 * TRAIN_D, lam=LAM, jitter=0.03, seed=7111, **geo)
    return scenes.gaussian_bundle(n, diameter=0.4 * TRAIN_D, lam=LAM, w0=100e-6, seed=7112, **geo)


def _cell():
    from tests.test_many_objects import _cell as cell

    system, origin, d = cell()
    return system, dict(origin=origin, d=d)


def _cell_coherent(kind, n):
    from tests.test_many_objects import _bundle, _cell as cell

    assert kind == "ray"
    _, origin, d = cell()
    return _bundle(n, origin, d)


# name -> (scene builder returning (system, parts), coherent bundle (kind, n), mixed-bundle seed)
SCENES = {
    "c2": (scenes.c2_scene, _c2_coherent, 20251101),
    "c5": (scenes.c5_scene, _c5_coherent, 20251102),
    "train": (generic_train, _train_coherent, 20251103),
    "cell": (_cell, _cell_coherent, 20251109),  # (of eight seeds tried, six give every wave its 8 mirrors; this one gives 9)
}
MAX_TREE = {"train": 40}  # beams per root kept in the train's mixed bundle: it has two splitters (mixed_bundle)


# ------------------------------------------------------------------ beam kinds
def _as_kind(kind, pos, dirs, rng):
    """Ray / PolarizedRay / GaussianBeamlet planes over given starts and unit directions: E0 a random unit vector made orthogonal to
    each direction; waist and divergence rays as the reference's constructor places them (scenes.gaussian_bundle), the support
    vector a random perpendicular of each direction, w0 = 50 um."""
    b = bmo.RayBundle.rays(pos, dirs, LAM)
    n = b.n
    d = b.planes[3:6].T
    if kind == "ray":
        return b
    if kind == "pol":
        E = _perpendicular(rng, d)
        for _ in range(3):  # Gram-Schmidt to 1e-16 (scenes.polarized_bundle)
            E = E - (E * d).sum(axis=1)[:, None] * d
        E = E / np.linalg.norm(E, axis=1)[:, None]
        P = np.zeros((14, n))
        P[:8] = b.planes
        P[8:14:2] = E.T
        return bmo.RayBundle(bmo.BEAM_POLARIZED, P)
    assert kind == "gauss"
    w0 = 50e-6
    s1 = _perpendicular(rng, d)
    tan_t = math.tan(LAM / (math.pi * w0))
    dd = d + s1 * tan_t
    dd = dd / np.sqrt((dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2])[:, None]
    p = b.planes[0:3].T
    P = np.zeros((25, n))
    P[0:3], P[3:6] = p.T, d.T
    P[6:9], P[9:12] = (p + s1 * w0).T, d.T
    P[12:15], P[15:18] = p.T, dd.T
    P[18], P[19], P[20] = LAM, 1.0, w0
    P[21] = math.sqrt(2 * (2 * 1e-3 / (math.pi * w0 ** 2)) * bmo.linalg.Z_vacuum)
    return bmo.RayBundle(bmo.BEAM_GAUSSIAN, P)


# ------------------------------------------------------------------ the families
def scene_box(scene):
    """(lo, hi) of the box around the compiled shapes' bounding spheres."""
    n = scene.desc.n_shapes
    c = np.array([scene._shapes[i].bs_center[:] for i in range(n)])
    r = np.array([scene._shapes[i].bs_radius for i in range(n)])
    ok = r > 0
    return (c[ok] - r[ok, None]).min(axis=0), (c[ok] + r[ok, None]).max(axis=0)


def _is_sdf(scene, sid):
    return sid >= 0 and scene._shapes[sid].kind != sh.K_MESH


def _family_rays(scene, coherent, ref, oracle, counts, rng):
    """(positions, directions) of counts[f] rays of every family f, from the scene's coherent Ray bundle and the oracle's solve of it."""
    P, D = {}, {}
    rec, rshape = ref.rec, ref.rec_shape
    rp, rd, rn, rt = rec[0:3].T, rec[3:6].T, rec[6], rec[7]
    hit = rshape >= 0
    sdf_hit = hit & np.array([_is_sdf(scene, int(s)) for s in rshape])
    assert sdf_hit.sum() >= 100
    # no start with a random direction in or on a plate or cube splitter, and no side-on ray aimed at one: a ray that total reflection
    # keeps inside the glass meets the coating on every pass, and its beam tree doubles with every pass
    trap = np.array([isinstance(o, (bmo.CubeBeamsplitter, bmo.RectangularPlateBeamsplitter)) for o in scene.leaf_objects] + [False])
    free = ~trap[ref.rec_obj]

    def pick(mask, m):
        idx = np.flatnonzero(mask)
        return idx[rng.integers(0, len(idx), m)]

    # forward: the scene's own rays
    m = counts[FORWARD]
    cols = np.arange(m) % coherent.n
    P[FORWARD], D[FORWARD] = coherent.planes[0:3, cols].T.copy(), coherent.planes[3:6, cols].T.copy()

    # backward: from a point on the last segment of a root's beam, behind the train, back along it (1 mrad of jitter)
    m = counts[BACKWARD]
    roots = np.flatnonzero(ref.node_parent < 0)
    last = (ref.node_first_rec[roots] + ref.node_nseg[roots] - 1)[ref.node_nseg[roots] >= 2]
    last = last[rng.integers(0, len(last), m)]
    s = np.where(np.isfinite(rt[last]), 0.5 * np.minimum(rt[last], 20 * mm), 5 * mm)
    P[BACKWARD] = rp[last] + s[:, None] * rd[last]
    D[BACKWARD] = _unit(-rd[last] + 1e-3 * rng.normal(size=(m, 3)))

    # around: between random points around and inside the scene's box
    m = counts[AROUND]
    lo, hi = scene_box(scene)
    span = hi - lo
    a = lo - 0.25 * span + rng.uniform(0, 1, (m, 3)) * 1.5 * span
    # (six in seven of the second points lie in the inner third of a shape's bounding sphere: in a box that is mostly empty, such
    #  as the cell's, uniform points alone would hardly ever put a shape in a ray's way)
    #  The shapes are taken in turn from a random order, so neighbouring rays aim at different ones.  The seventh ray of seven runs from its
    #  first point away from the middle of the box: whatever the scene, some lanes of a wave find nothing.)
    k = rng.permutation(scene.desc.n_shapes)[np.arange(m) % scene.desc.n_shapes]
    ball = _random_units(rng, m) * rng.uniform(0, 1, (m, 1)) ** (1 / 3)
    aimed = np.array([scene._shapes[int(i)].bs_center[:] for i in k]) + 0.3 * np.array([max(scene._shapes[int(i)].bs_radius, 0.0) for i in k])[:, None] * ball
    outward = a + (a - 0.5 * (lo + hi)) + 0.2 * span * rng.normal(size=(m, 3))
    b = np.where((np.arange(m) % 7 != 6)[:, None], aimed, outward)
    P[AROUND], D[AROUND] = a, _unit(b - a)

    # on-surface starts: recorded hit points (two thirds of them on SDF shapes) with the recorded direction, its reverse, a random one
    m = counts[SURFACE]
    r = np.where(np.arange(m) % 3 < 2, pick(sdf_hit, m), pick(hit, m))
    how = np.where(free[r], rng.integers(0, 3, m), rng.integers(0, 2, m))
    P[SURFACE] = rp[r] + rt[r, None] * rd[r]
    D[SURFACE] = np.where((how == 0)[:, None], rd[r], np.where((how == 1)[:, None], -rd[r], _random_units(rng, m)))

    # in-glass starts: mid-points of recorded segments with n > 1, random directions
    m = counts[GLASS]
    r = pick(hit & (rn > 1.0) & free, m)
    P[GLASS] = rp[r] + 0.5 * rt[r, None] * rd[r]
    D[GLASS] = _random_units(rng, m)

    # the SDF shapes that were hit, with the mean direction of the rays that hit them (the train's axis where they stand)
    sids = np.unique(rshape[sdf_hit & free])
    axis = {int(s): _unit(rd[rshape == s].mean(axis=0)) for s in sids}
    centre = {int(s): np.array(scene._shapes[int(s)].bs_center[:]) for s in sids}
    radius = {int(s): float(scene._shapes[int(s)].bs_radius) for s in sids}

    # side-on: across the axis onto barrels and mechanical rings
    m = counts[SIDE]
    s = sids[rng.integers(0, len(sids), m)]
    A = np.array([axis[int(k)] for k in s])
    C = np.array([centre[int(k)] for k in s])
    R = np.array([radius[int(k)] for k in s])[:, None]
    u = _perpendicular(rng, A)
    P[SIDE] = C + 1.5 * R * u + rng.uniform(-0.5, 0.5, (m, 1)) * R * A
    D[SIDE] = _unit(-u + 0.2 * rng.normal(size=(m, 3)))

    # near misses: lines through the outer shell of a shape's bounding sphere (0.9 - 0.999 R from its centre)
    m = counts[NEARMISS]
    s = sids[rng.integers(0, len(sids), m)]
    C = np.array([centre[int(k)] for k in s])
    R = np.array([radius[int(k)] for k in s])[:, None]
    w = _random_units(rng, m)
    d = _perpendicular(rng, w)
    P[NEARMISS] = C + rng.uniform(0.9, 0.999, (m, 1)) * R * w - 2 * R * d
    D[NEARMISS] = d

    # grazing: along the axis, within +-1e-7 m of the offset at which the line stops hitting the shape (bisected with the oracle)
    m = counts[GRAZE]
    rims = []
    for _ in range(200):
        if len(rims) >= max(4, m // 8):
            break
        k = int(sids[rng.integers(0, len(sids))])
        A, C, R = axis[k], centre[k], radius[k]
        u = _perpendicular(rng, A[None, :])[0]
        shape = scene.shape_list[k]

        def hits(off):
            return oracle.intersect_shape(scene, shape, C + off * u - 2 * R * A, A) is not None

        inner, outer = 0.0, 1.01 * R
        if not hits(inner) or hits(outer):
            continue
        while outer - inner > 1e-9:
            mid = 0.5 * (inner + outer)
            if hits(mid):
                inner = mid
            else:
                outer = mid
        rims.append((C + inner * u - 2 * R * A, u, A))
    assert len(rims) >= 4, "no rim found"
    which = np.arange(m) % len(rims)
    off = rng.uniform(-1e-7, 1e-7, m)
    P[GRAZE] = np.array([rims[j][0] + o * rims[j][1] for j, o in zip(which, off)])
    D[GRAZE] = np.array([rims[j][2] for j in which])
    return P, D


def _coherent_solution(name, n):
    import pyoracle

    system, parts = SCENES[name][0]()
    coherent = SCENES[name][1]("ray", n)
    scene = bmo.CompiledScene(system, coherent.lambdas)
    return system, parts, scene, coherent, pyoracle.trace(scene, coherent, R_MAX, threads=8)


def _bounded_trees(scene, pos, dirs, max_tree):
    """Mask of the rays whose beam tree has at most max_tree beams.  A train with a plate and a cube splitter traps some of the rays
    that come from all around: total reflection keeps them in the glass, they meet a coating on every pass and their tree doubles each
    time; neither the oracle nor the engine would finish them.  Only the host build of the lane code stops at a beam limit, so it
    does the selecting, in chunks, and ray by ray where a chunk runs away.  What the selected rays give is read from the oracle alone."""
    from tests.parity import emu_trace

    def trees(idx):
        part = bmo.RayBundle.rays(pos[idx], dirs[idx], LAM)
        try:
            res = emu_trace(scene, part, R_MAX, max_beams=max_tree * len(idx))
        except RuntimeError:
            if len(idx) == 1:
                return np.array([False])
            return np.concatenate([trees(idx[:len(idx) // 2]), trees(idx[len(idx) // 2:])])
        return np.bincount(res.node_root, minlength=len(idx)) <= max_tree

    idx = np.arange(len(pos))
    return np.concatenate([trees(idx[i:i + 32]) for i in range(0, len(idx), 32)])


def mixed_bundle(system, kind, n, seed, coherent, ref=None, scene=None, max_tree=0):
    """(bundle, family per ray): n beams of `kind` on `system`, ray i of family PATTERN[i % 32].  `coherent(kind, m)` is the system's
    own coherent bundle; the families are derived from the oracle's solve (`ref`, made here when not given) of its Ray form.
    max_tree > 0: three times as many rays are drawn and those with larger beam trees are left out (_bounded_trees)."""
    import pyoracle

    rng = np.random.default_rng(seed)
    fam = PATTERN[np.arange(n) % 32]
    counts = {f: int((fam == f).sum()) for f in range(8)}
    base = coherent("ray", max(256, counts[FORWARD]))
    if scene is None:
        scene = bmo.CompiledScene(system, base.lambdas)
    if ref is None:
        ref = pyoracle.trace(scene, base, R_MAX, threads=8)
    draw = {f: counts[f] * (3 if max_tree and f != FORWARD else 1) for f in range(8)}
    P, D = _family_rays(scene, base, ref, pyoracle, draw, rng)
    if max_tree:
        for f in range(1, 8):
            keep = np.flatnonzero(_bounded_trees(scene, P[f], D[f], max_tree))[:counts[f]]
            assert len(keep) == counts[f], (FAMILIES[f], len(keep), counts[f])
            P[f], D[f] = P[f][keep], D[f][keep]
    pos, dirs = np.zeros((n, 3)), np.zeros((n, 3))
    for f in range(8):
        pos[fam == f], dirs[fam == f] = P[f], D[f]
    bundle = _as_kind(kind, pos, dirs, rng)
    if kind != "ray":  # the forward family keeps the coherent bundle's own fields and beamlets
        own = coherent(kind, counts[FORWARD])
        planes = bundle.planes.copy()
        planes[:, fam == FORWARD] = own.planes
        bundle = bmo.RayBundle(bundle.kind, planes)
    return bundle, fam


@functools.lru_cache(maxsize=None)
def case(name, kind="ray", n=N_RAYS):
    """(system, parts, bundle, family per ray) of one of SCENES under its mixed bundle; built once per process."""
    system, parts, scene, coherent, ref = _coherent_solution(name, max(256, int((PATTERN[np.arange(n) % 32] == FORWARD).sum())))
    bundle, fam = mixed_bundle(system, kind, n, SCENES[name][2], SCENES[name][1], ref=ref, scene=scene, max_tree=MAX_TREE.get(name, 0))
    return system, parts, bundle, fam


def fresh_system(name):
    """A new instance of the scene (same numbers as case(name)'s) for a test that moves its parts."""
    return SCENES[name][0]()[0]


def move_first_doublet(system):
    """Moves the first DoubletLens of the system by 0.05 mm and turns it by 0.3 deg: the stored paths of the roots that cross it break."""
    doublet = next(o for o in system.objects() if isinstance(o, bmo.DoubletLens))
    bmo.translate3d(doublet, [0.05 * mm, 0.0, 0.0])
    bmo.xrotate3d(doublet, math.radians(0.3))
    return doublet


def head(bundle, n):
    return bmo.RayBundle(bundle.kind, bundle.planes[:, :n].copy())


def permuted(bundle, order):
    return bmo.RayBundle(bundle.kind, bundle.planes[:, order].copy())


def family_order(fam):
    """The permutation that numbers a mixed bundle family after family (coherent waves), each family in its own order."""
    return np.argsort(fam, kind="stable")


# ------------------------------------------------------------------ bad lanes
def bad_lanes(bundle):
    """(bundle, bad mask): every 97th ray (index 0, lane 0 of a wave, included) replaced in turn by the six rows of
    tests/test_degenerate_rays.py::special_bundle: NaN position, NaN direction, zero direction, infinite position, infinite direction,
    a start 1e30 m away.  The planes are written directly, so the good rays stay the same doubles."""
    from tests.mesh_scenes import with_bad_lanes

    pos, dirs, bad = with_bad_lanes(bundle.planes[0:3].T, bundle.planes[3:6].T)
    planes = bundle.planes.copy()
    planes[0:3], planes[3:6] = pos.T, dirs.T
    return bmo.RayBundle(bundle.kind, planes), bad


# ------------------------------------------------------------------ root by root
NODE_FIELDS = ("node_nseg", "node_status", "node_aux")


def by_root(res):
    """Per root, what its beam tree holds, free of the numbering of roots, nodes and records: a list (one entry per root) of dicts
    with the nodes' nseg / status / aux, parent and first child as positions within the root's own node list (-1: none), and the
    records' obj / shape / planes.  Nodes come root by root and breadth-first within a root, records node by node (include/bmo.h)."""
    root = res.node_root
    assert (np.diff(root) >= 0).all(), "nodes are not grouped root by root"
    first = np.searchsorted(root, np.arange(res.n_roots), side="left")
    end = np.searchsorted(root, np.arange(res.n_roots), side="right")
    out = []
    for r in range(res.n_roots):
        a, b = int(first[r]), int(end[r])
        r0 = int(res.node_first_rec[a]) if b > a else 0
        r1 = int(res.node_first_rec[b - 1] + res.node_nseg[b - 1]) if b > a else 0
        par, kid = res.node_parent[a:b], res.node_first_child[a:b]
        out.append(dict(
            nseg=res.node_nseg[a:b], status=res.node_status[a:b], aux=res.node_aux[a:b],
            parent=np.where(par >= 0, par - a, -1), first_child=np.where(kid >= 0, kid - a, -1),
            first_rec=res.node_first_rec[a:b] - r0,
            rec_obj=res.rec_obj[r0:r1], rec_shape=res.rec_shape[r0:r1], rec=np.ascontiguousarray(res.rec[:, r0:r1])))
    return out


def _same_bits(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    if x.shape != y.shape:
        return False
    if x.dtype.kind == "f":
        return bool(((x.view(np.int64) == y.view(np.int64)) | (np.isnan(x) & np.isnan(y))).all())
    return bool(np.array_equal(x, y))


def roots_differing(a, b, pairs):
    """The (i, j) of `pairs` for which root i of by_root list `a` and root j of `b` differ in any field, bit for bit."""
    return [(int(i), int(j)) for i, j in pairs if not all(_same_bits(a[i][k], b[j][k]) for k in a[i])]

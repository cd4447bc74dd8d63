"""Tessellated meshes and the two mesh scenes of the BVH tests (DESIGN.md §3 "mesh BVH").

H: the config-2 train (tests/scenes.py c2_scene) inside a tessellated spherical housing of 20 480 faces, an IntersectableObject: every
   ray tests it at every bounce, and whatever leaves the train ends on it.
M: a concave spherical mirror of ~20 000 faces, tilted, focusing a collimated bundle onto a Spotdetector off the incoming beam.

And the inputs of the traversal tests: five meshes with seven families of directed rays (tests/test_mesh_bvh.py), the same rays dealt so
that every wave of 64 holds all seven families, with non-finite rays among them, and the light trap, a scene of several BVH meshes in which
rays bounce in all directions (tests/test_mesh_bvh_waves.py, tests/test_mesh_bvh_waves_gpu.py).
"""
import functools
import math

import numpy as np

import bmo_amd as bmo

from tests import scenes

mm = 1e-3


def icosphere(level, radius=1.0, center=(0.0, 0.0, 0.0)):
    """(vertices, faces) of an icosahedron subdivided `level` times onto the sphere: 20 * 4**level faces."""
    p = (1 + math.sqrt(5)) / 2
    v = [[-1, p, 0], [1, p, 0], [-1, -p, 0], [1, -p, 0], [0, -1, p], [0, 1, p], [0, -1, -p], [0, 1, -p], [p, 0, -1], [p, 0, 1], [-p, 0, -1], [-p, 0, 1]]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
         [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    verts = [np.array(x, dtype=np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        mids, nf = {}, []

        def mid(a, b):
            k = (min(a, b), max(a, b))
            if k not in mids:
                m = verts[a] + verts[b]
                verts.append(m / np.linalg.norm(m))
                mids[k] = len(verts) - 1
            return mids[k]

        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        f = nf
    return np.array(verts) * radius + np.asarray(center, dtype=np.float64), np.array(f, dtype=np.int64)


def spherical_cap(R, aperture, n_rings, n_seg):
    """(vertices, faces) of a spherical cap of radius R around +y, centre of curvature at the origin, rim radius aperture / 2:
    n_seg * (2 n_rings - 1) faces (a fan at the pole, quads split in two outside it)."""
    a_max = math.asin(aperture / 2 / R)
    verts = [[0.0, R, 0.0]]
    for i in range(1, n_rings + 1):
        a = a_max * i / n_rings
        for j in range(n_seg):
            b = 2 * math.pi * j / n_seg
            verts.append([R * math.sin(a) * math.cos(b), R * math.cos(a), R * math.sin(a) * math.sin(b)])
    ring = lambda i, j: 1 + (i - 1) * n_seg + (j % n_seg)  # noqa: E731
    faces = [[0, ring(1, j), ring(1, j + 1)] for j in range(n_seg)]
    for i in range(1, n_rings):
        for j in range(n_seg):
            faces += [[ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)], [ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)]]
    return np.array(verts, dtype=np.float64), np.array(faces, dtype=np.int64)


def housing_scene(level=5):
    """H: c2_scene inside an icosphere housing (level 5: 20 480 faces) of radius 40 mm around the middle of the train."""
    system, parts = scenes.c2_scene()
    v, f = icosphere(level, 40 * mm, (0.0, 0.0, 16 * mm))
    housing = bmo.IntersectableObject(bmo.Mesh(v, f))
    return bmo.System(list(system.objects()) + [housing]), dict(parts, system=system, housing=housing)


def housing_bundle(n, seed=scenes.SEED):
    """The vignetted config-2 bundle: part of it misses the train and runs into the housing."""
    return scenes.c2_vignetted_bundle(n, seed=seed)


R_M = 100 * mm        # radius of curvature of M
Y_M = 60 * mm         # vertex of M on the y axis
TILT_M = math.radians(10)


def mirror_scene(n_rings=50, n_seg=200):
    """M: a concave spherical mirror (R = 100 mm, 25 mm across; 50 rings x 200 segments = 19 800 faces) facing -y with its vertex at
    y = 60 mm, tilted 10 deg about x, and a 6 mm Spotdetector at its paraxial focus (off the incoming beam)."""
    v, f = spherical_cap(R_M, 25 * mm, n_rings, n_seg)
    v = v - np.array([0.0, R_M, 0.0])  # vertex at the origin, centre of curvature at -R y: concave to rays coming from -y
    mesh = bmo.Mesh(v, f)
    mirror = bmo.Mirror(mesh)
    bmo.xrotate3d(mirror, TILT_M)
    bmo.translate3d(mirror, [0, Y_M, 0])
    # the chief ray along +y hits the vertex, where the normal is y turned by the tilt; the focus is R/2 along the reflected ray
    n = np.array([0.0, math.cos(TILT_M), math.sin(TILT_M)])
    d = np.array([0.0, 1.0, 0.0])
    r = d - 2 * np.dot(d, n) * n
    focus = np.array([0.0, Y_M, 0.0]) + r * (R_M / 2)
    det = bmo.Spotdetector(6 * mm)
    # Spotdetector's surface normal is its local y axis: turn it onto the reflected chief ray
    bmo.xrotate3d(det, math.atan2(r[2], r[1]))
    bmo.translate3d(det, list(focus))
    return bmo.System([mirror, det]), dict(mirror=mirror, det=det, focus=focus, axis=r)


def mirror_bundle(n, seed=scenes.SEED):
    """Collimated (2 mrad jitter) disc 20 mm across along +y."""
    return scenes.disc_bundle(n, center=[0, 0, 0], direction=[0, 1, 0], diameter=20 * mm, lam=1.064e-6, e1=[1, 0, 0], seed=seed)


def bundle_of(kind, scene_name, n, seed=scenes.SEED):
    """Ray / PolarizedRay / GaussianBeamlet bundles for H and M."""
    if scene_name == "H":
        center, direction, diameter = [0, 0, -0.77 * mm], [0, 0, 1], 2.0 * mm
    else:
        center, direction, diameter = [0, 0, 0], [0, 1, 0], 20 * mm
    if kind == "ray":
        return housing_bundle(n, seed) if scene_name == "H" else mirror_bundle(n, seed)
    if kind == "pol":
        return scenes.polarized_bundle(n, center=center, direction=direction, diameter=diameter, seed=seed)
    return scenes.gaussian_bundle(n, center=center, direction=direction, diameter=diameter, w0=50e-6, cone=0.3 if scene_name == "H" else None,
                                  seed=seed)


# ------------------------------------------------------------------ the five meshes of the traversal tests (tests/test_mesh_bvh.py)
KEPS = 1e-9  # mt_keps of CompiledScene
LEPS = 1e-9


def _sphere():
    return icosphere(3, 7 * mm, (1 * mm, -2 * mm, 3 * mm))  # 1 280 faces


def _soup(rng, n=1000):
    """Random triangles of mixed scales (edges from 1 um to 10 mm) in a 20 mm box."""
    c = rng.uniform(-10 * mm, 10 * mm, (n, 1, 3))
    s = 10.0 ** rng.uniform(-6, -2, (n, 1, 1))
    v = (c + s * rng.normal(size=(n, 3, 3))).reshape(-1, 3)
    return v, np.arange(3 * n).reshape(n, 3)


def _slivers(rng, n=600):
    """Needle triangles: two vertices far apart, the third a hair off their line."""
    a = rng.uniform(-10 * mm, 10 * mm, (n, 3))
    b = a + rng.normal(size=(n, 3)) * 5 * mm
    w = rng.uniform(0, 1, (n, 1))
    c = a + w * (b - a) + rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-12, -7, (n, 1))
    v = np.stack([a, b, c], axis=1).reshape(-1, 3)
    return v, np.arange(3 * n).reshape(n, 3)


def _cuboid_grid(k=8, size=(10 * mm, 6 * mm, 8 * mm)):
    """A cuboid whose six sides are k x k grids of coplanar face pairs (6 * 2 k^2 faces) sharing edges and vertices."""
    verts, faces = [], []
    sx, sy, sz = size
    for ax in range(3):
        for side in (0.0, 1.0):
            u, w = [a for a in range(3) if a != ax]
            base = len(verts)
            for i in range(k + 1):
                for j in range(k + 1):
                    p = [0.0, 0.0, 0.0]
                    p[ax], p[u], p[w] = side, i / k, j / k
                    verts.append([p[0] * sx, p[1] * sy, p[2] * sz])
            for i in range(k):
                for j in range(k):
                    a, b, c, d = base + i * (k + 1) + j, base + (i + 1) * (k + 1) + j, base + (i + 1) * (k + 1) + j + 1, base + i * (k + 1) + j + 1
                    faces += [[a, b, c], [a, c, d]]
    return np.array(verts), np.array(faces)


def _fan():
    m = bmo.CircularFlatMesh(20 * mm, 2400)  # test_fuzz.py::test_scene_larger_than_lds's mirror
    bmo.xrotate3d(m, math.radians(20))
    bmo.translate3d(m, [0, 60 * mm, 0])
    return m.vertices, m.faces


MESHES = {
    "sphere": (lambda rng: _sphere(), 250_000),
    "soup": (_soup, 200_000),
    "slivers": (_slivers, 150_000),
    "cuboid": (lambda rng: _cuboid_grid(), 250_000),
    "fan": (lambda rng: _fan(), 150_000),
}


# ------------------------------------------------------------------ rays
def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def _ray_families(rng, v, f, n):
    """The seven families of _rays as two lists of (m_k, 3) arrays, positions and directions."""
    tri = v[f]
    lo, hi = v.min(axis=0), v.max(axis=0)
    span = hi - lo
    k = n // 7
    P, D = [], []

    def origins(m):
        return lo - span + rng.uniform(0, 1, (m, 3)) * 3 * span

    def face_points(m):
        i = rng.integers(0, len(f), m)
        w = rng.dirichlet([1, 1, 1], m)
        return i, np.einsum("mk,mkj->mj", w, tri[i])

    # random lines through random points of faces (hits)
    o = origins(k)
    _, q = face_points(k)
    P.append(o), D.append(q - o)
    # through vertices (every face around a vertex is hit at the same t)
    o = origins(k)
    P.append(o), D.append(v[rng.integers(0, len(v), k)] - o)
    # through midpoints of edges (two faces share the edge)
    o = origins(k)
    i = rng.integers(0, len(f), k)
    e = rng.integers(0, 3, k)
    a, b = tri[i, e], tri[i, (e + 1) % 3]
    P.append(o), D.append(0.5 * a + 0.5 * b - o)
    # grazing: in the face's plane plus a normal part that puts |Det| just above (or at) kϵ
    i, q = face_points(k)
    E1, E2 = tri[i, 1] - tri[i, 0], tri[i, 2] - tri[i, 0]
    N = np.cross(E1, E2)
    nn = np.linalg.norm(N, axis=1)
    ok = nn > 0
    inplane = _unit(np.cross(N[ok], rng.normal(size=(ok.sum(), 3))))
    alpha = (KEPS * rng.choice([0.999, 1.0, 1.0 + 1e-9, 1.001, 1.1, 2.0], ok.sum()) / nn[ok])[:, None]
    d = inplane + alpha * (N[ok] / nn[ok, None])
    P.append(q[ok] - d * rng.uniform(0.01, 1.0, (ok.sum(), 1)) * np.linalg.norm(span)), D.append(d)
    # axis-parallel, origins with coordinates taken from vertices (on the faces' box planes)
    o = origins(k)
    vv = v[rng.integers(0, len(v), (k, 3))]
    axis = rng.integers(0, 3, k)
    for c in range(3):
        m = axis != c
        o[m, c] = vv[m, c, c]
    d = np.zeros((k, 3))
    d[np.arange(k), axis] = rng.choice([-1.0, 1.0], k)
    P.append(o), D.append(d)
    # starting on a face: t around lϵ for the face it starts on
    i, q = face_points(k)
    d = _unit(rng.normal(size=(k, 3)))
    back = rng.choice([0.0, 0.5 * LEPS, LEPS, 1.5 * LEPS, 3 * LEPS, 1e-6], k)[:, None]
    P.append(q - back * d), D.append(d)
    # inside the leaf boxes
    m = n - 6 * k
    i = rng.integers(0, len(f), m)
    o = tri[i].mean(axis=1) + rng.normal(size=(m, 3)) * 1e-9
    P.append(o), D.append(_unit(rng.normal(size=(m, 3))))
    return P, D


def _rays(rng, v, f, n):
    """n rays in seven families: random, through vertices, through shared-edge midpoints, grazing (|Det| just above kϵ),
    axis-parallel (origins on vertex coordinates, i.e. on slab planes), starting on a face (t around lϵ), starting inside the mesh's
    leaf boxes (a face's centroid, a hair off)."""
    P, D = _ray_families(rng, v, f, n)
    return np.concatenate(P), np.concatenate(D)


# ------------------------------------------------------------------ incoherent waves (tests/test_mesh_bvh_waves*.py)
WAVE = 64  # rays 64 w .. 64 w + 63 of a bundle are wave w of the first launch when the root order is left alone (BMO_ROOT_ORDER=none)


def interleaved_rays(rng, v, f, n):
    """The rays of _rays(rng, v, f, n) dealt round-robin over the seven families: ray i comes from family i mod 7 until a family runs
    out, so every full wave holds all seven.  Returns (pos, dir, family index per ray)."""
    P, D = _ray_families(rng, v, f, n)
    fam = np.concatenate([np.full(len(p), j) for j, p in enumerate(P)])
    rank = np.concatenate([np.arange(len(p)) for p in P])
    order = np.lexsort((fam, rank))  # by position within the family, then by family
    return np.concatenate(P)[order], np.concatenate(D)[order], fam[order]


DIRECTED_SEED = 20251016
DIRECTED_N = 7 * 2048 + 1  # 224 full waves and one ray


@functools.lru_cache(maxsize=None)
def directed_case(name):
    """(v, f, bundle, family per ray) of one of MESHES under DIRECTED_N interleaved rays.  The rays the engine gets are
    bundle.planes[0:6]: RayBundle.rays normalises the directions again, and a host query must see the same doubles as the trace."""
    rng = np.random.default_rng(DIRECTED_SEED)
    v, f = MESHES[name][0](rng)
    pos, dir, fam = interleaved_rays(rng, v, f, DIRECTED_N)
    return v, f, bmo.RayBundle.rays(pos, dir, 1.064e-6), fam


BAD_STRIDE = 97  # coprime with 64: over a bundle the bad lane takes every lane position (index 0 and 6208 = 97 * 64: lane 0)


def with_bad_lanes(pos, dir):
    """(pos, dir, bad mask): every ray whose index is a multiple of 97 replaced, in turn, by one of the six non-finite rows of
    tests/test_degenerate_rays.py::special_bundle — NaN position, NaN direction, zero direction, infinite position, infinite
    direction, position 1e30."""
    from tests.test_degenerate_rays import special_bundle

    rows = special_bundle("c1").planes[0:6, 1:7].T
    assert not np.isfinite(rows[:5]).all(axis=1).any() and rows[5, 0] == 1e30
    pos, dir = np.array(pos, dtype=np.float64), np.array(dir, dtype=np.float64)
    idx = np.arange(0, len(pos), BAD_STRIDE)
    pos[idx] = rows[np.arange(len(idx)) % 6, 0:3]
    dir[idx] = rows[np.arange(len(idx)) % 6, 3:6]
    bad = np.zeros(len(pos), dtype=bool)
    bad[idx] = True
    return pos, dir, bad


def bad_lane_bundle(bundle):
    """(a Ray bundle with with_bad_lanes' rows in place of every 97th ray, bad mask).  The planes are written directly: RayBundle.rays
    would normalise the directions once more, and the good rays must stay the same doubles."""
    pos, dir, bad = with_bad_lanes(bundle.planes[0:3].T, bundle.planes[3:6].T)
    planes = bundle.planes.copy()
    planes[0:3], planes[3:6] = pos.T, dir.T
    return bmo.RayBundle(bundle.kind, planes), bad


def one_mesh_scene(v, f, lambdas=(1.064e-6,), mesh_bvh=True):
    return bmo.CompiledScene(bmo.System([bmo.IntersectableObject(bmo.Mesh(v, f))]), list(lambdas), mesh_bvh=mesh_bvh)


# ------------------------------------------------------------------ the light trap
TRAP_SEED = 20251017
TRAP_SOURCE = (10 * mm, 0.0, 0.0)


def light_trap_scene():
    """Four BVH meshes and one brute-force mesh that rays bounce between for as long as r_max lets them: a glass ball (1 280 faces)
    off-centre between two flat mirrors of 63 faces (one below the BVH threshold) and 64 faces (the smallest mesh with a BVH), all inside
    a mirror shell of 1 280 faces, and `shell2`, a second mirror over a copy of the shell's vertices and faces: every hit of the shell is
    a tie between the two, which the later object loses (`offer` accepts only t < x_t)."""
    ball = bmo.Lens(bmo.Mesh(*icosphere(3, 5 * mm, (0.3 * mm, -0.2 * mm, 0.1 * mm))), 1.5)
    flat63 = bmo.Mirror(bmo.CircularFlatMesh(6 * mm, bmo.shapes.MESH_BVH_MIN_FACES - 1))
    bmo.translate3d(flat63, [0, 12 * mm, 0])
    flat64 = bmo.Mirror(bmo.CircularFlatMesh(6 * mm, bmo.shapes.MESH_BVH_MIN_FACES))
    bmo.translate3d(flat64, [0, -12 * mm, 0])
    v, f = icosphere(3, 20 * mm)
    shell = bmo.Mirror(bmo.Mesh(v, f))
    shell2 = bmo.Mirror(bmo.Mesh(v.copy(), f.copy()))
    objs = [ball, flat63, flat64, shell, shell2]
    return bmo.System(objs), dict(ball=ball, flat63=flat63, flat64=flat64, shell=shell, shell2=shell2, objects=objs)


def light_trap_bundle(kind, n, seed=TRAP_SEED):
    """n beams from a 6 mm cube around (10, 0, 0) mm inside the shell, going everywhere: Ray positions uniform in the cube with isotropic
    directions; PolarizedRay and GaussianBeamlet from scenes.polarized_bundle / gaussian_bundle (a 6 mm disc facing the ball, directions
    up to 1.2 rad off its axis).  The columns are permuted, so neighbouring lanes hold unrelated beams."""
    rng = np.random.default_rng(seed)
    if kind == "ray":
        pos = np.array(TRAP_SOURCE) + rng.uniform(-3 * mm, 3 * mm, (n, 3))
        b = bmo.RayBundle.rays(pos, rng.normal(size=(n, 3)), 1.064e-6)
    elif kind == "pol":
        b = scenes.polarized_bundle(n, center=TRAP_SOURCE, direction=[-1, 0, 0], diameter=6 * mm, jitter=1.2, seed=seed)
    else:
        b = scenes.gaussian_bundle(n, center=TRAP_SOURCE, direction=[-1, 0, 0], diameter=6 * mm, w0=50e-6, support=(0.0, 0.0, 1.0), cone=1.2,
                                   seed=seed)
    return bmo.RayBundle(b.kind, b.planes[:, np.random.default_rng(seed + 1).permutation(n)])

"""Tessellated meshes and the two mesh scenes of the BVH tests (DESIGN.md §3 "mesh BVH").

H: the config-2 train (tests/scenes.py c2_scene) inside a tessellated spherical housing of 20 480 faces, an IntersectableObject: every
   ray tests it at every bounce, and whatever leaves the train ends on it.
M: a concave spherical mirror of ~20 000 faces, tilted, focusing a collimated bundle onto a Spotdetector off the incoming beam.
"""
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

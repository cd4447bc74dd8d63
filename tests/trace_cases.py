"""The scenes of tests/test_trace_reference.py and tests/test_trace_reference_gpu.py, and the comparison both make (not a test file).

A scene is written twice from the same prescription: once for the host mirror (bmo objects, what oracle, emulator and engine trace) and once
for the exact evaluator of tests/trace_ref.py, which gets the prescription's numbers and the pose doubles position() / orientation() of each
object and nothing else of the host's scene."""
import dataclasses
import math

import numpy as np

import bmo_amd as bmo
import trace_ref as tr

mm = 1e-3
R_MAX = 30


@dataclasses.dataclass
class Case:
    """What a scene carries.  The builders fill the first block, compile_case the second, the tests the third."""

    name: str = ""
    system: object = None      # bmo.System: what oracle, emulator and engine trace
    exact: list = None         # the same objects for tests/trace_ref.py, in the order of the system's leaves
    bundle: object = None      # bmo.RayBundle
    lens: object = None        # the singlet / asphere scenes' lens (the retrace test moves it)
    det: object = None

    scene: object = None       # bmo.CompiledScene
    consts: dict = None        # the march constants of the compiled scene
    shape_part: dict = None    # shape id of the record -> part of its doublet

    res: object = None         # the oracle's TraceResult
    cache: dict = None         # exact evaluation and bound per bounce of res
    held: object = None        # Held of res
    small: object = None       # the bundle before widen()

    __hash__ = object.__hash__


# ------------------------------------------------------------------------------------------------ ray fans
def _frame(axis):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    e1 = np.cross(a, [0.0, 0.0, 1.0] if abs(a[2]) < 0.9 else [1.0, 0.0, 0.0])
    e1 /= np.linalg.norm(e1)
    return a, e1, np.cross(a, e1)


def ring(center, axis, radius, n, back=30 * mm, phase=0.1, slope=0.0):
    """n rays through a ring of `radius` about `center`, starting `back` before it along their own direction; slope tilts each ray outwards
    (the tangent of its angle to the axis)."""
    a, e1, e2 = _frame(axis)
    phi = phase + 2 * math.pi * np.arange(n) / n
    rad = np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2
    d = a[None, :] + slope * rad
    d = d / np.linalg.norm(d, axis=1)[:, None]
    return np.asarray(center) + radius * rad - back * d, d


def disc(center, direction, diameter, n, back=30 * mm):
    """A Fibonacci disc of n parallel rays (BeamGroups.jl:232-243) through `center`."""
    a, e1, e2 = _frame(direction)
    k = np.arange(n)
    r = diameter / 2 * np.sqrt((k + 0.5) / n)
    phi = k * (2 * math.pi / (1 + math.sqrt(5)))
    pos = np.asarray(center) + (r * np.cos(phi))[:, None] * e1 + (r * np.sin(phi))[:, None] * e2 - back * a
    return pos, np.tile(a, (n, 1))


def bundle(kind, pos, dirs, lam=1.064e-6):
    pos, dirs = np.vstack(pos), np.vstack(dirs)
    b = bmo.RayBundle.rays(pos, dirs, lam)
    if kind == "ray":
        return b
    d = b.planes[3:6].T
    E = np.tile(np.array([1.0, 0.2, 0.5]), (b.n, 1))
    for _ in range(3):  # Gram-Schmidt against the direction, to 1e-16 (PolarizedRays.jl:54: orthogonal to 1e-14)
        E = E - (E * d).sum(axis=1)[:, None] * d
    E = E / np.linalg.norm(E, axis=1)[:, None]
    P = np.zeros((14, b.n))
    P[:8] = b.planes
    P[8:14:2] = E.T
    P[9:14:2] = 0.3 * np.cross(d, E).T  # an elliptical state: Im(E0) = 0.3 dir x Re(E0), orthogonal to dir as well
    return bmo.RayBundle(bmo.BEAM_POLARIZED, P)


def gauss_bundle(pos, dirs, lam=1.064e-6, w0=50e-6, support=(1.0, 0.0, 0.0)):
    """GaussianBeamlet(pos, dir, lam, w0; support) per ray, as the reference's constructor builds chief, waist and divergence ray
    (Gaussian.jl:215-256; the layout of tests/scenes.py gaussian_bundle)."""
    b = bmo.RayBundle.rays(np.vstack(pos), np.vstack(dirs), lam)
    p, d = b.planes[0:3].T, b.planes[3:6].T
    s1 = np.asarray(support, dtype=np.float64)
    tan_t = np.tan(np.asarray(lam, dtype=np.float64) / (math.pi * w0)) * np.ones(b.n)
    dd = d + s1[None, :] * tan_t[:, None]
    dd = dd / np.sqrt((dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2])[:, None]
    P = np.zeros((25, b.n))
    P[0:3], P[3:6] = p.T, d.T
    P[6:9], P[9:12] = (p + s1[None, :] * w0).T, d.T
    P[12:15], P[15:18] = p.T, dd.T
    P[18], P[19], P[20] = lam, 1.0, w0
    P[21] = math.sqrt(2 * (2 * 1e-3 / (math.pi * w0 ** 2)) * bmo.linalg.Z_vacuum)
    return bmo.RayBundle(bmo.BEAM_GAUSSIAN, P)


def widen(b, n):
    """The case's bundle repeated with small deterministic offsets up to n rays (the GPU tests' 1 024)."""
    reps = -(-n // b.n)
    P = np.tile(b.planes, (1, reps))[:, :n].copy()
    k = np.arange(n) // b.n
    for x in ((0, 6, 12) if b.kind == bmo.BEAM_GAUSSIAN else (0,)):
        P[x] += 1.7e-6 * k
        P[x + 2] -= 2.3e-6 * k
    return bmo.RayBundle(b.kind, P)


# ------------------------------------------------------------------------------------------------ scene 1: biconvex singlet
S1 = dict(r1=40 * mm, r2=-60 * mm, l=4 * mm, d=25.4 * mm, n=1.6)


def singlet(kind="ray", planted=None, move=None):
    """SphericalLens(40 mm, -60 mm, 4 mm, 25.4 mm, 1.6) tilted 7 degrees about x and decentred 1.5 mm, a PSFDetector 60 mm behind it.  Rays: a
    12 degree oblique disc over 0.9 of the aperture, two rays on the lens's own axis (the apex tie), rings at 0.5 and 0.99 of the clear aperture
    along the axis, and a steep outward ring that enters through the face and meets the barrel from inside."""
    c = Case()
    lens = bmo.SphericalLens(S1["r1"], S1["r2"], S1["l"], S1["d"], S1["n"])
    bmo.xrotate3d(lens, math.radians(7))
    bmo.translate3d(lens, [1.5 * mm, 20 * mm, 0])
    # a PSFDetector takes Rays only (PSFDetector.jl:77), a Spotdetector Beams only (Spotdetector.jl:50): beamlets end on a plain stop
    det = {"ray": lambda: bmo.PSFDetector(90 * mm), "pol": lambda: bmo.Spotdetector(90 * mm),
           "gauss": lambda: bmo.IntersectableObject(bmo.QuadraticFlatMesh(90 * mm))}[kind]()
    dk = {"ray": "psf", "pol": "spot", "gauss": "stop"}[kind]
    bmo.translate3d(det, [0, 80 * mm, 0])
    if move is not None:  # the kinematic move of the retrace test
        bmo.translate3d(lens, move[0])
        bmo.zrotate3d(lens, move[1])
    c.system, c.lens, c.det = bmo.System([lens, det]), lens, det
    c.exact = [tr.ExactLens(tr.Surface(S1["r1"]), tr.Surface(S1["r2"]), S1["l"], S1["d"], lambda lam: S1["n"], lens.position(), lens.orientation(), planted),
               tr.ExactFlat(90 * mm, det.position(), det.orientation(), dk)]
    p0 = np.array([1.5 * mm, 20 * mm, 0.0])                 # where the un-moved lens's front vertex is: the fans do not follow a move
    t7 = math.radians(7)
    axis = np.array([0.0, math.cos(t7), math.sin(t7)])      # its axis: +y turned by 7 degrees about x
    mid = p0 + 2 * mm * axis
    ob = math.radians(12)
    P, D = zip(disc(mid, [math.sin(ob), math.cos(ob), 0.0], 0.9 * S1["d"], 36),
               ring(p0, axis, 0.0, 2),
               ring(p0, axis, 0.5 * S1["d"] / 2, 8),
               ring(p0, axis, 0.99 * S1["d"] / 2, 8, phase=0.37),
               ring(p0 + 1.9 * mm * axis, axis, 0.985 * S1["d"] / 2, 10, back=6 * mm, phase=0.2, slope=0.8))
    c.bundle = gauss_bundle(P[:3] + (ring(p0, axis, 0.25 * S1["d"] / 2, 2, phase=1.3)[0],), D[:3] + (ring(p0, axis, 0.25 * S1["d"] / 2, 2, phase=1.3)[1],)) if kind == "gauss" else bundle(kind, P, D)  # beamlets: without the edge rings (their three rays part there)
    c.name = "singlet-" + kind
    return c


# ------------------------------------------------------------------------------------------------ scene 4: AL50100J asphere
AL = dict(R=50.3583 * mm, D=50 * mm, CT=10.2 * mm, K=-0.789119, N=1.5036, A=[0, 2.10405e-7 * (1e3) ** 3, 1.76468e-11 * (1e3) ** 5, 1.02641e-15 * (1e3) ** 7])


def asphere(flip=False, planted=None):
    """Thorlabs AL50100J (the prescription of the reference's test, runtests.jl: radius, conic constant, A4 - A8, 50 mm, 10.2 mm), curved side
    (flip: plane side) towards a bundle that fills 0.98 of the aperture, 3 degrees oblique."""
    c = Case()
    lens = bmo.Lens(bmo.EvenAsphericalSurface(AL["R"], AL["D"], AL["K"], AL["A"]), AL["CT"], lambda lam: AL["N"])
    if flip:
        bmo.xrotate3d(lens, math.radians(180))
        bmo.translate3d(lens, [0, AL["CT"], 0])
    bmo.zrotate3d(lens, math.radians(2))
    bmo.translate3d(lens, [0.4 * mm, 30 * mm, -0.3 * mm])
    det = bmo.PSFDetector(120 * mm)
    bmo.translate3d(det, [0, 90 * mm, 0])
    c.system, c.lens, c.det = bmo.System([lens, det]), lens, det
    c.exact = [tr.ExactLens(tr.Surface(AL["R"], AL["K"], AL["A"]), tr.Surface(math.inf), AL["CT"], AL["D"], lambda lam: AL["N"], lens.position(),
                            lens.orientation(), planted),
               tr.ExactFlat(120 * mm, det.position(), det.orientation(), "psf")]
    mid = np.array([0.4 * mm, 30 * mm + AL["CT"] / 2, -0.3 * mm])
    ob = math.radians(3)
    P, D = zip(disc(mid, [0.0, math.cos(ob), math.sin(ob)], 0.9 * AL["D"], 40, back=40 * mm),
               ring(mid, [0, 1, 0], 0.98 * AL["D"] / 2, 8, back=40 * mm, phase=0.3),
               ring(mid, [0, 1, 0], 0.0, 1, back=40 * mm))
    c.bundle = bundle("ray", P, D)
    c.name = "asphere-" + ("plane-first" if flip else "curved-first")
    return c


_K = 1e3
L3 = dict(front=(3.618e-3, 3.04e-3, -44.874, [0, -0.14756 * _K ** 3, 0.035194 * _K ** 5, -0.0032262 * _K ** 7, 0.0018592 * _K ** 9, 0.00036658 * _K ** 11,
                                              -0.00016039 * _K ** 13, -3.1846e-5 * _K ** 15]),
          back=(2.161e-3, 3.7e-3, -10.719, [0, -0.096568 * _K ** 3, 0.026771 * _K ** 5, -0.011261 * _K ** 7, 0.0019879 * _K ** 9, 0.00015579 * _K ** 11,
                                            -0.00012433 * _K ** 13, 1.5264e-5 * _K ** 15]),
          ct=0.7e-3, n=1.580200)  # (radius, clear aperture, conic constant, A2 .. A16) of element L3 (runtests.jl:1581-1696; tests/test_asphere_system.py)


L3_CREST = 0.600108e-3  # where the front profile's sag is largest (22.51 um): sag' = 0, found in the test in 50 digits


def phone_l3(planted=None, crest=False):
    """Element L3 of the phone objective: two even aspheres of order 16 whose profiles are INFLECTED (the sag rises to 22 um / 90 um and falls to
    -188 um / -404 um at the edge), clear apertures 3.04 mm and 3.7 mm.  The reference closes the front leaf at its largest sag and the back
    leaf at its edge height, and levels the step with a ring that reaches down to the front edge (Lenses.jl:234-246): the centre thickness,
    both largest sags and both edge sags decide where every face lies.  A line can cross such a profile more than once.  Rays: a 3 degree oblique
    disc over 0.98 of the front aperture (38 rays: none within 15 um of the crest of the front profile, which is a seam - crest=True aims there),
    axis-parallel rays onto the ring's plane face, one on the axis."""
    c = Case()
    E = bmo.EvenAsphericalSurface
    (r1, d1, k1, a1), (r2, d2, k2, a2) = L3["front"], L3["back"]
    lens = bmo.Lens(E(r1, d1, k1, a1), E(r2, d2, k2, a2), L3["ct"], lambda lam: L3["n"])
    bmo.xrotate3d(lens, math.radians(2))
    bmo.translate3d(lens, [0.05 * mm, 5 * mm, -0.03 * mm])
    det = bmo.PSFDetector(12 * mm)
    bmo.translate3d(det, [0, 9 * mm, 0])
    c.system, c.lens, c.det = bmo.System([lens, det]), lens, det
    c.exact = [tr.ExactRingLens(tr.Surface(r1, k1, a1), tr.Surface(r2, k2, a2), L3["ct"], lambda lam: L3["n"], d1, d2, d1, d2, lens.position(),
                                lens.orientation(), planted),
               tr.ExactFlat(12 * mm, det.position(), det.orientation(), "psf")]
    at = np.array([0.05 * mm, 5 * mm, -0.03 * mm])
    ob = math.radians(2.5)
    P, D = zip(disc(at, [0.0, math.cos(ob), math.sin(ob)], 0.98 * d1, 38, back=3 * mm), ring(at, [0, 1, 0], 1.7 * mm, 9, back=3 * mm, phase=0.2),
               ring(at, [0, 1, 0], 0.0, 1, back=3 * mm))
    # two rays across the face, 50 um and 90 um in front of the vertex plane: in through the ring's barrel, out through the falling profile, over
    # the air in front of the central rise, in through the profile again and out of the far barrel - the line crosses the ASPHERE twice, and the
    # inside march records one segment from barrel to barrel (AbstractSDF.jl:132-159)
    o, p0 = np.asarray(lens.orientation()), np.asarray(lens.position())
    P += (np.array([p0 + o @ np.array([-3 * mm, y, 0.2 * mm]) for y in (-0.05 * mm, -0.09 * mm)]),)
    D += (np.array([o @ np.array([1.0, 0.004, 0.02]), o @ np.array([1.0, -0.003, -0.05])]),)
    if crest:  # eight rays along the lens's own axis onto the crest of the front profile, where the leaf under the surface thins to nothing
        o = np.asarray(lens.orientation())
        P, D = ring(np.asarray(lens.position()), o[:, 1], L3_CREST + 0.5e-6, 8, back=3 * mm, phase=0.4)
        P, D = [P], [D]
    c.bundle = bundle("ray", P, D)
    c.name = "phone-l3"
    return c


L1 = dict(front=(1.054e-3, 1.333024e-3, -0.14294, [0, 0.038162 * _K ** 3, 0.06317 * _K ** 5, -0.020792 * _K ** 7, 0.18432 * _K ** 9, -0.04827 * _K ** 11,
                                                   0.094529 * _K ** 13]),
          back=(2.027e-3, 1.216472e-3, 8.0226, [0, 0.0074974 * _K ** 3, 0.064686 * _K ** 5, 0.19354 * _K ** 7, -0.50703 * _K ** 9, -0.34529 * _K ** 11,
                                                5.9938 * _K ** 13]),
          ct=0.72e-3, n=1.580200)
L2 = dict(front=(-3.116e-3, 1.4e-3, -49.984, [0, -0.31608 * _K ** 3, 0.34755 * _K ** 5, -0.17102 * _K ** 7, -0.41506 * _K ** 9, -1.342 * _K ** 11,
                                              5.0594 * _K ** 13, -2.7483 * _K ** 15]),
          back=(-4.835e-3, 1.9e-3, 1.6674, [0, -0.079727 * _K ** 3, 0.13899 * _K ** 5, -0.044057 * _K ** 7, -0.019369 * _K ** 9, 0.016993 * _K ** 11,
                                            0.093716 * _K ** 13, -0.080329 * _K ** 15]),
          ct=0.55e-3, n=1.804700)  # elements L1 and L2 of the same objective (runtests.jl:1581-1696), as L3 above
PHONE_FLATS = ((4.2e-3, 0.15e-3, 1.516800, 0.19e-3), (4.9e-3, 0.5e-3, 1.469200, 0.18e-3))  # filter, cover: diameter, thickness, n, the gap in front
PHONE_GAPS = (0.39e-3, 0.63e-3)  # L1 - L2, L2 - L3


def _ring_lens(q, obj, planted=None):
    (r1, d1, k1, a1), (r2, d2, k2, a2) = q["front"], q["back"]
    return tr.ExactRingLens(tr.Surface(r1, k1, a1), tr.Surface(r2, k2, a2), q["ct"], lambda lam: q["n"], d1, d2, d1, d2, obj.position(), obj.orientation(), planted)


def _asphere_lens(q):
    E = bmo.EvenAsphericalSurface
    return bmo.Lens(E(*q["front"]), E(*q["back"]), q["ct"], lambda lam: q["n"])


def phone_l12(which, planted=None, apex=False):
    """Elements L1 and L2 of the phone objective, each alone as phone-l3 is: tilted 2 degrees and decentred, a PSFDetector behind.
    L1: a convex aspheric front over 1.333 mm and a concave aspheric back (R > 0) over 1.216 mm; the step is levelled BEHIND, by a ring
    that reaches up to the back edge (Lenses.jl:247-266).  L2: a concave aspheric front (R < 0, closed along its vertex plane,
    AsphericalLensSDF.jl:285-305) over 1.4 mm and a convex aspheric back (R < 0 behind: the leaf between the plane of its edge height and the
    profile) over 1.9 mm; the ring in FRONT starts at the front's negative edge sag (Lenses.jl:232-246).  No profile of the two is inflected.
    Rays: a 2.5 degree oblique disc over 0.98 of the front aperture, one on the axis, and nine onto the ring's plane face - from behind on L1."""
    c = Case()
    q = (L1, L2)[which - 1]
    lens = _asphere_lens(q)
    bmo.xrotate3d(lens, math.radians(2))
    at = np.array([0.05 * mm, 5 * mm, -0.03 * mm])
    bmo.translate3d(lens, at)
    det = bmo.PSFDetector(12 * mm)
    bmo.translate3d(det, [0, 9 * mm, 0])
    c.system, c.lens, c.det = bmo.System([lens, det]), lens, det
    c.exact = [_ring_lens(q, lens, planted), tr.ExactFlat(12 * mm, det.position(), det.orientation(), "psf")]
    ob = math.radians(2.5)
    d1, d2 = q["front"][1], q["back"][1]
    onto = ring(at + [0, q["ct"], 0], [0, -1, 0], (d1 + d2) / 4, 9, back=3 * mm, phase=0.2) if which == 1 else ring(at, [0, 1, 0], (d1 + d2) / 4, 9, back=3 * mm, phase=0.2)
    # L2's concave aspheric apex is a seam (the leaf under it is thinner than the central-difference stencil out to 11 um): its 'axis' ray
    # runs 50 um beside the apex; apex=True: eight rays along the lens's own axis ON the apex and 3, 6 and 9 um beside it
    P, D = zip(disc(at, [0.0, math.cos(ob), math.sin(ob)], 0.98 * d1, 38, back=3 * mm), onto,
               ring(at + ([0, 0, 0] if which == 1 else [50e-6, 0, 0]), [0, 1, 0], 0.0, 1, back=3 * mm))
    if apex:
        axis = np.asarray(lens.orientation())[:, 1]
        P, D = zip(ring(at, axis, 0.0, 2, back=3 * mm), ring(at, axis, 3e-6, 2, back=3 * mm), ring(at, axis, 6e-6, 2, back=3 * mm), ring(at, axis, 9e-6, 2, back=3 * mm))
    c.bundle = bundle("ray", P, D)
    c.name = "phone-l%d" % which
    return c


def phone(planted=None, kat=False):
    """The phone objective of the reference's test (runtests.jl:1581-1696; tests/test_asphere_system.py): L1, L2, L3, filter and cover glass at
    their poses there, and a PSFDetector 0.12 mm behind the cover: ten refractions per ray.  The first three rays are the test's own, parallel
    to the axis at z = -0.65 mm and 0.65 mm and - the apex of L2's concave aspheric front being a seam - 50 um beside it instead of on it
    (kat=True: the test's three rays themselves); then a collimated disc over 0.9 of L1's aperture and two fields of 3 and 6 degrees."""
    c = Case()
    lenses = [_asphere_lens(q) for q in (L1, L2, L3)]
    for (d, t, n, _) in PHONE_FLATS:
        lenses.append(bmo.Lens(bmo.CircularFlatSurface(d), t, (lambda v: (lambda lam: v))(n)))
    gaps = PHONE_GAPS + tuple(f[3] for f in PHONE_FLATS)
    for prev, cur, gap in zip(lenses, lenses[1:], gaps):
        bmo.translate_to3d(cur, prev.position())
        bmo.translate3d(cur, [0, prev.thickness + gap, 0])
    det = bmo.PSFDetector(6 * mm)
    bmo.translate_to3d(det, lenses[-1].position())
    bmo.translate3d(det, [0, lenses[-1].thickness + 0.12e-3, 0])
    c.system, c.lens, c.det = bmo.System(lenses + [det]), lenses[0], det
    c.exact = [_ring_lens(q, o, planted) for q, o in zip((L1, L2, L3), lenses)]
    c.exact += [tr.ExactLens(tr.Surface(math.inf), tr.Surface(math.inf), t, d, (lambda v: (lambda lam: v))(n), o.position(), o.orientation())
                for (d, t, n, _), o in zip(PHONE_FLATS, lenses[3:])]
    c.exact.append(tr.ExactFlat(6 * mm, det.position(), det.orientation(), "psf"))
    kat = (np.array([[0, -0.5e-3, z] for z in (-1.3e-3 / 2, 0.0 if kat else 50e-6, 1.3e-3 / 2)]), np.tile([0.0, 1.0, 0.0], (3, 1)))
    at = np.zeros(3)
    f3, f6 = math.radians(3), math.radians(6)
    P, D = zip(kat, disc(at, [0, 1, 0], 0.9 * L1["front"][1], 25, back=0.5 * mm), disc(at, [0.0, math.cos(f3), math.sin(f3)], 0.7 * L1["front"][1], 10, back=0.5 * mm),
               disc(at, [math.sin(f6), math.cos(f6), 0.0], 0.6 * L1["front"][1], 10, back=0.5 * mm))
    c.bundle = bundle("ray", P, D, lam=0.5876e-6)
    c.name = "phone"
    return c


# ------------------------------------------------------------------------------------------------ scene 5: cylinder and acylinder lenses
AYL = dict(R=15.538 * mm, D=25 * mm, H=50 * mm, K=-1.0, CT=7.5 * mm, N=1.777,
           A=[0, 1.1926075e-5 * (1e3) ** 3, -2.9323497e-9 * (1e3) ** 5, -1.8718889e-11 * (1e3) ** 7, -1.7009961e-14 * (1e3) ** 9,
              3.5481542e-17 * (1e3) ** 11, 6.5241296e-20 * (1e3) ** 13])  # Thorlabs AYL2520 (runtests.jl:1744-1785)


def cylinders(acyl=False, planted=None):
    """A convex cylinder lens (R = 30 mm) and a concave one (R = -40 mm) rolled 20 degrees about the beam, 40 mm x 40 mm; or the AYL2520
    acylinder, convex, and concave rolled 35 degrees.  The bundle fills the long (uncurved) axis of the first lens to 0.98; the second lens is
    rolled under it, so part of the bundle meets its plane side faces, from outside and from inside (some in total internal reflection)."""
    c = Case()
    if acyl:
        q = AYL
        mk = lambda sgn, n: bmo.Lens(bmo.AcylindricalSurface(sgn * q["R"], q["D"], q["H"], q["K"], q["A"]), q["CT"], lambda lam: n)
        ex = lambda o, sgn, n: tr.ExactCylLens(tr.Surface(sgn * q["R"], q["K"], q["A"]), tr.Surface(math.inf), q["CT"], q["D"], q["H"], lambda lam: n,
                                               o.position(), o.orientation(), planted)
        l1, l2, n1, n2, roll, gap, d, hgt = mk(1, 1.777), mk(-1, 1.6), 1.777, 1.6, 35, 20 * mm, q["D"], q["H"]
    else:
        mk = lambda r, ct, n: bmo.Lens(bmo.CylindricalSurface(r, 40 * mm, 40 * mm), ct, lambda lam: n)
        l1, l2, n1, n2, roll, gap, d, hgt = mk(30 * mm, 8 * mm, 1.517), mk(-40 * mm, 4 * mm, 1.6), 1.517, 1.6, 20, 25 * mm, 40 * mm, 40 * mm
    bmo.xrotate3d(l1, math.radians(2))
    bmo.translate3d(l1, [0, 30 * mm, 0])
    bmo.translate3d(l2, [0, 30 * mm + gap, 0])
    bmo.yrotate3d(l2, math.radians(roll))
    det = bmo.PSFDetector(150 * mm)
    bmo.translate3d(det, [0, 120 * mm, 0])
    c.system = bmo.System([l1, l2, det])
    if acyl:
        c.exact = [ex(l1, 1, n1), ex(l2, -1, n2)]
    else:
        cyl = lambda o, r, ct, n: tr.ExactCylLens(tr.Surface(r), tr.Surface(math.inf), ct, 40 * mm, 40 * mm, lambda lam: n, o.position(), o.orientation(), planted)
        c.exact = [cyl(l1, 30 * mm, 8 * mm, n1), cyl(l2, -40 * mm, 4 * mm, n2)]
    c.exact.append(tr.ExactFlat(150 * mm, det.position(), det.orientation(), "psf"))
    at = np.array([0.0, 30 * mm, 0.0])
    k = np.arange(48)
    x = 0.98 * hgt / 2 * np.cos(k * 2.399963)  # the long axis is x: filled to 0.98
    z = 0.9 * d / 2 * np.sqrt((k + 0.5) / 48) * np.sin(k * 2.399963) * (0.5 if acyl else 0.6)  # the concave second lens is rolled: stay inside it
    P = at + np.stack([x, np.full(48, -30 * mm), z], axis=1)
    D = np.tile(np.array([0.004, 1.0, -0.006]), (48, 1))
    c.bundle = bundle("ray", [P], [D])
    c.name = "acylinders" if acyl else "cylinders"
    return c


# ------------------------------------------------------------------------------------------------ scene 6: a block of glass
def block(kind="ray", planted=None):
    """Lens(BoxSDF(12 mm, 6 mm, 10 mm), 1.52) tilted 17 / -8 degrees: flat faces only, where the march may end on or inside the surface and the
    normal fall back to central differences; a steep ring meets the side faces from inside beyond the critical angle."""
    c = Case()
    box = bmo.Lens(bmo.BoxSDF(12 * mm, 6 * mm, 10 * mm), lambda lam: 1.52)
    bmo.xrotate3d(box, math.radians(17))
    bmo.zrotate3d(box, math.radians(-8))
    bmo.translate3d(box, [0.2 * mm, 30 * mm, -0.1 * mm])
    det = bmo.PSFDetector(150 * mm) if kind == "ray" else bmo.Spotdetector(150 * mm)
    bmo.translate3d(det, [0, 70 * mm, 0])
    c.system = bmo.System([box, det])
    c.exact = [tr.ExactBox(12 * mm, 6 * mm, 10 * mm, lambda lam: 1.52, box.position(), box.orientation()),
               tr.ExactFlat(150 * mm, det.position(), det.orientation(), "psf" if kind == "ray" else "spot")]
    at = np.array([0.2 * mm, 30 * mm, -0.1 * mm])
    P, D = zip(disc(at, [0.03, 1.0, -0.02], 7 * mm, 40), ring(at - [0, 3 * mm, 0], [0, 1, 0], 3.4 * mm, 12, back=10 * mm, phase=0.3, slope=0.9))
    c.bundle = bundle(kind, P, D)
    c.name = "block-" + kind
    return c


def prism(kind="ray", planted=None):
    """RightAnglePrism(20 mm, 15 mm, 1.5) used in total internal reflection: the bundle enters through the leg x = -10 mm, meets the hypotenuse
    at about 45 degrees (beyond the critical angle of 41.8), and leaves through the other leg; the prism is tilted 3 / -2 degrees."""
    c = Case()
    pr = bmo.RightAnglePrism(20 * mm, 15 * mm, lambda lam: 1.5)
    bmo.zrotate3d(pr, math.radians(3))
    bmo.xrotate3d(pr, math.radians(-2))
    bmo.translate3d(pr, [40 * mm, 1 * mm, -0.5 * mm])
    det = bmo.PSFDetector(80 * mm) if kind == "ray" else bmo.Spotdetector(80 * mm)
    bmo.translate3d(det, [37 * mm, -40 * mm, 0])
    c.system = bmo.System([pr, det])
    c.exact = [tr.ExactPrism(20 * mm, 15 * mm, lambda lam: 1.5, pr.position(), pr.orientation()),
               tr.ExactFlat(80 * mm, det.position(), det.orientation(), "psf" if kind == "ray" else "spot")]
    at = np.array([30 * mm, -2.5 * mm, -0.5 * mm])
    P, D = zip(disc(at, [1.0, 0.02, -0.01], 5 * mm, 40), ring(at, [1, 0, 0], 1.5 * mm, 8, slope=0.06))
    c.bundle = bundle(kind, P, D)
    c.name = "prism-" + kind
    return c


RHOMB = dict(x=0.5, y=1.25, z=0.5, theta=math.radians(53.3), n=1.5, shift=[-0.25, 0, -0.25], roll=math.radians(135))


def rhomb(planted=None):
    """The Fresnel rhomb of the reference's test (runtests.jl:2339-2362): Lens(CuboidMesh(0.5, 1.25, 0.5, 53.3 degrees), 1.5), a mesh of glass,
    rolled 135 degrees so that a field along z enters at 45 degrees to the plane of the two total internal reflections: complex rs / rp on flat
    mesh faces, and a known answer - the field that leaves is circular, arg(Ez) - arg(Ex) = pi / 2."""
    c = Case()
    q = RHOMB
    s1 = bmo.CuboidMesh(q["x"], q["y"], q["z"], q["theta"])
    l1 = bmo.Lens(s1, lambda lam: q["n"])
    bmo.translate3d(l1, q["shift"])
    bmo.set_new_origin3d(s1)
    bmo.yrotate3d(l1, q["roll"])
    c.system = bmo.System([l1])
    c.exact = [tr.ExactMesh.cuboid(q["x"], q["y"], q["z"], q["theta"], q["shift"], l1.position(), l1.orientation(), lambda lam: q["n"])]
    at = np.array([0.0, 0.0, 0.0])
    P, D = zip(ring(at, [0, 1, 0], 0.0, 1, back=1.0), disc(at, [0.0, 1.0, 0.0], 0.2, 39, back=1.0), ring(at, [0, 1, 0], 0.05, 8, back=1.0, slope=0.01))
    pos, dirs = np.vstack(P), np.vstack(D)
    b = bmo.RayBundle.rays(pos, dirs, 1000e-9)
    Pl = np.zeros((14, b.n))
    Pl[:8] = b.planes
    E = np.tile(np.array([0.0, 0.0, 1.0]), (b.n, 1))  # [0, 0, electric_field(1)] up to its modulus; made orthogonal to the oblique rays
    d = b.planes[3:6].T
    for _ in range(3):
        E = E - (E * d).sum(axis=1)[:, None] * d
    Pl[8:14:2] = E.T
    c.bundle = bmo.RayBundle(bmo.BEAM_POLARIZED, Pl)
    c.name = "rhomb"
    return c


# ------------------------------------------------------------------------------------------------ scene 9: the miniscope's first three elements
MS = dict(n={532e-9: 1.5195, 1064e-9: 1.5066},  # N-BK7 at the two wavelengths of the train's table
          l1=(math.inf, -1.448 * mm, 1.3 * mm, 2.288 * mm),
          # (r_front, d_front, md_front, r_back, d_back, md_back, centre thickness) of the four lenses of the two cemented doublets
          dl11=(38.184 * mm, 3.68 * mm, 4.76 * mm, 3.467 * mm, 4.12 * mm, 4.76 * mm, 0.5 * mm),
          dl12=(3.467 * mm, 4.12 * mm, 4.76 * mm, -5.020 * mm, 4.76 * mm, 4.76 * mm, 2.5 * mm),
          dl21=(7.744 * mm, 5.624 * mm, 6 * mm, -3.642 * mm, 6 * mm, 6 * mm, 3.4 * mm),
          dl22=(-3.642 * mm, 6 * mm, 6 * mm, -14.413 * mm, 5.624 * mm, 6 * mm, 1.0 * mm))


def miniscope(planted=None):
    """The first three elements of the miniscope train of tests/scenes.py (objective lens, two cemented doublets whose four lenses have unequal
    clear apertures and mechanical rings: five lenses, ten surface crossings), turned onto the z axis as there, and a PSFDetector behind them.
    Rays leave an object point field 0.77 mm in front of the first face in cones of up to 0.14 rad.  Rays only: the reference's DoubletLens has an
    interact3d method for Beam{T, Ray} alone (DoubletLenses.jl:66), so a PolarizedRay cannot pass the two doublets of this train."""
    from scenes import miniscope_objects

    c = Case()
    group = miniscope_objects()[0]
    o1, d1, d2 = group.objects
    det = bmo.PSFDetector(8 * mm)
    bmo.xrotate3d(det, math.radians(90))
    bmo.translate3d(det, [0, 0, 17 * mm])
    c.system = bmo.System([o1, d1, d2, det])
    n = lambda lam: MS["n"][lam]
    rl = lambda o, q: tr.ExactRingLens(tr.Surface(q[0]), tr.Surface(q[3]), q[6], n, q[1], q[4], q[2], q[5], o.position(), o.orientation())
    q = MS["l1"]
    c.exact = [tr.ExactLens(tr.Surface(q[0]), tr.Surface(q[1]), q[2], q[3], n, o1.position(), o1.orientation()),
               tr.ExactParts([rl(d1.front, MS["dl11"]), rl(d1.back, MS["dl12"])]),
               tr.ExactParts([rl(d2.front, MS["dl21"]), rl(d2.back, MS["dl22"])]),
               tr.ExactFlat(8 * mm, det.position(), det.orientation(), "psf")]
    P, D = [], []
    for k, (x, z) in enumerate(((0.0, 0.0), (0.1 * mm, 0.0), (-0.07 * mm, 0.08 * mm), (0.03 * mm, -0.12 * mm))):
        for slope, cnt in ((0.0, 1), (0.07, 5), (0.14, 6)) if k else ((0.0, 1), (0.05, 5), (0.12, 6)):
            p, d = ring([x, z, -0.77 * mm], [0, 0, 1], 0.0, cnt, back=0.0, phase=0.3 + k, slope=slope)
            P.append(p)
            D.append(d)
    c.bundle = bundle("ray", P, D)
    c.name = "miniscope"
    return c


# ------------------------------------------------------------------------------------------------ scene 7: plane mirror, retroreflector
def mirror(kind="ray", angle=45.0, planted=None):
    """SquarePlanoMirror2D(120 mm) turned about x until the bundle along +y meets it at `angle` degrees from its normal (45: a fold, 85: near
    grazing), a detector 50 mm down the reflected beam."""
    c = Case()
    m = bmo.SquarePlanoMirror2D(120 * mm)
    th = math.radians(angle)
    bmo.xrotate3d(m, th)
    bmo.zrotate3d(m, math.radians(3))
    bmo.translate3d(m, [0.5 * mm, 40 * mm, -0.2 * mm])
    out = np.array([0.0, -math.cos(2 * th), -math.sin(2 * th)])  # the reflected direction before the 3 degree roll
    det = bmo.PSFDetector(60 * mm) if kind == "ray" else bmo.Spotdetector(60 * mm)
    bmo.xrotate3d(det, math.atan2(out[2], out[1]))
    bmo.translate3d(det, np.array([0.5 * mm, 40 * mm, -0.2 * mm]) + 50 * mm * out)
    c.system = bmo.System([m, det])
    c.exact = [tr.ExactFlat(120 * mm, m.position(), m.orientation(), "mirror"),
               tr.ExactFlat(60 * mm, det.position(), det.orientation(), "psf" if kind == "ray" else "spot")]
    at = np.array([0.5 * mm, 40 * mm, -0.2 * mm])
    P, D = zip(disc(at, [0.01, 1.0, 0.005], (6 if angle < 80 else 4) * mm, 40), ring(at, [0, 1, 0], 1 * mm, 8, slope=0.02), ring(at, [0, 1, 0], 0.0, 1))
    c.bundle = bundle(kind, P, D)
    c.name = "mirror%g-%s" % (angle, kind)
    return c


def retro(kind="ray", planted=None):
    """Retroreflector(30 mm) (the three faces of a cube corner, mesh triangles), rolled and decentred; the bundle comes down the cube diagonal,
    1.5 mm beside the corner, bounces three times and lands on a detector behind its source."""
    c = Case()
    rr = bmo.Retroreflector(30 * mm)
    bmo.zrotate3d(rr, math.radians(4))
    bmo.xrotate3d(rr, math.radians(-3))
    bmo.translate3d(rr, [1 * mm, 2 * mm, 0])
    det = bmo.PSFDetector(80 * mm) if kind == "ray" else bmo.Spotdetector(80 * mm)
    bmo.translate3d(det, [80 * mm, 80 * mm, 80 * mm])
    c.system = bmo.System([rr, det])
    c.exact = [tr.ExactMesh.retro(30 * mm, rr.position(), rr.orientation()),
               tr.ExactFlat(80 * mm, det.position(), det.orientation(), "psf" if kind == "ray" else "spot")]
    diag = np.array([1.0, 1.0, 1.0]) / math.sqrt(3)
    at = np.array([6 * mm, 7.5 * mm, 5 * mm])
    P, D = zip(disc(at, -diag, 5 * mm, 40, back=40 * mm), ring(at, -diag, 1 * mm, 8, back=40 * mm, slope=0.03))
    c.bundle = bundle(kind, P, D)
    c.name = "retro-" + kind
    return c


# ------------------------------------------------------------------------------------------------ scene 8: thin splitter, a singlet per arm
def splitter(kind="ray", planted=None):
    """ThinBeamsplitter(20 mm) at 45 degrees; the transmitted arm goes on along +y through the singlet of scene 1 to a detector, the reflected
    arm along -z through a second one.  Held: the children's first rays and fields, and every bounce of both arms."""
    c = Case()
    bs = bmo.ThinBeamsplitter(20 * mm)
    bmo.xrotate3d(bs, math.radians(45))
    bmo.translate3d(bs, [0, 30 * mm, 0])
    lt = bmo.SphericalLens(S1["r1"], S1["r2"], S1["l"], S1["d"], S1["n"])
    bmo.xrotate3d(lt, math.radians(2))
    bmo.translate3d(lt, [0.3 * mm, 50 * mm, 0])
    lr = bmo.SphericalLens(S1["r1"], S1["r2"], S1["l"], S1["d"], S1["n"])
    bmo.xrotate3d(lr, math.radians(-88))
    bmo.translate3d(lr, [0, 30 * mm, -20 * mm])
    D = bmo.PSFDetector if kind == "ray" else bmo.Spotdetector
    dt, dr = D(60 * mm), D(60 * mm)
    bmo.translate3d(dt, [0, 110 * mm, 0])
    bmo.xrotate3d(dr, math.radians(90))
    bmo.translate3d(dr, [0, 30 * mm, -80 * mm])
    c.system = bmo.System([bs, lt, dt, lr, dr])
    dk = "psf" if kind == "ray" else "spot"
    lens = lambda o: tr.ExactLens(tr.Surface(S1["r1"]), tr.Surface(S1["r2"]), S1["l"], S1["d"], lambda lam: S1["n"], o.position(), o.orientation(), planted)
    c.exact = [tr.ExactFlat(20 * mm, bs.position(), bs.orientation(), "thin_bs", reflectance=0.5), lens(lt), tr.ExactFlat(60 * mm, dt.position(), dt.orientation(), dk),
               lens(lr), tr.ExactFlat(60 * mm, dr.position(), dr.orientation(), dk)]
    at = np.array([0.0, 30 * mm, 0.0])
    P, Dn = zip(disc(at, [0.02, 1.0, -0.01], 9 * mm, 40), ring(at, [0, 1, 0], 2 * mm, 8, slope=0.05))
    c.bundle = bundle(kind, P, Dn)
    c.name = "splitter-" + kind
    return c


# ------------------------------------------------------------------------------------------------ scene 2: biconcave lens and meniscus
S2A = dict(r1=-30 * mm, r2=40 * mm, l=3 * mm, d=25.4 * mm, n=1.5)
S2B = dict(r1=30 * mm, r2=60 * mm, l=2.5 * mm, d=25.4 * mm, n=1.6)


def concave(kind="ray", planted=None, pairs=False):
    """A biconcave SphericalLens(-30 mm, 40 mm, 3 mm) tilted 3 degrees and a positive meniscus SphericalLens(30 mm, 60 mm, 2.5 mm) behind it.  Rays
    parallel to the biconcave lens's own axis 5 um, 24 um and 1 mm beside the concave apex (where the cap's wedge of glass is thinner than the
    central-difference stencil: the normals there must be the dual-number ones), a 2 degree oblique disc, and two skew rays that enter through
    the barrel inside the rim, cross the air pocket of the concave face and re-enter the rim on the far side: the inside march returns the LAST
    crossing before its first 1 m step outside, so the record holds one segment from barrel to barrel."""
    c = Case()
    a, b = S2A, S2B
    md = 30 * mm  # pairs: the same lens from two SphericalSurface records with a mechanical ring out to 30 mm (another path of the host builder)
    if pairs:
        la_ = bmo.Lens(bmo.SphericalSurface(a["r1"], a["d"], md), bmo.SphericalSurface(a["r2"], a["d"], md), a["l"], lambda lam: a["n"])
    else:
        la_ = bmo.SphericalLens(a["r1"], a["r2"], a["l"], a["d"], a["n"])
    bmo.xrotate3d(la_, math.radians(3))
    bmo.translate3d(la_, [0.4 * mm, 20 * mm, 0])
    lb_ = bmo.SphericalLens(b["r1"], b["r2"], b["l"], b["d"], b["n"])
    assert isinstance(lb_.shape, bmo.MeniscusLensSDF)
    bmo.zrotate3d(lb_, math.radians(-2))
    bmo.translate3d(lb_, [0.5 * mm, 35 * mm, -0.3 * mm])
    det = bmo.PSFDetector(90 * mm) if kind == "ray" else bmo.Spotdetector(90 * mm)
    bmo.translate3d(det, [0, 80 * mm, 0])
    c.system = bmo.System([la_, lb_, det])
    lens = lambda o, q: tr.ExactLens(tr.Surface(q["r1"]), tr.Surface(q["r2"]), q["l"], q["d"], lambda lam: q["n"], o.position(), o.orientation(), planted)
    c.exact = [lens(la_, a), lens(lb_, b), tr.ExactFlat(90 * mm, det.position(), det.orientation(), "psf" if kind == "ray" else "spot")]
    if pairs:
        c.exact[0] = tr.ExactRingLens(tr.Surface(a["r1"]), tr.Surface(a["r2"]), a["l"], lambda lam: a["n"], a["d"], a["d"], md, md, la_.position(),
                                      la_.orientation())
    p0, o = np.asarray(la_.position()), np.asarray(la_.orientation())
    axis = o[:, 1]
    rim_p = [p0 + o @ np.array([-20 * mm, y, 1 * mm]) for y in (-0.5 * mm, -0.9 * mm)]
    rim_d = [o @ np.array([1.0, 0.01, 0.03]), o @ np.array([1.0, -0.005, -0.02])]
    P, D = zip(disc(p0 + 1.5 * mm * axis, [math.sin(math.radians(2)), math.cos(math.radians(2)), 0.0], 0.85 * a["d"], 34),
               ring(p0, axis, 5e-6, 4), ring(p0, axis, 24e-6, 4, phase=0.5), ring(p0, axis, 1 * mm, 4, phase=0.9),
               (np.array(rim_p), np.array(rim_d)))
    c.bundle = bundle(kind, P, D)
    c.name = "concave-" + ("pairs-" if pairs else "") + kind
    return c


# ------------------------------------------------------------------------------------------------ scene 3: cemented doublet
AC254 = dict(r1=87.9 * mm, r2=-105.6 * mm, r3=math.inf, l1=6 * mm, l2=3 * mm, d=25.4 * mm, lams=[488e-9, 707e-9, 1064e-9],
             n1=[1.6591, 1.6456, 1.6374], n2=[1.7460, 1.7168, 1.7021])  # AC254-150-AB, N-LAK22 / N-SF10 (runtests.jl:1273-1321)


def doublet(kind="ray", planted=None):
    """SphericalDoubletLens AC254-150-AB at 488 / 707 / 1064 nm (a three-wavelength index table per glass), tilted 4 degrees, rolled 30 degrees
    about its axis and decentred; 16 rays per wavelength over 0.9 of the aperture, 2 degrees oblique."""
    c = Case()
    a = AC254
    dl = bmo.SphericalDoubletLens(a["r1"], a["r2"], a["r3"], a["l1"], a["l2"], a["d"], bmo.DiscreteRefractiveIndex(a["lams"], a["n1"]),
                                  bmo.DiscreteRefractiveIndex(a["lams"], a["n2"]))
    bmo.xrotate3d(dl, math.radians(4))
    bmo.rotate3d(dl, dl.orientation()[:, 1], math.radians(30))
    bmo.translate3d(dl, [-0.6 * mm, 25 * mm, 0.8 * mm])
    det = bmo.PSFDetector(60 * mm) if kind == "ray" else bmo.IntersectableObject(bmo.QuadraticFlatMesh(60 * mm))  # beamlets end on a plain stop
    bmo.translate3d(det, [0, 100 * mm, 0])
    c.system = bmo.System([dl, det])
    table = lambda ns: (lambda lam: dict(zip(a["lams"], ns))[lam])
    c.exact = [tr.ExactDoublet(a["r1"], a["r2"], a["r3"], a["l1"], a["l2"], a["d"], table(a["n1"]), table(a["n2"]), dl.position(), dl.orientation(), planted),
               tr.ExactFlat(60 * mm, det.position(), det.orientation(), "psf" if kind == "ray" else "stop")]
    at = np.array([-0.6 * mm, 25 * mm + 4 * mm, 0.8 * mm])
    ob = math.radians(2)
    P, D = disc(at, [math.sin(ob), math.cos(ob), 0.0], 0.9 * a["d"], 48)
    lam = np.tile(a["lams"], 16)
    c.bundle = bundle("ray", [P], [D], lam=lam) if kind == "ray" else gauss_bundle([P], [D], lam=lam)
    c.name = "doublet" if kind == "ray" else "doublet-gauss"
    return c


# ------------------------------------------------------------------------------------------------ scene 10: plate and cube splitters
PLATE = dict(w=30 * mm, h=25 * mm, l=3 * mm, d=25 * mm, n=1.5, refl=0.3)
CUBE = dict(leg=20 * mm, n=1.5, refl=0.3)


def _two_fans(at, kind, per_side=(16, 7, 1), back=15 * mm):
    """Half of the rays come up +y and half down -y onto `at`: a disc of 6 mm, a ring of 2 mm sloped by 0.05, one ray on the axis, per side."""
    P, D = [], []
    for sgn in (1.0, -1.0):
        for p, d in (disc(at, [0.02, sgn, -0.01], 6 * mm, per_side[0], back=back), ring(at, [0, sgn, 0], 2 * mm, per_side[1], back=back, slope=0.05),
                     ring(at, [0, sgn, 0], 0.0, per_side[2], back=back)):
            P.append(p)
            D.append(d)
    return gauss_bundle(P, D) if kind == "gauss" else bundle(kind, P, D)


def _detector(kind, width):
    """PSFDetector for Rays, Spotdetector for PolarizedRays, Photodetector for beamlets -> (object, the exact evaluator's kind)."""
    return {"ray": lambda: (bmo.PSFDetector(width), "psf"), "pol": lambda: (bmo.Spotdetector(width), "spot"),
            "gauss": lambda: (bmo.Photodetector(width, 8), "pd")}[kind]()


def _four_arms(c, splitter, exact, kind, at, axis, extra=(), extra_exact=()):
    """The splitter and a detector in each of its four arms: +y and -y (the transmitted arms of the two fans), and -axis / +axis (the reflected
    ones; axis 'z' or 'x'), 50 mm from `at`."""
    objs, ex = [splitter] + list(extra), [exact] + list(extra_exact)
    for off, rot in (([0, 50 * mm, 0], None), ([0, -50 * mm, 0], None), (-50 * mm, axis), (50 * mm, axis)):
        det, dk = _detector(kind, 40 * mm)
        if rot == "z":
            bmo.xrotate3d(det, math.radians(90))
            off = [0, 0, off]
        elif rot == "x":
            bmo.zrotate3d(det, math.radians(90))
            off = [off, 0, 0]
        bmo.translate3d(det, np.asarray(at) + np.asarray(off))
        objs.append(det)
        ex.append(tr.ExactFlat(40 * mm, det.position(), det.orientation(), dk))
    c.system, c.exact = bmo.System(objs), ex
    return c


def plate(kind="ray", planted=None, round_=False, move=None):
    """RectangularPlateBeamsplitter(30 mm, 25 mm, 3 mm, 1.5; reflectance 0.3) (round_: RoundPlateBeamsplitter(25 mm, 3 mm, ...)) at 45 degrees,
    rolled 2 degrees and decentred.  One fan meets the coated side (the coated-face tie of coating and substrate, both children start on the
    substrate's surface), the other enters the substrate through its back and meets the coating from inside: both values of isentering.  A
    detector in each of the four arms; 'pol': a singlet in the -y transmitted arm (the child of the fan that came through the substrate)."""
    c = Case()
    q = PLATE
    if round_:
        bs = bmo.RoundPlateBeamsplitter(q["d"], q["l"], lambda lam: q["n"], reflectance=q["refl"])
    else:
        bs = bmo.RectangularPlateBeamsplitter(q["w"], q["h"], q["l"], lambda lam: q["n"], reflectance=q["refl"])
    bmo.xrotate3d(bs, math.radians(45))
    bmo.zrotate3d(bs, math.radians(2))
    bmo.translate3d(bs, [0.3 * mm, 40 * mm, -0.2 * mm])
    if move is not None:
        bmo.translate3d(bs, move[0])
        bmo.zrotate3d(bs, move[1])
    c.lens = bs
    ex = tr.ExactPlateBS(q["d"] if round_ else q["w"], q["h"], q["l"], lambda lam: q["n"], q["refl"], bs.position(), bs.orientation(), round_=round_)
    at = np.array([0.3 * mm, 40 * mm, -0.2 * mm])
    extra, extra_exact = (), ()
    if kind == "pol":
        lt = bmo.SphericalLens(S1["r1"], S1["r2"], S1["l"], S1["d"], S1["n"])
        bmo.xrotate3d(lt, math.radians(2))
        bmo.translate3d(lt, [0.3 * mm, 12 * mm, 0])
        extra = (lt,)
        extra_exact = (tr.ExactLens(tr.Surface(S1["r1"]), tr.Surface(S1["r2"]), S1["l"], S1["d"], lambda lam: S1["n"], lt.position(), lt.orientation()),)
    _four_arms(c, bs, ex, kind, at, "z", extra, extra_exact)
    c.bundle = _two_fans(at, kind)
    c.name = ("roundplate-" if round_ else "plate-") + kind
    return c


def cube(kind="ray", planted=None, move=None):
    """CubeBeamsplitter(20 mm, 1.5; reflectance 0.3), rolled 2 / 1.5 degrees and decentred: one fan enters through the front prism, one through
    the back prism; both prisms hint at the coating, both children start in glass on the face the two prisms share."""
    c = Case()
    q = CUBE
    bs = bmo.CubeBeamsplitter(q["leg"], lambda lam: q["n"], reflectance=q["refl"])
    bmo.zrotate3d(bs, math.radians(2))
    bmo.xrotate3d(bs, math.radians(1.5))
    bmo.translate3d(bs, [0.3 * mm, 40 * mm, -0.2 * mm])
    if move is not None:
        bmo.translate3d(bs, move[0])
        bmo.zrotate3d(bs, move[1])
    c.lens = bs
    ex = tr.ExactCubeBS(q["leg"], lambda lam: q["n"], q["refl"], bs.position(), bs.orientation())
    at = np.array([0.3 * mm, 40 * mm, -0.2 * mm])
    _four_arms(c, bs, ex, kind, at, "x")
    c.bundle = _two_fans(at, kind, back=25 * mm)
    c.name = "cube-" + kind
    return c


def splitter_gauss(planted=None):
    """GaussianBeamlets through the singlet of scene 1 (their waist changes: a child's w0 is not the root's) and two ThinBeamsplitters in a row,
    reflectance 0.3 and 0.6: the first is met from behind its normal (phi = 0), the second, in the transmitted arm, faces the beam
    (phi = pi); its children are grandchildren whose length(gauss) runs over two parents.  A Photodetector in each of the three arms."""
    c = Case()
    lens = bmo.SphericalLens(S1["r1"], S1["r2"], S1["l"], S1["d"], S1["n"])
    bmo.xrotate3d(lens, math.radians(2))
    bmo.translate3d(lens, [0.3 * mm, 20 * mm, 0])
    b1, b2 = bmo.ThinBeamsplitter(20 * mm, reflectance=0.3), bmo.ThinBeamsplitter(20 * mm, reflectance=0.6)
    bmo.xrotate3d(b1, math.radians(45))
    bmo.zrotate3d(b1, math.radians(1))
    bmo.translate3d(b1, [0.2 * mm, 50 * mm, 0])
    bmo.xrotate3d(b2, math.radians(135))
    bmo.translate3d(b2, [0, 75 * mm, 0.2 * mm])
    dets = []
    for rot, at in ((90, [0, 50 * mm, -40 * mm]), (0, [0, 110 * mm, 0]), (90, [0, 75 * mm, 40 * mm])):
        d = bmo.Photodetector(40 * mm, 8)
        bmo.xrotate3d(d, math.radians(rot))
        bmo.translate3d(d, at)
        dets.append(d)
    c.system, c.lens = bmo.System([lens, b1, b2] + dets), lens
    c.exact = [tr.ExactLens(tr.Surface(S1["r1"]), tr.Surface(S1["r2"]), S1["l"], S1["d"], lambda lam: S1["n"], lens.position(), lens.orientation()),
               tr.ExactFlat(20 * mm, b1.position(), b1.orientation(), "thin_bs", reflectance=0.3),
               tr.ExactFlat(20 * mm, b2.position(), b2.orientation(), "thin_bs", reflectance=0.6)] + [
        tr.ExactFlat(40 * mm, d.position(), d.orientation(), "pd") for d in dets]
    at = np.array([0.3 * mm, 20 * mm, 0.0])
    P, D = zip(disc(at, [0.01, 1.0, -0.005], 6 * mm, 38, back=15 * mm), ring(at, [0, 1, 0], 2 * mm, 9, back=15 * mm, slope=0.02), ring(at, [0, 1, 0], 0.0, 1, back=15 * mm))
    c.bundle = gauss_bundle(P, D)
    c.name = "splitter-gauss"
    return c


# ------------------------------------------------------------------------------------------------ scene 11: polarization filters
def pol_bundle(pos, dirs, E, lam=1.064e-6):
    """PolarizedRays with the complex field E (one row per ray), made orthogonal to each ray's direction (PolarizedRays.jl:54)."""
    b = bmo.RayBundle.rays(np.vstack(pos), np.vstack(dirs), lam)
    d = b.planes[3:6].T
    E = np.array(E, dtype=np.complex128)
    for _ in range(3):
        E = E - (E * d).sum(axis=1)[:, None] * d
    P = np.zeros((14, b.n))
    P[:8] = b.planes
    P[8:14:2], P[9:14:2] = E.real.T, E.imag.T
    return bmo.RayBundle(bmo.BEAM_POLARIZED, P)


STATES = {"x": [1, 0, 0], "z": [0, 0, 1], "45": [math.sqrt(0.5), 0, math.sqrt(0.5)], "elliptical": [1.0, 0, 0.5 + 0.3j]}


def polarizers(planted=None, roll=30.0, tilt=10.0, states=("x", "z", "45", "elliptical"), fan=True, roll1=1.5):
    """Two PolarizationFilters in a row, the first rolled 1.5 degrees about the beam and decentred, the second rolled `roll` degrees about the
    beam and tilted `tilt` degrees (a rolled filter shows a transposed rotation, oblique incidence a dropped projection), a Spotdetector
    behind them.  Four input states: linear along x, along z, at 45 degrees, elliptical; per state a disc, a sloped ring and the axis ray.
    Beside them eight identical rays onto a third filter whose cutoff is the norm they are transmitted with: they end BLOCKED.
    fan=False, roll1, roll, tilt, states: the axis ray alone through two filters at the given rolls (the Malus cases of the tests)."""
    c = Case()
    f1, f2, f3 = bmo.PolarizationFilter(20 * mm), bmo.PolarizationFilter(20 * mm), None
    bmo.yrotate3d(f1, math.radians(roll1))
    bmo.translate3d(f1, [0.2 * mm, 20 * mm, -0.1 * mm])
    bmo.yrotate3d(f2, math.radians(roll))
    bmo.xrotate3d(f2, math.radians(tilt))
    bmo.translate3d(f2, [-0.2 * mm, 40 * mm, 0.1 * mm])
    det = bmo.Spotdetector(60 * mm)
    bmo.translate3d(det, [0, 70 * mm, 0])
    flt = lambda f: tr.ExactFlat(20 * mm, f.position(), f.orientation(), "polarizer", pre=math.pi, jones=f.jones, cutoff=f.cutoff)
    at = np.array([0.0, 20 * mm, 0.0])
    P, D, E = [], [], []
    for s in states:
        fans = (disc(at, [0.01, 1.0, -0.02], 6 * mm, 6), ring(at, [0, 1, 0], 2 * mm, 3, slope=0.05), ring(at, [0, 1, 0], 0.0, 1)) if fan else (ring(at, [0, 1, 0], 0.0, 1),)
        for p, d in fans:
            P.append(p)
            D.append(d)
            E += [STATES[s]] * len(p)
    objs, exact = [f1, f2, det], None
    if fan:  # the third filter, 40 mm beside the beam, tilted 5 degrees and rolled 20; its cutoff from the 50-digit evaluation of its own formula
        side = np.array([40 * mm, 20 * mm, 0.0])
        p8, d8 = np.tile(side - [0, 30 * mm, 0], (8, 1)), np.tile(_frame([0.03, 1.0, 0.02])[0], (8, 1))
        P.append(p8)
        D.append(d8)
        E += [STATES["elliptical"]] * 8
        b = pol_bundle(P, D, E)
        probe = bmo.PolarizationFilter(20 * mm)
        for f in (probe,):
            bmo.yrotate3d(f, math.radians(20))
            bmo.xrotate3d(f, math.radians(5))
            bmo.translate3d(f, side)
        mp = tr._mp()
        with mp.workdps(50):
            r = root_of(b, b.n - 1)
            cut = float(tr.interact_polarizer(flt(probe), tr._v(r["dir"]), mp.mpf(1), tr._c(r["E0"]))[0]["norm"])
        f3 = bmo.PolarizationFilter(20 * mm, cutoff_strength=cut)
        bmo.yrotate3d(f3, math.radians(20))
        bmo.xrotate3d(f3, math.radians(5))
        bmo.translate3d(f3, side)
        objs = [f1, f2, det, f3]
    c.bundle = pol_bundle(P, D, E)
    c.system = bmo.System(objs)
    c.exact = [flt(f1), flt(f2), tr.ExactFlat(60 * mm, det.position(), det.orientation(), "spot")] + ([flt(f3)] if f3 is not None else [])
    c.name = "polarizers"
    return c


# ------------------------------------------------------------------------------------------------ scene 12: mirrors made of SDFs and of a cuboid mesh
def _wall(kind, width, at, rot=None):
    """A detector `width` wide at `at`, turned by rot = (axis, degrees) before it is moved there -> (object, its exact flat)."""
    det, dk = _detector(kind, width)
    if rot is not None:
        {"x": bmo.xrotate3d, "z": bmo.zrotate3d}[rot[0]](det, math.radians(rot[1]))
    bmo.translate3d(det, at)
    return det, tr.ExactFlat(width, det.position(), det.orientation(), dk)


def _local_rays(obj, hits, dirs, back=30 * mm):
    """Rays given in an object's own frame: through the local points `hits` along the local directions `dirs`, started `back` before them."""
    o, p0 = np.asarray(obj.orientation()), np.asarray(obj.position())
    D = np.array([o @ (np.asarray(d, dtype=np.float64) / np.linalg.norm(d)) for d in dirs])
    return np.array([p0 + o @ np.asarray(h, dtype=np.float64) for h in hits]) - back * D, D


CM = dict(R=100 * mm, l=6 * mm, d=25.4 * mm)


def concave_mirror(kind="ray", planted=None, tilt=4.0, decentre=(0.8 * mm, -0.5 * mm)):
    """ConcaveSphericalMirror(100 mm, 6 mm, 25.4 mm) (Mirrors.jl:195-200: a concave leaf in front of a plano cylinder, the only curved sdf
    that reflects from outside), tilted 4 degrees about x and decentred; the dish opens towards -y.  Rays: a collimated disc along +y over 0.95
    of the aperture, two rays on the mirror's own axis, rays parallel to it 5 um and 24 um beside the apex (the wedge of DESIGN.md section 2,
    rule ii), one ray onto the barrel and one onto the flat back (leaf and cylinder have one diameter: there is no flat annulus in front).  The
    reflected bundle converges onto a detector BEHIND the rays' starting points; a second detector behind the mirror takes the ray its back
    reflects.  tilt, decentre: the untilted mirror of the known-answer test."""
    c = Case()
    q = CM
    m = bmo.ConcaveSphericalMirror(q["R"], q["l"], q["d"])
    bmo.xrotate3d(m, math.radians(tilt))
    p0 = np.array([decentre[0], 60 * mm, decentre[1]])
    bmo.translate3d(m, p0)
    front, xf = _wall(kind, 120 * mm, [0, 20 * mm, 0])
    rear, xr = _wall(kind, 120 * mm, [0, 100 * mm, 0])
    c.system, c.lens = bmo.System([m, front, rear]), m
    # the sphere's centre lies R in FRONT of the vertex (ps = p + (0, R, 0), SphericalLensSDF.jl:167): a front surface of signed radius -R
    c.exact = [tr.ExactLens(tr.Surface(q["R"] if planted == "mirror_centre_wrong_side" else -q["R"]), tr.Surface(math.inf), q["l"], q["d"], None,
                            m.position(), m.orientation(), kind="mirror"), xf, xr]
    axis = np.asarray(m.orientation())[:, 1]
    P, D = zip(disc(p0, [0, 1, 0], 0.95 * q["d"], 36), ring(p0, axis, 0.0, 2), ring(p0, axis, 5e-6, 4), ring(p0, axis, 24e-6, 4, phase=0.5),
               _local_rays(m, [[q["d"] / 2, 3 * mm, 1 * mm], [3 * mm, q["l"], -2 * mm]], [[-0.3, -1.0, 0.0], [0.02, -1.0, 0.05]], back=25 * mm))
    c.bundle = bundle(kind, P, D)
    c.name = "concave-mirror-" + kind
    return c


RM = dict(d=25.4 * mm, l=5 * mm)


def round_mirror(kind="ray", planted=None):
    """Two RoundPlanoMirror(25.4 mm, 5 mm) (Mirrors.jl:161-164: a bare PlanoSurfaceSDF, whose flat faces take central-difference normals),
    70 mm apart, turned about x until the bundle along +y meets their front faces at 45 and at 80 degrees, rolled 1.5 degrees.  At 80
    degrees the front face is 4.4 mm high as the bundle sees it and the barrel 4.9 mm: eight rays meet the barrel FIRST.  A detector down each
    front-reflected beam, and one behind the rays' starting points for what the barrel sends back."""
    c = Case()
    q = RM
    objs, exact, P, D = [], [], [], []
    for ang, x0 in ((45.0, 0.0), (80.0, 70 * mm)):
        m = bmo.RoundPlanoMirror(q["d"], q["l"])
        th = math.radians(ang)
        bmo.xrotate3d(m, th)
        bmo.zrotate3d(m, math.radians(1.5))
        p0 = np.array([x0 + 0.3 * mm, 40 * mm, -0.2 * mm])
        bmo.translate3d(m, p0)
        out = np.array([0.0, -math.cos(2 * th), -math.sin(2 * th)])
        det, dk = _detector(kind, 60 * mm)
        bmo.xrotate3d(det, math.atan2(out[2], out[1]))
        bmo.translate3d(det, p0 + 50 * mm * out)
        objs += [m, det]
        exact += [tr.ExactLens(tr.Surface(math.inf), tr.Surface(math.inf), q["l"], q["d"], None, m.position(), m.orientation(), kind="mirror"),
                  tr.ExactFlat(60 * mm, det.position(), det.orientation(), dk)]
        if ang < 80:
            fans = (disc(p0, [0.01, 1.0, 0.005], 14 * mm, 20), ring(p0, [0, 1, 0], 1 * mm, 4, slope=0.02))
        else:
            fans = (disc(p0, [0.0, 1.0, 0.0], 3.5 * mm, 14), ring(p0, [0, 1, 0], 0.0, 2), disc(p0 + [0, 0, 4.6 * mm], [0.0, 1.0, 0.0], 3 * mm, 8))
        for p, d in fans:
            P.append(p)
            D.append(d)
    wall, xw = _wall(kind, 300 * mm, [35 * mm, -40 * mm, 0])
    c.system, c.exact = bmo.System(objs + [wall]), exact + [xw]
    c.bundle = bundle(kind, P, D)
    c.name = "round-mirror-" + kind
    return c


PM = dict(leg=10 * mm, h=10 * mm)


def prism_mirror(planted=None):
    """Two RightAnglePrismMirror(10 mm, 10 mm) (Mirrors.jl:226-230: a RightAnglePrismSDF turned by the double deg2rad(45 + 180) about z, so
    that the hypotenuse faces -y and the two legs form a roof towards +y).  The first is tilted 2 degrees about x; rays along -y fold once on
    its left leg (towards -x, onto a detector) and once on its right leg (towards +x).  A convex solid cannot be met twice, so the paths of
    TWO bounces go on to the second prism, which is turned upside down 40 mm to the right and rolled 1 degree: its leg folds them down onto
    the detector below.  A fan from below folds on the first prism's hypotenuse, and one ray meets each of its triangular end faces.  The
    evaluator gets the pose WITHOUT the builder's rotation (the orientation of a twin that made the scene's moves alone) and applies the
    double angle itself, in 50 digits (ExactPrism's pre)."""
    c = Case()
    q = PM
    pre = math.radians(45 if planted == "prism_mirror_pre_45" else 45 + 180)
    moves = ([(bmo.xrotate3d, math.radians(2))], [(bmo.zrotate3d, math.radians(180)), (bmo.zrotate3d, math.radians(1))])
    at = ([0.2 * mm, 40 * mm, -0.1 * mm], [40 * mm, 40 * mm + q["leg"] / math.sqrt(2), 0.0])
    objs, exact = [], []
    for mv, p in zip(moves, at):
        m, twin = bmo.RightAnglePrismMirror(q["leg"], q["h"]), bmo.RoundPlanoMirror(1 * mm, 1 * mm)
        for f, a in mv:
            f(m, a)
            f(twin, a)
        bmo.translate3d(m, p)
        objs.append(m)
        exact.append(tr.ExactPrism(q["leg"], q["h"], None, m.position(), twin.orientation(), pre=pre, kind="mirror"))
    for w, p, rot in ((100 * mm, [-50 * mm, 43 * mm, 0], ("z", 90)), (300 * mm, [20 * mm, -20 * mm, 0], None)):
        det, x = _wall("ray", w, p, rot)
        objs.append(det)
        exact.append(x)
    c.system, c.exact, c.lens = bmo.System(objs), exact, objs[0]
    p1 = np.asarray(at[0])
    top = p1 + [0, 3.5 * mm, 0]
    ends = [(p1 + [0.5 * mm, 3 * mm, s * q["h"] / 2], np.array([0.0, -0.5, -s])) for s in (1.0, -1.0)]
    P, D = zip(disc(top + [-3.5 * mm, 0, 0], [0, -1, 0], 4 * mm, 16), disc(top + [3.5 * mm, 0, 0], [0, -1, 0], 4 * mm, 16),
               disc(p1, [0.3, 1.0, 0.02], 6 * mm, 14),
               (np.array([h - 30 * mm * d / np.linalg.norm(d) for h, d in ends]), np.array([d / np.linalg.norm(d) for _, d in ends])))
    c.bundle = bundle("ray", P, D)
    c.name = "prism-mirror-ray"
    return c


RECT = dict(w=30 * mm, h=20 * mm, l=5 * mm)


def rect_mirror(planted=None):
    """RectangularPlanoMirror(30 mm, 20 mm, 5 mm) (Mirrors.jl:110-119: CuboidMesh(width, thickness, height) moved by (-width / 2, 0,
    -height / 2) and made its own origin), turned 45 degrees about x, rolled 1.5 degrees and decentred: four kinematic steps have re-rounded
    its vertex table.  The exact mesh derives the twelve triangles from the three lengths, that translation and the pose.  Rays along +y onto
    the front face, ten onto the side face z = +height / 2 beside it, four oblique ones onto the side face x = +width / 2; a detector in
    each of the three reflected directions."""
    c = Case()
    q = RECT
    m = bmo.RectangularPlanoMirror(q["w"], q["h"], q["l"])
    bmo.xrotate3d(m, math.radians(45))
    bmo.zrotate3d(m, math.radians(1.5))
    p0 = np.array([0.3 * mm, 40 * mm, -0.2 * mm])
    bmo.translate3d(m, p0)
    walls = [_wall("ray", 120 * mm, p0 + [0, 0, -50 * mm], ("x", 90)), _wall("ray", 120 * mm, p0 + [0, 0, 50 * mm], ("x", 90)),
             _wall("ray", 300 * mm, [20 * mm, 100 * mm, 0])]
    c.system, c.lens = bmo.System([m] + [w[0] for w in walls]), m
    c.exact = [tr.ExactMesh.cuboid(q["w"], q["l"], q["h"], math.pi / 2, [-q["w"] / 2, 0, -q["h"] / 2], m.position(), m.orientation(), None,
                                   kind="mirror", steps=4)] + [w[1] for w in walls]
    side = _local_rays(m, [[q["w"] / 2, 1.5 * mm + 0.6 * mm * k, (-3 + 2 * k) * mm] for k in range(4)], [np.asarray(m.orientation()).T @ np.array([-0.5, 1.0, 0.0])] * 4)
    P, D = zip(disc(p0, [0.01, 1.0, 0.005], 12 * mm, 30), ring(p0, [0, 1, 0], 1 * mm, 4, slope=0.02), disc(p0 + [0, 0, 8.8 * mm], [0, 1, 0], 2 * mm, 10), side)
    c.bundle = bundle("ray", P, D)
    c.name = "rect-mirror-ray"
    return c


# ------------------------------------------------------------------------------------------------ scene 13: plano and thin spherical lenses
FUSED_SILICA = (0.6961663, 0.4079426, 0.8974794, 0.0684043 ** 2, 0.1162414 ** 2, 9.896161 ** 2)  # the coefficients of tests/test_oracle_kat.py
PCX = dict(r=38.6 * mm, ct=4.1 * mm, d=25.4 * mm, lams=[486e-9, 588e-9, 1064e-9])


def plano_convex(planted=None):
    """One plano-convex prescription (r = 38.6 mm, 4.1 mm thick, 25.4 mm) built twice: Lens(SphericalSurface(r, d), ct, n), the
    three-argument path (Lenses.jl:293-301), met curved side first, and Lens(PlanoConvexLensSDF(r, ct, d), n) (SphericalLensSDF.jl:338-347)
    turned round and met plane side first, 20 mm behind it.  The glass is a SellmeierEquation with fused silica's coefficients under three
    wavelengths: the host evaluates it in doubles, the exact lenses in 50 digits from the coefficient doubles (trace_ref.sellmeier)."""
    c = Case()
    q = PCX
    n_host = bmo.SellmeierEquation(*FUSED_SILICA)
    a = bmo.Lens(bmo.SphericalSurface(q["r"], q["d"]), q["ct"], n_host)
    bmo.xrotate3d(a, math.radians(3))
    bmo.translate3d(a, [0.4 * mm, 20 * mm, -0.2 * mm])
    b = bmo.Lens(bmo.PlanoConvexLensSDF(q["r"], q["ct"], q["d"]), n_host)
    bmo.xrotate3d(b, math.radians(180))
    bmo.translate3d(b, [0, q["ct"], 0])
    bmo.zrotate3d(b, math.radians(-2))
    bmo.translate3d(b, [-0.3 * mm, 40 * mm, 0.3 * mm])
    det = bmo.PSFDetector(90 * mm)
    bmo.translate3d(det, [0, 100 * mm, 0])
    c.system, c.lens = bmo.System([a, b, det]), a
    n = tr.sellmeier(*FUSED_SILICA, planted=planted if planted == "sellmeier_metres" else None)
    lens = lambda o: tr.ExactLens(tr.Surface(q["r"]), tr.Surface(math.inf), q["ct"], q["d"], n, o.position(), o.orientation())
    c.exact = [lens(a), lens(b), tr.ExactFlat(90 * mm, det.position(), det.orientation(), "psf")]
    ob = math.radians(2)
    P, D = disc([0.4 * mm, 22 * mm, -0.2 * mm], [math.sin(ob), math.cos(ob), 0.0], 0.9 * q["d"], 48)
    c.bundle = bundle("ray", [P], [D], lam=np.tile(q["lams"], 16))
    c.name = "plano-convex"
    return c


PCV = dict(r=40 * mm, l=3 * mm, d=25.4 * mm, md=30 * mm, n=1.5)


def plano_concave(kind="ray", planted=None, axial=False):
    """Lens(PlanoConcaveLensSDF(40 mm, 3 mm, 25.4 mm, 30 mm), 1.5) (SphericalLensSDF.jl:349-381): a plano cylinder, a concave leaf behind it
    and a mechanical ring as thick as the lens at its edge, _l = l + sag, centred on _l / 2 (the biconcave one's ring sits at l / 2, :315-325),
    tilted 3 degrees.  Rays: a 2 degree oblique disc over 0.85 of the aperture, rings along the lens's own axis 1 mm beside it and at 14 mm - on
    the ring's plane faces - and two skew rays that enter through the ring's barrel, cross the air pocket of the concave face and re-enter.
    PolarizedRays take the two rings 0.004 off the axis' direction: ALONG it they meet the plane face along its normal and end there (axial=True:
    the fans of test_normal_incidence_on_a_flat_face_ends_a_polarized_ray)."""
    c = Case()
    q = PCV
    off = 0.0 if (kind == "ray" or axial) else 0.004
    lens = bmo.Lens(bmo.PlanoConcaveLensSDF(q["r"], q["l"], q["d"], q["md"]), lambda lam: q["n"])
    bmo.xrotate3d(lens, math.radians(3))
    bmo.translate3d(lens, [0.4 * mm, 20 * mm, 0])
    det = bmo.PSFDetector(90 * mm) if kind == "ray" else bmo.Spotdetector(90 * mm)
    bmo.translate3d(det, [0, 80 * mm, 0])
    c.system, c.lens = bmo.System([lens, det]), lens
    c.exact = [tr.ExactRingLens(tr.Surface(math.inf), tr.Surface(q["r"]), q["l"], lambda lam: q["n"], q["d"], q["d"], q["md"], q["md"], lens.position(),
                                lens.orientation(), planted),
               tr.ExactFlat(90 * mm, det.position(), det.orientation(), "psf" if kind == "ray" else "spot")]
    p0, axis = np.asarray(lens.position()), np.asarray(lens.orientation())[:, 1]
    P, D = zip(disc(p0 + 1.5 * mm * axis, [math.sin(math.radians(2)), math.cos(math.radians(2)), 0.0], 0.85 * q["d"], 34),
               ring(p0, axis, 1 * mm, 4, phase=0.9, slope=off), ring(p0, axis, 14 * mm, 8, phase=0.3, slope=off),
               _local_rays(lens, [[-q["md"] / 2, 4.0 * mm, 1 * mm], [-q["md"] / 2, 4.5 * mm, 1 * mm]], [[1.0, 0.01, 0.03], [1.0, -0.005, -0.02]], back=5 * mm))
    c.bundle = bundle(kind, P, D)
    c.name = "plano-concave-" + kind
    return c


TL = dict(R1=80 * mm, R2=120 * mm, d=25.4 * mm, n=1.5)


def thin_lens(planted=None):
    """SphericalLens(80 mm, 120 mm, 0, 25.4 mm, 1.5): a centre thickness of zero dispatches to ThinLens / ThinLensSDF (SphericalLenses.jl:20-45;
    both radii positive there, the back surface's signed radius is -120 mm): two caps, no barrel, a sharp rim.  Tilted 5 / -3 degrees and
    decentred.  Rays: a 2 degree oblique disc over 0.9 of the aperture and rings along the lens's own axis at 0.5 and at 0.98 of it (the
    lens is 66 um thick there)."""
    c = Case()
    q = TL
    lens = bmo.SphericalLens(q["R1"], q["R2"], 0, q["d"], q["n"])
    bmo.xrotate3d(lens, math.radians(5))
    bmo.zrotate3d(lens, math.radians(-3))
    bmo.translate3d(lens, [0.5 * mm, 20 * mm, -0.4 * mm])
    det = bmo.PSFDetector(90 * mm)
    bmo.translate3d(det, [0, 80 * mm, 0])
    c.system, c.lens = bmo.System([lens, det]), lens
    c.exact = [tr.ExactThinLens(q["R1"], q["R2"], q["d"], lambda lam: q["n"], lens.position(), lens.orientation(), planted),
               tr.ExactFlat(90 * mm, det.position(), det.orientation(), "psf")]
    p0, axis = np.asarray(lens.position()), np.asarray(lens.orientation())[:, 1]
    ob = math.radians(2)
    P, D = zip(disc(p0 + 0.8 * mm * axis, [math.sin(ob), math.cos(ob), 0.0], 0.9 * q["d"], 36), ring(p0, axis, 0.5 * q["d"] / 2, 4),
               ring(p0, axis, 0.98 * q["d"] / 2, 8, phase=0.37))
    c.bundle = bundle("ray", P, D)
    c.name = "thin-lens"
    return c


# ------------------------------------------------------------------------------------------------ scene 14: stand-alone primitive bodies
PRIM = dict(cyl=(5 * mm, 3 * mm), cut=(10 * mm, 4 * mm), ball=6 * mm, n=(1.52, 1.5, 1.6))


def primitives(kind="ray", planted=None):
    """Three bodies as Lens(shape, n), in a row along +y: CylinderSDF(5 mm, 3 mm) - the second number is the HALF height (PrimitiveSDF.jl:71-76)
    - tilted 20 / 5 degrees so that the bundle meets an end cap and, beside it, the barrel; CutSphereSDF(10 mm, 4 mm), the part of the ball above
    the plane y = 4 mm (:112-124), tilted -4 degrees, entered through the cut and left through the cap; SphereSDF(6 mm), whose orientation is
    fixed (SphericalLensSDF.jl:82-84), decentred.  A detector close behind the ball takes what it focuses.  Four rays run along the cylinder's
    own axis; PolarizedRays 0.004 off it (see plano_concave)."""
    c = Case()
    q = PRIM
    cyl = bmo.Lens(bmo.CylinderSDF(*q["cyl"]), lambda lam: q["n"][0])
    bmo.xrotate3d(cyl, math.radians(20))
    bmo.zrotate3d(cyl, math.radians(5))
    pc = np.array([0.2 * mm, 20 * mm, -0.1 * mm])
    bmo.translate3d(cyl, pc)
    cut = bmo.Lens(bmo.CutSphereSDF(*q["cut"]), lambda lam: q["n"][1])
    bmo.xrotate3d(cut, math.radians(-4))
    bmo.translate3d(cut, [-0.1 * mm, 36 * mm, 0.3 * mm])
    ball = bmo.Lens(bmo.SphereSDF(q["ball"]), lambda lam: q["n"][2])
    bmo.translate3d(ball, [0.15 * mm, 58 * mm, -0.1 * mm])
    det = bmo.PSFDetector(300 * mm) if kind == "ray" else bmo.Spotdetector(300 * mm)
    bmo.translate3d(det, [0, 72 * mm, 0])
    c.system, c.lens = bmo.System([cyl, cut, ball, det]), cyl
    mist = lambda *names: planted if planted in names else None
    c.exact = [tr.ExactCylinder(q["cyl"][0], q["cyl"][1], lambda lam: q["n"][0], cyl.position(), cyl.orientation(), mist("cylinder_axis_x")),
               tr.ExactCutSphere(q["cut"][0], q["cut"][1], lambda lam: q["n"][1], cut.position(), cut.orientation(), mist("cut_height_negated")),
               tr.ExactBall(q["ball"], lambda lam: q["n"][2], ball.position(), ball.orientation()),
               tr.ExactFlat(300 * mm, det.position(), det.orientation(), "psf" if kind == "ray" else "spot")]
    axis = np.asarray(cyl.orientation())[:, 1]
    P, D = zip(disc(pc + [0, 0, -1 * mm], [0.01, 1.0, 0.005], 7 * mm, 28, back=15 * mm), disc(pc + [0, 0, 4.7 * mm], [0, 1, 0], 1.6 * mm, 8, back=15 * mm),
               ring(pc, axis, 2 * mm, 4, back=15 * mm, slope=0.0 if kind == "ray" else 0.004), ring(pc + [0, 0, -1 * mm], [0, 1, 0], 3 * mm, 8, back=15 * mm, phase=0.4, slope=0.03))
    c.bundle = bundle(kind, P, D)
    c.name = "primitives-" + kind
    return c


SCENES = {
    "concave-mirror-ray": lambda **kw: concave_mirror("ray", **kw),
    "concave-mirror-pol": lambda **kw: concave_mirror("pol", **kw),
    "round-mirror-ray": lambda **kw: round_mirror("ray", **kw),
    "round-mirror-pol": lambda **kw: round_mirror("pol", **kw),
    "prism-mirror-ray": prism_mirror,
    "rect-mirror-ray": rect_mirror,
    "plano-convex": plano_convex,
    "plano-concave-ray": lambda **kw: plano_concave("ray", **kw),
    "plano-concave-pol": lambda **kw: plano_concave("pol", **kw),
    "thin-lens": thin_lens,
    "primitives-ray": lambda **kw: primitives("ray", **kw),
    "primitives-pol": lambda **kw: primitives("pol", **kw),
    "phone-l1": lambda **kw: phone_l12(1, **kw),
    "phone-l2": lambda **kw: phone_l12(2, **kw),
    "phone": phone,
    "plate-ray": lambda **kw: plate("ray", **kw),
    "plate-pol": lambda **kw: plate("pol", **kw),
    "roundplate-ray": lambda **kw: plate("ray", round_=True, **kw),
    "cube-ray": lambda **kw: cube("ray", **kw),
    "cube-pol": lambda **kw: cube("pol", **kw),
    "plate-gauss": lambda **kw: plate("gauss", **kw),
    "cube-gauss": lambda **kw: cube("gauss", **kw),
    "splitter-gauss": splitter_gauss,
    "polarizers": polarizers,
    "phone-l3": phone_l3,
    "prism-ray": lambda **kw: prism("ray", **kw),
    "prism-pol": lambda **kw: prism("pol", **kw),
    "rhomb": rhomb,
    "miniscope": miniscope,
    "concave-pairs-ray": lambda **kw: concave("ray", pairs=True, **kw),
    "concave-pairs-pol": lambda **kw: concave("pol", pairs=True, **kw),
    "doublet-gauss": lambda **kw: doublet("gauss", **kw),
    "cylinders": lambda **kw: cylinders(False, **kw),
    "acylinders": lambda **kw: cylinders(True, **kw),
    "block-ray": lambda **kw: block("ray", **kw),
    "block-pol": lambda **kw: block("pol", **kw),
    "concave-ray": lambda **kw: concave("ray", **kw),
    "concave-pol": lambda **kw: concave("pol", **kw),
    "doublet": doublet,
    "mirror45-ray": lambda **kw: mirror("ray", 45.0, **kw),
    "mirror45-pol": lambda **kw: mirror("pol", 45.0, **kw),
    "mirror85-ray": lambda **kw: mirror("ray", 85.0, **kw),
    "mirror85-pol": lambda **kw: mirror("pol", 85.0, **kw),
    "retro-ray": lambda **kw: retro("ray", **kw),
    "retro-pol": lambda **kw: retro("pol", **kw),
    "splitter-ray": lambda **kw: splitter("ray", **kw),
    "splitter-pol": lambda **kw: splitter("pol", **kw),
    "singlet-gauss": lambda **kw: singlet("gauss", **kw),
    "singlet-ray": lambda **kw: singlet("ray", **kw),
    "singlet-pol": lambda **kw: singlet("pol", **kw),
    "asphere-curved-first": lambda **kw: asphere(False, **kw),
    "asphere-plane-first": lambda **kw: asphere(True, **kw),
}
NO_EXCLUSIONS = ("phone-l3", "cylinders", "acylinders", "doublet", "doublet-gauss", "asphere-curved-first", "asphere-plane-first",  # the issue's scenes 3 - 5 allow none
                 "plate-ray", "plate-pol", "plate-gauss", "roundplate-ray", "cube-ray", "cube-pol", "cube-gauss", "splitter-gauss", "polarizers",
                 "concave-mirror-ray", "concave-mirror-pol", "round-mirror-ray", "round-mirror-pol", "prism-mirror-ray", "rect-mirror-ray", "plano-convex",
                 "phone-l1", "phone-l2", "phone")
# Each planted mistake, and the scenes that exercise it.
PLANTED_ON = [
    ("conic_sign", "phone-l3"),
    ("coef_shift", "phone-l3"),
    ("conic_sign", "asphere-curved-first"),
    ("coef_shift", "asphere-curved-first"),
    ("coef_shift", "asphere-plane-first"),
    ("back_vertex_edge_sag", "singlet-ray"),
    ("cylinder_extruded_along_z", "cylinders"),
    ("cylinder_extruded_along_z", "acylinders"),
    ("exit_normal_not_flipped", "singlet-ray"),
    ("exit_normal_not_flipped", "asphere-curved-first"),
    ("n2_glass_on_exit", "singlet-ray"),
    ("ts_tp_swapped", "singlet-pol"),
    ("tir_phase_conjugated", "singlet-pol"),
    ("tir_phase_conjugated", "block-pol"),
    ("tir_phase_conjugated", "rhomb"),
    ("tir_phase_conjugated", "prism-pol"),
    ("opl_next_medium", "singlet-ray"),
    ("plate_no_refraction", "plate-ray"),
    ("plate_no_refraction", "roundplate-ray"),
    ("plate_normal_not_flipped", "plate-ray"),
    ("plate_normal_not_flipped", "plate-gauss"),
    ("plate_indices_swapped", "plate-ray"),
    ("plate_indices_swapped", "plate-gauss"),
    ("cube_children_in_air", "cube-ray"),
    ("cube_children_in_air", "cube-pol"),
    ("gauss_no_phase_flip", "cube-gauss"),
    ("gauss_no_phase_flip", "splitter-gauss"),
    ("gauss_flip_on_both_sides", "plate-gauss"),
    ("gauss_flip_on_both_sides", "splitter-gauss"),
    ("gauss_child_keeps_w0", "splitter-gauss"),
    ("gauss_child_keeps_w0", "plate-gauss"),
    ("gauss_w0_at_start", "splitter-gauss"),
    ("polarizer_rotation_transposed", "polarizers"),
    ("polarizer_not_projected", "polarizers"),
    ("coating_loses_tie", "plate-ray"),
    ("coating_loses_tie", "plate-pol"),
    ("mirror_centre_wrong_side", "concave-mirror-ray"),
    ("prism_mirror_pre_45", "prism-mirror-ray"),
    ("ring_centred_half_l", "plano-concave-ray"),
    ("thin_back_not_shifted", "thin-lens"),
    ("cut_height_negated", "primitives-ray"),
    ("cylinder_axis_x", "primitives-ray"),
    ("sellmeier_metres", "plano-convex"),
    ("aspheric_edge_sag_unsigned", "phone-l2"),
]


# ------------------------------------------------------------------------------------------------ the comparison
QUANT = ("t", "n", "pos", "dir", "index", "E0", "opl", "row_pos", "row_dir", "proj", "k", "w0", "E0_child")


class Held:
    """What hold() found: worst absolute differences and worst difference / bound per quantity, the counts, and the bounces over their bound."""

    def __init__(self):
        self.abs = {q: 0.0 for q in QUANT}
        self.ratio = {q: 0.0 for q in QUANT}
        self.bounces = self.excluded = self.tir = self.barrel = self.leaving = self.children = self.ortho = self.blocked = self.ties = 0
        self.facing = {True: 0, False: 0}  # coatings met with dot(dir, normal) < 0 / > 0
        self.phase = {True: 0, False: 0}   # beamlets reflected with phi = pi / phi = 0
        self.pieces = {}                   # held bounces per (object, piece of its exact boundary, 'in' / 'out'); a mesh's piece is 'face<k>'
        self.over = []

    def note(self, q, diff, bound, where):
        diff, bound = float(diff), float(bound)
        self.abs[q] = max(self.abs[q], diff)
        r = diff / bound if bound > 0 else (0.0 if diff == 0 else math.inf)
        self.ratio[q] = max(self.ratio[q], r)
        if r > 1.0:
            self.over.append((q, where, diff, bound))

    def worst(self):
        return max(self.ratio.values())

    def worst_finite(self):
        """The largest ratio among the quantities whose bound is not zero."""
        return max([r for r in self.ratio.values() if math.isfinite(r)], default=0.0)

    def line(self, name):
        return ("%s: %d bounces (%d leaving, %d on the barrel, %d TIR, %d splits), %d excluded; worst |dt| %.3g m, |dn| %.3g, |ddir| %.3g, |dE0| %.3g, |dopl| %.3g m; "
                "worst recorded / bound %.3g (%s)" % (name, self.bounces, self.leaving, self.barrel, self.tir, self.children, self.excluded, self.abs["t"], self.abs["n"],
                                                    self.abs["dir"], self.abs["E0"], self.abs["opl"], self.worst(), max(self.ratio, key=self.ratio.get)))


def hold(res, case, consts, nodes=None, wrong=None, planted=None, cache=None):
    """Every recorded bounce of beams `nodes` of the TraceResult against exact_step within step_bound -> Held.  wrong / planted: the exact
    objects built with a planted mistake, and the switch: then the differences are taken to THAT evaluation (the bound stays the right one's).
    cache: a dict that keeps the right evaluation and the bound of every bounce of THIS result between calls."""
    mp = tr._mp()
    h = Held()
    with mp.workdps(50):
        det_row = {}
        for slot in range(res.n_detectors):
            for row, nd in zip(res.detector_hits(slot), res.detector_nodes(slot)):
                det_row[int(nd)] = row
        for node, sub in [(n, j) for n in (range(res.n_nodes) if nodes is None else nodes) for j in range(3 if res.rec_planes == 33 else 1)]:
            segs = tr.segments_of(res, node, sub)
            anc = tr.ancestors(res, node)
            base = tr.exact_opl(anc, len(anc))
            for k, seg in enumerate(segs):
                if seg["obj"] < 0:
                    continue
                where = (int(node), k, sub)
                seg = dict(seg, opl=base + tr.exact_opl(segs, k))
                obj = solid_of(case, case.exact, seg)
                if sub and obj.kind == "plate_coating":  # waist and divergence ray take n_t / n_r by the CHIEF ray's isentering
                    chief = tr.segments_of(res, node, 0)[k]
                    seg["chief_entering"] = bool(tr.exact_step(chief, obj, consts)["hit"]["cos"] < 0)
                if cache is not None and where in cache:
                    ex, b = cache[where]
                else:
                    ex = tr.exact_step(seg, obj, consts)
                    assert ex is not None, ("the record has a hit where the exact evaluator has none", where)
                    b = None if tr.excluded(ex) else tr.step_bound(seg, ex, obj, consts, n_seg=len(anc) + k + 1)
                    if cache is not None:
                        cache[where] = (ex, b)
                h.bounces += 1
                if b is None:
                    h.excluded += 1
                    continue
                h.leaving += bool(ex["hit"]["leaving"])
                h.barrel += ex["hit"]["piece"] == "barrel"
                if sub == 0:
                    key = (seg["obj"], "face%d" % ex["hit"]["face"] if "face" in ex["hit"] else ex["hit"]["piece"], "out" if ex["hit"]["leaving"] else "in")
                    h.pieces[key] = h.pieces.get(key, 0) + 1
                # where the reference's PolarizedRay constructor throws (PolarizedRays.jl:54-56) or a filter blocks, the record ends there with that status
                status, last = int(res.node_status[node]), k == len(segs) - 1
                assert (ex["end"] == "err_ortho") == bool(last and status & 256), (where, ex["end"], status)
                assert (ex["end"] == "blocked") == bool(last and status & 128), (where, ex["end"], status)
                h.ortho += ex["end"] == "err_ortho"
                h.blocked += ex["end"] == "blocked"
                if obj.kind in ("thin_bs", "plate_coating", "cube_coating") and sub == 0:
                    h.facing[bool(ex["hit"]["cos"] < 0)] += 1
                    if obj.kind == "plate_coating" and (cache is None or ("tie", where) not in cache):
                        # the coated-face tie: the substrate's exact length is approximately the coating's (PlateBeamsplitter.jl:176)
                        s = tr.exact_hit(case.exact[seg["obj"]].parts[0], tr._v(seg["pos"]), tr._v(seg["dir"]), consts)
                        tie = s is not None and abs(s["t"] - ex["t"]) <= 2.0 ** -26 * max(abs(s["t"]), abs(ex["t"]))
                        if cache is not None:
                            cache[("tie", where)] = tie
                    if obj.kind == "plate_coating":
                        h.ties += bool(cache[("tie", where)] if cache is not None else tie)
                cmp_ = ex
                if planted is not None:
                    solid = solid_of(case, wrong, seg)
                    if planted == "coating_loses_tie" and obj.kind == "plate_coating":
                        # the evaluator that lets the substrate win the tie of the coated face meets the substrate where the record has the coating
                        at_sub = tr.exact_step(seg, wrong[seg["obj"]].parts[0], consts)
                        if at_sub is not None and abs(at_sub["t"] - ex["t"]) <= 2.0 ** -26 * max(abs(at_sub["t"]), abs(ex["t"])):
                            solid = wrong[seg["obj"]].parts[0]
                    cmp_ = tr.exact_step(dict(seg, opl=base + tr.exact_opl(segs, k, planted)), solid, consts, planted)
                    if cmp_ is None or (cmp_["next"] is None) != (ex["next"] is None):
                        h.note("t", math.inf, 1.0, where)
                        continue
                dt = tr._f(seg["t"]) - cmp_["t"]
                h.note("t", abs(dt), b["t_lo"] if dt < 0 else b["t_hi"], where)
                h.note("n", tr.fdiff(seg["normal"], cmp_["normal"]), b["n"], where)
                nx = cmp_["next"]
                if nx is not None and k + 1 < len(segs):
                    h.tir += bool(cmp_["interaction"]["tir"]) and obj.kind == "lens"
                    s2 = segs[k + 1]
                    h.note("pos", tr.fdiff(s2["pos"], nx["pos"]), b["pos"], where)
                    h.note("dir", tr.fdiff(s2["dir"], nx["dir"]), b["dir"], where)
                    h.note("index", tr.fdiff(s2["n"], nx["n"]), b.get("index", 0.0), where)
                    if nx["E0"] is not None:
                        h.note("E0", tr.fdiff(s2["E0"], nx["E0"]), b["E0"], where)
                if cmp_["children"] is not None:  # the first rays of the two beams a splitter spawns, transmitted first (Beamsplitters.jl:16-19)
                    first = int(res.node_first_child[node])
                    assert first >= 0, where
                    h.children += sub == 0
                    for i, o in enumerate(cmp_["children"]):
                        s2 = tr.segments_of(res, first + i, sub)[0]  # the child's chief, waist or divergence ray: each is split as a Ray of its own
                        assert int(res.node_parent[first + i]) == node
                        h.note("pos", tr.fdiff(s2["pos"], o["pos"]), b["pos"], where)
                        h.note("dir", tr.fdiff(s2["dir"], o["dir"]), b["outs"][i]["dir"], where)
                        h.note("index", tr.fdiff(s2["n"], o["n"]), 0.0, where)
                        if o["E0"] is not None:
                            h.note("E0", tr.fdiff(s2["E0"], o["E0"]), b["outs"][i]["E0"], where)
                    if res.rec_planes == 33 and sub == 0:  # once per split: the waist and the field the two child beamlets are built with
                        facing = bool(ex["hit"]["cos"] < 0)
                        key = ("gauss", int(node))
                        if cache is not None and key in cache:
                            right = cache[key]
                        else:
                            right = tr.exact_gauss_children(tr.gauss_record(res, node), obj, facing)
                            if cache is not None:
                                cache[key] = right
                        g = right if planted is None else tr.exact_gauss_children(tr.gauss_record(res, node), obj, facing, planted)
                        h.phase[facing] += 1
                        for i, E in enumerate((g["E_t"], g["E_r"])):
                            aux = res.node_aux[first + i]
                            h.note("w0", tr.fdiff(float(aux[0]), g["w0"]), right["b_w0"], where)
                            h.note("E0_child", tr.fdiff(complex(aux[1], aux[2]), E), right["b_E"][i], where)
                if cmp_["row"] is not None:
                    row = det_row[int(node)]
                    x = cmp_["row"]
                    u = tr.U
                    if len(x) == 2:  # a Spotdetector's (x, z): two dot products of hit - position with the axes (Spotdetector.jl:50-61)
                        mag = float(tr._norm(cmp_["point"])) + obj.pos_mag
                        h.note("row_pos", tr.fdiff(row[0:2], x), 1.5 * b["pos"] + 8 * u * mag, where)
                        continue
                    h.note("row_pos", tr.fdiff(row[0:3], x[0:3]), b["pos"], where)
                    h.note("row_dir", tr.fdiff(row[3:6], x[3:6]), 0.0, where)
                    h.note("opl", tr.fdiff(row[6], x[6]), b["opl"] + u * float(x[6]), where)
                    h.note("proj", tr.fdiff(row[7], x[7]), b["proj"], where)
                    h.note("k", tr.fdiff(row[8], x[8]), 3 * u * float(x[8]), where)
    return h


def solid_of(case, exact, seg):
    """The solid of the exact scene that the record says was hit: the object, and for a doublet the part whose shape the record names."""
    obj = exact[seg["obj"]]
    return obj.parts[case.shape_part[seg["shape"]]] if hasattr(obj, "parts") else obj


def compile_case(c):
    """The compiled scene of a case, the march constants, and which part of a doublet every shape id of the record means."""
    c.scene = bmo.CompiledScene(c.system, c.bundle.lambdas)
    c.consts = tr.consts_of(c.scene)
    # a plate splitter's parts are substrate 0 / coating 1, a cube's front 0 / back 1 / coating 2 (shape(pbs), shape(cbs))
    multi = (bmo.DoubletLens, bmo.RectangularPlateBeamsplitter, bmo.CubeBeamsplitter)
    c.shape_part = {c.scene.shape_id(s): i for o in c.system.objects() if isinstance(o, multi) for i, s in enumerate(o.parts())}
    return c


def tree_nodes(res, roots):
    """The beams of the trees of the given root rays (indices into the bundle): the root's node and everything below it."""
    top = np.flatnonzero(res.node_parent < 0)
    out, todo = [], [int(top[i]) for i in roots]
    while todo:
        n = todo.pop()
        out.append(n)
        first = int(res.node_first_child[n])
        if first >= 0:
            todo += [first, first + 1]
    return sorted(out)


def root_of(bundle, i):
    P = bundle.planes
    if bundle.kind == bmo.BEAM_GAUSSIAN:  # the chief ray
        return dict(pos=P[0:3, i].copy(), dir=P[3:6, i].copy(), lam=float(P[18, i]), n=float(P[19, i]), E0=None)
    r = dict(pos=P[0:3, i].copy(), dir=P[3:6, i].copy(), lam=float(P[6, i]), n=float(P[7, i]), E0=None)
    if bundle.kind == bmo.BEAM_POLARIZED:
        r["E0"] = [complex(P[8, i], P[9, i]), complex(P[10, i], P[11, i]), complex(P[12, i], P[13, i])]
    return r


def sequence(res, node, case):
    """((object, part of a doublet) per segment, detected) of a recorded beam."""
    first, nseg = int(res.node_first_rec[node]), int(res.node_nseg[node])
    return [(int(o), case.shape_part.get(int(sh), 0)) for o, sh in zip(res.rec_obj[first:first + nseg], res.rec_shape[first:first + nseg])], bool(
        res.node_status[node] & 16)


def exact_sequence(trace, case):
    objs = [(s["obj"], s["part"]) for s in trace]
    detected = trace[-1]["ex"] is not None and getattr(case.exact[trace[-1]["obj"]], "kind", None) in ("psf", "spot", "pd")
    return objs, detected


def left_out(trace):
    """True where some bounce of the exact trace (its children's included) meets the exclusion criterion."""
    return any((s["ex"] is not None and tr.excluded(s["ex"], s["tie"])) or any(left_out(c) for c in s.get("children", ())) for s in trace)


def same_tree(trace, res, node, case):
    """The exact trace and the recorded beam tree below `node`: the same objects in the same order, the same end, the same children."""
    assert exact_sequence(trace, case) == sequence(res, node, case), node
    end = trace[-1]["ex"]["end"] if trace[-1]["ex"] is not None else None
    assert (end == "err_ortho", end == "blocked") == (bool(res.node_status[node] & 256), bool(res.node_status[node] & 128)), (node, end)
    kids = trace[-1].get("children")
    first = int(res.node_first_child[node])
    assert (kids is None) == (first < 0), node
    for i, sub in enumerate(kids or ()):
        same_tree(sub, res, first + i, case)


def _part(case, s):
    obj = case.exact[s["obj"]]
    return obj.parts[s["part"]] if hasattr(obj, "parts") else obj


def end_to_end(res, case, consts, roots):
    """exact_trace from the root doubles to the detector against the recorded detector row, inside
    sum_bounces |d(final) / d(bounce output)| step_bound, each sensitivity a difference of the exact trace in 50 digits -> Held (row_pos, row_dir, opl)."""
    mp = tr._mp()
    h = Held()
    with mp.workdps(50):
        det_row = {int(nd): row for slot in range(res.n_detectors) for row, nd in zip(res.detector_hits(slot), res.detector_nodes(slot))}
        step = mp.mpf(10) ** -13
        for i in roots:
            if i not in det_row:
                continue
            root = root_of(case.bundle, i)
            base = tr.exact_trace(root, case.exact, consts, R_MAX)
            if base[-1]["ex"] is None or base[-1]["ex"]["row"] is None or any(tr.excluded(s["ex"], s["tie"]) for s in base):
                continue
            final = base[-1]["ex"]["row"]
            last = base[-1]
            bl = tr.step_bound(last["seg"], last["ex"], _part(case, last), consts, n_seg=len(base))
            bound = dict(pos=bl["pos"], dir=mp.mpf(0), opl=bl["opl"] + tr.U * final[6])
            for j, s in enumerate(base[:-1]):
                b = tr.step_bound(s["seg"], s["ex"], _part(case, s), consts, n_seg=j + 1)
                bound["opl"] += b["opl_inc"]
                d_in = s["seg"]["dir"]
                dt = max(b["t_lo"], b["t_hi"])
                kicks = [((tr._scale(step, d_in), [0, 0, 0]), dt)]
                for e in ([1, 0, 0], [0, 1, 0], [0, 0, 1]):
                    kicks.append(((tr._scale(step, e), [0, 0, 0]), b["pos"] - dt))
                for e in tr._tangents(s["ex"]["next"]["dir"]):
                    kicks.append((([0, 0, 0], tr._scale(step, e)), b["dir"]))
                for (dp, dd), size in kicks:
                    # the ray that leaves bounce j, moved; it is followed through the solids the un-moved trace met (a kick of 1e-13 changes none)
                    nx = s["ex"]["next"]
                    moved = tr.exact_trace(dict(pos=tr._add(nx["pos"], dp), dir=tr._unit(tr._add(nx["dir"], dd)), n=nx["n"], lam=root["lam"], opl=s["ex"]["opl"]),
                                           case.exact, consts, R_MAX, follow=[(m["obj"], m["part"]) for m in base[j + 1:]])
                    assert len(moved) == len(base) - j - 1 and moved[-1]["ex"] is not None
                    f2 = moved[-1]["ex"]["row"]
                    bound["pos"] += tr._norm(tr._sub(f2[0:3], final[0:3])) / step * size
                    bound["dir"] += tr._norm(tr._sub(f2[3:6], final[3:6])) / step * size
                    bound["opl"] += abs(f2[6] - final[6]) / step * size
            row = det_row[i]
            h.bounces += 1
            h.note("row_pos", tr.fdiff(row[0:3], final[0:3]), bound["pos"], (i, "end"))
            h.note("row_dir", tr.fdiff(row[3:6], final[3:6]), bound["dir"], (i, "end"))
            h.note("opl", tr.fdiff(row[6], final[6]), bound["opl"], (i, "end"))
    return h

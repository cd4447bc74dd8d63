"""Host-side mirror of the reference's optical components (constructors + kinematics only).

The optical *interaction* of every component (interact3d) runs inside the HIP engine; the
classes here only carry geometry and parameters into the flat object table.  Citations are
relative to /root/reference/src/OpticalComponents.
"""
import math

import numpy as np

from . import linalg as la
from . import shapes as sh

# object kinds (include/bmo.h enum bmo_object_kind)
(O_MIRROR, O_REFRACTIVE, O_DOUBLET, O_THIN_BS, O_PLATE_BS, O_CUBE_BS, O_SPOT, O_PSF, O_INTERSECTABLE, O_NONINTERACTABLE,
 O_POLARIZER, O_PHOTODETECTOR) = range(12)


# ------------------------------------------------------------------ refractive indices
class DiscreteRefractiveIndex:
    """Utils/RefractiveIndexUtils.jl:8-31: exact-key lookup, KeyError otherwise."""

    def __init__(self, lambdas, ns):
        if len(lambdas) != len(ns):  # RefractiveIndexUtils.jl:23-25 (ArgumentError)
            raise ValueError("Number of wavelengths must match number of ref. indices")
        self.data = {float(l): float(n) for l, n in zip(lambdas, ns)}

    def __call__(self, lam):
        return self.data[float(lam)]


class SellmeierEquation:
    """Utils/RefractiveIndexUtils.jl:82-98."""

    def __init__(self, B1, B2, B3, C1, C2, C3):
        self.c = (B1, B2, B3, C1, C2, C3)

    def __call__(self, lam):
        B1, B2, B3, C1, C2, C3 = self.c
        lam = lam * 1e6
        n2 = 1 + (B1 * lam ** 2) / (lam ** 2 - C1) + (B2 * lam ** 2) / (lam ** 2 - C2) + (B3 * lam ** 2) / (lam ** 2 - C3)
        return math.sqrt(n2)


def _as_index(n):
    if callable(n):
        return n
    val = float(n)
    return lambda lam: val


# ---------------------------------------------------------------------- object bases
class AbstractObject:
    """AbstractTypes/AbstractObject.jl:36 with the SingleShape trait (AbstractShapeTrait.jl:31-52)."""

    kind = None

    def __init__(self, shape):
        self.shape = shape

    def parts(self):
        return [self.shape]

    def position(self):
        return self.shape.pos

    def orientation(self):
        return self.shape.dir

    def _translate3d(self, offset):
        self.shape._translate3d(offset)

    def _rotate3d(self, axis, theta):
        self.shape._rotate3d(axis, theta)

    def _align3d(self, axis):
        self.shape._align3d(axis)

    def _reset_translation3d(self):
        self.shape._reset_translation3d()

    def _reset_rotation3d(self):
        self.shape._reset_rotation3d()

    @property
    def thickness(self):
        return sh.thickness(self.shape)


class _MultiShape(AbstractObject):
    """MultiShape trait kinematics, AbstractShapeTrait.jl:54-128."""

    def subparts(self):
        raise NotImplementedError

    def position(self):
        return sh.position(self.subparts()[0])

    def orientation(self):
        return sh.orientation(self.subparts()[0])

    def _set_position(self, pos):
        pass

    def _set_orientation(self, d):
        pass

    def _translate3d(self, offset):
        off = la.vec3(offset)
        self._set_position(self.position() + off)
        for p in self.subparts():
            p._translate3d(off)

    def _rotate3d(self, axis, theta):
        R = la.rotate3d(axis, theta)
        self._set_orientation(R @ self.orientation())
        for p in self.subparts():
            p._rotate3d(axis, theta)
            v = sh.position(p) - self.position()  # position(object) re-read per part (AbstractShapeTrait.jl:122)
            v = (R @ v) - v
            p._translate3d(v)

    def _reset_translation3d(self):  # AbstractShapeTrait.jl:144-150 (sub-part relative translations are kept)
        self._translate3d(-self.position())
        self._set_position(np.zeros(3))

    def _reset_rotation3d(self):  # AbstractShapeTrait.jl:160-173: undo the net rotation about its axis (sub-part rotations are kept)
        R = self.orientation()
        theta = math.acos(min(1.0, max(-1.0, (np.trace(R) - 1) / 2)))
        if theta == 0:
            return
        axis = 1 / (2 * math.sin(theta)) * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
        self._rotate3d(axis, -theta)
        self._set_orientation(np.eye(3))


class ObjectGroup(_MultiShape):
    """ObjectGroups.jl:21-47."""

    kind = None

    def __init__(self, objects):
        self.objects = list(objects)
        self.center = np.zeros(3)
        self.dir = np.eye(3)

    def subparts(self):
        return self.objects

    def position(self):
        return self.center

    def orientation(self):
        return self.dir

    def _set_position(self, pos):
        self.center = np.array(pos, dtype=np.float64)

    def _set_orientation(self, d):
        self.dir = np.array(d, dtype=np.float64)


def leaves(objs):
    """Leaves(system.objects) System.jl:21: depth-first flattening of object groups."""
    out = []
    for o in objs:
        if isinstance(o, ObjectGroup):
            out.extend(leaves(o.objects))
        else:
            out.append(o)
    return out


# ------------------------------------------------------------------------- components
class Mirror(AbstractObject):  # Mirrors.jl:76-78
    kind = O_MIRROR


def SquarePlanoMirror2D(size):  # Mirrors.jl:93-96
    return Mirror(sh.QuadraticFlatMesh(size))


def RectangularPlanoMirror2D(width, height):
    return Mirror(sh.RectangularFlatMesh(width, height))


def RectangularPlanoMirror(width, height, thickness):  # Mirrors.jl:110-119
    shape = sh.CuboidMesh(width, thickness, height)
    sh.translate3d(shape, [-width / 2, 0, -height / 2])
    shape.set_new_origin3d()
    return Mirror(shape)


def SquarePlanoMirror(width, thickness):  # Mirrors.jl:134-136
    return RectangularPlanoMirror(width, width, thickness)


def RoundPlanoMirror(diameter, thickness):  # Mirrors.jl:161-164
    return Mirror(sh.PlanoSurfaceSDF(thickness, diameter))


def ConcaveSphericalMirror(radius, thickness, diameter):  # Mirrors.jl:195-200
    cylinder = sh.PlanoSurfaceSDF(thickness, diameter)
    concave = sh.ConcaveSphericalSurfaceSDF(abs(radius), diameter)
    return Mirror(concave + cylinder)


def RightAnglePrismMirror(leg_length, height):  # Mirrors.jl:226-230
    shape = sh.RightAnglePrismSDF(leg_length, height)
    sh.zrotate3d(shape, math.radians(45 + 180))
    return Mirror(shape)


def Retroreflector(scale):  # Misc.jl:34-49
    return Mirror(sh.RetroMesh(scale))


class Lens(AbstractObject):
    """Lenses.jl:145-155.  Lens(shape, n) or Lens(front_surface, back_surface, thickness, n) (:176-311)."""

    kind = O_REFRACTIVE

    def __init__(self, *args):
        if len(args) == 2:
            shape, n = args
        elif len(args) == 4:
            shape = sh.lens_shape_from_surfaces(args[0], args[1], args[2])
            n = args[3]
        elif len(args) == 3:  # Lens(front_surface, center_thickness, n) :293-302 / :390-399
            flat = sh.RectangularFlatSurface if isinstance(args[0], sh.CylindricalSurface) else sh.CircularFlatSurface
            shape = sh.lens_shape_from_surfaces(args[0], flat(args[0].diameter), args[1])
            n = args[2]
        else:
            raise TypeError("Lens(shape, n) or Lens(front, back, thickness, n)")
        super().__init__(shape)
        self.n = _as_index(n)


class Prism(Lens):  # Prisms.jl:1-16
    pass


def RightAnglePrism(leg_length, height, n):  # Prisms.jl:28-31
    return Prism(sh.RightAnglePrismSDF(leg_length, height), n)


def SphericalLens(r1, r2, l, d=la.inch, n=1.5):  # SphericalLenses.jl:20-32
    if l == 0:
        return ThinLens(r1, r2, d, n)
    return Lens(sh.SphericalSurface(r1, d), sh.SphericalSurface(r2, d), l, n)


def ThinLens(R1, R2, d, n):  # SphericalLenses.jl:40-44
    return Lens(sh.ThinLensSDF(R1, R2, d), n)


class DoubletLens(_MultiShape):  # DoubletLenses.jl:26-38
    kind = O_DOUBLET

    def __init__(self, front, back):
        self.front, self.back = front, back

    def subparts(self):
        return [self.front, self.back]

    def parts(self):
        return [self.front.shape, self.back.shape]

    @property
    def thickness(self):
        return sh.thickness(self.front.shape) + sh.thickness(self.back.shape)


def SphericalDoubletLens(r1, r2, r3, l1, l2, d, n1, n2):  # DoubletLenses.jl:57-64
    front = SphericalLens(r1, r2, l1, d, n1)
    back = SphericalLens(r2, r3, l2, d, n2)
    sh.translate3d(back, [0, sh.thickness(front.shape), 0])
    return DoubletLens(front, back)


class ThinBeamsplitter(AbstractObject):  # Beamsplitters/ThinBeamsplitter.jl:16-67
    kind = O_THIN_BS

    def __init__(self, *args, reflectance=0.5, _shape=None):
        if _shape is None:
            if reflectance >= 1 or abs(reflectance) <= 1.4901161193847656e-08 * abs(reflectance):
                raise ValueError("Splitting ratio in (0, 1)!")
            width = args[0]
            height = args[1] if len(args) > 1 else width
            _shape = sh.RectangularFlatMesh(width, height)
        super().__init__(_shape)
        self.reflectance = math.sqrt(reflectance)
        self.transmittance = math.sqrt(1 - self.reflectance ** 2)


def RoundThinBeamsplitter(diameter, reflectance=0.5):  # ThinBeamsplitter.jl:59-67
    return ThinBeamsplitter(reflectance=reflectance, _shape=sh.CircularFlatMesh(diameter / 2))


class RectangularPlateBeamsplitter(_MultiShape):  # Beamsplitters/PlateBeamsplitter.jl:66-104
    kind = O_PLATE_BS

    def __init__(self, width, height, thickness, n, reflectance=0.5, _round=False):
        if _round:
            self.substrate = Prism(sh.PlanoSurfaceSDF(thickness, width), n)
            self.coating = RoundThinBeamsplitter(width, reflectance=reflectance)
        else:
            self.substrate = Prism(sh.BoxSDF(width, thickness, height), n)
            sh.translate3d(self.substrate, [0, thickness / 2, 0])
            self.coating = ThinBeamsplitter(width, height, reflectance=reflectance)
            sh.zrotate3d(self.coating, math.pi)
        self.n = self.substrate.n

    def subparts(self):  # shape(pbs) = (substrate, coating) PlateBeamsplitter.jl:30
        return [self.substrate, self.coating]

    def position(self):  # PlateBeamsplitter.jl:26-27
        return sh.position(self.coating)

    def orientation(self):
        return sh.orientation(self.substrate)

    def parts(self):
        return [self.substrate.shape, self.coating.shape]


def RoundPlateBeamsplitter(diameter, thickness, n, reflectance=0.5):  # PlateBeamsplitter.jl:141-158
    return RectangularPlateBeamsplitter(diameter, diameter, thickness, n, reflectance=reflectance, _round=True)


class CubeBeamsplitter(_MultiShape):  # Beamsplitters/CubeBeamsplitter.jl:23-61
    kind = O_CUBE_BS

    def __init__(self, leg_length, n, reflectance=0.5):
        self.front = RightAnglePrism(leg_length, leg_length, n)
        self.back = RightAnglePrism(leg_length, leg_length, n)
        self.coating = ThinBeamsplitter(math.sqrt(2) * leg_length, leg_length, reflectance=reflectance)
        sh.zrotate3d(self.back, math.radians(180))
        sh.zrotate3d(self.coating, math.radians(180 - 45))
        self.coating.shape.set_new_origin3d()
        self.n = self.front.n

    def subparts(self):
        return [self.front, self.back, self.coating]

    def parts(self):
        return [self.front.shape, self.back.shape, self.coating.shape]


class Spotdetector(AbstractObject):  # Detectors/Spotdetector.jl:21-45
    kind = O_SPOT

    def __init__(self, width):
        shape = sh.QuadraticFlatMesh(width)
        sh.zrotate3d(shape, math.pi)
        super().__init__(shape)
        self.hw = width / 2
        self.data = np.zeros((0, 2))

    def empty(self):
        self.data = np.zeros((0, 2))

    # ---- read-out on the GPU engine (bmo_spot_image / bmo_spot_stats; the reference leaves `data` to its users)
    def stats(self, device=0):
        """The twelve spot statistics (abi.SPOT_* columns: N, centroid, extrema, central moments, RMS and geometric radius) of all rows
        accumulated so far (the detector is not reset between solves, like the reference)."""
        from . import abi

        return abi.spot_stats(self.data, device=device)[0]

    def image(self, nx, nz=None, window=None, device=0):
        """The spot diagram of all rows accumulated so far as an image: (x_edges [nx + 1], z_edges [nz + 1], counts int64 [nx, nz], outside).
        window: (x0, x1, z0, z1); None is the detector face (-hw, hw, -hw, hw); "extent" the extrema of the rows (ValueError without rows
        or with a zero extent).  Membership is the floor rule of include/bmo.h, not a search in the edges: a row is inside iff
        x0 <= x <= x1 and z0 <= z <= z1 and counts in bin i = min(floor((x - x0) * (nx / (x1 - x0))), nx - 1), j likewise; `outside`
        counts the other rows.  The edges are linrange(x0, x1, nx + 1), for plotting."""
        from . import abi

        nz = nx if nz is None else nz
        if window is None:
            window = (-self.hw, self.hw, -self.hw, self.hw)
        elif isinstance(window, str):
            if window != "extent":
                raise ValueError('Spotdetector.image: window must be (x0, x1, z0, z1), None or "extent"')
            window = spot_extent_window(self.stats(device), "Spotdetector.image")
        counts, outside, _ = abi.spot_image(self.data, window, nx, nz, device=device)
        return la.linrange(window[0], window[1], nx + 1), la.linrange(window[2], window[3], nz + 1), counts, outside

    def encircled_energy(self, radii, center=None, shape="circle", device=0):
        """The share of all rows accumulated so far inside a circle (shape "circle": r2 <= R * R) or a square ("square": |ax| <= R and
        |az| <= R) of half-size R about `center` = (x, z), for every R of `radii` (bmo_spot_ee): (fraction [nr], inside int64 [nr], n_rows).
        center None: the centroid CX, CZ of stats().  Without rows the fraction is NaN."""
        from . import abi

        if center is None:
            center = spot_ee_centers(self.stats(device))
        inside, _ = abi.spot_ee(self.data, center, radii, shape=shape, device=device)
        return spot_ee_fraction(inside, len(self.data)), inside, len(self.data)


def spot_ee_centers(stats):
    """The centroid (CX, CZ) of spot statistics ([12] or [K, 12]) as the centre of an encircled-energy curve; (0, 0) where there is no row."""
    st = np.asarray(stats, dtype=np.float64)
    return np.where(st[..., 0:1] > 0, st[..., 1:3], 0.0)


def spot_ee_fraction(inside, n_rows):
    """inside / n_rows ([nr] with one count, [K, nr] with [K]); NaN where there is no row."""
    n = np.asarray(n_rows, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(n[..., None] > 0, np.asarray(inside, dtype=np.float64) / n[..., None], np.nan)


def spot_extent_window(stats, who):
    """The window X_MIN .. Z_MAX of spot statistics [12]; ValueError (starting with `who`) without rows or with a zero extent."""
    if stats[0] == 0:
        raise ValueError(f"{who}: no row, so no extent")
    x0, x1, z0, z1 = (float(v) for v in stats[3:7])
    if not (x1 > x0 and z1 > z0):
        raise ValueError(f"{who}: the rows have a zero extent")
    return x0, x1, z0, z1


# The sampling window of a PSFDetector's read-out as a function of its rows ([H, 9], include/bmo.h det_data) and its pose, so that a sweep
# (SweepSolution.psf_intensity) can apply it to each configuration's rows and pose.  PSFDetector's methods of the same names call these.
def psf_local_pos(rows, position, orientation):  # PSFDetector.jl:91-101
    loc = rows[:, 0:3] - np.asarray(position)[None, :]
    o = np.asarray(orientation)
    return np.stack([loc @ o[:, 0], loc @ o[:, 2]], axis=1)


def psf_local_lims(rows, position, orientation, crop_factor=1.0, center="centroid"):  # PSFDetector.jl:116-144
    hits = psf_local_pos(rows, position, orientation)
    xs, zs = hits[:, 0], hits[:, 1]
    if center == "centroid":
        w = rows[:, 7]
        w_sum = w.sum()
        x0, z0 = (w * xs).sum() / w_sum, (w * zs).sum() / w_sum
    else:
        x0, z0 = (xs.min() + xs.max()) / 2, (zs.min() + zs.max()) / 2
    hwx, hwy = np.abs(xs - x0).max() * crop_factor, np.abs(zs - z0).max() * crop_factor
    return x0 - hwx, x0 + hwx, z0 - hwy, z0 + hwy


def psf_sample_axes(rows, position, orientation, n=100, crop_factor=1.0, center="centroid", x_min=math.inf, x_max=math.inf, z_min=math.inf,
                    z_max=math.inf, x0_shift=0.0, z0_shift=0.0):
    """The (xs, zs) sample coordinates of intensity(psf; ...) PSFDetector.jl:205-217 for hit rows `rows` at the detector pose
    (position, orientation)."""
    _x_min, _x_max, _z_min, _z_max = psf_local_lims(rows, position, orientation, crop_factor=crop_factor, center=center)
    if x_min != math.inf and x_max != math.inf:
        _x_min, _x_max = x_min, x_max
    if z_min != math.inf and z_max != math.inf:
        _z_min, _z_max = z_min, z_max
    return la.linrange(_x_min, _x_max, n) + x0_shift, la.linrange(_z_min, _z_max, n) + z0_shift


def psf_axes_from_stats(stats, n=100, crop_factor=1.0, center="centroid", x_min=math.inf, x_max=math.inf, z_min=math.inf, z_max=math.inf,
                        x0_shift=0.0, z0_shift=0.0):
    """The rule of psf_sample_axes applied to wavefront statistics (abi.PSF_* columns, bmo_psf_stats) instead of rows: (xs, zs) of [n] for
    one row of statistics, of [K, n] for [K, 21].  "centroid": CX -+ HWX * crop_factor; otherwise the centre of the bounding box,
    (X_MIN + X_MAX) / 2, and the half-width about it from the extrema (the largest |x - centre| is attained at X_MIN or X_MAX)."""
    from . import abi

    st = np.asarray(stats, dtype=np.float64)
    s2 = st.reshape(-1, abi.PSF_STAT_N)
    if center == "centroid":
        x0, z0 = s2[:, abi.PSF_CX], s2[:, abi.PSF_CZ]
        hx, hz = s2[:, abi.PSF_HWX], s2[:, abi.PSF_HWZ]
    else:
        x0, z0 = (s2[:, abi.PSF_X_MIN] + s2[:, abi.PSF_X_MAX]) / 2, (s2[:, abi.PSF_Z_MIN] + s2[:, abi.PSF_Z_MAX]) / 2
        hx = np.maximum(np.abs(s2[:, abi.PSF_X_MIN] - x0), np.abs(s2[:, abi.PSF_X_MAX] - x0))
        hz = np.maximum(np.abs(s2[:, abi.PSF_Z_MIN] - z0), np.abs(s2[:, abi.PSF_Z_MAX] - z0))
    hwx, hwz = hx * crop_factor, hz * crop_factor
    lims = [x0 - hwx, x0 + hwx, z0 - hwz, z0 + hwz]
    if x_min != math.inf and x_max != math.inf:
        lims[0], lims[1] = np.full(len(s2), float(x_min)), np.full(len(s2), float(x_max))
    if z_min != math.inf and z_max != math.inf:
        lims[2], lims[3] = np.full(len(s2), float(z_min)), np.full(len(s2), float(z_max))
    t = np.arange(int(n), dtype=np.float64) / max(int(n) - 1, 1)  # la.linrange, row by row
    xs = ((1 - t)[None, :] * lims[0][:, None] + t[None, :] * lims[1][:, None]) + x0_shift
    zs = ((1 - t)[None, :] * lims[2][:, None] + t[None, :] * lims[3][:, None]) + z0_shift
    return (xs[0], zs[0]) if st.ndim == 1 else (xs, zs)


def psf_marechal(stats):
    """The extended Marechal estimate exp(-(k W_RMS)^2) of the Strehl ratio from wavefront statistics ([21] or [K, 21]); NaN where the rows
    hold more than one wave number (K_MIN != K_MAX) or no row."""
    from . import abi

    st = np.asarray(stats, dtype=np.float64)
    k, rms = st[..., abi.PSF_K_MIN], st[..., abi.PSF_W_RMS]
    with np.errstate(invalid="ignore"):
        return np.where(k == st[..., abi.PSF_K_MAX], np.exp(-(k * rms) ** 2), np.nan)


def best_focus(offsets, values, kind="min"):
    """(offset, value) of the extremum of a focus curve sampled at `offsets`: the vertex of the parabola through the extremal sample
    (kind "min" or "max"; NaN samples are passed over) and its two neighbours; at an end of the range, the end sample itself."""
    if kind not in ("min", "max"):
        raise ValueError('best_focus: kind must be "min" or "max"')
    x, y = np.asarray(offsets, dtype=np.float64).reshape(-1), np.asarray(values, dtype=np.float64).reshape(-1)
    if len(x) != len(y) or len(x) == 0 or np.isnan(y).all():
        raise ValueError("best_focus: offsets and values must be two arrays of one length with a sample that is not NaN")
    i = int(np.nanargmin(y) if kind == "min" else np.nanargmax(y))
    if i == 0 or i == len(x) - 1 or math.isnan(y[i - 1]) or math.isnan(y[i + 1]):
        return float(x[i]), float(y[i])
    d1, d2 = (y[i] - y[i - 1]) / (x[i] - x[i - 1]), (y[i + 1] - y[i]) / (x[i + 1] - x[i])
    a = (d2 - d1) / (x[i + 1] - x[i - 1])  # Newton's form: y = y0 + d1 (x - x0) + a (x - x0)(x - x1)
    if a == 0:
        return float(x[i]), float(y[i])
    xv = (x[i - 1] + x[i]) / 2 - d1 / (2 * a)
    return float(xv), float(y[i - 1] + d1 * (xv - x[i - 1]) + a * (xv - x[i - 1]) * (xv - x[i]))


def psf_through_focus(stats_fn, stack_fn, orientation, offsets, n=100, axis=None, follow="centroid", window_plane=None, crop_factor=1.0, half_width=None):
    """The through-focus stack of PSF rows read through stats_fn(axis, offsets) -> focus statistics [M, 12] and stack_fn(displacements, xs, zs)
    -> I[M, n, n]: what PSFDetector.through_focus and EngineSolution.psf_through_focus share.  Plane m is the detector plane moved by
    offsets[m] along `axis` (None: the detector's local y).  The window is common to the stack: the half-widths of plane `window_plane`
    (None: the plane of least RMS radius) times crop_factor, or `half_width` (one number, or (hwx, hwz)) where it is given, xs and zs running
    over -hw .. +hw about each plane's centre.  The centre of plane m is its own centroid (follow="centroid": the grid follows the chief
    ray) or the centroid of the window plane (follow=None).
    Returns (xs, zs, displacements [M, 3], I[M, n, n], stats): the point (i, j) of plane m lies at origin + xs[i] e1 + zs[j] e2 + d_m."""
    ax, off = focus_planes(orientation, offsets, axis, follow, "through_focus")
    st = stats_fn(ax, off)
    xs, zs, d = through_focus_plan(st, orientation, ax, off, n=n, follow=follow, window_plane=window_plane, crop_factor=crop_factor, half_width=half_width)
    return xs, zs, d, stack_fn(d, xs, zs), st


def focus_planes(orientation, offsets, axis, follow, who):
    """(axis [3], offsets [M]) of a stack of planes as the focus statistics take them (axis None: the detector's local y), after the
    checks the through-focus read-outs share.  The single path and the sweep path (one call per configuration) both plan through here."""
    if follow not in ("centroid", None):
        raise ValueError('%s: follow must be "centroid" or None' % who)
    o = np.asarray(orientation, dtype=np.float64)
    ax = o[:, 1] if axis is None else np.asarray(axis, dtype=np.float64).reshape(3)
    off = np.asarray(offsets, dtype=np.float64).reshape(-1)
    if len(off) == 0:
        raise ValueError("%s: no offsets" % who)
    return ax, off


def through_focus_plan(stats, orientation, axis, offsets, n=100, follow="centroid", window_plane=None, crop_factor=1.0, half_width=None):
    """What psf_through_focus hands its stack_fn, from the focus statistics [M, 12] of the planes (axis, offsets) of focus_planes:
    (xs [n], zs [n], displacements [M, 3]).  ValueError for statistics without rows or without a plane that has any."""
    from . import abi

    st, ax, off = np.asarray(stats, dtype=np.float64), np.asarray(axis, dtype=np.float64), np.asarray(offsets, dtype=np.float64)
    o = np.asarray(orientation, dtype=np.float64)
    e1, e2 = o[:, 0], o[:, 2]
    if st[0, abi.FOCUS_N] == 0:
        raise ValueError("through_focus: the PSFDetector recorded no hit")
    if np.isnan(st[:, abi.FOCUS_RMS_R]).all():
        raise ValueError("through_focus: no plane has statistics (a row runs parallel to the detector plane)")
    w = int(np.nanargmin(st[:, abi.FOCUS_RMS_R])) if window_plane is None else int(window_plane)
    hwx, hwz = st[w, abi.FOCUS_HWX] * crop_factor, st[w, abi.FOCUS_HWZ] * crop_factor
    if half_width is not None:
        hwx, hwz = (float(v) for v in np.broadcast_to(np.asarray(half_width, dtype=np.float64), (2,)))
    xs, zs = la.linrange(-hwx, hwx, n), la.linrange(-hwz, hwz, n)
    centre = st[:, [abi.FOCUS_CX, abi.FOCUS_CZ]] if follow == "centroid" else np.tile(st[w, [abi.FOCUS_CX, abi.FOCUS_CZ]], (len(off), 1))
    d = off[:, None] * ax[None, :] + centre[:, 0:1] * e1[None, :] + centre[:, 1:2] * e2[None, :]
    return xs, zs, d


# The MTF read-out (include/bmo.h "MTF read-out").  Frequencies are (fx, fz) in cycles per metre in the detector's local frame.
def mtf_frequencies(f_max, n, azimuth_deg=0.0):
    """[n, 2]: n frequencies from 0 to f_max along the direction at `azimuth_deg` from the local x axis (0: tangential x, 90: z)."""
    a = math.radians(float(azimuth_deg))
    f = float(f_max) * np.arange(int(n), dtype=np.float64) / max(int(n) - 1, 1)
    return np.stack([f * math.cos(a), f * math.sin(a)], axis=1)


def mtf_cutoff(k_max, rho):
    """The incoherent cutoff 2 NA / lambda = rho k / pi in cycles per metre: rho the pupil radius in direction cosines (abi.ZERN_RHO of the
    Zernike info), k the wave number (abi.PSF_K_MAX of the wavefront statistics)."""
    return float(rho) * float(k_max) / math.pi


def mtf_diffraction_limit(s):
    """The MTF of an aberration-free circular pupil at s = |f| / cutoff: 2 / pi (acos s - s sqrt(1 - s^2)), and 0 beyond 1."""
    s = np.abs(np.asarray(s, dtype=np.float64))
    t = np.minimum(s, 1.0)
    return np.where(s < 1.0, 2.0 / math.pi * (np.arccos(t) - t * np.sqrt(1.0 - t * t)), 0.0)


def mtf_window(k_max, rho, n_rows, f_max, airy_radii=10):
    """(half_width, n) of the image grid whose transform is the diffraction MTF up to f_max.  A sum of H plane waves repeats: a disc of H
    directions has the spacing du = rho sqrt(pi / H), so the PSF has replicas at L = 2 pi / (k du), and a window wider than L transforms
    them too.  The half-width is the smaller of `airy_radii` Airy radii (1.22 pi / (k rho) each) and 0.35 L; n makes the pitch
    2 half_width / (n - 1) at most 0.75 of the Nyquist pitch 1 / (2 f_max)."""
    k, rho, H = float(k_max), float(rho), int(n_rows)
    if not (k > 0 and rho > 0 and H > 0 and math.isfinite(k) and math.isfinite(rho)):
        raise ValueError("mtf_window: needs a wave number, a pupil radius and a row count above zero (give half_width and n instead)")
    replica = 2 * math.pi / (k * rho * math.sqrt(math.pi / H))
    hw = min(float(airy_radii) * 1.22 * math.pi / (k * rho), 0.35 * replica)
    return hw, mtf_grid_points(hw, f_max)


def mtf_grid_points(half_width, f_max):
    """The least n at which the pitch 2 half_width / (n - 1) is at most 0.75 / (2 f_max); at least 2."""
    hw = float(np.max(half_width))
    if not float(f_max) > 0:
        return 2
    return max(2, int(math.ceil(2 * hw / (0.75 / (2 * float(f_max))) * (1 - 1e-12))) + 1)


def mtf_check_pitch(xs, zs, freqs):
    """Raises ValueError where the grid (xs, zs) samples too coarsely for `freqs`: a pitch above 1 / (2 max |f|) along its axis aliases."""
    fq = np.abs(np.asarray(freqs, dtype=np.float64).reshape(-1, 2))
    for name, ax, f in (("x", xs, fq[:, 0].max()), ("z", zs, fq[:, 1].max())):
        if len(ax) > 1 and f > 0:
            pitch = float(np.max(np.abs(np.diff(ax))))
            if pitch > 1 / (2 * f):
                raise ValueError("mtf: the %s pitch %.3e m exceeds 1 / (2 max |f%s|) = %.3e m: the image would alias (raise n or shrink the window)"
                                 % (name, pitch, name, 1 / (2 * f)))


def mtf_geo_centers(stats, follow):
    """[M, 2]: the point of each plane the geometric MTF counts its phase from, from the planes' focus statistics [M, 12]: each plane's
    centroid (follow="centroid"), or the centroid of the plane of least RMS radius for all (follow=None)."""
    from . import abi

    st = np.asarray(stats, dtype=np.float64)
    centers = st[:, [abi.FOCUS_CX, abi.FOCUS_CZ]]
    if follow is None and not np.isnan(st[:, abi.FOCUS_RMS_R]).all():
        centers = np.tile(centers[int(np.nanargmin(st[:, abi.FOCUS_RMS_R]))], (len(st), 1))
    return np.ascontiguousarray(centers)


def mtf_image_grid(window, freqs, n=None, half_width=None):
    """(half_width, n) of the image grid of the diffraction MTF at `freqs`: half_width None takes mtf_window's for window = (k_max, rho,
    n_rows), n None the least n that the pitch rule allows for the half-width."""
    f_max = float(np.abs(np.asarray(freqs, dtype=np.float64)).max())
    if half_width is None:
        half_width, n_rule = mtf_window(*window, f_max)
    else:
        n_rule = mtf_grid_points(half_width, f_max)
    return half_width, (n_rule if n is None else int(n))


def psf_mtf(stats_fn, geo_fn, otf_fn, window_fn, orientation, freqs, offsets=(0.0,), kind="diffraction", n=None, half_width=None, axis=None,
            follow="centroid"):
    """The MTF of PSF rows on the detector plane moved by each of `offsets` along `axis` (None: local y), at `freqs` [nf, 2] in cycles per
    metre: what PSFDetector.mtf and EngineSolution.psf_mtf share.  stats_fn(axis, offsets) -> focus statistics [M, 12];
    geo_fn(axis, offsets, freqs, centers) and otf_fn(displacements, xs, zs, freqs) -> (mtf, otf, sums); window_fn() -> (k_max, rho, n_rows).
    kind "geometric": the transform of the propagated rows, the phase counted from each plane's centroid (follow="centroid") or from the
    centroid of the plane of least RMS radius (follow=None).  kind "diffraction": the transform of the through-focus stack on the grid of
    psf_through_focus with the same `follow`; half_width None takes mtf_window's, n None the least n that mtf_window's pitch rule allows.
    Returns (mtf [M, nf], otf [M, nf] complex, sums [M], stats [M, 12])."""
    if kind not in ("diffraction", "geometric"):
        raise ValueError('mtf: kind must be "diffraction" or "geometric"')
    if follow not in ("centroid", None):
        raise ValueError('mtf: follow must be "centroid" or None')
    fq = np.asarray(freqs, dtype=np.float64).reshape(-1, 2)
    if len(fq) == 0 or not np.isfinite(fq).all():
        raise ValueError("mtf: needs at least one frequency, all finite")
    if kind == "geometric":
        ax, off = focus_planes(orientation, offsets, axis, follow, "mtf")
        st = stats_fn(ax, off)
        mtf, otf, sums = geo_fn(ax, off, fq, mtf_geo_centers(st, follow))
        return mtf, otf, sums, st
    half_width, n = mtf_image_grid(window_fn() if half_width is None else None, fq, n=n, half_width=half_width)
    out = {}

    def stack_fn(d, xs, zs):
        mtf_check_pitch(xs, zs, fq)
        out["r"] = otf_fn(d, xs, zs, fq)

    _, _, _, _, st = psf_through_focus(stats_fn, stack_fn, orientation, offsets, n=n, axis=axis, follow=follow, half_width=half_width)
    return out["r"] + (st,)


# The polychromatic read-out (include/bmo.h "Polychromatic read-out"): a slot's rows split by wave number (abi.PsfBands), every band read by
# the single-call read-outs through its device pointer, and the incoherent sum of the bands' images.
def poly_coefficients(weights, S, normalize="energy"):
    """The coefficients c_b of the incoherent sum of the bands' PSFs from the spectral weights w_b (None: all 1) and the bands' sums of proj
    S_b (abi.FOCUS_S of each band's focus statistics).  normalize "energy": c_b = w_b / (S_b * S_b), which scales every band's PSF to the peak
    of its own in-phase sum before the weights apply (a band without rows, S_b zero or NaN, gets 0); None: c_b = w_b."""
    S = np.asarray(S, dtype=np.float64).reshape(-1)
    w = np.ones(len(S)) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
    if len(w) != len(S):
        raise ValueError("poly_coefficients: %d weights for %d bands" % (len(w), len(S)))
    if not np.isfinite(w).all():
        raise ValueError("poly_coefficients: every weight must be finite")
    if normalize is None:
        return w.copy()
    if normalize != "energy":
        raise ValueError('poly_coefficients: normalize must be "energy" or None')
    c = np.zeros(len(S))
    ok = np.isfinite(S) & (S != 0)
    c[ok] = w[ok] / (S[ok] * S[ok])
    return c


def poly_combine(coeffs, images):
    """((c_0 I_0 + c_1 I_1) + c_2 I_2) + ...: the combination rule of bmo_psf_poly_through_focus, a multiply and an add per band in band
    order, restated in numpy (equal to the device's bit for bit).  images: [B, ...]; no band: ValueError."""
    c, I = np.asarray(coeffs, dtype=np.float64).reshape(-1), np.asarray(images, dtype=np.float64)
    if len(c) != len(I) or len(c) == 0:
        raise ValueError("poly_combine: needs one coefficient per image and at least one band")
    acc = c[0] * I[0]
    for b in range(1, len(c)):
        acc = acc + c[b] * I[b]
    return acc


def psf_chromatic_focus(stats_fn_per_band, ks, offsets, axis, plane=None):
    """Where each colour focuses and where it lands, from the focus statistics of every band: stats_fn_per_band(b, axis, offsets) -> [M, 12]
    (abi.FOCUS_* columns) of band b's rows on the detector plane moved by each of `offsets` along `axis`.  Returns
    (stats [B, M, 12], focus [B], rms [B], centroids [B, 2], plane):
      focus, rms : best_focus of each band's RMS_R curve, the offset of its least spot and the radius there: the spread of `focus` over the
                   bands is the longitudinal colour;
      centroids  : (CX, CZ) of each band on one common plane, `plane` (an index into offsets; None: the sample nearest the mean of the bands'
                   foci): their spread is the lateral colour.
    A band without rows (or with a row parallel to the planes) has NaN in its entries."""
    from . import abi

    off = np.asarray(offsets, dtype=np.float64).reshape(-1)
    B = len(np.asarray(ks).reshape(-1))
    if len(off) == 0:
        raise ValueError("chromatic_focus: no offsets")
    st = np.full((B, len(off), abi.FOCUS_STAT_N), np.nan)
    focus, rms = np.full(B, np.nan), np.full(B, np.nan)
    for b in range(B):
        st[b] = np.asarray(stats_fn_per_band(b, axis, off), dtype=np.float64).reshape(len(off), abi.FOCUS_STAT_N)
        if not np.isnan(st[b, :, abi.FOCUS_RMS_R]).all():
            focus[b], rms[b] = best_focus(off, st[b, :, abi.FOCUS_RMS_R])
    if plane is None:
        plane = 0 if np.isnan(focus).all() else int(np.argmin(np.abs(off - np.nanmean(focus))))
    plane = int(plane)
    if not 0 <= plane < len(off):
        raise ValueError("chromatic_focus: plane must be an index into offsets")
    return st, focus, rms, st[:, plane, [abi.FOCUS_CX, abi.FOCUS_CZ]].copy(), plane


def _band_rows(bands, b):
    """The keyword arguments that hand band b of an abi.PsfBands to a single-call read-out."""
    ptr, cnt = bands.rows(b)
    return dict(device=bands.device, hits_device_ptr=ptr, n_hits=cnt)


def chromatic_focus_of(bands, position, orientation, offsets, axis=None, plane=None):
    """psf_chromatic_focus of the bands of an abi.PsfBands at the pose (position, orientation), every band read by bmo_psf_focus_stats through
    its device pointer.  Returns (psf_chromatic_focus's tuple, kernel ms)."""
    from . import abi

    o = np.asarray(orientation, dtype=np.float64)
    ax = o[:, 1] if axis is None else np.asarray(axis, dtype=np.float64).reshape(3)
    ms = []

    def per_band(b, a, off):
        st, t = abi.psf_focus_stats(None, position, o[:, 0], o[:, 2], a, off, **_band_rows(bands, b))
        ms.append(t)
        return st

    return psf_chromatic_focus(per_band, bands.ks, offsets, ax, plane=plane), float(sum(ms))


def _band_sums(bands, position, o):
    """S_b, the sum of proj of every band (abi.FOCUS_S of its focus statistics at offset 0; it does not depend on the plane), and the ms."""
    from . import abi

    out = [abi.psf_focus_stats(None, position, o[:, 0], o[:, 2], o[:, 1], [0.0], **_band_rows(bands, b)) for b in range(len(bands))]
    return np.array([st[0, abi.FOCUS_S] for st, _ in out]), float(sum(t for _, t in out))


def poly_through_focus_of(all_rows, bands, position, orientation, offsets, weights=None, n=100, normalize="energy", axis=None, follow="centroid",
                          window_plane=None, crop_factor=1.0, half_width=None, want_bands=False):
    """The polychromatic through-focus stack of an abi.PsfBands.  The window and the centres are psf_through_focus's from the focus statistics of
    ALL rows (`all_rows`: the keyword arguments that hand them to abi.psf_focus_stats): they are geometric and shared by the bands, because
    intensities add only at the same physical point.  Returns ((xs, zs, displacements, I[M, n, n], stats, coeffs, I_b or None), kernel ms)."""
    from . import abi

    o = np.asarray(orientation, dtype=np.float64)
    if len(bands) == 0:
        raise ValueError("poly_through_focus: no wavelength band (the PSFDetector recorded no hit)")
    S, ms = _band_sums(bands, position, o)
    coeffs = poly_coefficients(weights, S, normalize)
    hits, kw = all_rows.get("hits"), {k: v for k, v in all_rows.items() if k != "hits"}
    t, keep = [ms], {}

    def stats_fn(ax, off):
        st, ms_ = abi.psf_focus_stats(hits, position, o[:, 0], o[:, 2], ax, off, **kw)
        t.append(ms_)
        return st

    def stack_fn(d, xs, zs):
        I, keep["bands"], ms_ = abi.psf_poly_through_focus(bands, position, o[:, 0], o[:, 2], d, xs, zs, coeffs, want_bands=want_bands)
        t.append(ms_)
        return I

    xs, zs, d, I, st = psf_through_focus(stats_fn, stack_fn, o, offsets, n=n, axis=axis, follow=follow, window_plane=window_plane, crop_factor=crop_factor,
                                         half_width=half_width)
    return (xs, zs, d, I, st, coeffs, keep.get("bands")), float(sum(t))


def poly_mtf_of(all_rows, bands, position, orientation, freqs, offsets=(0.0,), weights=None, normalize="energy", n=None, half_width=None, axis=None,
                follow="centroid"):
    """The white-light diffraction MTF of an abi.PsfBands: psf_mtf's grid with bmo_psf_poly_otf as the transform.  half_width None takes
    mtf_window's at the SMALLEST wave number of the rows (the longest wavelength has the widest PSF and the nearest replicas); the cutoff of
    the sum is that of the largest, mtf_cutoff(bands.ks.max(), rho), and the pitch follows the largest |f| asked for as in psf_mtf.
    Returns ((mtf [M, nf], otf [M, nf] complex, sums [M], stats [M, 12], coeffs), kernel ms)."""
    from . import abi

    o = np.asarray(orientation, dtype=np.float64)
    e1, e2 = o[:, 0], o[:, 2]
    if len(bands) == 0:
        raise ValueError("poly_mtf: no wavelength band (the PSFDetector recorded no hit)")
    S, ms = _band_sums(bands, position, o)
    coeffs = poly_coefficients(weights, S, normalize)
    hits, kw = all_rows.get("hits"), {k: v for k, v in all_rows.items() if k != "hits"}
    t = [ms]

    def timed(out):
        t.append(out[-1])
        return out

    def window_fn():
        st = timed(abi.psf_stats(hits, position, e1, e2, **kw))[0]
        info = timed(abi.psf_zernike(hits, position, e1, e2, order=0, **kw))[1]
        return st[abi.PSF_K_MIN], info[abi.ZERN_RHO], int(st[abi.PSF_N])

    out = psf_mtf(lambda ax, off: timed(abi.psf_focus_stats(hits, position, e1, e2, ax, off, **kw))[0], None,
                  lambda d, xs, zs, fq: timed(abi.psf_poly_otf(bands, position, e1, e2, d, xs, zs, coeffs, fq))[:3],
                  window_fn, o, freqs, offsets=offsets, kind="diffraction", n=n, half_width=half_width, axis=axis, follow=follow)
    return out + (coeffs,), float(sum(t))


# The encircled-energy read-out (include/bmo.h "Encircled-energy read-out").  Radii are half-sizes in metres in the detector's local frame.
def ee_radii(r_max, n):
    """[n]: n radii from 0 to r_max in equal steps (the first is 0: only the points at the centre itself)."""
    return float(r_max) * np.arange(int(n), dtype=np.float64) / max(int(n) - 1, 1)


def ee_radius_at(radii, ee, fraction):
    """The radius at which an energy curve first reaches `fraction`: `radii` ascending, `ee` [n] the curve on them ([..., n]: one answer per
    curve); linear interpolation between the last sample below and the first at or above, the first radius if the curve starts there, NaN
    if the curve never reaches it (or is NaN)."""
    r = np.asarray(radii, dtype=np.float64).reshape(-1)
    e = np.asarray(ee, dtype=np.float64)
    if e.shape[-1] != len(r) or len(r) == 0 or np.any(np.diff(r) < 0):
        raise ValueError("ee_radius_at: radii must be ascending and ee must hold one value per radius")
    f = float(fraction)
    out = np.full(e.shape[:-1], np.nan)
    for idx in np.ndindex(*e.shape[:-1]):
        curve = e[idx]
        hit = np.nonzero(curve >= f)[0]
        if len(hit) == 0:
            continue
        q = int(hit[0])
        if q == 0 or curve[q] == curve[q - 1] or not np.isfinite(curve[q - 1]):
            out[idx] = r[q]
        else:
            out[idx] = r[q - 1] + (f - curve[q - 1]) / (curve[q] - curve[q - 1]) * (r[q] - r[q - 1])
    return float(out) if out.ndim == 0 else out


def _bessel_j01(v):
    """(J0(v), J1(v)) from Bessel's integral J_n(v) = 1 / (2 pi) int_0^2pi cos(n t - v sin t) dt by the trapezoid rule on N points: the
    integrand is periodic and entire, so the rule's error is the aliased orders J_(n + m N)(v), below 1e-20 with N >= |v| + 48."""
    v = np.asarray(v, dtype=np.float64)
    N = max(64, int(math.ceil(float(np.max(np.abs(v), initial=0.0)))) + 48)
    t = 2.0 * math.pi * np.arange(N, dtype=np.float64) / N
    arg = v[..., None] * np.sin(t)
    return np.cos(arg).mean(axis=-1), np.cos(t - arg).mean(axis=-1)


def ee_diffraction_limit(v):
    """The encircled energy of an aberration-free circular pupil (the Airy pattern) inside the radius r: 1 - J0(v)^2 - J1(v)^2 at
    v = k_max rho r, with the k_max and rho of mtf_cutoff (v = pi r cutoff)."""
    j0, j1 = _bessel_j01(v)
    return np.clip(1.0 - j0 * j0 - j1 * j1, 0.0, 1.0)  # a share: the rounding at v = 0 must not leave -1e-33


def psf_encircled_energy(stats_fn, geo_fn, ee_fn, window_fn, orientation, radii, offsets=(0.0,), kind="geometric", shape="circle", n=None, half_width=None,
                         axis=None, follow="centroid"):
    """The encircled (shape "circle") or ensquared ("square") energy of PSF rows on the detector plane moved by each of `offsets` along `axis`
    (None: local y), inside every half-size of `radii`: what PSFDetector.encircled_energy and EngineSolution.psf_encircled_energy share.
    stats_fn(axis, offsets) -> focus statistics [M, 12]; geo_fn(axis, offsets, radii, centers, shape) -> (ee, energy, sums);
    ee_fn(displacements, xs, zs, radii, shape) -> (ee, energy, sums, centers of the grid's coordinates); window_fn() -> (k_max, rho, n_rows).
    kind "geometric": the proj-weighted share of the propagated rows about each plane's centroid (follow="centroid") or about the centroid
    of the plane of least RMS radius (follow=None).  kind "diffraction": the share of the pixel sums of the through-focus stack on the grid
    of psf_through_focus with the same `follow`, about each image's intensity centroid; half_width None takes mtf_window's at the cutoff
    frequency (the band limit of the intensity), n None the least n that mtf_window's pitch rule allows there.  The curve is normalised by
    the energy inside the window, so a radius whose circle or square leaves the window is refused (ValueError).
    Returns (ee [M, nr], energy [M, nr], sums [M], centers [M, 2] in the plane's local coordinates, stats [M, 12])."""
    from . import abi

    if kind not in ("diffraction", "geometric"):
        raise ValueError('encircled_energy: kind must be "diffraction" or "geometric"')
    if shape not in abi.EE_SHAPES:
        raise ValueError('encircled_energy: shape must be "circle" or "square"')
    if follow not in ("centroid", None):
        raise ValueError('encircled_energy: follow must be "centroid" or None')
    r = np.asarray(radii, dtype=np.float64).reshape(-1)
    if len(r) == 0 or not np.isfinite(r).all() or (r < 0).any():
        raise ValueError("encircled_energy: needs at least one radius, all finite and not negative")
    off = np.asarray(offsets, dtype=np.float64).reshape(-1)
    if len(off) == 0:
        raise ValueError("encircled_energy: no offsets")
    if kind == "geometric":
        o = np.asarray(orientation, dtype=np.float64)
        ax = o[:, 1] if axis is None else np.asarray(axis, dtype=np.float64).reshape(3)
        st = stats_fn(ax, off)
        centers = st[:, [abi.FOCUS_CX, abi.FOCUS_CZ]]
        if follow is None and not np.isnan(st[:, abi.FOCUS_RMS_R]).all():
            centers = np.tile(centers[int(np.nanargmin(st[:, abi.FOCUS_RMS_R]))], (len(off), 1))
        centers = np.ascontiguousarray(centers)
        if st[0, abi.FOCUS_N] == 0 or not np.isfinite(centers).all():
            raise ValueError("encircled_energy: no plane has a centroid (no hit, or a row runs parallel to the detector plane)")
        ee, energy, sums = geo_fn(ax, off, r, centers, shape)
        return ee, energy, sums, centers, st
    if half_width is None or n is None:
        k_max, rho, n_rows = window_fn()
        if half_width is None:
            half_width, n_rule = mtf_window(k_max, rho, n_rows, mtf_cutoff(k_max, rho))
        else:
            n_rule = mtf_grid_points(half_width, mtf_cutoff(k_max, rho))
        n = n_rule if n is None else int(n)
    hw = np.broadcast_to(np.asarray(half_width, dtype=np.float64), (2,))
    if r.max() > hw.min():
        raise ValueError("encircled_energy: the radius %.3e m leaves the sampled window of half-width %.3e m (shrink the radii or give half_width)"
                         % (r.max(), hw.min()))
    out = {}

    def stack_fn(d, xs, zs):
        out["d"], out["r"] = d, ee_fn(d, xs, zs, r, shape)

    _, _, d, _, st = psf_through_focus(stats_fn, stack_fn, orientation, off, n=int(n), axis=axis, follow=follow, half_width=half_width)
    ee, energy, sums, cen = out["r"]
    reach = np.abs(cen) + r.max()
    if np.any(reach > hw[None, :]):  # a NaN centre (an image without energy) compares false
        m = int(np.argmax(np.any(reach > hw[None, :], axis=1)))
        raise ValueError("encircled_energy: about the centroid of plane %d the radius %.3e m leaves the sampled window of half-width %.3e m" % (m, r.max(), hw.min()))
    grid = st[:, [abi.FOCUS_CX, abi.FOCUS_CZ]]
    if follow is None:
        grid = np.tile(grid[int(np.nanargmin(st[:, abi.FOCUS_RMS_R]))], (len(off), 1))
    return ee, energy, sums, cen + grid, st


def zernike_terms(order):
    """The (n, m) of the Zernike terms up to radial order `order` in OSA/ANSI order: j = (n (n + 2) + m) / 2."""
    return [(n, m) for n in range(int(order) + 1) for m in range(-n, n + 1, 2)]


def zernike_radial(n, am):
    """[q_0 .. q_K], K = (n - am) / 2: the integer coefficients of R_n^am(rho) / rho^am as a polynomial in t = rho^2."""
    K, f = (n - am) // 2, math.factorial
    return [(-1) ** (K - s) * (f(n - K + s) // (f(K - s) * f((n + am) // 2 - K + s) * f(s))) for s in range(K + 1)]


def zernike_basis(x, y, order):
    """Z [J, ...] of the terms at the points (x, y) of the unit disc, by the expressions of include/bmo.h "Zernike read-out" in elementwise
    numpy (+, -, * only, one rounding each, left to right): what the engine evaluates, bit for bit.  Orthonormal over the uniform disc."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    t = x * x + y * y
    Cc, Sc = [np.ones_like(x)], [np.zeros_like(x)]
    for k in range(int(order)):
        Cc.append(Cc[k] * x - Sc[k] * y)
        Sc.append(Sc[k] * x + Cc[k] * y)
    out = []
    for n, m in zernike_terms(order):
        q = zernike_radial(n, abs(m))
        r = np.full_like(t, float(q[-1]))
        for s in range(len(q) - 2, -1, -1):
            r = r * t + float(q[s])
        nrm = math.sqrt(float(n + 1)) if m == 0 else math.sqrt(float(2 * (n + 1)))
        out.append(nrm * (r * (Cc[m] if m >= 0 else Sc[-m])))
    return np.array(out)


def zernike_surface(coef, n, order):
    """The fitted surface sum_j coef_j Z_j on an n x n grid of the unit square [-1, 1]^2, indexed [i, j] = (x_i, y_j); NaN outside the disc."""
    t = np.linspace(-1.0, 1.0, int(n))
    x, y = np.meshgrid(t, t, indexing="ij")
    Z = zernike_basis(x, y, order)
    c = np.asarray(coef, dtype=np.float64).reshape(len(Z))
    return np.where(x * x + y * y <= 1.0, np.tensordot(c, Z, axes=1), np.nan)


def opd_remove_terms(remove, order):
    """The (n, m) of the Zernike terms up to `order` that an OPD map removes: "none", "tilt" (n <= 1: piston and tilt), "defocus" (those
    and (2, 0)), "fit" (every term: the residual map), or an iterable of (n, m)."""
    terms = zernike_terms(order)
    if isinstance(remove, str):
        if remove not in ("none", "tilt", "defocus", "fit"):
            raise ValueError('opd_map: remove must be "none", "tilt", "defocus", "fit" or an iterable of (n, m)')
        if remove == "none":
            return []
        if remove == "fit":
            return terms
        return [t for t in terms if t[0] <= 1 or (remove == "defocus" and t == (2, 0))]
    want = [(int(n), int(m)) for n, m in remove]
    missing = [t for t in want if t not in terms]
    if missing:
        raise ValueError("opd_map: no term %s at order %d" % (missing[0], order))
    return [t for t in terms if t in want]


def psf_opd_map(zernike_fn, map_fn, n=64, order=4, remove="tilt", ref=None, pupil=None, coef=None):
    """The binned wavefront (OPD) map shared by PSFDetector.opd_map, EngineSolution.psf_opd_map and SweepSolution.psf_opd_map.
    zernike_fn(order, ref, pupil) -> (coef [.., J], info [.., 13]) is the Zernike read-out, map_fn(order, coef, ref, pupil) ->
    (opd, weight, count, info) the map read-out (both of one configuration, or of every configuration of a sweep with a leading axis).
    With `remove` other than "none" (and no `coef` given) the wavefront is fitted at `order`, the coefficients of the terms to keep are
    zeroed, and the map is read about that fit's reference point (X_REF, Z_REF) and pupil (U0, V0, RHO) with the rest removed; a given
    `coef` is removed as it stands.  Returns (opd [.., n, n] indexed [i, j] in metres, NaN in bins without rows; weight; count; info [.., 20]
    at the abi.OPD_* columns; coef_removed [.., J])."""
    from . import abi

    if coef is not None:
        cf = np.asarray(coef, dtype=np.float64)
        return (*map_fn(order, cf, ref, pupil), cf)
    removed = opd_remove_terms(remove, order)
    if not removed:
        out = map_fn(0, None, ref, pupil)
        return (*out, np.zeros(np.shape(out[3])[:-1] + (1,)))
    cf, zi = zernike_fn(order, ref, pupil)
    keep = [j for j, t in enumerate(zernike_terms(order)) if t not in removed]
    cf = np.array(cf, dtype=np.float64)
    cf[..., keep] = 0.0
    cf = np.where(np.isfinite(cf), cf, 0.0)  # a fit that was not solved removes nothing
    r, q = zi[..., [abi.ZERN_X_REF, abi.ZERN_Z_REF]], zi[..., [abi.ZERN_U0, abi.ZERN_V0, abi.ZERN_RHO]]
    usable = np.isfinite(r).all(axis=-1) & np.isfinite(q).all(axis=-1) & (q[..., 2] > 0)
    if zi.ndim == 1:
        if not usable:  # no rows, or a single direction: the map computes (and reports) what the fit did
            r, q = ref, pupil
    elif not usable.all():  # a batched call takes a pupil for every configuration: those without one are read on the unit pupil
        r, q = np.where(usable[:, None], r, 0.0), np.where(usable[:, None], q, np.array([0.0, 0.0, 1.0]))
    return (*map_fn(order, cf, r, q), cf)


def opd_axes(info, n):
    """(us, vs): the centres of the n bins per axis of an OPD map in direction cosines, from its info row: U0 + RHO x_i with
    x_i = -1 + (2 i + 1) / n."""
    from . import abi

    x = -1.0 + (2.0 * np.arange(int(n)) + 1.0) / int(n)
    return info[abi.OPD_U0] + info[abi.OPD_RHO] * x, info[abi.OPD_V0] + info[abi.OPD_RHO] * x


class PSFDetector(AbstractObject):  # Detectors/PSFDetector.jl:44-68
    kind = O_PSF

    def __init__(self, width):
        shape = sh.QuadraticFlatMesh(width)
        sh.zrotate3d(shape, math.pi)
        super().__init__(shape)
        self.data = np.zeros((0, 9))

    def empty(self):
        self.data = np.zeros((0, 9))

    # ---- read-out (PSFDetector.jl:91-237); the n x n coherent sum runs on the GPU engine (bmo_psf_intensity)
    def calc_local_pos(self):  # PSFDetector.jl:91-101
        return psf_local_pos(self.data, self.position(), self.orientation())

    def calc_local_lims(self, crop_factor=1.0, center="centroid"):  # PSFDetector.jl:116-144
        return psf_local_lims(self.data, self.position(), self.orientation(), crop_factor=crop_factor, center=center)

    def sample_axes(self, n=100, crop_factor=1.0, center="centroid", x_min=math.inf, x_max=math.inf, z_min=math.inf, z_max=math.inf,
                    x0_shift=0.0, z0_shift=0.0):
        """The (xs, zs) sample coordinates of intensity(psf; ...) PSFDetector.jl:205-217."""
        return psf_sample_axes(self.data, self.position(), self.orientation(), n=n, crop_factor=crop_factor, center=center, x_min=x_min,
                               x_max=x_max, z_min=z_min, z_max=z_max, x0_shift=x0_shift, z0_shift=z0_shift)

    def stats(self, ref=None, device=0):
        """The 21 wavefront statistics (abi.PSF_* columns: window, RMS wavefront error, peak-to-valley, Strehl ratio) of all rows accumulated so
        far at the detector's pose, about the reference point ref = (x, z) in local coordinates (None: the centroid)."""
        from . import abi

        o = self.orientation()
        return abi.psf_stats(self.data, self.position(), o[:, 0], o[:, 2], ref=ref, device=device)[0]

    def zernike(self, order=4, ref=None, pupil=None, device=0):
        """The Zernike fit of the wavefront of all rows accumulated so far (bmo_psf_zernike): (coef [J] in metres, OSA/ANSI order as
        zernike_terms(order); info [13] at the abi.ZERN_* columns).  ref = (x, z): the reference point in local coordinates (None: the
        centroid); pupil = (U0, V0, RHO) in direction cosines (None: the rows' own centre and largest radius)."""
        from . import abi

        o = self.orientation()
        coef, info, _, _ = abi.psf_zernike(self.data, self.position(), o[:, 0], o[:, 2], order=order, ref=ref, pupil=pupil, device=device)
        return coef, info

    def opd_map(self, n=64, order=4, remove="tilt", ref=None, pupil=None, device=0):
        """The binned wavefront (OPD) map of all rows accumulated so far (bmo_psf_opd_map): (opd [n, n] indexed [i, j] in metres, weight,
        count, info [20] at the abi.OPD_* columns, coef_removed [J]) as psf_opd_map describes them; opd_axes(info, n) gives the bin centres.
        remove: "none", "tilt", "defocus", "fit" or an iterable of (n, m), the terms of a fit at `order` taken out of the map."""
        from . import abi

        o, pos = self.orientation(), self.position()
        return psf_opd_map(lambda od, r, q: abi.psf_zernike(self.data, pos, o[:, 0], o[:, 2], order=od, ref=r, pupil=q, device=device)[:2],
                           lambda od, cf, r, q: abi.psf_opd_map(self.data, pos, o[:, 0], o[:, 2], n=n, order=od, coef=cf, ref=r, pupil=q, device=device)[:4],
                           n=n, order=order, remove=remove, ref=ref, pupil=pupil)

    def focus_stats(self, offsets, axis=None, device=0):
        """The twelve spot statistics (abi.FOCUS_* columns) of all rows accumulated so far, propagated along their directions to the detector
        plane moved by each of `offsets` along `axis` (None: the detector's local y): [M, 12] (bmo_psf_focus_stats)."""
        from . import abi

        o = self.orientation()
        return abi.psf_focus_stats(self.data, self.position(), o[:, 0], o[:, 2], o[:, 1] if axis is None else axis, offsets, device=device)[0]

    def through_focus(self, offsets, n=100, axis=None, follow="centroid", window_plane=None, crop_factor=1.0, device=0):
        """The PSF of all rows accumulated so far on the detector plane moved by each of `offsets` along `axis`, in one pass over the rows
        (bmo_psf_through_focus; no re-trace): (xs, zs, displacements, I[M, n, n], stats) as psf_through_focus describes them."""
        from . import abi

        o, pos = self.orientation(), self.position()
        return psf_through_focus(lambda ax, off: abi.psf_focus_stats(self.data, pos, o[:, 0], o[:, 2], ax, off, device=device)[0],
                                 lambda d, xs, zs: abi.psf_through_focus(self.data, pos, o[:, 0], o[:, 2], d, xs, zs, device=device)[0],
                                 o, offsets, n=n, axis=axis, follow=follow, window_plane=window_plane, crop_factor=crop_factor)

    def mtf(self, freqs, offsets=(0.0,), kind="diffraction", n=None, half_width=None, axis=None, follow="centroid", device=0):
        """The MTF of all rows accumulated so far at `freqs` [nf, 2] (cycles per metre, local x and z; mtf_frequencies makes a radial cut) on
        the detector plane moved by each of `offsets` along `axis`: (mtf [M, nf], otf [M, nf] complex, sums [M], stats [M, 12]) as psf_mtf
        describes them.  kind "diffraction": bmo_psf_otf, the transform of the through-focus stack; "geometric": bmo_psf_geo_otf."""
        from . import abi

        o, pos = self.orientation(), self.position()
        e1, e2 = o[:, 0], o[:, 2]

        def window_fn():
            st = abi.psf_stats(self.data, pos, e1, e2, device=device)[0]
            info = abi.psf_zernike(self.data, pos, e1, e2, order=0, device=device)[1]
            return st[abi.PSF_K_MAX], info[abi.ZERN_RHO], int(st[abi.PSF_N])

        return psf_mtf(lambda ax, off: abi.psf_focus_stats(self.data, pos, e1, e2, ax, off, device=device)[0],
                       lambda ax, off, fq, cen: abi.psf_geo_otf(self.data, pos, e1, e2, ax, off, fq, centers=cen, device=device)[:3],
                       lambda d, xs, zs, fq: abi.psf_otf(self.data, pos, e1, e2, d, xs, zs, fq, device=device)[:3],
                       window_fn, o, freqs, offsets=offsets, kind=kind, n=n, half_width=half_width, axis=axis, follow=follow)

    def encircled_energy(self, radii, offsets=(0.0,), kind="geometric", shape="circle", n=None, half_width=None, axis=None, follow="centroid", device=0):
        """The encircled (shape "circle") or ensquared ("square") energy of all rows accumulated so far inside every half-size of `radii`
        (metres; ee_radii makes an even list) on the detector plane moved by each of `offsets` along `axis`: (ee [M, nr], energy [M, nr],
        sums [M], centers [M, 2], stats [M, 12]) as psf_encircled_energy describes them.  kind "geometric": bmo_psf_geo_ee, the proj-weighted
        share of the propagated rows; "diffraction": bmo_psf_ee, the share of the pixel sums of the through-focus stack."""
        from . import abi

        o, pos = self.orientation(), self.position()
        e1, e2 = o[:, 0], o[:, 2]

        def window_fn():
            st = abi.psf_stats(self.data, pos, e1, e2, device=device)[0]
            info = abi.psf_zernike(self.data, pos, e1, e2, order=0, device=device)[1]
            return st[abi.PSF_K_MAX], info[abi.ZERN_RHO], int(st[abi.PSF_N])

        def geo_fn(ax, off, r, cen, sh_):
            ee, energy, _, sums, _ = abi.psf_geo_ee(self.data, pos, e1, e2, ax, off, r, centers=cen, shape=sh_, device=device, want_count=False)
            return ee, energy, sums

        return psf_encircled_energy(lambda ax, off: abi.psf_focus_stats(self.data, pos, e1, e2, ax, off, device=device)[0], geo_fn,
                                    lambda d, xs, zs, r, sh_: abi.psf_ee(self.data, pos, e1, e2, d, xs, zs, r, shape=sh_, device=device)[:4],
                                    window_fn, o, radii, offsets=offsets, kind=kind, shape=shape, n=n, half_width=half_width, axis=axis, follow=follow)

    def bands(self, ks=None, device=0):
        """All rows accumulated so far split by wave number on the device (bmo_psf_bands_create): an abi.PsfBands, to be closed by the caller
        (a context manager).  ks None: one band per distinct wave number, ascending; otherwise exactly the bands `ks`."""
        from . import abi

        return abi.psf_bands(self.data, ks=ks, device=device)

    def chromatic_focus(self, offsets, axis=None, ks=None, plane=None, device=0):
        """Where each colour of the rows accumulated so far focuses and lands: (ks [B], stats [B, M, 12], focus [B], rms [B], centroids [B, 2],
        plane) as psf_chromatic_focus describes them (longitudinal colour: the spread of `focus`; lateral colour: that of `centroids`)."""
        with self.bands(ks=ks, device=device) as b:
            out, _ = chromatic_focus_of(b, self.position(), self.orientation(), offsets, axis=axis, plane=plane)
            return (b.ks.copy(),) + out

    def poly_through_focus(self, offsets, weights=None, n=100, normalize="energy", axis=None, follow="centroid", window_plane=None, crop_factor=1.0,
                           half_width=None, ks=None, want_bands=False, device=0):
        """The incoherent, spectrally weighted through-focus stack of the rows accumulated so far (bmo_psf_poly_through_focus): (xs, zs,
        displacements, I[M, n, n], stats, ks, coeffs, I_b or None).  weights: one per band (None: 1); normalize: poly_coefficients's."""
        with self.bands(ks=ks, device=device) as b:
            out, _ = poly_through_focus_of(dict(hits=self.data, device=device), b, self.position(), self.orientation(), offsets, weights=weights, n=n,
                                           normalize=normalize, axis=axis, follow=follow, window_plane=window_plane, crop_factor=crop_factor,
                                           half_width=half_width, want_bands=want_bands)
            return out[:5] + (b.ks.copy(),) + out[5:]

    def poly_mtf(self, freqs, offsets=(0.0,), weights=None, normalize="energy", n=None, half_width=None, axis=None, follow="centroid", ks=None, device=0):
        """The white-light diffraction MTF of the rows accumulated so far (bmo_psf_poly_otf): (mtf [M, nf], otf [M, nf] complex, sums [M],
        stats [M, 12], ks, coeffs) as poly_mtf_of describes them."""
        with self.bands(ks=ks, device=device) as b:
            out, _ = poly_mtf_of(dict(hits=self.data, device=device), b, self.position(), self.orientation(), freqs, offsets=offsets, weights=weights,
                                 normalize=normalize, n=n, half_width=half_width, axis=axis, follow=follow)
            return out[:4] + (b.ks.copy(),) + out[4:]

    def intensity(self, n=100, device=0, _intensity_fn=None, **kw):
        """intensity(psf; n, crop_factor, center, x_min, ...) -> (xs, zs, I) with I[i, j] (PSFDetector.jl:190-237)."""
        from . import abi

        xs, zs = self.sample_axes(n=n, **kw)
        o = self.orientation()
        fn = _intensity_fn or (lambda *a: abi.psf_intensity(*a, device=device)[0])
        return xs, zs, fn(self.data, self.position(), o[:, 0], o[:, 2], xs, zs)


class Photodetector(AbstractObject):  # Detectors/Photodetector.jl:31-55
    """Flat square detector whose complex field `field[i, j]` (local x = pd.x[i], local y = pd.y[j]) is the superposition of all
    GaussianBeamlets that hit it (Photodetector.jl:69-107).  The trace records the hits; solve_system adds their field with the
    engine's bmo_photodetector_field right after the solve, so `field` reads like the reference's after solve_system!."""
    kind = O_PHOTODETECTOR

    def __init__(self, width, n):
        shape = sh.QuadraticFlatMesh(width)
        super().__init__(shape)
        sz = float(np.max(shape.vertices))
        self.x = la.linrange(-sz, sz, n)
        self.y = la.linrange(-sz, sz, n)
        self.field = np.zeros((n, n), dtype=np.complex128)

    def empty(self):  # empty!(pd) Photodetector.jl:119
        self.field[...] = 0

    def resolution(self, n):  # photodetector_resolution! Photodetector.jl:126-131
        self.x = la.linrange(self.x[0], self.x[-1], n)
        self.y = la.linrange(self.y[0], self.y[-1], n)
        self.field = np.zeros((n, n), dtype=np.complex128)

    def intensity(self):  # intensity.(pd.field), OpticUtils.jl:108
        return (self.field.real ** 2 + self.field.imag ** 2) / (2 * la.Z_vacuum)

    def optical_power(self):  # trapz((pd.x, pd.y), intensity(pd)) Photodetector.jl:116 (Trapz.jl: trapezoid rule along x, then y)
        I = self.intensity()
        inner = np.sum((I[1:, :] + I[:-1, :]) * np.diff(self.x)[:, None], axis=0) / 2
        return float(np.sum((inner[1:] + inner[:-1]) * np.diff(self.y)) / 2)


class IntersectableObject(AbstractObject):  # Intersectable.jl:10-15
    kind = O_INTERSECTABLE


class NonInteractableObject(AbstractObject):  # NonInteractable.jl:14-22
    kind = O_NONINTERACTABLE


class PolarizationFilter(AbstractObject):  # Polarizers/PolarizationFilter.jl:6-28
    kind = O_POLARIZER

    def __init__(self, edge_length, cutoff_strength=np.finfo(np.float64).eps, jones=None):
        shape = sh.QuadraticFlatMesh(edge_length)
        sh.zrotate3d(shape, math.pi)
        shape.set_new_origin3d()
        super().__init__(shape)
        # XZBasis(1, 0, 0, 0) PolarizedRays.jl:151: [j11 0 j12; 0 1 0; j21 0 j22]
        self.jones = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 0]], dtype=np.complex128) if jones is None else np.asarray(jones, dtype=np.complex128)
        self.cutoff = float(cutoff_strength)

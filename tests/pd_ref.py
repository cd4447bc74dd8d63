"""Helpers of the Photodetector field tests (not a test file).

1. pd_field_exact: interact3d(::Photodetector, ::GaussianBeamlet, ray_id) (Photodetector.jl:69-107 of the reference) at 50 significant
   digits, for the beamlets a solve recorded on one Photodetector.  Per beamlet and grid point (x_i, y_j), with T = transpose(orientation):

       p1 = T[:, 1] x + T[:, 3] y + p                                              Photodetector.jl:91-96
       l1 = dot(p1 - p0, d0),  p2 = p0 + l1 d0,  r = |p1 - p2|,  z = l0 + l1       :97-101   (p0, d0: the last chief ray,
                                                                                     l0 = length(gauss) - length(ray), :74)
       (point, index) = point_on_beam(gauss.chief, z)                              Beam.jl:177-205: temp = length(parent), plus the length
                                                                                     of every ray but the last until z < temp
       (w, R, psi, w0) = gauss_parameters(gauss, z, hint = (point, index))         Gaussian.jl:298-353, line_plane_distance3d and angle3d
                                                                                     LinearAlgebraUtils.jl:103-108, :127-136
       E = E0 (beam_waist / w0) w0 / w exp(-r^2 / w^2) exp(i (k z + psi + k r^2 R / 2)) exp(i ref_phi) sqrt(proj)
                                                                                     Gaussian.jl:381-392, OpticUtils.jl:65, :87-89,
                                                                                     Photodetector.jl:84, :103
       ref_phi = (optical_path_length(gauss) - length(gauss)) / lambda 2 pi         Gaussian.jl:388-390, Beam.jl:125-169

   Every input is the exact value of a double of the oracle's solved records (pd_records): the chief / waist / divergence rays of every
   segment, their lengths and refractive indices, the ancestors' lengths, beam_waist, E0, lambda of node_aux, proj of the detector row; and
   the pose and axes.  It is written from those formulas alone, not from oracle/bmo_oracle.cpp or the kernel: mpmath arithmetic, pi is pi
   (not its double), no prescribed operation order, and the NaN catches of Gaussian.jl:348-350 apply only where exact arithmetic divides
   zero by zero (it does not on any scene here; 1 / (R z) with R z = 0 is the IEEE limit psi = 0).
   About 1 ms per (point, beamlet).

2. pd_oracle_bound: a pointwise bound on |F_oracle - F_exact|, first order in u = 2^-53, for the operation sequence of
   bmo_cpu_photodetector_field.  Model: fl(a op b) = (a op b)(1 + e), |e| <= u; sqrt likewise; a library function (exp, sin, cos, tan, acos,
   atan) is within 1 ulp = 2 u.  |v| is the 2-norm of a vector, A_k the sum of the moduli of the terms that form component k.

   a. Intermediates that come out of a cancelling subtraction.  Their error bound eps_q is counted below; the field's first-order
      sensitivity to q is taken by a difference in 50 digits: |E(q + t eps_q) - E(q)| / t with t = 2^20 (the step is about 1e-10 of q).

      r    p1_k = (ox_k x + oy_k y) + p_k passes 3 roundings: |dp1| <= 3 u |A|, A_k = |ox_k x| + |oy_k y| + |p_k|.
           dp = p1 - p0 (+ u |dp|);  l1 = dot(dp, d0): |dl1| <= |ddp| + 3 u |dp| = 3 u |A| + 4 u |dp|   (|d0| = 1);
           p2_k = p0_k + l1 d0_k: |dp2| <= |dl1| + u |l1| + u |p2|;   d = p1 - p2: |dd| <= |dp1| + |dp2| + u |d|;
           r = sqrt(dot(d, d)): the norm is 1-Lipschitz, 3 u of its own.
               eps_r = u (6 |A| + 4 |dp| + |l1| + |p2| + 4 r)            (0.05 - 0.1 m cancel to r = 1e-5 - 1e-3 m)
      z    length(gauss) is a sum of N_len lengths (the parent chain's included): N_len u length;  l0 = length - length(ray) (+ u |l0|);
           z = l0 + l1 (+ u |z|):
               eps_z = u (N_len length + |l0| + |z| + 3 |A| + 4 |dp|)     (enters E through k z, 3.5e5 rad, and through the next line)
      y_d, y_w, m_d, m_w   (the heights and slopes of the divergence and waist rays at the plane through point_on_beam's point)
           s = z - temp, or length(ray) - (temp - z) on an earlier segment; temp is a sum of N_len terms at most:
               eps_s = eps_z + u (N_len temp + |temp - z| + |s|);   point = pos + s dir: eps_pt = eps_s + u |s| + u |point|.
           denom = dot(dir_c, dir): 3 u;  c = dot(point - pos_ray, dir_c): eps_pt + 4 u |q|, q = point - pos_ray;  il = c / denom:
               eps_il = (eps_pt + 4 u |q|) / |denom| + 4 u |il|
           y0_k = (pos_k + il dir_k) - point_k: |dy0| <= eps_il + u |il| + u |pos + il dir| + eps_pt + u |y0|
               eps_y0 = eps_pt (1 + 1 / |denom|) + u (4 |q| / |denom| + 5 |il| + |pos + il dir| + y)    (0.05 - 0.1 m cancel to y = 5e-5 - 3e-4 m)
           y = |y0|:  eps_y = eps_y0 + 3 u y.
           arg = dot(y0 / y, dir) / (|y0 / y| |dir|) depends on the direction of y0 only: eps_y0 / y, plus 3 u for the dot product
           (terms of modulus <= 1 cancel to the slope, 1e-3) and 8 u |arg| for the norms, their product and the quotient: 11 u.
           angle = acos(arg): eps_arg / sqrt(1 - arg^2) + 2 u pi;  alpha = pi / 2 - angle: + u pi / 2 for the double of pi / 2, + u |alpha|;
           m = tan(alpha): (1 + m^2) eps_alpha + 2 u |m|
               eps_m = (1 + m^2) ((eps_y0 / y + 11 u) / sqrt(1 - arg^2) + u (5 pi / 2 + |alpha|)) + 2 u |m|
      E_kt = y_d m_d + y_w m_w (the two terms cancel at a focus):  eps_E = 2 u (|y_d m_d| + |y_w m_w|)
      H    = |n (y_w m_d - y_d m_w)|:  eps_H = 3 u n (|y_w m_d| + |y_d m_w|)   (w0 = H / (n F) cancels in E0 (w0_g / w0) w0: its sensitivity is 0)
      x1   = 1 / (R zz) - 1 (cancels in the far field, where psi -> -pi / 2).  R = E_kt / (w w), zz = E_kt / (F F) with w, F = sqrt(a a + b b)
           (3 u each): 8 u each beyond E_kt's own error; the product and the reciprocal 2 u:  eps_x1 = 18 u / (R zz) + u |x1|.
      The sensitivities to y_d .. x1 are differences of gauss_parameters' closing formulas and electric_field together.

   b. The well-conditioned remainder, relative to |E|:
        amplitude   w0_g / w0 (1), E0 * (1), * w0 (1), / w (1 + 3 for w), exp (2), * (1), cis(ph) (3: 2 u per component), complex product (3),
                    cis(ref_phi) (3), product (3), sqrt(proj) (1), * (1):  24 u
        exp's argument a = r r / (w w): 3 u + 2 * 3 u for w:  9 u a
        ph = k z + psi + (k (r r) R) / 2:  k = 2 pi / lambda (2 u: pi's double, the quotient), k z (1): 3 u |k z|;  t3 = k r^2 R / 2: k (2), r r (1),
                    two products (2), R (8): 13 u |t3|;  psi = -atan(1, sqrt(x1)): 2 u |psi| + u / 2 (the root's u moves atan by at most u / 2);  the
                    two additions: 2 u (|k z| + |psi| + |t3|) >= 2 u |ph|
        ref_phi     dl = opl - length: N_len u (2 opl + length) (a product and a sum per term), + u |dl|; / lambda, * 2 pi (3 u):
                    k (N_len u (2 opl + length)) + 4 u |ref_phi|

   c. The sequential sum over H beamlets, re and im: 2 (H - 1) u sum_h |E_h|.

   Nothing in the bound is computed from oracle or engine output.  The NEAR-TIE z ~ cum[k] (the oracle's z on the other side of a segment
   end than the exact z) is outside it, as the exact tie is outside the tests.

3. The scenes of tests/test_pd_field_reference.py and tests/test_pd_field_edges_gpu.py; solved_case solves one on the oracle and pd_case adds
   the exact field and the bound, both once per process.
"""
import functools
import math

import numpy as np

U = 2.0 ** -53
mm = 1e-3
PLANTED = ("gouy_sign", "no_ref_phi", "proj_not_sqrt", "last_segment_rays", "no_parent_length", "curvature_reciprocal")


# ------------------------------------------------------------------------------------------------ records
def pd_records(res, nodes, slot):
    """The beamlets recorded on Photodetector `slot` of a solve, in the reference's order: res is the oracle's TraceResult, nodes the beam objects
    filled from it (bmo.system._fill_beams).  A record holds plain doubles:
      segs: per chief ray (pos, dir, n, t), with the waist and divergence rays (pos, dir) of the same segment
      parents: the (t, n) of every ray of every ancestor, nearest ancestor first
      w0, E0, lam (node_aux), proj (column 0 of the beamlet's first detector row)."""
    rows, nd = res.detector_hits(slot), res.detector_nodes(slot)
    assert len(rows) % 3 == 0
    out = []
    for h in range(len(rows) // 3):
        g = nodes[int(nd[3 * h])]
        segs = []
        for c, w, d in zip(g.chief.rays, g.waist.rays, g.divergence.rays):
            assert c.intersection is not None  # a detected beamlet: its last ray ends on the detector
            segs.append(dict(pos=c.pos.copy(), dir=c.dir.copy(), n=float(c.n), t=float(c.intersection.t), wpos=w.pos.copy(), wdir=w.dir.copy(),
                             dpos=d.pos.copy(), ddir=d.dir.copy()))
        parents, p = [], g.chief.parent
        while p is not None:
            parents.append([(float(r.intersection.t), float(r.n)) for r in p.rays if r.intersection is not None])
            p = p.parent
        out.append(dict(segs=segs, parents=parents, w0=float(g.w0), E0=complex(g.E0), lam=float(g.lam), proj=float(rows[3 * h, 0]),
                        normal=g.chief.rays[-1].intersection.n.copy()))
    return out


# ------------------------------------------------------------------------------------------------ 50-digit evaluation
def _mp():
    import mpmath

    return mpmath


def _v(a):
    mp = _mp()
    return [mp.mpf(float(x)) for x in a]  # a double is a dyadic rational: mpf(float) is exact


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _sub(a, b):
    return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]


def _axpy(p, t, d):
    return [p[0] + t * d[0], p[1] + t * d[1], p[2] + t * d[2]]


def _norm(a):
    return _mp().sqrt(_dot(a, a))


class _Beamlet:
    """The constants of one record in mpmath numbers."""

    def __init__(self, rec, planted):
        mp = _mp()
        f = mp.mpf
        self.planted = planted
        self.segs = [dict(pos=_v(s["pos"]), dir=_v(s["dir"]), n=f(s["n"]), t=f(s["t"]), wpos=_v(s["wpos"]), wdir=_v(s["wdir"]), dpos=_v(s["dpos"]),
                          ddir=_v(s["ddir"])) for s in rec["segs"]]
        # length(parent), optical_path_length(parent): Beam.jl:125-169, the parents' parents included
        self.l_parent = sum((f(t) for chain in rec["parents"] for t, n in chain), f(0))
        self.opl_parent = sum((f(t) * f(n) for chain in rec["parents"] for t, n in chain), f(0))
        self.n_len = len(self.segs) + sum(len(c) for c in rec["parents"]) + 1  # the additions of length(gauss) (one joins the parent's share)
        self.length = self.l_parent + sum((s["t"] for s in self.segs), f(0))
        self.opl = self.opl_parent + sum((s["t"] * s["n"] for s in self.segs), f(0))
        last = self.segs[-1]
        self.p0, self.d0 = last["pos"], last["dir"]
        self.l0 = self.length - last["t"]                                      # Photodetector.jl:74
        self.lam = f(rec["lam"])
        self.k = 2 * mp.pi / self.lam                                           # OpticUtils.jl:65
        self.ref_phi = (self.opl - self.length) / self.lam * 2 * mp.pi          # Gaussian.jl:388-390
        self.E0 = mp.mpc(rec["E0"].real, rec["E0"].imag)
        self.w0 = f(rec["w0"])
        self.proj = f(rec["proj"])

    def point_on_beam(self, t):
        """Beam.jl:177-205 -> (point, index (1-based), signed distance along the selected ray, temp)."""
        temp = self.l_parent if self.planted != "no_parent_length" else _mp().mpf(0)
        num = len(self.segs)
        for index, s in enumerate(self.segs, start=1):
            if index == num:
                break
            temp = temp + s["t"]
            if t < temp:
                b = temp - t
                return _axpy(s["pos"], s["t"] - b, s["dir"]), index, s["t"] - b, temp
        s = self.segs[-1]
        return _axpy(s["pos"], t - temp, s["dir"]), num, t - temp, temp

    def height_slope(self, point, cdir, pos, dir):
        """Gaussian.jl:314-321 for one of the two rays: (y, m) and what the bound needs of the way there."""
        mp = _mp()
        denom = _dot(cdir, dir)
        if not abs(denom) > 1e-6:  # line_plane_distance3d returns nothing: the reference then fails
            raise ArithmeticError("line_plane_distance3d: parallel")
        q = _sub(point, pos)
        il = _dot(q, cdir) / denom
        foot = _axpy(pos, il, dir)
        y0 = _sub(foot, point)
        y = _norm(y0)
        y0 = [c / y for c in y0]
        arg = _dot(y0, dir) / (_norm(y0) * _norm(dir))
        arg = max(-1, min(1, arg))
        alpha = mp.pi / 2 - mp.acos(arg)
        m = mp.tan(alpha)
        return y, m, dict(denom=denom, q=_norm(q), il=il, foot=_norm(foot), arg=arg, alpha=alpha)

    def closing(self, y_d, m_d, y_w, m_w, n, r, z, E_kt=None, H=None, x1=None):
        """Gaussian.jl:332-352 from the heights and slopes, then electric_field (Gaussian.jl:381-392, OpticUtils.jl:87-89) times sqrt(proj).
        E_kt, H, x1 override the intermediate of that name (the bound's differences)."""
        mp = _mp()
        if H is None:
            H = abs(n * (y_w * m_d - y_d * m_w))
            if not abs(H - self.lam / mp.pi) <= 1e-6:  # isapprox(H, lambda / pi, atol = 1e-6): rtol is 0 when atol is given
                H = self.lam / mp.pi
        if E_kt is None:
            E_kt = y_d * m_d + y_w * m_w
        F_kt = mp.sqrt(m_d ** 2 + m_w ** 2)
        w = mp.sqrt(y_d ** 2 + y_w ** 2)
        R = E_kt / w ** 2
        zz = E_kt / F_kt ** 2
        if x1 is None:
            x1 = 1 / (R * zz) - 1 if R * zz != 0 else mp.inf
        psi = -mp.atan2(1, mp.sqrt(x1)) if x1 != mp.inf else mp.mpf(0)
        w0 = H / (n * F_kt)
        if R < 0:
            psi = -psi
        if self.planted == "gouy_sign":
            psi = -psi
        Rf = 1 / R if self.planted == "curvature_reciprocal" else R
        E0 = self.E0 * (self.w0 / w0)
        a = r ** 2 / w ** 2
        t3 = self.k * r ** 2 * Rf / 2
        E = E0 * w0 / w * mp.exp(-a) * mp.expj(self.k * z + psi + t3)
        if self.planted != "no_ref_phi":
            E = E * mp.expj(self.ref_phi)
        E = E * (self.proj if self.planted == "proj_not_sqrt" else mp.sqrt(self.proj))
        return E, dict(w=w, R=R, psi=psi, w0=w0, a=a, t3=t3, x=R * zz, x1=x1, E_kt=E_kt, H=H)

    def _eps_point(self, eps_z, z, s, temp, point):
        """2a: the error bound of point_on_beam's point from that of z."""
        u = _mp().mpf(U)
        eps_s = eps_z + u * (self.n_len * abs(temp) + abs(temp - z) + abs(s))
        return eps_s + u * abs(s) + u * _norm(point)

    @staticmethod
    def _eps_height_slope(eps_pt, y, m, g):
        """2a: (eps_y, eps_m) of one ray's height and slope from the point's error bound and height_slope's third result."""
        mp = _mp()
        u = mp.mpf(U)
        ad = abs(g["denom"])
        eps_y0 = eps_pt * (1 + 1 / ad) + u * (4 * g["q"] / ad + 5 * abs(g["il"]) + g["foot"] + y)
        eps_m = (1 + m ** 2) * ((eps_y0 / y + 11 * u) / mp.sqrt(1 - g["arg"] ** 2) + u * (5 * mp.pi / 2 + abs(g["alpha"]))) + 2 * u * abs(m)
        return eps_y0 + 3 * u * y, eps_m

    def waist_at(self, z):
        """The fourth result of gauss_parameters(gauss, z) (Gaussian.jl:298-353), the waist radius w0 a beamlet takes on at z, with a first-order
        bound of what the same formulas give in doubles -> (w0, bound).  z = length(gauss) is what a splitter's children are built with
        (ThinBeamsplitter.jl:123, :134).  w0 = H / (n F), F = sqrt(m_d^2 + m_w^2): the error model of m_d, m_w and H of section 2a; z itself is a
        sum of n_len lengths (n_len u z); H carries the errors of the four heights and slopes and 3 u of its terms, or is the double of
        lambda / pi (2 u) where it is NOT approximately that (Gaussian.jl:336-339); F 3 u, the product and the quotient 2 u."""
        mp = _mp()
        u = mp.mpf(U)
        point, index, s, temp = self.point_on_beam(z)
        seg = self.segs[index - 1]
        y_d, m_d, gd = self.height_slope(point, seg["dir"], seg["dpos"], seg["ddir"])
        y_w, m_w, gw = self.height_slope(point, seg["dir"], seg["wpos"], seg["wdir"])
        n = seg["n"]
        H = abs(n * (y_w * m_d - y_d * m_w))
        eps_pt = self._eps_point(u * self.n_len * abs(z), z, s, temp, point)
        (e_yd, e_md), (e_yw, e_mw) = self._eps_height_slope(eps_pt, y_d, m_d, gd), self._eps_height_slope(eps_pt, y_w, m_w, gw)
        if not abs(H - self.lam / mp.pi) <= 1e-6:                              # Gaussian.jl:332-337, as closing() has it
            H, eps_H = self.lam / mp.pi, 2 * u * self.lam / mp.pi
        else:
            eps_H = n * (abs(m_d) * e_yw + abs(y_w) * e_md + abs(m_w) * e_yd + abs(y_d) * e_mw) + 3 * u * n * (abs(y_w * m_d) + abs(y_d * m_w))
        F = mp.sqrt(m_d ** 2 + m_w ** 2)
        w0 = H / (n * F)
        return w0, w0 * (eps_H / H + (abs(m_d) * e_md + abs(m_w) * e_mw) / F ** 2 + 5 * u)

    def at(self, p1, A, bound):
        """The field at detector point p1 -> (E, index, info); with `bound` also this beamlet's share of pd_oracle_bound (A: the |A| of 2a)."""
        mp = _mp()
        dp = _sub(p1, self.p0)
        l1 = _dot(dp, self.d0)
        p2 = _axpy(self.p0, l1, self.d0)
        r = _norm(_sub(p1, p2))
        z = self.l0 + l1
        point, index, s, temp = self.point_on_beam(z)
        seg = self.segs[-1] if (self.planted == "last_segment_rays") else self.segs[index - 1]
        cdir, n = seg["dir"], seg["n"]
        y_d, m_d, gd = self.height_slope(point, cdir, seg["dpos"], seg["ddir"])
        y_w, m_w, gw = self.height_slope(point, cdir, seg["wpos"], seg["wdir"])
        E, c = self.closing(y_d, m_d, y_w, m_w, n, r, z)
        info = dict(index=index, z=z, r=r, R=c["R"], psi=c["psi"], w=c["w"], w0=c["w0"], l_parent=self.l_parent)
        if not bound:
            return E, info, None
        u, t = mp.mpf(U), mp.mpf(2) ** 20
        absE = abs(E)
        ndp = _norm(dp)
        # 2a: the error bounds of the intermediates
        eps_r = u * (6 * A + 4 * ndp + abs(l1) + _norm(p2) + 4 * r)
        eps_z = u * (self.n_len * self.length + abs(self.l0) + abs(z) + 3 * A + 4 * ndp)
        eps_pt = self._eps_point(eps_z, z, s, temp, point)
        eps = {"r": eps_r, "z": eps_z}
        for name, y, m, g in (("d", y_d, m_d, gd), ("w", y_w, m_w, gw)):
            eps["y_" + name], eps["m_" + name] = self._eps_height_slope(eps_pt, y, m, g)
        eps["E_kt"] = 2 * u * (abs(y_d * m_d) + abs(y_w * m_w))
        eps["H"] = 3 * u * n * (abs(y_w * m_d) + abs(y_d * m_w))
        eps["x1"] = (18 * u / c["x"] + u * abs(c["x1"])) if c["x1"] != mp.inf else mp.mpf(0)
        # ... times the sensitivities, by differences
        args = dict(y_d=y_d, m_d=m_d, y_w=y_w, m_w=m_w, r=r, z=z)
        terms = {}
        for q, e in eps.items():
            if e == 0:
                terms[q] = mp.mpf(0)
                continue
            if q in args:
                E2, _ = self.closing(**dict(args, **{q: args[q] + t * e}), n=n)
            else:
                E2, _ = self.closing(**args, n=n, **{q: c[q] + t * e})
            terms[q] = abs(E2 - E) / t
        # 2b: the well-conditioned remainder
        kz = abs(self.k * z)
        phase = 3 * kz + 13 * abs(c["t3"]) + 2 * abs(c["psi"]) + mp.mpf(1) / 2 + 2 * (kz + abs(c["psi"]) + abs(c["t3"]))
        ref = self.k * self.n_len * (2 * abs(self.opl) + self.length) + 4 * abs(self.ref_phi)
        terms["rounding"] = absE * u * (24 + 9 * c["a"] + phase + ref)
        return E, info, terms


class PdExact:
    """What pd_field_exact returns.  [nx, ny] arrays indexed [i, j] like the reference's Matrix; a leading axis runs over the beamlets.
      F         the 50-digit sum over the beamlets (object array of mpmath complex numbers)
      E_abs     |E_h| per beamlet (float);  scale = sum_h |E_h|
      index     1-based index of the segment point_on_beam selects, per beamlet
      z, r, R, psi, w   per beamlet (float roundings of the 50-digit values);  l_parent [H]
      bound     pd_oracle_bound (None unless asked for);  terms: its parts per name, summed over the beamlets"""

    def error(self, field):
        """|field - F| [nx, ny] as floats, the difference taken in 50 digits."""
        mp = _mp()
        with mp.workdps(50):
            return np.array([[float(abs(mp.mpc(complex(field[i, j])) - self.F[i, j])) for j in range(self.F.shape[1])] for i in range(self.F.shape[0])])


def pd_field_exact(records, position, orientation, xs, ys, planted=None, bound=False):
    """The exact field of `records` (pd_records) on the detector pose (position, orientation) at (xs[i], ys[j]) -> PdExact.
    planted: one of PLANTED, a deliberate mistake (the tests show that the bound catches each)."""
    assert planted is None or planted in PLANTED
    mp = _mp()
    nx, ny, H = len(xs), len(ys), len(records)
    out = PdExact()
    out.F = np.zeros((nx, ny), dtype=object)
    out.E_abs = np.zeros((H, nx, ny))
    out.index = np.zeros((H, nx, ny), dtype=np.int64)
    out.z, out.r, out.R, out.psi, out.w = (np.zeros((H, nx, ny)) for _ in range(5))
    out.l_parent = np.zeros(H)
    out.terms = {}
    with mp.workdps(50):
        beamlets = [_Beamlet(rec, planted) for rec in records]
        o = np.asarray(orientation, dtype=np.float64).reshape(3, 3)
        ox, oy, p = _v(o[0]), _v(o[2]), _v(position)  # T[k, 1] = orientation[1, k], T[k, 3] = orientation[3, k]
        tot = np.zeros((nx, ny), dtype=object)
        for i, x in enumerate(_v(xs)):
            for j, y in enumerate(_v(ys)):
                p1 = [ox[k] * x + oy[k] * y + p[k] for k in range(3)]
                A = mp.sqrt(sum((abs(ox[k] * x) + abs(oy[k] * y) + abs(p[k])) ** 2 for k in range(3)))
                acc, b_acc, s_acc = mp.mpc(0), mp.mpf(0), mp.mpf(0)
                for h, bl in enumerate(beamlets):
                    E, info, terms = bl.at(p1, A, bound)
                    acc += E
                    s_acc += abs(E)
                    out.E_abs[h, i, j] = float(abs(E))
                    out.index[h, i, j] = info["index"]
                    for name in ("z", "r", "R", "psi", "w"):
                        getattr(out, name)[h, i, j] = float(info[name])
                    out.l_parent[h] = float(info["l_parent"])
                    if bound:
                        for name, v in terms.items():
                            out.terms.setdefault(name, np.zeros((nx, ny)))[i, j] += float(v)
                            b_acc += v
                out.F[i, j] = acc
                if bound:
                    summation = 2 * (H - 1) * mp.mpf(U) * s_acc  # 2c
                    out.terms.setdefault("summation", np.zeros((nx, ny)))[i, j] = float(summation)
                    tot[i, j] = b_acc + summation
    out.scale = out.E_abs.sum(axis=0)
    out.bound = np.array(tot, dtype=np.float64) if bound else None
    return out


def pd_oracle_bound(records, position, orientation, xs, ys):
    """The pointwise bound on |F_oracle - F_exact| of the module docstring, [nx, ny] (pd_field_exact(..., bound=True) gives both at once)."""
    return pd_field_exact(records, position, orientation, xs, ys, bound=True).bound


# ------------------------------------------------------------------------------------------------ scenes
def _lens(thickness=4 * mm):
    import bmo_amd as bmo

    lens = bmo.SphericalLens(0.05, -0.05, thickness, 12.7 * mm, 1.5)
    bmo.translate3d(lens, [0, 0.05, 0])
    return lens


def _root(lam=1e-6, pos=(0, 0, 0), direction=(0.002, 1, -0.003)):
    import bmo_amd as bmo

    return bmo.GaussianBeamlet(list(pos), list(direction), lam, 0.3 * mm, P0=1e-3)


def _steep_detector(at, tilt=70, width=4 * mm):
    import bmo_amd as bmo

    pd = bmo.Photodetector(width, 21)
    bmo.xrotate3d(pd, math.radians(tilt))
    bmo.zrotate3d(pd, math.radians(4))
    bmo.translate3d(pd, at)
    return pd


def scene_earlier_segment():
    """A steep detector 1.5 mm behind the lens: part of the grid projects onto the beamlet's path inside the glass (segment 2 of 3)."""
    import bmo_amd as bmo

    pd = _steep_detector([0.1 * mm, 0.05 + 5.6 * mm, -0.2 * mm])
    return bmo.System([_lens(), pd]), pd, [_root()], pd.x, pd.y


def scene_three_segments():
    """The same pose with longer ys: the grid reaches the path in front of the lens, inside it and behind it."""
    import bmo_amd as bmo

    pd = _steep_detector([0.1 * mm, 0.05 + 5.6 * mm, -0.2 * mm], width=16 * mm)
    xs = bmo.linalg.linrange(-0.9 * mm, 0.9 * mm, 21)
    ys = bmo.linalg.linrange(-7.5 * mm, 1.0 * mm, 21)
    return bmo.System([_lens(), pd]), pd, [_root()], xs, ys


def scene_child():
    """A thin beamsplitter at 45 degrees, the steep detector 1.2 mm behind it: the transmitted child (one segment) is detected, and part of the
    grid projects onto the axis in front of the splitter, z < length(parent)."""
    import bmo_amd as bmo

    bs = bmo.ThinBeamsplitter(10 * mm)
    bmo.xrotate3d(bs, math.radians(45))
    bmo.translate3d(bs, [0, 0.05, 0])
    pd = _steep_detector([0.1 * mm, 0.05 + 1.2 * mm, -0.2 * mm])
    return bmo.System([bs, pd]), pd, [_root()], pd.x, pd.y


FOCUS_Y = 0.103  # where an on-axis solve finds the lens's focus (w = 54 um); test_pd_field_reference.py asserts the sign change of R there


def scene_focus():
    """A detector tilted by 75 degrees, centred on the focus of the lens: R changes sign on the grid."""
    import bmo_amd as bmo

    pd = _steep_detector([0.2 * mm, FOCUS_Y, -0.3 * mm], tilt=75, width=3 * mm)
    xs = bmo.linalg.linrange(-0.25 * mm, 0.25 * mm, 21)
    ys = bmo.linalg.linrange(-1.5 * mm, 1.5 * mm, 21)
    return bmo.System([_lens(), pd]), pd, [_root()], xs, ys


def scene_three_wavelengths():
    """Three roots of different wavelength and direction through the lens onto the steep detector: the sum and the per-beamlet k."""
    import bmo_amd as bmo

    pd = _steep_detector([0.1 * mm, 0.05 + 5.6 * mm, -0.2 * mm])
    roots = [_root(1e-6), _root(633e-9, pos=(0.2 * mm, 0, 0.1 * mm), direction=(-0.001, 1, 0.002)),
             _root(1.55e-6, pos=(-0.1 * mm, 0, -0.2 * mm), direction=(0.003, 1, 0.001))]
    return bmo.System([_lens(), pd]), pd, roots, pd.x, pd.y


SCENES = {"earlier_segment": scene_earlier_segment, "three_segments": scene_three_segments, "child": scene_child, "focus": scene_focus,
          "three_wavelengths": scene_three_wavelengths}


class PdCase:
    pass


def solve_case(oracle, name, r_max=20):
    """Scene `name` solved on the oracle -> PdCase with system, pd, roots, bundle, scene, xs, ys, res, osol (to be freed by the caller), records."""
    import bmo_amd as bmo

    c = PdCase()
    c.name = name
    c.system, c.pd, c.roots, c.xs, c.ys = SCENES[name]()
    c.bundle = bmo.RayBundle.from_beams(c.roots)
    c.scene = bmo.CompiledScene(c.system, c.bundle.lambdas)
    c.slot = c.scene.detectors.index(c.pd)
    c.res, c.osol = oracle.trace(c.scene, c.bundle, r_max, keep=True)
    c.nodes = bmo.system._fill_beams(c.scene, c.res, c.roots)
    c.records = pd_records(c.res, c.nodes, c.slot)
    c.position, c.orientation = np.array(c.pd.position(), dtype=np.float64), np.array(c.pd.orientation(), dtype=np.float64)
    return c


def oracle_field(c):
    f = np.zeros((len(c.xs), len(c.ys)), dtype=np.complex128)
    c.osol.photodetector_field(c.slot, c.position, c.orientation, c.xs, c.ys, f)
    return f


@functools.lru_cache(maxsize=None)
def solved_case(oracle, name):
    """solve_case plus the oracle's field (c.oracle_field): once per process and shared (treat it as read-only; the solution is never freed)."""
    c = solve_case(oracle, name)
    c.oracle_field = oracle_field(c)
    c.exact = None
    return c


def pd_case(oracle, name):
    """solved_case plus the exact field and the bound (c.exact, a PdExact), computed once per process."""
    c = solved_case(oracle, name)
    if c.exact is None:
        c.exact = pd_field_exact(c.records, c.position, c.orientation, c.xs, c.ys, bound=True)
    return c


def restated_z(rec, position, orientation, xs, ys):
    """z = l0 + l1 (Photodetector.jl:74, :97-101) of one record at the grid points in plain doubles, [nx, ny]: values of z to feed to
    gauss_parameters, not an expected value of anything."""
    o = np.asarray(orientation, dtype=np.float64).reshape(3, 3)
    p = np.asarray(position, dtype=np.float64)
    x, y = np.asarray(xs, dtype=np.float64)[:, None], np.asarray(ys, dtype=np.float64)[None, :]
    last = rec["segs"][-1]
    dp = [o[0, k] * x + o[2, k] * y + p[k] - last["pos"][k] for k in range(3)]
    l1 = (dp[0] * last["dir"][0] + dp[1] * last["dir"][1]) + dp[2] * last["dir"][2]
    length = sum(s["t"] for s in rec["segs"]) + sum(t for chain in rec["parents"] for t, n in chain)
    return (length - last["t"]) + l1

"""Helpers of the trace-against-exact-optics tests (not a test file).

1. exact_step / exact_trace: one bounce, and a whole root, of the reference's trace evaluated in 50 significant digits (mpmath).
   Written from the reference's formulas alone, cited by file and line; not from oracle/, csrc/ or the sub-shape tables of shapes.py.
   What enters is the test scenes' input data only: each object's prescription (radii, conic constant, coefficients, diameter, centre
   thickness, detector width, n(lambda)) and its pose doubles (position(), orientation()).  Vertex positions, edge sags, barrel ends
   and sphere centres are derived here in mpmath, so a mistake of the host scene builder shows like one of the oracle or the lane code.

   Boundary of a solid = analytic pieces, each with a validity region, in the solid's frame  local = transpose(orientation) (p - position)
   (AbstractSDF.jl:35-40), optical axis +y, front vertex at the origin (SphericalLensSDF.jl:16-20):

       surface of revolution  y = y_v + sag(r),  r^2 = x^2 + z^2 <= (d / 2)^2           front y_v = 0, back y_v = centre thickness
                                                                                         (Lenses.jl:186-219: mid shifted by thickness(front),
                                                                                         back by thickness(mid) + thickness(back))
           sphere     sag = R - sign(R) sqrt(R^2 - r^2)                                  SphericalLensSDF.jl:159-232, OpticUtils.jl:153
           asphere    sag = c r^2 / (1 + sqrt(1 - (1 + k) c^2 r^2)) + sum_i a_i r^(2 i)  AsphericalLensSDF.jl:133-141 (i from 1: a_1 is A2)
           plane      sag = 0  (radius Inf: no sub-shape, the plano face of the mid cylinder, Lenses.jl:189-192)
       barrel                 r = d / 2,  y between the two edge heights y_v + sag(d / 2)  SphericalLensSDF.jl:60-65
       box face               |p_k| = half edge k, the other two coordinates inside          PrimitiveSDF.jl:29-46 (centred on the position)
       prism hypotenuse       x + y = 0 inside the box, outward normal (1, 1, 0) / sqrt(2); the box faces where x + y <= 0   PrimitiveSDF.jl:195-210
       plane annulus, ring barrel   y = const on r0 <= r <= r1, r = const between two heights: the levelling and outer rings of a lens whose clear
                              apertures or mechanical diameters differ (RingSDF, PrimitiveSDF.jl:146-166; Lenses.jl:222-287), ExactRingLens
       flat square mesh       y = 0, |x|, |z| <= w / 2, normal +y of the mesh frame       Mesh.jl:183-192, :282-303; a detector's mesh is
                                                                                         rotated by pi about z before use (PSFDetector.jl:62-68)
       mesh triangle          its plane with an exact barycentric inclusion test, normal by the right-hand rule of the vertex order
                              (Mesh.jl:183-192): the three faces of RetroMesh(scale) (Misc.jl:8-22), the twelve of a sheared CuboidMesh of glass (Mesh.jl:362-395)
       ball, cut ball, cylinder   norm(p) = R; its part above the plane y = h with the cut disc; norm(x, z) = r, |y| <= HALF height with two end caps
                              (SphereSDF SphericalLensSDF.jl:72-89, CutSphereSDF PrimitiveSDF.jl:83-124, CylinderSDF :53-76): ExactBall, ExactCutSphere,
                              ExactCylinder - all three exact distances on both sides
       two caps, no barrel    ThinLensSDF (SphericalLensSDF.jl:245-253): ExactThinLens, centre thickness = the two sags, a sharp rim
   A solid of kind 'mirror' reflects on every face (Mirrors.jl:76-81): ConcaveSphericalMirror is ExactLens(Surface(-R), plane) - the sphere's centre
   lies R in FRONT of the vertex (SphericalLensSDF.jl:159-170) -, RoundPlanoMirror ExactLens(plane, plane), RightAnglePrismMirror ExactPrism with
   pre = the double of deg2rad(225) (Mirrors.jl:226-230), RectangularPlanoMirror ExactMesh.cuboid (Mirrors.jl:110-119).
   The inner faces between the sub-shapes of a union are not boundary (UnionSDF.jl:53-56: the minimum is negative there).  A spherical lens
   of any sign combination - biconvex, biconcave, meniscus (MeniscusLensSDF.jl:42-46, :62-78: cap and cylinder minus a ball) - is the same
   three pieces: two surfaces y = y_v + sag(r) and the barrel between their edge heights.  A cemented doublet is two such lenses, the back
   one's position derived here from the front one's thickness (DoubletLenses.jl:57-64).

   exact_hit follows the reference's rules:
     * start further than eps_srf from the solid (AbstractSDF.jl:171): the first boundary point of the ray, closed form for sphere, plane
       and barrel; for an aspheric profile every sign change of the residual y(t) - y_v - sag(r(t)) on the part of the ray inside the
       aperture cylinder is found by a scan of 96 samples and refined in mpmath, so no root between start and result is skipped.
     * start on or inside it: the outward normal n at the start decides, dot(dir, n) <= 0 marches inside (AbstractSDF.jl:175-178), else no
       hit.  Inside, the reference steps eps_ins = 1 m until it is outside and marches back (AbstractSDF.jl:132-159): the result is the LAST
       boundary crossing before the first 1 m step that lands outside.  Every solid here is smaller than 1 m, so that is the last crossing.
     * a mesh: Moeller-Trumbore, t >= 1e-9 (Mesh.jl:203-237); in exact arithmetic the plane with an exact inclusion test.
   The normal is the outward unit normal of the piece at the hit point: the gradient of the sdf, for entering and leaving hits alike
   (AbstractSDF.jl:79-95); interact3d flips it when the ray leaves (Lenses.jl:53-66).

   The next ray: refraction3d / reflection3d with the TIR branch (OpticUtils.jl:7-45), n2 = n(lambda) of the lens on entry, 1 on exit, the
   lens's n after a total internal reflection (Lenses.jl:46-77); a mirror reflects and keeps the index, J = diag(-1, 1) (Mirrors.jl:39-69); a
   thin splitter ends the beam and spawns a transmitted and a reflected child in n = 1 with J = diag(T, T) and diag(-R, R), R = sqrt(reflectance),
   T = sqrt(1 - R^2) (ThinBeamsplitter.jl:43-115).  PolarizedRay: theta_i = angle3d(dir, -normal) (LinearAlgebraUtils.jl:103-108),
   fresnel_coefficients(theta_i, n2 / n1) with the principal complex root above the critical angle (OpticUtils.jl:121-131),
   is_internally_reflected (:144-146), J = diag(-rs, rp) or diag(ts, tp) (Lenses.jl:110-121), E0' = O_out J O_in E0 (PolarizedRays.jl:165-207).
   The optical path grows by n t* (Beam.jl:125-169); a PSFDetector row is (hit, dir, opl, |dot(dir, normal)|, 2 pi / lambda)
   (PSFDetector.jl:77-89), pi being pi.

   exact_trace iterates exact_step from a root ray's doubles and picks the nearest object at every bounce by itself (System.jl:57-72).  The
   reference tests a hinted object alone first (System.jl:74-85); no two objects of the scenes here overlap, so the nearest is the same.

2. step_bound: a first-order bound on recorded-minus-exact for every quantity of one bounce, u = 2^-53, fl(a op b) = (a op b)(1 + e),
   |e| <= u; Base's sin / cos / acos are faithful: 2 u.  The constants of the march are read from the compiled
   scene, which has them from one place (system.py, CompiledScene: eps_ray, eps_srf, grad_h, march_iters).  NOTHING in the bound is
   computed from oracle or engine output: its inputs are the exact hit (t*, the piece, its curvature, the exact incidence angle theta)
   and the magnitudes of the exact coordinates.

   t    _raymarch_outside (AbstractSDF.jl:102-125) moves pos by the sdf until sdf(q) < eps_ray and returns t0 = (sum of the steps) + sdf(q):
        the distance travelled to q plus the last sdf.  With s = sdf(q) in [0, eps_ray) the ray still has rho = s / |cos theta| to go on a
        plane; on a curved piece the foot of q is s tan(theta) beside the hit, where the tangent plane has turned by kappa s tan(theta):
        rho = s / |cos theta| (1 + e2), |e2| <= c2 = 2 kappa eps_ray (1 + tan^2 theta) / |cos theta|.  So
            t - t*  in  [-eps_ray (1 / |cos theta| - 1) (1 + c2), 0]        entering (the hit stops short of the surface)
        and mirrored for a leaving hit, t = 1 m-steps - t0 of the march back (AbstractSDF.jl:148-152: the hit lies past the surface).
        The unions here are convex or the hit piece is exact (sphere, plane, barrel: exact distances, UnionSDF.jl:4-6).  An aspheric leaf
        returns the pseudo-distance |y - sag(r)| / sqrt(1 + g^2), g = sag'(r) (AsphericalLensSDF.jl:209-210): along the ray the residual
        y - sag falls at the rate |v_y - g v_r| = |cos theta| sqrt(1 + g^2), so rho = s / |cos theta| to first order as well; the second-order
        term of the estimate is the profile's curvature at the hit, kappa = max(|sag''| / (1 + g^2)^(3/2), |g| / (r sqrt(1 + g^2))), in c2.
        One face understates its distance by a constant factor: the rim between the vertex plane and the edge of a CONCAVE aspheric or
        acylindric profile belongs to that leaf's closed perimeter, whose segments the reference divides by m = |grad_z_boundary| =
        sqrt(1 + sag'(d / 2)^2) (AsphericalLensSDF.jl:247-306).  There sdf(q) = s / m < eps_ray while the ray has s / |cos theta| to go, so the
        interval is eps_ray (m / |cos theta| - 1) (1 + c2) and the distance shrinks by 1 - |cos theta| / m per step m is computed here, in mpmath,
        from the prescription; no measured number enters the bound.  (A cross-check only: on the AYL2520 acylinder m = 1.2348, and the sdf
        read through the oracle's check entry is 0.8098 of the distance at that rim.)
        Roundings: the running sum t0 takes one per step, N u t_run; pos = pos + dist dir two per component and step, 2 N u P off the ideal
        ray, which moves the hit by that much along the ray and by tan(theta) times that across; the last sdf is off by e_sdf = 6 u S
        (the frame change T (p - pos): 4 u (|p| + |pos|); the norm and the subtraction of the radius: 2 u more of S), S = |hit| + |pos| + |R|
        (+ |y| + |sag| on an asphere), the magnitudes that cancel in the sdf.  N is not read from a counter: a convex solid lies behind
        the tangent plane at the hit, so sdf >= rho |cos theta| and rho shrinks by 1 - |cos theta| per step:
            N = 2 + ceil(log(t_run / eps_ray) / -log(1 - |cos theta| + kappa t_run sin^2(theta) / 2)), at most march_iters;
            t_run = t* entering, 1 m - t* leaving; the kappa term covers a piece that curves TOWARDS the ray (the concave face of a doublet's
            back lens met from inside the front one: the distance to a sphere from inside is rho cos(theta) - rho^2 sin^2(theta) / (2 R) + ...).
            rnd_t = u (N t_run + 2 N P (1 + tan theta) + 6 S (1 + 1 / |cos theta|)) + u t
        A mesh hit has no march: Moeller-Trumbore's t = dot(E2, Qv) / Det is about 30 operations on magnitudes M = |pos| + |vertices| + t:
            |t - t*| <= 32 u M / |cos theta|.
        Mesh vertices: the evaluator derives a mesh's world vertices exactly from the prescription and the pose doubles; the traces read a vertex
        table that every kinematic step has rewritten in doubles (Mesh.jl:78-96): a translation rounds each component once, a rotation about the
        mesh's position is fl(p + R (v - p)), five roundings of magnitudes up to M = |position| + size per component (sqrt(3) 5 u M < 9 u M as a
        vector), and the orientation doubles the evaluator multiplies with are themselves fl(R dir), 3 u per entry (another 9 u M): each vertex
        lies within dv = 18 u M steps of its exact place.  A face's plane then moves by dv and turns by 2 dv / a, a its smallest altitude, which
        moves a hit up to `size` from a vertex by 2 dv size / a more:  t takes dv (1 + 2 size / a) / |cos theta|, the normal 2 dv / a more.  Where
        faces are as large as positions (the rhomb, the retroreflector: steps = 0) the 8 u and 32 u M above have covered it; the cuboid mirror
        (5 mm faces 40 mm from the origin, four steps) states its steps.
   n    taken at q, not at the returned point (AbstractSDF.jl:118-120): the foot of q is at most eps_ray tan(theta) / ... beside the hit,
            dn = kappa eps_ray tan(theta) (1 + c2) + kappa (2 N u P + 6 u S) + 12 u          dual-number normals (normalize, rotation)
        Central differences (AbstractSDF.jl:81-88; aspheres always, AsphericalLensSDF.jl:5; flat faces and the barrel where the fallback of
        DESIGN.md section 2 applies) add  11 u S / grad_h + grad_h^2 |f'''| / 6: each of the six sdf values is off by e_sdf = 6 u S, a
        component is their difference over 2 grad_h, three components (sqrt(3) 6 = 11); |f'''| <= 3 kappa^2 for a distance field, the
        profile's third derivative on an asphere.  The evaluator does not predict which rule a flat-face or barrel hit takes: both
        terms are in the bound there, and the piece's exact normal is inside it.  A mesh normal is a normalised cross product: 8 u.
   dir, E0   the exact derivative of refraction3d / reflection3d / the Jones transform with respect to the normal, taken by differences
        of the 50-digit evaluation along the two tangents e1, e2 of the normal (step 2^-60; |d.e1| + |d.e2| <= sqrt(2) |d|), times dn; dir and
        E0 of the incoming ray are the record's doubles, exact.  Roundings: refraction 14 u (n, cos_i, sin_t^2, the root, three
        components of two products and a sum), reflection 8 u.  The field: fresnel_coefficients is ~12 operations and three faithful
        functions, (16 + 6 X) u of each coefficient with X = (n^2 + sin^2) / |n^2 - sin^2| for the cancellation under the root; the s axis
        is a normalised cross product of in and out, whose components carry 2 u absolute, so the axis turns by 4 u / |in x out|, which
        moves E0' only through the DIFFERENCE of the two Jones entries; two 3 x 3 products and a matrix-vector product, 3 terms each:
            dE = (D_e1 + D_e2) dn + |E0| (u (30 + 16 + 6 X) jmax + 8 u |j11 - j22| / |in x out|),  jmax = max(|j11|, |j22|, 1).
   index   the next ray's refractive index is held EXACTLY (bound 0) where n(lambda) is a constant or a table.  Where the host evaluates a formula
        (SellmeierEquation) the record carries its double, within k u of the 50-digit value, relative, k the count of roundings of the host's
        expression (sellmeier() derives k = 16); dir and E0 take k u times their derivative with respect to ln n, a difference of the 50-digit
        interaction like D above.
   pos  next pos = pos + t dir (Lenses.jl:69):  |dt| + 2 u (|pos| + t) + u |pos'|.
   opl  n t per segment (Beam.jl:125-169):  n |dt| + u n t, summed, plus (k - 1) u opl for the k - 1 additions.
   row  a PSFDetector row repeats the hit point (dpos of the last segment), dir (exact copy), opl, proj = |dot(dir, n)| (dn + 4 u) and
        2 pi / lambda (2 u: pi's double and the quotient).

3. PLANTED: switches that plant one mistake each in the exact evaluator; the tests show that the bound catches every one by four orders.
   Of the builders: the concave mirror's sphere centre behind the vertex, the prism mirror turned by 45 instead of 225 degrees, the plano-concave
   lens's ring centred on l / 2 (where the biconcave one's sits), the thin lens's back cap moved by its own thickness alone, the cut sphere's
   height negated, the cylinder's axis along x, the wavelength put into Sellmeier's formula in metres, an aspheric surface's edge sag taken
   unsigned as a spherical one's is (the levelling ring of L2 then starts above the vertex plane instead of below it).
   Not among them, but built (VIA_AIR): a doublet interface refracted glass -> air -> glass.  For a Ray that is no mistake the direction can
   show: n sin(theta) is the same after one refraction and after two across a gap of zero width (it differs in the Fresnel amplitudes only,
   and the reference's doublet has no method for PolarizedRays, DoubletLenses.jl:66).  The tests show both halves: on the doublet scene the switch changes no
   direction beyond 50-digit rounding, and beyond the critical angle glass -> air it turns a refraction into a reflection.

4. Composite interactions.
   Plate splitter (ExactPlateBS, parts substrate 0 / coating 1; PlateBeamsplitter.jl:160-228): both parts are tested and the coating wins where
   the two lengths are approximately equal (rtol sqrt(eps)) or it is nearer; their exact faces coincide, so at the coated face that tie is the
   rule (like the interface of a doublet: no tie exclusion inside one object).  At the substrate the lens interaction, then a hint at the
   coating; at the coating the thin splitter's children, the transmitted one's direction replaced by refraction3d(ray, n2) with the normal
   flipped by the ray's own isentering, the indices (n_optics, 1) entering and (1, n_optics) leaving - for a beamlet by the CHIEF ray's
   isentering.  The transmitted child's E0 stays that of the straight-through direction.  The round plate's coating is a 30-gon mesh
   (Mesh.jl:322-348): its triangles are slivers, and the doubles of its world vertices turn a sliver's normal by 2 (8 u M) / (R sin(2 pi / 30)).
   Cube splitter (ExactCubeBS, front 0 / back 1 / coating 2; CubeBeamsplitter.jl:49-92): both prisms hint at the coating, both children keep
   their directions and start in glass, on the face the two prisms share.
   Children start ON surfaces, and exact_hit gives the reference's answer there (AbstractSDF.jl:166-181): within eps_srf of a solid and heading
   outwards nothing is found on it, heading inwards the inside march runs; a mesh met below mt_leps is no hit.
   Every new Ray and PolarizedRay is normalised by its constructor (Rays.jl:32-42, PolarizedRays.jl:80-95): a child's direction is
   normalize(dir), 4 u (this shows inside the cube, where the parent's direction is a refracted one of length 1 to a few u).
   Polarization filter (interact_polarizer; PolarizationFilter.jl:31-48, JonesCalculus.jl:29-45): E' = Q (R J R^T) Q E0 with R the filter's
   orientation doubles and Q = I - d d^T, direction and index kept, blocked when norm(E') is approximately the cutoff; a Ray or a beamlet stops
   there.  Bound of E': four 3 x 3 products and a matrix-vector product at 3 u |A| |B| each, Q's entries 2 u twice, the moduli of Q, R, R^T, Q
   with 2-norms up to sqrt(3): 171 u |J| |E0|; nothing of it depends on the normal.  An outcome whose exact norm lies within that bound
   (+ 4 u for the norm) of the threshold is the one the evaluator does not predict (excluded()).
   The PolarizedRay constructor's check (PolarizedRays.jl:54-56: |dot(dir, E0)| <= 1e-14) runs wherever the reference builds one; where it fails
   the reference throws and the record ends with BMO_NODE_ERR_ORTHO | BMO_NODE_STOPPED: exact_step's 'end'.  This is what ends the child a
   plate transmits, at its next refraction.
   GaussianBeamlet children (exact_gauss_children; ThinBeamsplitter.jl:117-168): w0 = gauss_parameters(gauss, length(gauss))[4], evaluated by
   tests/pd_ref.py's one 50-digit gauss_parameters (waist_at, with the error model of its section 2a for the bound), E_t = T E0 (w0_g / w0),
   E_r = R E0 (w0_g / w0) exp(i phi), phi = pi where the chief ray faces the normal; the bound adds 10 u and, for phi = pi, |sin(fl(pi))| = 1.3e-16.

5. Two properties of the reference that the scenes of the plano lenses and of the phone objective turned up (both are
   reproduced by tests/test_trace_reference.py):
   a) a PolarizedRay that meets a flat sdf face ALONG its normal may end ERR_ORTHO: the march lands on the face, the normal comes from central
      differences (1e-11 off), isparallel3d's window (eps() in 1 - |dot|, an angle of 2e-8) still calls everything parallel, the new field is
      built orthogonal to the INCOMING direction and the refracted direction has turned by more than the constructor's 1e-14 allows.  The
      evaluator, with the exact normal, lets the ray pass; exclusion is not the remedy (no seam, no tie): the fans of PolarizedRays avoid
      exact normal incidence on flat sdf faces, and a test of its own shows the mechanism with the RECORDED normal.
   b) an aspheric leaf's sdf is |y - sag(r)| / sqrt(1 + sag'(r)^2) at the point's own r: along an oblique ray it can EXCEED the length left to
      the surface, a long step of the march (the march back of a leaving hit starts 1 m out) passes through the surface and lands micrometres
      inside, where sdf < eps_ray ends the march.  The premise 0 <= sdf(q) < eps_ray of `t` above fails there.  overshoot() derives the
      remedy from the exact ray and the hit leaf's formula alone: the union's sdf is at most the leaf's value U, so a step from the length rho
      before the hit lands at most D = max_rho (U(rho) - rho) deep; at the depth delta the march ends with sdf = -a(delta) and the returned
      point is |delta - a(delta)| from the exact hit - second order in delta where the landing point is nearer to the profile than to the leaf's
      other faces, at most max(delta, a) elsewhere; the normal is the profile's at the landing point's radius.  step_bound adds the two maxima
      over delta <= D to t and to n on every aspheric piece of a lens with rings (D = 0 where no rho overstates: nothing is added).  The
      record's landing depths, replayed with the oracle's sdf, lie below D on every such bounce (the tests assert it); on L2 the worst bounce
      reaches 0.997 of the bound of t.  ExactRingLens builds L1 and L2 of the phone objective with it (a concave aspheric front, closed along
      its vertex plane, :285-305; a convex aspheric back, the leaf between the plane of its edge height and the profile, :229-238).  The branch
      of an INFLECTED concave aspheric front (:266-283) is written but no scene drives it: no such surface is in the reference's tests.
   The apex of a CONCAVE ASPHERIC face is a seam like L3's crest: the leaf over the mid cylinder's plane is thinner than the central-difference
   stencil within sqrt(2 |R| grad_h) of it (7.9 um on L2), aspheres always take central differences, and a hit ON the apex is 0.73 rad off.
   The scenes keep their rays 50 um from it.

Not covered yet (no pieces for them here): the read-out of a
beamlet's field (tests/pd_ref.py has that); a RETRACE of beamlets through a moved splitter, where the reference computes the children's w0 over
a stale tail.

The perimeter with which the reference closes an INFLECTED aspheric leaf (element L3 of the phone objective) enters through ExactRingLens: the
convex leaf ends at the plane of its largest sag and the mid cylinder starts there, the concave leaf at the plane of its edge height
(AsphericalLensSDF.jl:211-228, :266-283).  In a lens those planes and the leaf's rim are inner faces (mid cylinder, levelling ring and back leaf
cover them), so no hit lands on them and their 1 / |grad_z_boundary| scale does not enter a bound; where they lie decides where every outer
face lies.  One place remains where they show: on the crest circle of the profile the leaf between profile and plane thins to nothing, and a
hit where it is thinner than 1e-8 m lies on a seam (hit['leaf']).
"""
import math

import numpy as np

U = 2.0 ** -53
PLANTED = ("conic_sign", "coef_shift", "back_vertex_edge_sag", "cylinder_extruded_along_z", "exit_normal_not_flipped", "n2_glass_on_exit", "ts_tp_swapped",
           "tir_phase_conjugated", "opl_next_medium", "plate_no_refraction", "plate_normal_not_flipped", "plate_indices_swapped", "cube_children_in_air",
           "gauss_no_phase_flip", "gauss_flip_on_both_sides", "gauss_child_keeps_w0", "gauss_w0_at_start", "polarizer_rotation_transposed",
           "polarizer_not_projected", "coating_loses_tie", "mirror_centre_wrong_side", "prism_mirror_pre_45", "ring_centred_half_l",
           "thin_back_not_shifted", "cut_height_negated", "cylinder_axis_x", "sellmeier_metres", "aspheric_edge_sag_unsigned")
# The planted mistakes that show only in something held EXACTLY - a child's refractive index, or which part of a plate splitter is met at all -
# and the quantity whose mismatch shows them: its bound is zero, so the ratio is infinite, not a number of bounds.
PLANTED_EXACT = {"plate_indices_swapped": "index", "cube_children_in_air": "index", "coating_loses_tie": "t"}
VIA_AIR = "doublet_via_air"  # not a mistake a Ray's direction can show (n sin(theta) is kept), except beyond the critical angle glass -> air
SEAM = 1e-8       # a bounce whose exact hit lies this close to a seam between two pieces or to an aperture edge is left out
TIE = 1e-9        # ... or whose two nearest objects' exact t* differ by less than this


def _mp():
    import mpmath

    return mpmath


def consts_of(scene):
    """The march constants of a CompiledScene (set in one place, system.py CompiledScene)."""
    d = scene.desc
    return dict(eps_ray=float(d.eps_ray), eps_srf=float(d.eps_srf), grad_h=float(d.grad_h), march_iters=int(d.march_iters), eps_ins=float(d.eps_ins),
                mt_leps=float(d.mt_leps))


# ------------------------------------------------------------------------------------------------ vectors
def _f(x):
    mp = _mp()
    return x if isinstance(x, mp.mpf) else mp.mpf(float(x))  # a double is a dyadic rational: exact; a 50-digit number stays what it is


def _v(a):
    return [_f(x) for x in a]


def _c(E):
    """A complex 3-vector of doubles (or of 50-digit numbers) as mpmath complex numbers."""
    mp = _mp()
    if E is None:
        return None
    return [z if isinstance(z, (mp.mpc, mp.mpf)) else mp.mpc(complex(z).real, complex(z).imag) for z in E]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _sub(a, b):
    return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]


def _add(a, b):
    return [a[0] + b[0], a[1] + b[1], a[2] + b[2]]


def _axpy(p, t, d):
    return [p[0] + t * d[0], p[1] + t * d[1], p[2] + t * d[2]]


def _scale(s, a):
    return [s * a[0], s * a[1], s * a[2]]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _norm(a):
    return _mp().sqrt(sum(abs(x) ** 2 for x in a))


def _unit(a):
    n = _norm(a)
    return [x / n for x in a]


def _tangents(n):
    """Two unit vectors orthogonal to the unit vector n and to each other."""
    k = min(range(3), key=lambda i: abs(n[i]))
    e = [0, 0, 0]
    e[k] = 1
    e1 = _unit(_cross(n, e))
    return e1, _cross(n, e1)


# ------------------------------------------------------------------------------------------------ solids
def _precise(cls):
    """The class with its constructors run at 50 digits, wherever they are called from: what they derive (edge heights, vertex positions,
    largest sags, the vertices of a mesh) is part of the exact evaluation."""
    def wrap(fn):
        def inner(*a, **kw):
            with _mp().workdps(50):
                return fn(*a, **kw)
        inner.__doc__, inner.__name__ = fn.__doc__, fn.__name__
        return inner

    for name, attr in list(vars(cls).items()):
        if name == "__init__":
            setattr(cls, name, wrap(attr))
        elif isinstance(attr, classmethod):
            setattr(cls, name, classmethod(wrap(attr.__func__)))
    return cls


@_precise
class _Solid:
    def __init__(self, position, orientation, pre=None):
        o = np.asarray(orientation, dtype=np.float64).reshape(3, 3)
        self.pos = _v(position)                      # doubles, or 50-digit numbers derived from doubles
        self.cols = [_v(o[:, k]) for k in range(3)]  # local axis k in world coordinates
        if pre is not None:  # the solid was turned about z by the DOUBLE angle `pre` before the pose applied: orientation Rz(pre), in 50 digits
            c, s = _mp().cos(_f(pre)), _mp().sin(_f(pre))
            c0, c1 = self.cols[0], self.cols[1]
            self.cols = [_add(_scale(c, c0), _scale(s, c1)), _sub(_scale(c, c1), _scale(s, c0)), self.cols[2]]
        self.pos_mag = float(_norm(self.pos))

    def to_local(self, p):
        d = _sub(p, self.pos)
        return [_dot(self.cols[k], d) for k in range(3)]

    def vec_local(self, v):
        return [_dot(self.cols[k], v) for k in range(3)]

    def vec_world(self, v):
        return [self.cols[0][i] * v[0] + self.cols[1][i] * v[1] + self.cols[2][i] * v[2] for i in range(3)]


class Surface:
    """One face of a lens: radius (Inf: plane), and for an even asphere the conic constant and the coefficients a_1 (r^2), a_2 (r^4), ..."""

    def __init__(self, radius, conic=None, coefficients=None):
        self.radius, self.conic, self.coefs = float(radius), conic, coefficients
        self.aspheric = conic is not None

    def sag(self, r2, planted=None):
        """sag as a function of r^2."""
        mp = _mp()
        if math.isinf(self.radius):
            return mp.mpf(0)
        R = _f(self.radius)
        if not self.aspheric:
            return R - mp.sign(R) * mp.sqrt(R * R - r2)                      # OpticUtils.jl:153 with the sign of the radius
        c, k = 1 / R, _f(self.conic)
        if planted == "conic_sign":
            k = -k
        shift = 1 if planted == "coef_shift" else 0
        poly = mp.mpf(0)
        for a in reversed(self._coefs50()):                                  # Horner: sum_i a_i r2^i
            poly = (poly + a) * r2
        if shift:
            poly = poly * r2
        arg = 1 - (1 + k) * c * c * r2
        if arg < 0:
            assert planted is not None  # only a planted conic constant can take the aperture out of the profile's domain: continued flat
            arg = mp.mpf(0)
        return c * r2 / (1 + mp.sqrt(arg)) + poly                            # AsphericalLensSDF.jl:133-141

    def _coefs50(self):
        if getattr(self, "_c50", None) is None or self._c50[0] != _mp().mp.prec:
            self._c50 = (_mp().mp.prec, [_f(a) for a in self.coefs])
        return self._c50[1]

    def r2_max(self):
        """The largest r^2 at which the (right) profile is defined."""
        if math.isinf(self.radius):
            return None
        R = _f(self.radius)
        if not self.aspheric:
            return R * R
        k1 = 1 + _f(self.conic)
        return R * R / k1 if k1 > 0 else None

    def dsag(self, r, planted=None):
        """d sag / d r, d^2 sag / d r^2, |d^3 sag / d r^3| at radius r >= 0."""
        mp = _mp()
        if math.isinf(self.radius):
            return mp.mpf(0), mp.mpf(0), mp.mpf(0)
        if not self.aspheric:
            R = _f(self.radius)
            w = mp.sqrt(R * R - r * r)
            return mp.sign(R) * r / w, mp.sign(R) * R * R / w ** 3, abs(3 * R * R * r / w ** 5)
        R = _f(self.radius)
        c, k = 1 / R, _f(self.conic)
        if planted == "conic_sign":
            k = -k
        shift = 1 if planted == "coef_shift" else 0
        w = 1 - (1 + k) * c * c * r * r                                      # d/dr of the conic part is c r / sqrt(w)
        if w < mp.mpf(10) ** -12:
            assert planted is not None
            w = mp.mpf(10) ** -12
        g, g2, g3 = c * r / mp.sqrt(w), c / w ** mp.mpf(1.5), 3 * c ** 3 * (1 + k) * r / w ** mp.mpf(2.5)
        for i, a in enumerate(self.coefs, start=1):
            m = 2 * (i + shift)
            g += m * _f(a) * r ** (m - 1)
            g2 += m * (m - 1) * _f(a) * r ** (m - 2)
            if m >= 3:
                g3 += m * (m - 1) * (m - 2) * _f(a) * r ** (m - 3)
        return g, g2, abs(g3)


@_precise
class ExactLens(_Solid):
    """Lens(front, back, centre thickness, n) (Lenses.jl:176-291) with both clear apertures equal to d: two surfaces of revolution and a barrel."""

    kind = "lens"
    axes = (0, 2)  # the coordinates the profile's r is made of: x and z for a surface of revolution

    def __init__(self, front, back, thickness, diameter, n, position, orientation, planted=None, kind="lens"):
        super().__init__(position, orientation)
        mp = _mp()
        self.front, self.back, self.n, self.planted, self.kind = front, back, n, planted, kind  # kind 'mirror': every face reflects (Mirrors.jl:76-81)
        self.l, self.d = _f(thickness), _f(diameter)
        self.h2 = (self.d / 2) ** 2
        self.yv = [mp.mpf(0), self.l]
        if planted == "back_vertex_edge_sag":  # the back vertex put where the back EDGE belongs
            self.yv[1] = self.l - back.sag(self.h2)
        self.edge = [self.yv[0] + front.sag(self.h2, planted), self.yv[1] + back.sag(self.h2, planted)]
        assert self.edge[0] < self.edge[1], "no barrel: not a shape this evaluator knows"
        self.size = float(max(self.d, abs(self.edge[1]), abs(self.edge[0]), self.l))
        assert self.size < 0.5  # the 1 m step of the inside march leaves the solid at once

    def index(self, lam):
        return _f(self.n(float(lam)))

    def index_tol(self):
        """The relative bound, in units of u, of the index the host hands to the traces: 0 for a constant or a table (the double itself), the
        count of roundings of a formula the host evaluates in doubles (sellmeier)."""
        return getattr(self.n, "roundings", 0)

    # ---- the line p(t) = o + t v in the local frame against each piece -> [(t, piece, outward normal (local), kappa, f3, S)]
    def _surface_roots(self, which, o, v):
        mp = _mp()
        srf = (self.front, self.back)[which]
        yv, out_sign = self.yv[which], (-1, 1)[which]
        roots = []
        if math.isinf(srf.radius):
            if v[1] != 0:
                roots.append((yv - o[1]) / v[1])
        elif not srf.aspheric:
            R = _f(srf.radius)
            w = _sub(o, [0, yv + R, 0])
            ks = self.axes + (1,)                                           # a sphere, or a circle extruded along the axis left out
            a, b, c = sum(v[k] ** 2 for k in ks), sum(w[k] * v[k] for k in ks), sum(w[k] ** 2 for k in ks) - R * R
            disc = b * b - a * c
            if disc >= 0 and a > 0:
                s = mp.sqrt(disc)
                for t in ((-b - s) / a, (-b + s) / a):
                    if mp.sign(R) * (o[1] + t * v[1] - (yv + R)) < 0:  # the vertex side
                        roots.append(t)
        else:
            roots = self._aspheric_roots(srf, yv, o, v)
        out = []
        for t in roots:
            p = _axpy(o, t, v)
            r2 = sum(p[k] ** 2 for k in self.axes)
            if r2 > self.h2 or not self.in_aperture(p):
                continue
            r = mp.sqrt(r2)
            g, g2, g3 = srf.dsag(r, self.planted)
            grad = [mp.mpf(0), mp.mpf(1), mp.mpf(0)]
            for k in self.axes:
                grad[k] = -g * p[k] / r if r > 0 else mp.mpf(0)
            w = mp.sqrt(1 + g * g)
            nrm = _scale(out_sign / w, grad)
            kappa = max(abs(g2) / w ** 3, ((abs(g) / (r * w)) if r > 0 else abs(g2)) if len(self.axes) == 2 else 0)
            f3 = 3 * kappa ** 2 if not srf.aspheric else g3 + 3 * kappa ** 2
            S = abs(srf.radius) if not (srf.aspheric or math.isinf(srf.radius)) else float(abs(p[1] - yv) + abs(srf.sag(r2, self.planted)) + self.d / 2)
            out.append(dict(t=t, piece=("front", "back")[which], n=nrm, kappa=kappa, f3=f3, S=S, central=self.central(srf),
                            exact_leaf=not srf.aspheric, edge_dist=min(self.d / 2 - r, self.aperture_gap(p))))
        return out

    def leaf_scale(self, y):
        """The factor by which the reference's sdf UNDERSTATES the distance to the rim face at height y.  The rim between the vertex plane and
        the edge of a concave ASPHERIC profile belongs to the aspheric leaf's closed perimeter, whose line segments are divided by
        |grad_z_boundary| = sqrt(1 + sag'(d / 2)^2) (AsphericalLensSDF.jl:247-306: sdl / norm(grad_z_boundary)); elsewhere the rim is the mid
        cylinder's or box's and exact."""
        mp = _mp()
        for srf, yv, sign in ((self.front, self.yv[0], -1), (self.back, self.yv[1], 1)):
            if srf.aspheric and sign * srf.sag(self.h2, self.planted) > 0 and sign * (y - yv) > 0:
                g = srf.dsag(self.d / 2, self.planted)[0]
                return mp.sqrt(1 + g * g)
        return mp.mpf(1)

    def in_aperture(self, p):
        return True

    def aperture_gap(self, p):
        return self.d

    def central(self, srf):
        """Whether the normal of this face may come from central differences: always on an asphere (AsphericalLensSDF.jl:5), on a plane."""
        return srf.aspheric or math.isinf(srf.radius)

    def _aspheric_roots(self, srf, yv, o, v):
        """Every sign change of y(t) - y_v - sag(r(t)^2) on the part of the line inside the aperture cylinder (and inside the profile's domain)."""
        mp = _mp()
        a = sum(v[k] ** 2 for k in self.axes)
        lim = self.h2 if srf.r2_max() is None else min(self.h2, srf.r2_max())
        o2 = sum(o[k] ** 2 for k in self.axes)
        if a == 0:
            return [(yv + srf.sag(o2, self.planted) - o[1]) / v[1]] if o2 <= lim and v[1] != 0 else []
        b, c = sum(o[k] * v[k] for k in self.axes), o2 - lim
        disc = b * b - a * c
        if disc <= 0:
            return []
        ta, tb = (-b - mp.sqrt(disc)) / a, (-b + mp.sqrt(disc)) / a
        res = lambda t: o[1] + t * v[1] - yv - srf.sag(min(sum((o[k] + t * v[k]) ** 2 for k in self.axes), lim), self.planted)
        M = 96
        ts = [ta + (tb - ta) * i / M for i in range(M + 1)]
        fs = [res(t) for t in ts]
        roots = []
        for i in range(M):
            if fs[i] == 0:
                roots.append(ts[i])
            elif fs[i] * fs[i + 1] < 0:
                roots.append(mp.findroot(res, (ts[i], ts[i + 1]), solver="anderson", tol=mp.mpf(10) ** -45, maxsteps=100))
        if fs[M] == 0:
            roots.append(ts[M])
        return roots

    def _barrel_roots(self, o, v):
        mp = _mp()
        a = v[0] ** 2 + v[2] ** 2
        if a == 0:
            return []
        b, c = o[0] * v[0] + o[2] * v[2], o[0] ** 2 + o[2] ** 2 - self.h2
        disc = b * b - a * c
        if disc < 0:
            return []
        out = []
        for t in ((-b - mp.sqrt(disc)) / a, (-b + mp.sqrt(disc)) / a):
            p = _axpy(o, t, v)
            if self.edge[0] <= p[1] <= self.edge[1]:
                r = self.d / 2
                out.append(dict(t=t, piece="barrel", n=[p[0] / r, mp.mpf(0), p[2] / r], kappa=2 / self.d, f3=3 * (2 / self.d) ** 2, S=float(self.d / 2),
                                central=True, exact_leaf=True, edge_dist=min(p[1] - self.edge[0], self.edge[1] - p[1]), scale=self.leaf_scale(p[1])))
        return out

    def crossings(self, o, v):
        c = self._surface_roots(0, o, v) + self._surface_roots(1, o, v) + self._barrel_roots(o, v)
        return sorted(c, key=lambda h: h["t"])


@_precise
class ExactRingLens(_Solid):
    """Lens(front_surface, back_surface, centre thickness, n) of two spherical or flat surfaces with clear apertures d_f, d_b and mechanical
    diameters md_f, md_b that need not agree (Lenses.jl:176-291, the branch with a mid cylinder, l0 > 0).  The solid is the union of regions
    of the (r, y) half-plane, r0 <= r <= r1, lo(r) <= y <= hi(r), each bound a constant or a surface y_v + sag(r):

        front leaf   r <= d_f / 2   sag_f(r) .. t_f  (convex, t_f = |sag_f(d_f / 2)|)   or   sag_f(r) .. 0  (concave, t_f = 0)   SphericalLensSDF.jl:159-232
        mid          r <= min(d_f, d_b) / 2   t_f .. t_f + l0,   l0 = ct - t_f - t_b                                            Lenses.jl:186-219
        back leaf    r <= d_b / 2   ct - t_b .. ct + sag_b(r)  (convex)   or   ct .. ct + sag_b(r)  (concave)
        levelling ring (d_f != d_b)   d_b > d_f:  d_f / 2 <= r <= d_b / 2,  s_f .. s_f + l0                                         Lenses.jl:231-246
                                      d_f > d_b:  d_b / 2 <= r <= d_f / 2,  t_f .. t_f + l0 (+ s_b + t_b under a concave back)       :247-266
        outer ring (md > max(d_f, d_b))   max(d) / 2 <= r <= md / 2,  s_f .. ct + s_b                                               :269-286
    with s = |sag(d / 2)| of the surface, as edge_sag returns it for a spherical surface of either sign (SphericalLensSDF.jl:421).  Candidate
    crossings are taken with every bound of every region - spheres, planes y = const, cylinders r = const (RingSDF, PrimitiveSDF.jl:146-166) -
    and kept where the solid lies on exactly one side (the union's inner faces drop out, UnionSDF.jl:53-56); that side gives the outward normal."""

    kind = "lens"
    DELTA = 1e-12  # the step to either side of a candidate face: far below every feature of these lenses, far above 50-digit rounding

    def __init__(self, front, back, thickness, n, d_f, d_b, md_f, md_b, position, orientation, planted=None):
        super().__init__(position, orientation)
        mp = _mp()
        self.n, self.planted = n, planted
        f = _f
        ct, hf, hb = f(thickness), f(d_f) / 2, f(d_b) / 2
        # thickness(sub-shape) and edge_sag(surface) as the reference has them: a spherical surface's edge sag is its positive sagitta whatever
        # its sign (SphericalLensSDF.jl:421); an aspheric one's is the signed sag at the edge (AsphericalLensSDF.jl:463-472), its leaf as thick
        # as the largest sag where the profile is inflected (:33-36, :97-100)
        s_f, t_f = self._edge_and_thickness(front, hf, convex=front.radius > 0)
        s_b, t_b = self._edge_and_thickness(back, hb, convex=back.radius < 0)
        l0 = ct - t_f - t_b
        assert l0 > 0, "the meniscus branch is not this class's"
        C, S = (lambda y: ("c", y)), (lambda srf, yv: ("s", srf, yv))
        reg = [dict(r0=0, r1=min(hf, hb), lo=C(t_f), hi=C(t_f + l0))]
        if not math.isinf(front.radius):
            if front.radius < 0 and t_f > 0:
                # an INFLECTED concave aspheric front: the leaf lies between the plane of its edge height and the profile (:266-283)
                reg.append(dict(r0=0, r1=hf, lo=C(front.sag(hf * hf, planted)), hi=S(front, mp.mpf(0))))
            else:  # convex: profile .. closing plane t_f; concave (a sphere, or an asphere closed along its vertex plane, :285-305): profile .. 0
                reg.append(dict(r0=0, r1=hf, lo=S(front, mp.mpf(0)), hi=C(t_f if front.radius > 0 else mp.mpf(0))))
        if not math.isinf(back.radius):
            reg.append(dict(r0=0, r1=hb, lo=C(ct - t_b), hi=S(back, ct)))
        md, d_min, d_max = max(f(md_f), f(md_b)) / 2, min(hf, hb), max(hf, hb)
        if md >= d_min:
            if hb > hf:
                lev = l0 + ((abs(s_f) + t_f) if s_f < 0 else 0)              # Lenses.jl:234-243
                reg.append(dict(r0=hf, r1=hb, lo=C(s_f), hi=C(s_f + lev)))
            elif hf > hb:
                lev = l0 + ((abs(s_b) + t_b) if s_b - t_b > 0 else 0)        # :249-257
                reg.append(dict(r0=hb, r1=hf, lo=C(t_f), hi=C(t_f + lev)))
            if md > d_max:
                reg.append(dict(r0=d_max, r1=md, lo=C(s_f), hi=C(ct + s_b)))
                if planted == "ring_centred_half_l":  # a ring of the right thickness ct + s_b - s_f centred on ct / 2, not on its own half thickness
                    reg[-1].update(lo=C(ct / 2 - (ct + s_b - s_f) / 2), hi=C(ct / 2 + (ct + s_b - s_f) / 2))
        self.regions = reg
        self.size = float(max(2 * md, 2 * d_max, ct + abs(s_f) + abs(s_b)))
        assert self.size < 0.5

    index, index_tol = ExactLens.index, ExactLens.index_tol
    axes = (0, 2)

    def _edge_and_thickness(self, srf, h, convex):
        """(edge_sag, thickness of the leaf) of one surface of half aperture h; convex: whether its leaf is the convex kind (R > 0 in front,
        R < 0 behind).  An aspheric leaf: max_aspheric_value (AsphericalLensSDF.jl:53-67) is the sag where sag' changes sign between 1e-8 and
        h, else the end value of larger modulus; the convex leaf is max_sag thick where max_sag > 0 > edge sag (an inflected profile, closed at
        its largest sag, :211-228) and |edge sag| otherwise, the concave one |edge sag| in that case (closed at the edge height, :266-283) and
        0 otherwise."""
        mp = _mp()
        if math.isinf(srf.radius):
            return mp.mpf(0), mp.mpf(0)
        edge = srf.sag(h * h, self.planted)
        if not srf.aspheric:
            return abs(edge), (abs(edge) if convex else mp.mpf(0))
        g = lambda r: srf.dsag(r, self.planted)[0]
        a = mp.mpf(10) ** -8
        if mp.sign(g(a)) == mp.sign(g(h)):
            fa = srf.sag(a * a, self.planted)
            max_sag = fa if abs(fa) > abs(edge) else edge
        else:
            rm = mp.findroot(g, (a, h), solver="anderson", tol=mp.mpf(10) ** -45, maxsteps=200, verify=False)
            assert a < rm < h
            max_sag = srf.sag(rm * rm, self.planted)
        inflected = max_sag > 0 and edge < 0
        s_edge = abs(edge) if self.planted == "aspheric_edge_sag_unsigned" else edge  # planted: the positive sagitta, as a SPHERICAL surface's is
        if convex:
            return s_edge, (max_sag if inflected else abs(edge))
        return s_edge, (abs(edge) if inflected else mp.mpf(0))

    def _y(self, bound, r2):
        return bound[1] if bound[0] == "c" else bound[2] + bound[1].sag(r2, self.planted)

    def inside(self, p):
        r2 = p[0] ** 2 + p[2] ** 2
        for g in self.regions:
            if g["r0"] ** 2 <= r2 <= g["r1"] ** 2 and self._y(g["lo"], r2) <= p[1] <= self._y(g["hi"], r2):
                return True
        return False

    def _corner_gap(self, p):
        mp = _mp()
        r = mp.sqrt(p[0] ** 2 + p[2] ** 2)
        out = []
        for g in self.regions:
            for rk in (g["r0"], g["r1"]):
                if rk == 0:
                    continue  # the axis is no seam
                for b in (g["lo"], g["hi"]):
                    out.append(mp.sqrt((r - rk) ** 2 + (p[1] - self._y(b, rk ** 2)) ** 2))
        return min(out)

    def crossings(self, o, v):
        mp = _mp()
        cand = []  # (t, geometric normal, kappa, f3, S, central, name)
        for g in self.regions:
            for b in (g["lo"], g["hi"]):
                if b[0] == "c" or math.isinf(b[1].radius):
                    y0 = self._y(b, 0)
                    if v[1] != 0:
                        cand.append(((y0 - o[1]) / v[1], [mp.mpf(0), mp.mpf(1), mp.mpf(0)], mp.mpf(0), mp.mpf(0), self.size, True, "plane", g))
                    continue
                srf, yv = b[1], b[2]
                if srf.aspheric:
                    self.h2 = g["r1"] ** 2                                    # what ExactLens._aspheric_roots scans within
                    for t in ExactLens._aspheric_roots(self, srf, yv, o, v):
                        p = _axpy(o, t, v)
                        r = mp.sqrt(p[0] ** 2 + p[2] ** 2)
                        gr, g2, g3 = srf.dsag(r, self.planted)
                        w_ = mp.sqrt(1 + gr * gr)
                        grad = [-gr * p[0] / r, mp.mpf(1), -gr * p[2] / r] if r > 0 else [mp.mpf(0), mp.mpf(1), mp.mpf(0)]
                        kap = max(abs(g2) / w_ ** 3, (abs(gr) / (r * w_)) if r > 0 else abs(g2))
                        cand.append((t, _scale(1 / w_, grad), kap, g3 + 3 * kap ** 2, float(abs(p[1] - yv) + abs(srf.sag(r * r, self.planted)) + g["r1"]),
                                     True, "asphere", g))
                    continue
                R = _f(srf.radius)
                w = _sub(o, [0, yv + R, 0])
                bb, cc = _dot(w, v), _dot(w, w) - R * R
                disc = bb * bb - cc
                if disc < 0:
                    continue
                for t in (-bb - mp.sqrt(disc), -bb + mp.sqrt(disc)):
                    p = _axpy(o, t, v)
                    if mp.sign(R) * (p[1] - (yv + R)) < 0:
                        cand.append((t, _scale(1 / abs(R), _sub(p, [0, yv + R, 0])), 1 / abs(R), 3 / (R * R), abs(srf.radius), False, "sphere", g))
            a = v[0] ** 2 + v[2] ** 2
            for rk in (g["r0"], g["r1"]):
                if rk == 0 or a == 0:
                    continue
                bb, cc = o[0] * v[0] + o[2] * v[2], o[0] ** 2 + o[2] ** 2 - rk * rk
                disc = bb * bb - a * cc
                if disc < 0:
                    continue
                for t in ((-bb - mp.sqrt(disc)) / a, (-bb + mp.sqrt(disc)) / a):
                    p = _axpy(o, t, v)
                    cand.append((t, [p[0] / rk, mp.mpf(0), p[2] / rk], 1 / rk, 3 / (rk * rk), float(rk), True, "barrel", g))
        out, seen = [], []
        d = mp.mpf(self.DELTA)
        for t, ng, kappa, f3, S, central, name, g in cand:
            p = _axpy(o, t, v)
            r2 = p[0] ** 2 + p[2] ** 2
            if name == "barrel":
                if not self._y(g["lo"], r2) - d <= p[1] <= self._y(g["hi"], r2) + d:
                    continue
            elif not max(g["r0"] - d, 0) ** 2 <= r2 <= (g["r1"] + d) ** 2:
                continue
            if any(abs(t - q) < mp.mpf(10) ** -30 for q in seen):
                if name == "asphere":  # ON the apex of a concave aspheric face the plane under it was taken first: the seam of the note below
                    for h in out:
                        if abs(t - h["t"]) < mp.mpf(10) ** -30:
                            h["edge_dist"] = min(h["edge_dist"], abs(self._y(g["hi"], r2) - self._y(g["lo"], r2)))
                continue
            a_in, b_in = self.inside(_axpy(p, d, ng)), self.inside(_axpy(p, -d, ng))
            if a_in == b_in or any(abs(t - q) < mp.mpf(10) ** -30 for q in seen):
                continue
            seen.append(t)
            # the seam distance: to the corners of the regions and, on an aspheric profile, to the OTHER bound of its leaf - where the leaf is
            # thinner than that, its closing face (the plane at an inflected profile's largest sag) lies as close behind the hit.  Not on a
            # sphere: the wedge under a concave apex is as thin, and the reference's dual-number normals are right there (rule ii)
            leaf = abs(self._y(g["hi"], r2) - self._y(g["lo"], r2)) if name == "asphere" else mp.inf
            out.append(dict(t=t, piece=name, n=ng if b_in else _scale(-1, ng), kappa=kappa, f3=f3, S=S, central=central, exact_leaf=True,
                            edge_dist=min(self._corner_gap(p), leaf), leaf=leaf))
            if name == "asphere":
                out[-1]["region"] = g  # the leaf: step_bound's overshoot term reads its profile and its closing plane
        out.sort(key=lambda h: h["t"])
        # Next to the apex of a concave face the leaf over the mid cylinder's plane is thinner than DELTA (r^2 / (2 R)), and the probe sees
        # the plane AND the sphere as faces: of two crossings of the same sense closer than 1e-15 m the outer one is the face, two of opposite
        # sense enclose nothing.
        merged = []
        for h in out:
            if merged and h["t"] - merged[-1]["t"] < mp.mpf(10) ** -15:
                if (_dot(v, h["n"]) > 0) == (_dot(v, merged[-1]["n"]) > 0):
                    # under an ASPHERIC concave apex that thin leaf is a seam like L3's crest (aspheres always take central differences,
                    # AsphericalLensSDF.jl:5): the face that is kept inherits the smaller seam distance.  A sphere's leaf is inf: unchanged
                    seam = min(h["edge_dist"], merged[-1]["edge_dist"])
                    merged[-1] = dict(h if _dot(v, h["n"]) > 0 else merged[-1], edge_dist=seam)
                else:
                    merged.pop()
                continue
            merged.append(h)
        return merged


@_precise
class ExactParts:
    """An object of several solids that are hit as shapes of their own, like a DoubletLens built from two Lens objects of any kind
    (DoubletLenses.jl:26-38): each part comes with its own pose."""

    kind = "doublet"

    def __init__(self, parts):
        self.parts = list(parts)


@_precise
class ExactCylLens(ExactLens):
    """Lens(front, back, centre thickness, n) of cylindrical or acylindrical surfaces (Lenses.jl:331-390): the profile y = y_v + sag(|z|) of a
    circle (CylindricalSDF.jl:62-85, :123-139) or of the aspheric equation (AcylindricalSDF.jl:55-74) extruded along x over the cylinder
    height, |z| <= d / 2, and four plane side faces in place of the barrel (the mid section is a box, Lenses.jl:355).  Every face may take a
    central-difference normal: the extrusion's sdf ends in norm(max.(w, 0)) (AbstractSDF.jl:229-234), whose dual is NaN at w <= 0."""

    axes = (2,)

    def __init__(self, front, back, thickness, diameter, height, n, position, orientation, planted=None):
        if planted == "cylinder_extruded_along_z":
            self.axes = (0,)
        super().__init__(front, back, thickness, diameter, n, position, orientation, planted)
        self.hx = _f(height) / 2
        self.size = max(self.size, float(height))
        self.other = 0 if self.axes == (2,) else 2  # the axis of the extrusion

    def in_aperture(self, p):
        return abs(p[self.other]) <= self.hx

    def aperture_gap(self, p):
        return self.hx - abs(p[self.other])

    def central(self, srf):
        return True

    def _barrel_roots(self, o, v):
        mp = _mp()
        out = []
        ax = self.axes[0]
        for k, half in ((ax, self.d / 2), (self.other, self.hx)):
            if v[k] == 0:
                continue
            for sgn in (-1, 1):
                t = (sgn * half - o[k]) / v[k]
                p = _axpy(o, t, v)
                r2 = p[ax] ** 2
                if r2 > self.h2 or abs(p[self.other]) > self.hx:
                    continue
                lo = self.yv[0] + self.front.sag(r2, self.planted)
                hi = self.yv[1] + self.back.sag(r2, self.planted)
                if not lo <= p[1] <= hi:
                    continue
                nrm = [mp.mpf(0)] * 3
                nrm[k] = mp.mpf(sgn)
                j = self.other if k == ax else ax
                out.append(dict(t=t, piece="side", n=nrm, kappa=mp.mpf(0), f3=mp.mpf(0), S=self.size, central=True, exact_leaf=True,
                                scale=self.leaf_scale(p[1]) if k == ax else mp.mpf(1), edge_dist=min(p[1] - lo, hi - p[1], (self.hx if j == self.other else self.d / 2) - abs(p[j]))))
        return out


@_precise
class ExactBox(_Solid):
    """Lens(BoxSDF(x, y, z), n): a block of glass centred on its position, edge lengths x, y, z (PrimitiveSDF.jl:29-46): six plane faces."""

    kind = "lens"

    def __init__(self, x, y, z, n, position, orientation, pre=None, kind="lens"):
        super().__init__(position, orientation, pre)
        self.half, self.n, self.kind = [_f(x) / 2, _f(y) / 2, _f(z) / 2], n, kind
        self.size = float(max(x, y, z))
        assert self.size < 0.5

    index, index_tol = ExactLens.index, ExactLens.index_tol

    def crossings(self, o, v):
        mp = _mp()
        out = []
        for k in range(3):
            if v[k] == 0:
                continue
            for sgn in (-1, 1):
                t = (sgn * self.half[k] - o[k]) / v[k]
                p = _axpy(o, t, v)
                gaps = [self.half[j] - abs(p[j]) for j in range(3) if j != k]
                if min(gaps) < 0:
                    continue
                nrm = [mp.mpf(0)] * 3
                nrm[k] = mp.mpf(sgn)
                out.append(dict(t=t, piece="face%s%d" % ("-+"[sgn > 0], k), n=nrm, kappa=mp.mpf(0), f3=mp.mpf(0), S=self.size, central=True, exact_leaf=True,
                                edge_dist=min(gaps)))
        return sorted(out, key=lambda h: h["t"])


@_precise
class ExactPrism(ExactBox):
    """Lens(RightAnglePrismSDF(leg, height), n) (PrimitiveSDF.jl:195-210, Prisms.jl:28-31): the box |x|, |y| <= leg / 2, |z| <= height / 2 cut by
    the plane x + y = 0: the two leg faces x = -leg / 2 and y = -leg / 2, the two triangular end faces, and the hypotenuse with the outward
    normal (1, 1, 0) / sqrt(2).  max(box, plane) is exact next to every face."""

    def __init__(self, leg, height, n, position, orientation, pre=None, kind="lens"):
        super().__init__(leg, leg, height, n, position, orientation, pre, kind)

    def crossings(self, o, v):
        mp = _mp()
        r2 = mp.sqrt(2)
        out = []
        for h in super().crossings(o, v):
            p = _axpy(o, h["t"], v)
            if p[0] + p[1] <= 0:
                h["edge_dist"] = min(h["edge_dist"], -(p[0] + p[1]) / r2)
                out.append(h)
        den = v[0] + v[1]
        if den != 0:
            t = -(o[0] + o[1]) / den
            p = _axpy(o, t, v)
            gaps = [self.half[j] - abs(p[j]) for j in range(3)]
            if min(gaps) >= 0:
                out.append(dict(t=t, piece="hypotenuse", n=[1 / r2, 1 / r2, mp.mpf(0)], kappa=mp.mpf(0), f3=mp.mpf(0), S=self.size, central=True,
                                exact_leaf=True, edge_dist=min(gaps[2], min(gaps[0], gaps[1]) * r2)))
        return sorted(out, key=lambda h: h["t"])


@_precise
class ExactThinLens(ExactLens):
    """ThinLens(R1, R2, d, n) = Lens(ThinLensSDF(R1, R2, d), n), what SphericalLens(r1, r2, 0, d, n) dispatches to (SphericalLenses.jl:20-45,
    SphericalLensSDF.jl:245-253; both radii POSITIVE, the back surface's signed radius is -R2): two convex caps, the front one sag_1 thick with
    its vertex at the origin, the back one turned by pi about z and moved by thickness(front) + thickness(back) = sag_1 + sag_2, so that its
    vertex lies there and the two flat sides meet in the plane y = sag_1.  No barrel: the caps meet in a sharp rim, the circle r = d / 2 at
    y = sag_1, and a hit within 1e-8 m of it is a seam.  Both sags are derived here from the radii and the diameter (OpticUtils.jl:153)."""

    def __init__(self, r1, r2, diameter, n, position, orientation, planted=None):
        _Solid.__init__(self, position, orientation)
        mp = _mp()
        self.front, self.back, self.n, self.planted, self.kind = Surface(r1), Surface(-float(r2)), n, planted, "lens"
        self.d = _f(diameter)
        self.h2 = (self.d / 2) ** 2
        s1, s2 = self.front.sag(self.h2), -self.back.sag(self.h2)
        self.l = s1 + s2
        self.yv = [mp.mpf(0), s2 if planted == "thin_back_not_shifted" else self.l]  # planted: moved by its own thickness alone
        self.edge = [s1, self.yv[1] - s2]
        self.size = float(max(self.d, self.l))
        assert self.size < 0.5

    def _barrel_roots(self, o, v):
        return []


@_precise
class ExactBall(_Solid):
    """Lens(SphereSDF(radius), n) (SphericalLensSDF.jl:72-89): the ball of that radius about the position; its orientation is fixed to the unit
    matrix (:82-84).  sdf = norm(p) - radius is the exact distance on both sides, and its dual-number gradient p / norm(p) is defined
    everywhere on the surface: no central differences."""

    kind = "lens"

    def __init__(self, radius, n, position, orientation):
        super().__init__(position, orientation)
        self.R, self.n = _f(radius), n
        self.size = float(2 * self.R)
        assert self.size < 0.5

    index, index_tol = ExactLens.index, ExactLens.index_tol

    def crossings(self, o, v):
        mp = _mp()
        a, b, c = _dot(v, v), _dot(o, v), _dot(o, o) - self.R ** 2
        disc = b * b - a * c
        if disc <= 0:
            return []
        out = []
        for t in ((-b - mp.sqrt(disc)) / a, (-b + mp.sqrt(disc)) / a):
            p = _axpy(o, t, v)
            out.append(dict(t=t, piece="sphere", n=_scale(1 / self.R, p), kappa=1 / self.R, f3=3 / self.R ** 2, S=float(self.R), central=False,
                            exact_leaf=True, edge_dist=mp.inf))
        return out


@_precise
class ExactCutSphere(_Solid):
    """Lens(CutSphereSDF(radius, height), n) (PrimitiveSDF.jl:83-124): with q = (norm(x, z), y) the sdf is norm(q) - radius where
    s = max((h - R) q1^2 + w^2 (h + R - 2 q2), h q1 - w q2) < 0, h - q2 where q1 < w, else the distance to the rim (w, h), w = sqrt(R^2 - h^2):
    the part of the ball about the position that lies ABOVE the plane y = height (on the axis above the ball s < 0 and the value is y - R;
    below the plane it is h - y > 0).  Pieces: the cap norm(p) = R, y >= h, and the cut disc y = h, r <= w, outward normal -y; they meet in
    the rim circle.  The three branches are the exact distances to cap, disc and rim outside, and inside the branch s < 0 is bounded by the
    parabola on which cap and disc are equally far: exact on both sides (exact_leaf).  Normals: the cap's dual-number gradient runs through
    norm(Point2(x, z)), whose partials are NaN on the axis - central differences there (taken within 1 um of it, where the bound carries both
    rules); the disc's value h - q2 has clean partials, and as on every flat face the bound carries both rules."""

    kind = "lens"

    def __init__(self, radius, height, n, position, orientation, planted=None):
        super().__init__(position, orientation)
        self.R, self.n = _f(radius), n
        self.h = -_f(height) if planted == "cut_height_negated" else _f(height)
        self.w = _mp().sqrt(self.R ** 2 - self.h ** 2)
        self.size = float(2 * self.R)
        assert self.size < 0.5

    index, index_tol = ExactLens.index, ExactLens.index_tol

    def crossings(self, o, v):
        mp = _mp()
        out = []
        a, b, c = _dot(v, v), _dot(o, v), _dot(o, o) - self.R ** 2
        disc = b * b - a * c
        if disc > 0:
            for t in ((-b - mp.sqrt(disc)) / a, (-b + mp.sqrt(disc)) / a):
                p = _axpy(o, t, v)
                if p[1] < self.h:
                    continue
                r = mp.sqrt(p[0] ** 2 + p[2] ** 2)
                out.append(dict(t=t, piece="cap", n=_scale(1 / self.R, p), kappa=1 / self.R, f3=3 / self.R ** 2, S=float(self.R), central=bool(r < 1e-6),
                                exact_leaf=True, edge_dist=mp.sqrt((r - self.w) ** 2 + (p[1] - self.h) ** 2)))
        if v[1] != 0:
            t = (self.h - o[1]) / v[1]
            p = _axpy(o, t, v)
            r = mp.sqrt(p[0] ** 2 + p[2] ** 2)
            if r <= self.w:
                out.append(dict(t=t, piece="cut", n=[mp.mpf(0), mp.mpf(-1), mp.mpf(0)], kappa=mp.mpf(0), f3=mp.mpf(0), S=self.size, central=True,
                                exact_leaf=True, edge_dist=self.w - r))
        return sorted(out, key=lambda h: h["t"])


@_precise
class ExactCylinder(_Solid):
    """Lens(CylinderSDF(radius, height), n) (PrimitiveSDF.jl:53-76): d = abs(norm(x, z), y) - (radius, height), so `height` is the HALF height:
    the solid is norm(x, z) <= radius, |y| <= height, centred on the position, its axis the local y.  min(max(d), 0) + norm(max(d, 0)) is
    the exact distance on both sides (exact_leaf); the norm of a zero vector in it has NaN partials, so barrel and end caps alike may take
    central-difference normals: the bound carries both rules on every face."""

    kind = "lens"

    def __init__(self, radius, height, n, position, orientation, planted=None):
        super().__init__(position, orientation)
        self.r, self.hh, self.n = _f(radius), _f(height), n
        self.ax = 0 if planted == "cylinder_axis_x" else 1
        self.size = float(2 * max(self.r, self.hh))
        assert self.size < 0.5

    index, index_tol = ExactLens.index, ExactLens.index_tol

    def crossings(self, o, v):
        mp = _mp()
        ax = self.ax
        j, k = [i for i in range(3) if i != ax]
        out = []
        a = v[j] ** 2 + v[k] ** 2
        if a != 0:
            b, c = o[j] * v[j] + o[k] * v[k], o[j] ** 2 + o[k] ** 2 - self.r ** 2
            disc = b * b - a * c
            if disc > 0:
                for t in ((-b - mp.sqrt(disc)) / a, (-b + mp.sqrt(disc)) / a):
                    p = _axpy(o, t, v)
                    if abs(p[ax]) <= self.hh:
                        nrm = [mp.mpf(0)] * 3
                        nrm[j], nrm[k] = p[j] / self.r, p[k] / self.r
                        out.append(dict(t=t, piece="barrel", n=nrm, kappa=1 / self.r, f3=3 / self.r ** 2, S=float(self.r), central=True, exact_leaf=True,
                                        edge_dist=self.hh - abs(p[ax])))
        if v[ax] != 0:
            for sgn in (-1, 1):
                t = (sgn * self.hh - o[ax]) / v[ax]
                p = _axpy(o, t, v)
                rho = mp.sqrt(p[j] ** 2 + p[k] ** 2)
                if rho <= self.r:
                    nrm = [mp.mpf(0)] * 3
                    nrm[ax] = mp.mpf(sgn)
                    out.append(dict(t=t, piece="end" + "-+"[sgn > 0], n=nrm, kappa=mp.mpf(0), f3=mp.mpf(0), S=self.size, central=True, exact_leaf=True,
                                    edge_dist=self.r - rho))
        return sorted(out, key=lambda h: h["t"])


def sellmeier(B1, B2, B3, C1, C2, C3, planted=None):
    """SellmeierEquation(B1, B2, B3, C1, C2, C3) (RefractiveIndexUtils.jl:82-98): n(lambda) = sqrt(1 + sum_i B_i x^2 / (x^2 - C_i)), x the
    wavelength in MICROMETRES (lambda 1e6; 10^6 is a double), evaluated at the working precision from the six coefficient doubles.
    The host evaluates the same expression in doubles and hands the result to every trace; `roundings` is the count k of roundings of that
    expression, so that the recorded index lies within k u of this one, relative:
        x = lambda 1e6                      1
        x^2 (a power function of libm: faithful, counted as 2)      2
        per term: the product B x^2, the difference x^2 - C, the quotient      3 x 3 = 9
        the three sums 1 + . + . + .        3
        the root                            1        k = 16
    Every rounding is counted at its full size on n.  That is an upper bound: the root halves what precedes it, no difference cancels
    (x^2 - C_1, x^2 - C_2 > 0.8 x^2 above 0.3 um and |x^2 - C_3| > 96 for fused silica, so x's error is carried on, not amplified), and the
    terms are positive or below 0.01.  planted 'sellmeier_metres': the wavelength put into the formula in metres."""
    coef = [float(c) for c in (B1, B2, B3, C1, C2, C3)]

    def n(lam):
        mp = _mp()
        x = _f(lam) * (1 if planted == "sellmeier_metres" else 10 ** 6)
        x2 = x * x
        return mp.sqrt(1 + sum(_f(B) * x2 / (x2 - _f(C)) for B, C in zip(coef[:3], coef[3:])))

    n.roundings = 16
    return n


@_precise
class ExactDoublet:
    """SphericalDoubletLens(r1, r2, r3, l1, l2, d, n1, n2) (DoubletLenses.jl:57-64): two lenses that share the surface r2, the back one moved
    along the axis by the front one's thickness; position() / orientation() are the front lens's (:35-36).  The two parts are hit as shapes
    of their own (AbstractRay.jl:130-155) and each refracts as its own Lens (DoubletLenses.jl:66-76): the interface is crossed ONCE, on
    the part the hint names (the back shape after a front hit and the other way round), with n1 = the ray's own index."""

    kind = "doublet"

    def __init__(self, r1, r2, r3, l1, l2, diameter, n1, n2, position, orientation, planted=None):
        o = np.asarray(orientation, dtype=np.float64).reshape(3, 3)
        back_pos = _axpy(_v(position), _f(l1), _v(o[:, 1]))
        self.parts = [ExactLens(Surface(r1), Surface(r2), l1, diameter, n1, position, orientation, planted),
                      ExactLens(Surface(r2), Surface(r3), l2, diameter, n2, back_pos, orientation, planted)]


@_precise
class ExactFlat(_Solid):
    """A flat square mesh of width w (Mesh.jl:282-310) at a pose: a detector (kind 'psf' / 'spot'), an IntersectableObject ('stop'), a plane
    mirror ('mirror', Mirrors.jl:93-96) or a thin splitter ('thin_bs' with its reflectance, ThinBeamsplitter.jl:43-51)."""

    def __init__(self, width, position, orientation, kind="psf", reflectance=None, height=None, pre=None, sides=None, n=None, jones=None, cutoff=None):
        """height: a RectangularFlatMesh(width, height) (x by z, Mesh.jl:282-303).  pre: the mesh was turned about z by that double angle and
        made its own origin (set_new_origin3d!, Mesh.jl:170-174) before the pose applied.  sides: a CircularFlatMesh of diameter `width`
        (Mesh.jl:322-348): a regular polygon of that many sides inscribed in the circle, normal -y; what lies between the polygon's inscribed
        circle and the circle is a seam.  n, jones, cutoff: the glass behind a plate's or cube's coating, a filter's Jones matrix and cutoff."""
        super().__init__(position, orientation, pre)
        self.kind, self.w, self.reflectance = kind, _f(width), reflectance
        self.h = self.w if height is None else _f(height)
        self.sides, self.n, self.jones, self.cutoff = sides, n, jones, cutoff
        self.size = float(max(self.w, self.h))

    index = ExactLens.index

    def crossings(self, o, v):
        mp = _mp()
        if v[1] == 0:
            return []
        t = -o[1] / v[1]
        p = _axpy(o, t, v)
        if self.sides is not None:
            r, R = mp.sqrt(p[0] ** 2 + p[2] ** 2), self.w / 2
            if r > R:
                return []
            return [dict(t=t, piece="mesh", n=[mp.mpf(0), mp.mpf(-1), mp.mpf(0)], kappa=mp.mpf(0), f3=mp.mpf(0), S=float(self.w), central=False, exact_leaf=True,
                         edge_dist=max(R * mp.cos(mp.pi / self.sides) - r, 0),
                         # the world vertices are doubles, re-rounded by every kinematic step (2 u M each, four steps at the most here: 8 u M,
                         # M = |position| + R); a triangle of the polygon is a sliver whose smallest altitude is R sin(2 pi / sides), and its
                         # normal turns by 2 (vertex error) / altitude
                         dn_vertices=16 * mp.mpf(U) * (self.pos_mag + R) / (R * mp.sin(2 * mp.pi / self.sides)))]
        hx, hz = self.w / 2, self.h / 2
        if abs(p[0]) > hx or abs(p[2]) > hz:
            return []
        diag = abs(p[0] + p[2]) / mp.sqrt(2)  # the seam between the two triangles (vertices 2 and 4, Mesh.jl:286-295) is no seam of the SURFACE
        return [dict(t=t, piece="mesh", n=[mp.mpf(0), mp.mpf(1), mp.mpf(0)], kappa=mp.mpf(0), f3=mp.mpf(0), S=self.size, central=False, exact_leaf=True,
                     edge_dist=min(hx - abs(p[0]), hz - abs(p[2])), diag=diag)]


@_precise
class ExactMesh(_Solid):
    """A triangle mesh given by its faces' vertices in the mesh frame (world = position + orientation local): every triangle is its plane with
    an exact barycentric inclusion test; the normal follows the right-hand rule of the vertex order (Mesh.jl:183-192) and is NOT turned
    towards the ray.  RetroMesh(scale): the three faces of a cube corner (Misc.jl:8-22)."""

    def __init__(self, faces, position, orientation, kind="mirror", n=None):
        super().__init__(position, orientation)
        self.kind, self.n = kind, n  # kind 'lens' with n(lambda): a mesh of glass, Lens(mesh, n)
        self.faces = [[_v(p) for p in f] for f in faces]
        self.size = float(max(abs(x) for f in faces for p in f for x in p))

    @classmethod
    def retro(cls, scale, position, orientation):
        v = [[0, 0, 0], [scale, 0, 0], [0, scale, 0], [0, 0, scale]]
        return cls([[v[i - 1] for i in f] for f in ((1, 3, 2), (1, 4, 3), (1, 2, 4))], position, orientation, "mirror")

    @classmethod
    def cuboid(cls, x, y, z, theta, shift, position, orientation, n, kind="lens", steps=0):
        """Lens(CuboidMesh(x, y, z, theta), n) (Mesh.jl:362-395) whose vertices were moved by `shift` before set_new_origin3d made that the mesh
        frame: a parallelepiped sheared along x by cos(theta) y - the Fresnel rhomb of the reference's test.  cos of the DOUBLE theta, in mpmath.
        kind 'mirror', theta = the double of pi / 2, shift = (-x / 2, 0, -z / 2): RectangularPlanoMirror(x, z, y) (Mirrors.jl:110-119).
        steps: the kinematic steps that re-rounded the vertices - the builder's translation and every move of the pose (Mesh.jl:78-96 rewrites
        the vertex table each time) - for the bound of the module docstring; 0: vertices and pose small against the faces (the rhomb)."""
        mp = _mp()
        dx = mp.cos(_f(theta)) * _f(y)
        x, y, z = _f(x), _f(y), _f(z)
        v = [[0, 0, 0], [x, 0, 0], [x + dx, y, 0], [dx, y, 0], [dx, y, z], [x + dx, y, z], [x, 0, z], [0, 0, z]]
        v = [_add([_f(q) if not isinstance(q, mp.mpf) else q for q in p], _v(shift)) for p in v]
        f = ((1, 3, 2), (1, 4, 3), (3, 4, 5), (3, 5, 6), (2, 3, 6), (2, 6, 7), (1, 8, 5), (1, 5, 4), (6, 5, 8), (6, 8, 7), (1, 7, 8), (1, 2, 7))
        obj = cls([[[0, 0, 0]] * 3], position, orientation, kind, n)
        obj.faces = [[v[i - 1] for i in face] for face in f]
        obj.size = float(max(abs(q) for p in v for q in p))
        obj.steps = steps
        return obj

    index = ExactLens.index
    steps = 0

    def _inner_edge(self, fid, e):
        """Whether the edge between vertices e of face fid is shared with another face in the same plane."""
        f = self.faces[fid]
        pair = [f[e[0]], f[e[1]]]
        n0 = _cross(_sub(f[1], f[0]), _sub(f[2], f[0]))
        for gid, g in enumerate(self.faces):
            if gid != fid and all(any(_norm(_sub(p, q)) == 0 for q in g) for p in pair):
                if _norm(_cross(n0, _cross(_sub(g[1], g[0]), _sub(g[2], g[0])))) == 0:
                    return True
        return False

    def crossings(self, o, v):
        mp = _mp()
        out = []
        for fid, (a, b, c) in enumerate(self.faces):
            e1, e2 = _sub(b, a), _sub(c, a)
            nrm = _cross(e1, e2)
            den = _dot(nrm, v)
            if den == 0 or _norm(nrm) == 0:
                continue
            t = _dot(nrm, _sub(a, o)) / den
            w = _sub(_axpy(o, t, v), a)
            d11, d12, d22, w1, w2 = _dot(e1, e1), _dot(e1, e2), _dot(e2, e2), _dot(w, e1), _dot(w, e2)
            det = d11 * d22 - d12 * d12
            bu, bv = (d22 * w1 - d12 * w2) / det, (d11 * w2 - d12 * w1) / det
            if bu < 0 or bv < 0 or bu + bv > 1:
                continue
            area2 = _norm(nrm)
            # distances to the three edges; an edge shared with a coplanar neighbour (the diagonal of a quad) is no seam of the surface
            dist = {(0, 1): bv * area2 / _norm(e1), (0, 2): bu * area2 / _norm(e2), (1, 2): (1 - bu - bv) * area2 / _norm(_sub(c, b))}
            edge = min([d for e, d in dist.items() if not self._inner_edge(fid, e)] or [mp.inf])
            out.append(dict(t=t, piece="mesh", face=fid, n=_scale(1 / area2, nrm), kappa=mp.mpf(0), f3=mp.mpf(0), S=self.size, central=False,
                            exact_leaf=True, edge_dist=edge))
            if self.steps:
                # the doubles of the world vertices, re-rounded by every kinematic step (module docstring, 'mesh vertices'): each vertex within
                # dv of its exact place; the face's plane moves by dv and turns by 2 dv / (its smallest altitude), which moves a hit up to
                # `size` from a vertex by 2 dv size / altitude more
                dv = 18 * mp.mpf(U) * (self.pos_mag + self.size) * self.steps
                alt = area2 / max(_norm(e1), _norm(e2), _norm(_sub(c, b)))
                out[-1].update(dn_vertices=2 * dv / alt, dt_vertices=dv * (1 + 2 * self.size / alt))
        return sorted(out, key=lambda h: h["t"])


@_precise
class ExactPlateBS:
    """RectangularPlateBeamsplitter(width, height, thickness, n; reflectance) / RoundPlateBeamsplitter(diameter, thickness, n; reflectance)
    (PlateBeamsplitter.jl:89-104, :146-158): parts = [substrate, coating].  position() is the coating's, orientation() the substrate's (:38-40):
    both parts are derived from these two alone.  The rectangular substrate is BoxSDF(width, thickness, height) centred thickness / 2 behind
    the coating along the plate's +y; the round one PlanoSurfaceSDF(thickness, diameter), the cylinder 0 <= y <= thickness (a lens of two
    flat faces).  The coating is a flat mesh at the position whose normal is the plate's -y (turned by the double pi about z; the round one
    is built that way).  The exact faces of substrate and coating coincide by construction, like the parts of a doublet."""

    kind = "plate_bs"

    def __init__(self, width, height, thickness, n, reflectance, position, orientation, round_=False):
        o = np.asarray(orientation, dtype=np.float64).reshape(3, 3)
        if round_:
            sub = ExactLens(Surface(math.inf), Surface(math.inf), thickness, width, n, position, orientation)
            coat = ExactFlat(width, position, orientation, "plate_coating", reflectance, sides=30, n=n)
        else:
            centre = _axpy(_v(position), _f(thickness) / 2, _v(o[:, 1]))
            sub = ExactBox(width, thickness, height, n, centre, orientation)
            coat = ExactFlat(width, position, orientation, "plate_coating", reflectance, height=height, pre=math.pi, n=n)
        self.parts = [sub, coat]


@_precise
class ExactCubeBS:
    """CubeBeamsplitter(leg, n; reflectance) (CubeBeamsplitter.jl:49-61): parts = [front, back, coating], two RightAnglePrism(leg, leg, n) on
    one position, the back one turned by the double deg2rad(180) about z, and a ThinBeamsplitter(sqrt(2) leg, leg) turned by the double
    deg2rad(135) about z and made its own origin: its plane is the two prisms' common hypotenuse x + y = 0, its normal (-1, -1, 0) / sqrt(2)
    points into the front prism.  position() / orientation() are the front prism's."""

    kind = "cube_bs"

    def __init__(self, leg, n, reflectance, position, orientation):
        mp = _mp()
        self.parts = [ExactPrism(leg, leg, n, position, orientation), ExactPrism(leg, leg, n, position, orientation, pre=math.radians(180)),
                      ExactFlat(mp.sqrt(2) * _f(leg), position, orientation, "cube_coating", reflectance, height=leg, pre=math.radians(180 - 45), n=n)]


# ------------------------------------------------------------------------------------------------ the hit
def exact_hit(obj, pos, dirv, consts):
    """The reference's intersect3d(obj, ray) in exact arithmetic -> None or dict(t, piece, n (world, outward), cos (dir . n), kappa, ...,
    leaving, seam: the distance of the hit to the nearest seam or aperture edge, t_run: the length the march that found it ran)."""
    mp = _mp()
    o, v = obj.to_local(pos), obj.vec_local(dirv)
    cr = obj.crossings(o, v)
    if not cr:
        return None
    if isinstance(obj, (ExactFlat, ExactMesh)):
        ahead = [h for h in cr if h["t"] >= consts["mt_leps"]]               # Mesh.jl:233, :251-259: the nearest face in front
        if not ahead:
            return None
        hit, leaving = ahead[0], False
    else:
        eps_srf = mp.mpf(consts["eps_srf"])
        near = [h for h in cr if abs(h["t"] * _dot(v, h["n"])) <= eps_srf]  # the start lies on the boundary (sdf <= eps_srf, first order)
        ahead = [h for h in cr if h["t"] > 0]
        if near:
            h0 = min(near, key=lambda h: abs(h["t"]))
            inside = _dot(v, h0["n"]) <= 0
            if not inside:
                return None                                                  # AbstractSDF.jl:175-180
            cand = [h for h in cr if h["t"] > h0["t"] and h is not h0]
        else:
            inside = len(ahead) % 2 == 1
            cand = ahead
        if not cand:
            return None
        if inside:
            assert cand[-1]["t"] < consts["eps_ins"]
            hit, leaving = cand[-1], True                                    # AbstractSDF.jl:142-153: the first 1 m step is outside, march back
        else:
            hit, leaving = cand[0], False
    out = dict(hit)
    out["n"] = _unit(obj.vec_world(hit["n"]))  # normalize(gradient), AbstractSDF.jl:91: the orientation's columns are unit vectors to u only
    out["cos"] = _dot(dirv, out["n"])
    out["leaving"] = leaving
    out["t_run"] = (mp.mpf(consts["eps_ins"]) - hit["t"]) if leaving else hit["t"]
    out["seam"] = hit["edge_dist"]
    out["point"] = _axpy(pos, hit["t"], dirv)
    out["others"] = [h["t"] for h in cr if h is not hit]
    return out


# ------------------------------------------------------------------------------------------------ the interaction
def _parallel(a, b):
    return abs(abs(_dot(_unit(a), _unit(b))) - 1) <= 2.0 ** -52             # LinearAlgebraUtils.jl:6-8: isapprox(., 1, atol = eps())


def fresnel(cos_i, n):
    """fresnel_coefficients(theta, n) OpticUtils.jl:121-131 from cos(theta): sin^2 = 1 - cos^2, the principal root."""
    mp = _mp()
    s2 = 1 - cos_i * cos_i
    g = mp.sqrt(mp.mpc(n * n - s2))
    rs = (cos_i - g) / (cos_i + g)
    rp = (-n * n * cos_i + g) / (n * n * cos_i + g)
    return rs, rp, rs + 1, 2 * n * cos_i / (n * n * cos_i + g), s2


def jones_global(d_in, d_out, normal, j11, j22, E0):
    """_calculate_global_E0 PolarizedRays.jl:165-207: O_out diag(j11, j22, 1) O_in E0."""
    par = _parallel(d_in, d_out)
    v = normal if par else d_out
    if _parallel(d_in, normal):
        v = _tangents(_unit(d_in))[0]                                        # normal3d(in_dir): any perpendicular (:173-176)
    s = _unit(_cross(d_in, v))
    p1 = _cross(d_in, s)
    if par and not _norm(_add(d_in, d_out)) <= _mp().sqrt(2.0 ** -52) * max(_norm(d_in), _norm(d_out)):
        p2, d3 = p1, d_in                                                    # :184-185
    else:
        p2, d3 = _cross(d_out, s), d_out
    a, b, c = j11 * _dot(s, E0), j22 * _dot(p1, E0), _dot(d_in, E0)
    return [s[i] * a + p2[i] * b + d3[i] * c for i in range(3)], _norm(_cross(d_in, d_out))


def interact_lens(dirv, normal, n_ray, n_glass, E0=None, planted=None):
    """interact3d(system, ::AbstractRefractiveOptic, beam, ray) Lenses.jl:46-126 -> dict(dir, n, E0, tir, ...)."""
    mp = _mp()
    entering = _dot(dirv, normal) < 0                                        # AbstractRay.jl:234-237
    if entering:
        n1, n2, nf = n_ray, n_glass, normal
    else:
        n1, n2 = n_glass, (n_glass if planted == "n2_glass_on_exit" else mp.mpf(1))
        nf = normal if planted == "exit_normal_not_flipped" else _scale(-1, normal)
    cos_i = -_dot(nf, dirv)
    out = dict(entering=entering, cos_i=cos_i, n1=n1)
    if planted == VIA_AIR and entering and n1 != 1 and E0 is None:          # glass -> air -> glass across a gap of zero width
        first = interact_lens(dirv, _scale(-1, normal), n1, n1)              # leaves the front glass into air (or is reflected there)
        if first["tir"]:
            out.update(dir=first["dir"], n=n1, tir=True)
            return out
        second = interact_lens(first["dir"], normal, mp.mpf(1), n_glass)
        out.update(dir=second["dir"], n=second["n"], tir=second["tir"])
        return out
    if E0 is None:
        eta = n1 / n2                                                        # OpticUtils.jl:31-45
        st2 = eta * eta * (1 - cos_i * cos_i)
        tir = st2 > 1
        if tir:
            nd = _sub(dirv, _scale(2 * _dot(dirv, nf), nf))
        else:
            nd = _add(_scale(eta, dirv), _scale(eta * cos_i - mp.sqrt(1 - st2), nf))
    else:
        ci = max(-1, min(1, cos_i))                                          # angle3d clamps; cos(acos(x)) = x
        rs, rp, ts, tp, s2 = fresnel(ci, n2 / n1)
        if planted == "ts_tp_swapped":
            ts, tp = tp, ts
        tir = abs(abs(rs) ** 2 - 1) <= 1e-6 and abs(abs(rp) ** 2 - 1) <= 1e-6  # OpticUtils.jl:144-146
        if tir:
            nd = _sub(dirv, _scale(2 * _dot(dirv, nf), nf))
            j11, j22 = -rs, rp
            if planted == "tir_phase_conjugated":
                j11, j22 = mp.conj(j11), mp.conj(j22)
        else:
            eta = n1 / n2
            st2 = eta * eta * (1 - cos_i * cos_i)
            nd = _sub(dirv, _scale(2 * _dot(dirv, nf), nf)) if st2 > 1 else _add(_scale(eta, dirv), _scale(eta * cos_i - mp.sqrt(1 - st2), nf))
            j11, j22 = ts, tp
        out["E0"], out["sin_dev"] = jones_global(dirv, nd, normal, j11, j22, E0)
        nn = (n2 / n1) ** 2
        out.update(j11=j11, j22=j22, X=(nn + s2) / abs(nn - s2))
    if tir:
        n2 = n_glass
    out.update(dir=nd, n=n2, tir=tir)
    return out


def interact_mirror(dirv, normal, n_ray, E0=None):
    """interact3d(system, ::AbstractReflectiveOptic, beam, ray) Mirrors.jl:39-69: reflection3d, the index stays, J = diag(-1, 1)."""
    mp = _mp()
    nd = _sub(dirv, _scale(2 * _dot(dirv, normal), normal))
    out = dict(role="next", dir=nd, n=n_ray, tir=True, rnd_dir=8, E0=None)
    if E0 is not None:
        out["E0"], out["sin_dev"] = jones_global(dirv, nd, normal, mp.mpf(-1), mp.mpf(1), E0)
        out.update(j11=mp.mpf(-1), j22=mp.mpf(1), j_rnd=0)
    return out


def interact_thin_bs(obj, dirv, normal, E0=None):
    """interact3d(system, ::ThinBeamsplitter, beam, ray) ThinBeamsplitter.jl:73-115: the transmitted child keeps the direction, the reflected one
    takes reflection3d; both are NEW rays in n = 1 (Ray(pos, dir, lambda), Rays.jl).  R = sqrt(reflectance), T = sqrt(1 - R^2) (:43-51);
    PolarizedRay: J = diag(T, T) and diag(-R, R)."""
    mp = _mp()
    R = mp.sqrt(_f(obj.reflectance))
    T = mp.sqrt(1 - R * R)
    nd = _sub(dirv, _scale(2 * _dot(dirv, normal), normal))
    # Ray(...) and PolarizedRay(...) normalise dir (Rays.jl:32-42, PolarizedRays.jl:80-95): 4 u, which shows where the parent's direction is a
    # refracted one whose length is 1 to a few u only (inside a cube splitter); a root's direction is returned unchanged
    outs = [dict(role="transmitted", dir=dirv, n=mp.mpf(1), tir=False, rnd_dir=4, E0=None),
            dict(role="reflected", dir=nd, n=mp.mpf(1), tir=True, rnd_dir=12, E0=None)]
    if E0 is not None:
        for o, (a, b) in zip(outs, ((T, T), (-R, R))):
            o["E0"], o["sin_dev"] = jones_global(dirv, o["dir"], normal, a, b, E0)
            o.update(j11=a, j22=b, j_rnd=4)  # the doubles of R and T: a root, a product, a difference, a root
    for o in outs:
        o["dir"] = _unit(o["dir"])           # the constructor's normalize, after E0 was made from the directions as they were
    return outs


def interact_plate_coating(obj, dirv, normal, n_ray, lam, E0=None, planted=None, chief_entering=None):
    """interact3d(system, ::AbstractPlateBeamsplitter, beam, ray) at the coating, PlateBeamsplitter.jl:203-225: the thin splitter's children,
    then the transmitted child's direction is replaced by refraction3d(ray, n2) (AbstractRay.jl:244-253: n1 the ray's own index, the normal
    flipped when the ray is not entering), n2 = n_optics entering, 1 leaving; the children's indices are (n_optics, 1) or (1, n_optics).  The
    transmitted child's E0 stays the thin splitter's, that of the straight-through direction (:221-223 set index and direction alone).
    chief_entering: a beamlet's waist and divergence ray take the indices by the CHIEF ray's isentering (:250-264) and flip the normal by
    their own."""
    mp = _mp()
    outs = interact_thin_bs(obj, dirv, normal, E0)
    entering = _dot(dirv, normal) < 0                                        # AbstractRay.jl:234-237
    ent_n = entering if chief_entering is None else chief_entering
    n_opt, one = obj.index(lam), mp.mpf(1)
    nt, nr = (n_opt, one) if ent_n else (one, n_opt)
    if planted == "plate_indices_swapped":
        nt, nr = nr, nt
    nf = normal if (entering or planted == "plate_normal_not_flipped") else _scale(-1, normal)
    eta = n_ray / (n_opt if ent_n else one)                                  # OpticUtils.jl:31-45
    cos_i = -_dot(nf, dirv)
    st2 = eta * eta * (1 - cos_i * cos_i)
    if st2 > 1:
        nd = _sub(dirv, _scale(2 * _dot(dirv, nf), nf))
    else:
        nd = _add(_scale(eta, dirv), _scale(eta * cos_i - mp.sqrt(1 - st2), nf))
    if planted != "plate_no_refraction":
        outs[0].update(dir=_unit(nd), rnd_dir=18)                            # direction! normalises (AbstractRay.jl:83-86)
    outs[0]["n"], outs[1]["n"] = nt, nr
    return outs


def interact_cube_coating(obj, dirv, normal, lam, E0=None, planted=None):
    """interact3d(system, ::CubeBeamsplitter, beam, ray) at the coating, CubeBeamsplitter.jl:76-84: the thin splitter's children, both in glass."""
    outs = interact_thin_bs(obj, dirv, normal, E0)
    if planted != "cube_children_in_air":
        outs[0]["n"] = outs[1]["n"] = obj.index(lam)
    return outs


def interact_polarizer(obj, dirv, n_ray, E0, planted=None):
    """interact3d(system, ::PolarizationFilter, beam, ray) PolarizationFilter.jl:31-48 with _calculate_global_E0 JonesCalculus.jl:29-45:
    E' = Q (R J R^T) Q E0, R = orientation(filter) (its doubles), Q = I - d d^T; direction and index are kept; the ray is blocked when
    norm(E') is approximately the cutoff (isapprox: |a - b| <= sqrt(eps) max(|a|, |b|))."""
    mp = _mp()
    R = [[obj.cols[k][i] for k in range(3)] for i in range(3)]               # R[i][k]: component i of local axis k
    if planted == "polarizer_rotation_transposed":
        R = [[R[k][i] for k in range(3)] for i in range(3)]
    J = [[mp.mpc(complex(z).real, complex(z).imag) for z in row] for row in obj.jones]
    mul = lambda A, B: [[sum(A[i][k] * B[k][j] for k in range(3)) for j in range(3)] for i in range(3)]
    P = mul(mul(R, J), [[R[j][i] for j in range(3)] for i in range(3)])
    if planted != "polarizer_not_projected":
        Q = [[(1 if i == j else 0) - dirv[i] * dirv[j] for j in range(3)] for i in range(3)]
        P = mul(mul(Q, P), Q)
    E = [sum(P[i][j] * E0[j] for j in range(3)) for i in range(3)]
    nrm, cut = _norm(E), _f(obj.cutoff)
    out = dict(role="next", dir=dirv, n=n_ray, tir=False, entering=False, rnd_dir=0, E0=E, norm=nrm, j11=mp.mpf(1), j22=mp.mpf(1), sin_dev=mp.mpf(0), j_rnd=0)
    # four 3 x 3 products and a matrix-vector product, 3 u of |A| |B| each; Q's entries carry 2 u, twice; the moduli of Q, R, R^T, Q have
    # 2-norms up to sqrt(3) each: (4 3 + 3 + 2 2) 9 u of |J| |E0|
    out["E_rnd"] = 171 * max(abs(z) for row in J for z in row)
    out["blocked"] = abs(nrm - cut) <= mp.sqrt(2.0 ** -52) * max(nrm, cut)
    # how far the outcome is from turning over, less what the recorded norm may be off: E0's bound and 4 u for the norm (three squares, two
    # sums, a root).  Negative: the one outcome this evaluator does not predict (excluded())
    out["block_margin"] = abs(abs(nrm - cut) - mp.sqrt(2.0 ** -52) * max(nrm, cut)) - _norm(E0) * mp.mpf(U) * (out["E_rnd"] + 4)
    return [out]


def gauss_record(res, node):
    """Beamlet `node` of a TraceResult as the record tests/pd_ref.py evaluates (its doubles): the three rays of every segment that ends on an
    object, the (length, index) of every ray of every ancestor, beam_waist, E0 and lambda of node_aux."""
    c, w, d = (segments_of(res, node, s) for s in range(3))
    segs = [dict(pos=a["pos"], dir=a["dir"], n=a["n"], t=a["t"], wpos=b["pos"], wdir=b["dir"], dpos=e["pos"], ddir=e["dir"])
            for a, b, e in zip(c, w, d) if math.isfinite(a["t"])]
    parents, p = [], int(res.node_parent[node])
    while p >= 0:
        parents.append([(s["t"], s["n"]) for s in segments_of(res, p) if math.isfinite(s["t"])])
        p = int(res.node_parent[p])
    aux = res.node_aux[node]
    return dict(segs=segs, parents=parents, w0=float(aux[0]), E0=complex(aux[1], aux[2]), lam=float(aux[3]), proj=1.0)


def exact_gauss_children(rec, splitter, facing, planted=None):
    """What a splitter's coating makes of a GaussianBeamlet beyond its three rays (ThinBeamsplitter.jl:117-168), rec = gauss_record(parent):
    both children's w0 = gauss_parameters(gauss, length(gauss))[4] - the waist the beamlet has taken on where it is split, the parents' lengths
    included (Beam.jl:177-205) -, E_t = T E0 (w0_g / w0), E_r = R E0 (w0_g / w0) exp(i phi) with phi = pi where the chief ray faces the normal
    (dot(dir, normal) < 0: `facing`) and 0 where not; pi is pi, so exp(i pi) = -1.  -> dict(w0, E_t, E_r and their bounds b_w0, b_E): the
    bound of w0 is pd_ref's (waist_at); E takes w0's relative bound, 4 u for the doubles of R and T, 6 u for two products and a quotient of
    a complex number, and - reflected with phi = pi - |sin(fl(pi))| = 1.3e-16, the imaginary part the double of pi leaves in the factor."""
    import pd_ref

    mp = _mp()
    bl = pd_ref._Beamlet(rec, None)
    w0, b_w0 = bl.waist_at(bl.length)
    if planted == "gauss_child_keeps_w0":
        w0 = bl.w0
    elif planted == "gauss_w0_at_start":  # on the beam's first ray (halfway along it: at its very start the divergence ray has no height)
        w0 = bl.waist_at(bl.l_parent + bl.segs[0]["t"] / 2)[0]
    R = mp.sqrt(_f(splitter.reflectance))
    T = mp.sqrt(1 - R * R)
    flip = {None: facing, "gauss_no_phase_flip": False, "gauss_flip_on_both_sides": True}.get(planted, facing)
    E_t = T * bl.E0 * (bl.w0 / w0)
    E_r = R * bl.E0 * (bl.w0 / w0) * (-1 if flip else 1)
    rel = b_w0 / w0 + 10 * mp.mpf(U)
    return dict(w0=w0, E_t=E_t, E_r=E_r, b_w0=b_w0, b_E=[abs(E_t) * rel, abs(E_r) * (rel + (mp.mpf("1.3e-16") if facing else 0))], flip=flip)


ORTHO_ATOL = 1e-14


def _not_orthogonal(dirv, E0):
    """The check of the PolarizedRay constructor, PolarizedRays.jl:54-56: isorthogonal3d(dir, E0; atol = 1e-14) (LinearAlgebraUtils.jl:15-17)."""
    return E0 is not None and abs(_dot(dirv, E0)) > _f(ORTHO_ATOL)


def interact(obj, dirv, normal, n_ray, lam, E0=None, planted=None, chief_entering=None):
    """The rays that leave the bounce: [] on a detector or a stop, one 'next' ray on a lens, a mirror or a polarization filter, two children on a
    splitter's coating.  Where the reference would build a PolarizedRay whose E0 is not orthogonal to its direction the constructor throws
    (PolarizedRays.jl:54-56): one entry of role 'err_ortho'; a filter that blocks the ray: one of role 'blocked'."""
    outs = []
    if obj.kind == "lens":
        ia = interact_lens(dirv, normal, n_ray, obj.index(lam), E0, planted)
        ia.update(role="next", rnd_dir=8 if ia["tir"] else 14)
        if E0 is not None:
            ia["j_rnd"] = 16 + 6 * ia["X"]
        else:
            ia["E0"] = None
        outs = [ia]
    elif obj.kind == "mirror":
        outs = [interact_mirror(dirv, normal, n_ray, E0)]
    elif obj.kind == "thin_bs":
        outs = interact_thin_bs(obj, dirv, normal, E0)
    elif obj.kind == "plate_coating":
        plain = interact_thin_bs(obj, dirv, normal, E0)                     # the constructor's check runs on the thin splitter's children, :205
        if any(_not_orthogonal(o["dir"], o["E0"]) for o in plain):
            return [dict(role="err_ortho")]
        return interact_plate_coating(obj, dirv, normal, n_ray, lam, E0, planted, chief_entering)
    elif obj.kind == "cube_coating":
        outs = interact_cube_coating(obj, dirv, normal, lam, E0, planted)
    elif obj.kind == "polarizer" and E0 is not None:                        # no method for a Ray or a beamlet: they stop (Intersectable.jl:15)
        outs = interact_polarizer(obj, dirv, n_ray, E0, planted)
        if outs[0]["blocked"]:
            return [dict(role="blocked", norm=outs[0]["norm"], block_margin=outs[0]["block_margin"])]
    if planted != "polarizer_not_projected" and any(_not_orthogonal(o["dir"], o["E0"]) for o in outs):  # (that mistake is to show in E0)
        return [dict(role="err_ortho")]
    return outs


# ------------------------------------------------------------------------------------------------ one bounce
def exact_step(seg, obj, consts, planted=None):
    """One recorded segment seg = dict(pos, dir, n, lam[, E0][, opl]) (the exact values of its doubles) against the object the record says was
    hit -> None (no hit) or dict(t, point, normal, hit, outs (the rays that leave: dict(role, pos, dir, n, E0)), next (outs[0] where the beam
    goes on, else None), children (the two outs of a splitter, else None), opl, row)."""
    mp = _mp()
    pos, dirv = _v(seg["pos"]), _v(seg["dir"])
    hit = exact_hit(obj, pos, dirv, consts)
    if hit is None:
        return None
    n_ray = _f(seg["n"])
    out = dict(t=hit["t"], point=hit["point"], normal=hit["n"], hit=hit, next=None, children=None, row=None)
    out["outs"] = interact(obj, dirv, hit["n"], n_ray, seg["lam"], _c(seg.get("E0")), planted, seg.get("chief_entering"))
    out["end"] = None  # 'err_ortho': the reference throws here (the record: BMO_NODE_ERR_ORTHO | BMO_NODE_STOPPED); 'blocked': a filter ends the ray
    if out["outs"] and out["outs"][0]["role"] in ("err_ortho", "blocked"):
        out["end"], out["ended"], out["outs"] = out["outs"][0]["role"], out["outs"][0], []
    for o in out["outs"]:
        o["pos"] = hit["point"]
    if out["outs"] and out["outs"][0]["role"] == "next":
        out["next"] = out["interaction"] = out["outs"][0]
    elif out["outs"]:
        out["children"] = out["outs"]
    n_opl = out["next"]["n"] if (planted == "opl_next_medium" and out["next"] is not None) else n_ray
    out["opl_inc"] = n_opl * hit["t"]
    out["opl"] = _f(seg.get("opl", 0.0)) + out["opl_inc"]
    if obj.kind == "psf":
        out["row"] = hit["point"] + dirv + [out["opl"], abs(_dot(dirv, hit["n"])), 2 * mp.pi / _f(seg["lam"])]  # PSFDetector.jl:77-89
    elif obj.kind == "spot":
        loc = _sub(hit["point"], obj.pos)
        out["row"] = [_dot(loc, obj.cols[0]), _dot(loc, obj.cols[2])]                                          # Spotdetector.jl:50-61
    return out


def overshoot(obj, seg, hit, consts):
    """The march that steps THROUGH an aspheric surface (module docstring, 5 b) -> (D, dt, dn): a ceiling of the depth at which it can land
    inside the glass, and of what that adds to |t - t*| and |n - n*|.  From the exact ray and the hit leaf's own formula alone:
      * outside, at the length rho before the hit along the ray, the union's sdf is at most the hit leaf's value U(rho): inside the leaf's
        aperture cylinder |y - y_v - sag(r)| / sqrt(1 + sag'(r)^2) (AsphericalLensSDF.jl:209-210; the min with the closing segments only lowers it),
        outside it at most the distance to the rim (h, edge sag) or (h, 0), whichever is larger, over m = sqrt(1 + sag'(h)^2) (:196-206, :250-258,
        :285-295).  A step of that length lands at most D = max_rho (U(rho) - rho) behind the surface; rho runs over 241 logarithmic samples from
        1e-8 m to the length of the march (1 m for a leaving hit, t* for an entering one).  D = 0: the premise 0 <= sdf(q) < eps_ray holds.
      * at the depth delta <= D the march ends with sdf = -a, t moves BACK by a: the returned point is |delta - a| from the exact hit.  Where the
        landing point lies in the leaf, nearer to the profile than to the leaf's closing plane and rim (over m), a is the leaf's value a(delta),
        second order in delta; elsewhere another sub-shape's inner distance may be the minimum, which is at most delta (the ray entered that
        sub-shape less than delta ago): then only |delta - a| <= max(delta, a(delta)) is claimed.  65 samples of delta in [0, D].
      * the central-difference normal there is that of the level set through the landing point, the profile's normal at ITS radius.
    A ceiling needs no 50 digits: the scan runs in doubles (its values are 1e-3 m and their differences 1e-9 m at the least)."""
    return _overshoot(obj, seg, hit, consts)


def _overshoot(obj, seg, hit, consts):
    g = hit["region"]
    b = g["lo"] if g["lo"][0] == "s" else g["hi"]
    other = g["hi"] if b is g["lo"] else g["lo"]
    srf, yv, h = b[1], float(b[2]), float(g["r1"])
    pl = obj.planted
    c, k = 1 / srf.radius, (-srf.conic if pl == "conic_sign" else srf.conic)
    coefs = [float(x) for x in srf.coefs]

    def profile(r2):
        """(sag, d sag / d r) at r^2 in doubles: AsphericalLensSDF.jl:133-156."""
        q = dq = 0.0
        for i in range(len(coefs), 0, -1):
            q, dq = q * r2 + coefs[i - 1], dq * r2 + i * coefs[i - 1]
        q, dq = q * r2, dq                                                   # q = sum a_i r2^i, dq = sum i a_i r2^(i - 1)
        if pl == "coef_shift":
            q, dq = q * r2, q + r2 * dq
        wq = math.sqrt(max(1 - (1 + k) * c * c * r2, 1e-12))
        r = math.sqrt(r2)
        return c * r2 / (1 + wq) + q, c * r / wq + 2 * r * dq

    o = [float(x) for x in obj.to_local(hit["point"])]
    v = [float(x) for x in obj.vec_local(_v(seg["dir"]))]
    w = v if hit["leaving"] else [-x for x in v]                            # along the ray, out of the glass
    zb, gb = profile(h * h)
    m = math.sqrt(1 + gb * gb)
    r2max = srf.r2_max()
    lim = h * h if r2max is None else min(h * h, float(r2max) * (1 - 1e-9))

    def value(p):
        r2 = p[0] * p[0] + p[2] * p[2]
        if r2 <= lim:
            z, gr = profile(r2)
            return abs(p[1] - yv - z) / math.sqrt(1 + gr * gr), gr
        r = math.sqrt(r2)
        return max(math.hypot(r - h, p[1] - yv - zb), math.hypot(r - h, p[1] - yv)) / m, gb

    far = float(consts["eps_ins"]) if hit["leaving"] else float(hit["t"])
    D = 0.0
    if far > 1e-8:
        for j in range(241):
            rho = 1e-8 * (far / 1e-8) ** (j / 240)
            D = max(D, value([o[i] + rho * w[i] for i in range(3)])[0] - rho)
    if D <= 0:
        return _f(0.0), _f(0.0), _f(0.0)
    y_of = lambda bound, r2: float(bound[1]) if bound[0] == "c" else float(bound[2]) + profile(r2)[0]
    dt = dn = 0.0
    base = None
    for j in range(65):
        delta = D * j / 64
        p = [o[i] - delta * w[i] for i in range(3)]
        r2 = p[0] * p[0] + p[2] * p[2]
        r = math.sqrt(r2)
        a, gr = value(p)
        ys = sorted((y_of(g["lo"], min(r2, lim)), y_of(g["hi"], min(r2, lim))))
        in_leaf = r2 <= lim and ys[0] <= p[1] <= ys[1]
        tight = in_leaf and a <= min(abs(p[1] - y_of(other, r2)), h - r) / m
        dt = max(dt, abs(delta - a) if tight else max(delta, a))
        nl = math.sqrt(1 + gr * gr)
        nrm = [-gr * p[0] / r / nl, 1 / nl, -gr * p[2] / r / nl] if r > 0 else [0.0, 1.0, 0.0]
        base = nrm if base is None else base
        dn = max(dn, math.sqrt(sum((x - y) ** 2 for x, y in zip(nrm, base))))
    return _f(D), _f(dt * (1 + 1e-9)), _f(dn * (1 + 1e-9) + 1e-15)


def step_bound(seg, ex, obj, consts, n_seg=1):
    """The bound of the module docstring for the bounce `ex` = exact_step(seg, obj): dict of t_lo, t_hi (bounds of t - t*), n, pos, opl_inc, opl,
    proj and outs = [dict(dir, E0)] per ray that leaves (absolute; E0: of the vector's 2-norm); dir, E0: those of outs[0].  n_seg: the
    segment's number in its beam, the ancestors' segments included (the additions of the optical path)."""
    mp = _mp()
    u = mp.mpf(U)
    hit = ex["hit"]
    t, c = hit["t"], min(abs(hit["cos"]), mp.mpf(1))  # the record's dir is a unit vector to 2 u only
    tan = mp.sqrt(1 - c * c) / c
    pos_mag = _norm(_v(seg["pos"]))
    P = max(pos_mag, _norm(hit["point"])) + (consts["eps_ins"] if hit["leaving"] else 0)
    b = {}
    if hit["piece"] == "mesh":
        M = pos_mag + obj.pos_mag + obj.size + t
        b["t_lo"] = b["t_hi"] = 32 * u * M / c + hit.get("dt_vertices", 0) / c
        dn = 8 * u + hit.get("dn_vertices", 0)
    else:
        eps, kappa = mp.mpf(consts["eps_ray"]), hit["kappa"]
        c2 = 2 * kappa * eps * (1 + tan * tan) / c
        m = hit.get("scale", mp.mpf(1))                                     # sdf = distance / m on the rim faces of a concave aspheric leaf
        gap = eps * (m / c - 1) * (1 + c2)
        t_run = hit["t_run"]
        shrink = 1 - c / m + kappa * t_run * (1 - c * c) / 2                # per step; the last term: a surface that curves towards the ray
        N = consts["march_iters"] if shrink >= 1 else (2 if shrink <= 0 else 2 + mp.ceil(mp.log(max(t_run / eps, 1)) / -mp.log(shrink)))
        N = min(N, consts["march_iters"])
        S = _norm(hit["point"]) + obj.pos_mag + hit["S"]
        rnd = u * (N * t_run + 2 * N * P * (1 + tan) + 6 * S * (1 + 1 / c)) + u * t
        b["t_lo"], b["t_hi"] = (rnd, gap + rnd) if hit["leaving"] else (gap + rnd, rnd)
        dn = kappa * eps * tan * (1 + c2) + kappa * (2 * N * u * P + 6 * u * S) + 12 * u
        if "region" in hit:  # an aspheric leaf of a lens with rings: the march may step through the surface (overshoot)
            b["depth"], b["over_t"], b["over_n"] = overshoot(obj, seg, hit, consts)
            b["t_lo"], b["t_hi"], dn = b["t_lo"] + b["over_t"], b["t_hi"] + b["over_t"], dn + b["over_n"]
        if hit["central"]:
            h = mp.mpf(consts["grad_h"])
            dn += 11 * u * S / h + h * h * hit["f3"] / 6
        b["N"] = N
    dt = max(b["t_lo"], b["t_hi"])
    b["n"] = dn
    b["proj"] = dn + 4 * u
    n_ray = _f(seg["n"])
    b["opl_inc"] = n_ray * dt + u * n_ray * t
    b["opl"] = b["opl_inc"] + (n_seg - 1) * u * ex["opl"]
    b["pos"] = dt + 2 * u * (pos_mag + t) + u * _norm(hit["point"])
    b["outs"] = []
    if ex["outs"]:
        dirv, Ein = _v(seg["dir"]), _c(seg.get("E0"))
        step = mp.mpf(2) ** -60
        D_dir, D_E = [mp.mpf(0)] * len(ex["outs"]), [mp.mpf(0)] * len(ex["outs"])
        for e in _tangents(hit["n"]):
            n2 = _axpy(hit["n"], step, e)  # its length changes in second order only
            for i, (oa, ob) in enumerate(zip(ex["outs"], interact(obj, dirv, n2, n_ray, seg["lam"], Ein, None, seg.get("chief_entering")))):
                D_dir[i] += _norm(_sub(ob["dir"], oa["dir"])) / step
                if Ein is not None:
                    D_E[i] += _norm(_sub(ob["E0"], oa["E0"])) / step
        for i, oa in enumerate(ex["outs"]):
            bo = dict(dir=D_dir[i] * dn + oa["rnd_dir"] * u, E0=None)
            if Ein is not None:
                jmax = max(abs(oa["j11"]), abs(oa["j22"]), 1)
                sd = oa["sin_dev"]
                basis = 8 * u * abs(oa["j11"] - oa["j22"]) / sd if sd > 0 else mp.mpf(0)
                bo["E0"] = D_E[i] * dn + _norm(Ein) * (u * (30 + oa["j_rnd"]) * jmax + basis)
                if "E_rnd" in oa:  # a polarization filter: no basis of s and p, the matrix chain of interact_polarizer
                    bo["E0"] = D_E[i] * dn + _norm(Ein) * u * oa["E_rnd"]
            b["outs"].append(bo)
        k_n = getattr(obj, "index_tol", lambda: 0)()
        b["index"] = mp.mpf(0)
        if k_n and obj.kind == "lens":
            # an index the host computed by a formula (sellmeier): the traces refract with its double, within k u of the 50-digit value,
            # relative.  The derivative of the rays that leave with respect to ln(n), a difference of the 50-digit evaluation like D above
            class _Shifted:
                kind = obj.kind

                @staticmethod
                def index(lam):
                    return obj.index(lam) * (1 + step)

            for bo, oa, ob in zip(b["outs"], ex["outs"], interact(_Shifted, dirv, hit["n"], n_ray, seg["lam"], Ein, None, seg.get("chief_entering"))):
                bo["dir"] += _norm(_sub(ob["dir"], oa["dir"])) / step * k_n * u
                if Ein is not None:
                    bo["E0"] += _norm(_sub(ob["E0"], oa["E0"])) / step * k_n * u
            if ex["outs"][0].get("entering") or ex["outs"][0].get("tir"):
                b["index"] = k_n * u * ex["outs"][0]["n"]  # the next ray is in the glass: its index is the double of the formula
        b["dir"], b["E0"] = b["outs"][0]["dir"], b["outs"][0]["E0"]
    return b


# ------------------------------------------------------------------------------------------------ a whole root
def exact_trace(root, objects, consts, r_max=30, planted=None, kick=None, depth=0, follow=None):
    """Iterates exact_step from a root's doubles root = dict(pos, dir, n, lam[, E0]) -> list of dict(obj (index), part, piece, ex, seg, tie) per
    segment, the last with ex = None where nothing is hit, or with children = [trace, trace] where a splitter ends the beam (transmitted first,
    Beamsplitters.jl:16-19).  It picks the nearest object itself (System.jl:57-72, the first of two equal lengths stays; the parts of a doublet in
    their order, AbstractRay.jl:130-155), after the hinted shape alone where the last bounce left a hint (System.jl:74-85): a lens hints at itself
    on entry and after a total internal reflection (Lenses.jl:53-74), a doublet at its other part (DoubletLenses.jl:66-76).
    kick = (k, dpos, ddir): added to the ray that leaves bounce k (the sensitivities of the end-to-end bound); the direction is renormalised.
    follow = [(object, part), ...]: do not choose, take these solids in turn (a trace that is known to meet what another one met)."""
    seg = dict(pos=_v(root["pos"]), dir=_v(root["dir"]), n=_f(root["n"]), lam=root["lam"], E0=root.get("E0"), opl=_f(root.get("opl", 0.0)))
    cands = [(k, p, solid) for k, obj in enumerate(objects) for p, solid in enumerate(getattr(obj, "parts", [obj]))]
    out, hint = [], None
    while len(out) < r_max:
        best, second = None, None
        if follow is not None:
            if len(out) >= len(follow):
                break
            k, p = follow[len(out)]
            ex = exact_step(seg, getattr(objects[k], "parts", [objects[k]])[p], consts, planted)
            if ex is None:
                break
            best = (k, p, ex)
        elif hint is not None:
            solid = getattr(objects[hint[0]], "parts", [objects[hint[0]]])[hint[1]]
            ex = exact_step(seg, solid, consts, planted)
            if ex is not None:
                best = (hint[0], hint[1], ex)
        searched = best is None
        if best is None:
            for k, p, solid in cands:
                if _dot(_sub(solid.pos, seg["pos"]), seg["dir"]) < -2 * solid.size:
                    continue  # wholly behind the ray: every point of a solid lies within 2 size of its position
                ex = exact_step(seg, solid, consts, planted)
                if ex is None:
                    continue
                if best is None or ex["t"] < best[2]["t"]:
                    second = None if best is None else best[2]["t"]
                    best = (k, p, ex)
                elif second is None or ex["t"] < second:
                    second = ex["t"]
        if best is None:
            out.append(dict(obj=-1, part=0, piece=None, ex=None, seg=seg, tie=None))
            break
        k, p, ex = best
        if searched and getattr(objects[k], "kind", None) == "plate_bs":
            # PlateBeamsplitter.jl:160-187: both parts are tested; the coating wins where the two lengths are approximately equal (isapprox,
            # rtol = sqrt(eps)) or it is nearer.  The nearest-first search above has taken care of 'nearer'.
            other = exact_step(seg, objects[k].parts[1 - p], consts, planted)
            if other is not None and abs(other["t"] - ex["t"]) <= _mp().sqrt(2.0 ** -52) * max(abs(other["t"]), abs(ex["t"])):
                if p == (1 if planted == "coating_loses_tie" else 0):
                    p, ex = 1 - p, other
        same_object = second is not None and hasattr(objects[k], "parts")    # the parts of a doublet meet at their interface by construction
        out.append(dict(obj=k, part=p, piece=ex["hit"]["piece"], ex=ex, seg=seg, tie=None if (second is None or same_object) else second - ex["t"]))
        if ex["children"] is not None and depth < 4:
            out[-1]["children"] = [exact_trace(dict(pos=o["pos"], dir=o["dir"], n=o["n"], lam=root["lam"], E0=o["E0"], opl=ex["opl"]), objects, consts,
                                               r_max, planted, None, depth + 1) for o in ex["children"]]
        if ex["next"] is None:
            break
        nx = ex["next"]
        if getattr(objects[k], "kind", None) in ("plate_bs", "cube_bs"):
            hint = (k, len(objects[k].parts) - 1)                            # PlateBeamsplitter.jl:199, CubeBeamsplitter.jl:72, :89: at the coating
        elif hasattr(objects[k], "parts"):
            hint = (k, 1 - p)
        elif objects[k].kind == "lens" and (nx["entering"] or nx["tir"]):
            hint = (k, 0)
        else:
            hint = None
        seg = dict(pos=nx["pos"], dir=nx["dir"], n=nx["n"], lam=root["lam"], E0=nx["E0"], opl=ex["opl"])
        if kick is not None and kick[0] == len(out) - 1:
            seg["pos"] = _add(seg["pos"], kick[1])
            seg["dir"] = _unit(_add(seg["dir"], kick[2]))
    return out


def excluded(ex, second_gap=None):
    """The only criterion by which a bounce may be left out, computed from the exact geometry alone; at a polarization filter also an exact
    norm(E') that lies within the bound of E0 of the threshold at which the filter blocks."""
    pol = ex.get("ended") if ex.get("end") == "blocked" else (ex["next"] if ex.get("next") is not None else None)
    if pol is not None and pol.get("block_margin", 1) < 0:
        return True
    return ex["hit"]["seam"] < SEAM or (second_gap is not None and abs(second_gap) < TIE)


# ------------------------------------------------------------------------------------------------ records
def segments_of(res, node, sub=0):
    """The recorded segments of beam `node` of a TraceResult as dicts of doubles, with the optical path so far.  A GaussianBeamlet's record holds
    three rays of 11 planes each: sub = 0 chief, 1 waist, 2 divergence (each is traced and refracted as a Ray of its own, Gaussian.jl:124-135)."""
    first, nseg = int(res.node_first_rec[node]), int(res.node_nseg[node])
    gauss = res.rec_planes == 33
    lam = float(res.node_aux[node, 3 if gauss else 0])
    out, opl = [], 0.0
    for k in range(first, first + nseg):
        r = res.rec[11 * sub:, k] if gauss else res.rec[:, k]
        seg = dict(pos=r[0:3].copy(), dir=r[3:6].copy(), n=float(r[6]), t=float(r[7]), normal=r[8:11].copy(), lam=lam, obj=int(res.rec_obj[k]),
                   shape=int(res.rec_shape[k]), opl=opl, E0=None)
        if res.rec_planes == 17:
            seg["E0"] = [complex(r[11], r[12]), complex(r[13], r[14]), complex(r[15], r[16])]
        out.append(seg)
        if math.isfinite(seg["t"]):
            opl = opl + seg["n"] * seg["t"]  # the left fold of optical_path_length (Beam.jl:125-169), as doubles; exact_step adds in 50 digits
    return out


def ancestors(res, node):
    """The recorded segments of the beams above `node`, the root's first: (segments, count)."""
    chain, p = [], int(res.node_parent[node])
    while p >= 0:
        chain = [s for s in segments_of(res, p) if math.isfinite(s["t"])] + chain
        p = int(res.node_parent[p])
    return chain


def exact_opl(segs, k, planted=None):
    """The optical path of the recorded segments before segment k, summed exactly (Beam.jl:125-169: n of the segment itself)."""
    mp = _mp()
    n_of = (lambda j: segs[j + 1]["n"]) if planted == "opl_next_medium" else (lambda j: segs[j]["n"])
    return sum((_f(n_of(j)) * _f(segs[j]["t"]) for j in range(k)), mp.mpf(0))


def fdiff(recorded, exact):
    """|recorded - exact| of a vector (or a scalar) of doubles against mpmath numbers, taken in 50 digits -> float."""
    mp = _mp()
    if np.ndim(recorded) == 0 and not isinstance(recorded, (list, tuple)):
        return float(abs(mp.mpmathify(recorded) - exact)) if isinstance(recorded, complex) else float(abs(_f(recorded) - exact))
    acc = mp.mpf(0)
    for a, b in zip(recorded, exact):
        a = mp.mpc(a.real, a.imag) if isinstance(a, complex) else _f(a)
        acc += abs(a - b) ** 2
    return float(mp.sqrt(acc))

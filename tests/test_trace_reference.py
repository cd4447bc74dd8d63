"""Traced rays against a 50-digit evaluation of each bounce (tests/trace_ref.py), inside a bound that is derived and not measured.

Oracle, lane code and host scene builders were written from one reading of the reference; a mistake they share passes every parity test.  Here
every recorded bounce of the oracle's solve - hit distance, normal, the next ray's position, direction, refractive index and field, the optical
path, the detector row - is compared with an evaluation of the optics written from the reference's formulas and from the scene's prescription
and pose alone, within

    t - t*  in  [-eps_ray (1 / |cos theta| - 1)(1 + c2), 0] + roundings     (mirrored for a leaving hit),
    |n - n*| <= kappa eps_ray tan(theta) + roundings  (+ 11 u S / grad_h + grad_h^2 |f'''| / 6 for central-difference normals),

and what follows from these for the next ray (trace_ref.py derives every term; nothing in it comes from oracle or engine output).  The emulator
(the host build of the lane code) must equal the oracle bit for bit on every scene, so the same holds for it; tests/test_trace_reference_gpu.py
repeats the comparison on the engine's own records.  Each case prints its figures ("Trace against exact optics")."""
import cmath
import functools

import pytest

import bmo_amd as bmo
import trace_cases as tc
import trace_ref as tr
from parity import compare, emu_trace

mp = pytest.importorskip("mpmath")


@functools.lru_cache(maxsize=None)
def solved(oracle, name):
    """Scene `name` solved on the oracle, once per process and shared (read-only): the case with scene, consts, res and the held figures."""
    c = tc.SCENES[name]()
    tc.compile_case(c)
    c.res = oracle.trace(c.scene, c.bundle, tc.R_MAX)
    c.cache = {}
    c.held = tc.hold(c.res, c, c.consts, cache=c.cache)
    return c


def test_march_constants_are_the_references():
    """AbstractSDF.jl:1-3, :83, :105: the constants the bound is built from."""
    c = tc.SCENES["singlet-ray"]()
    k = tr.consts_of(bmo.CompiledScene(c.system, c.bundle.lambdas))
    assert (k["eps_ray"], k["eps_srf"], k["eps_ins"], k["grad_h"], k["march_iters"], k["mt_leps"]) == (1e-10, 1e-9, 1.0, 1e-8, 1000, 1e-9)


@pytest.mark.parametrize("name", sorted(tc.SCENES))
def test_every_bounce_within_its_bound(oracle, name):
    c = solved(oracle, name)
    assert 48 <= c.bundle.n <= 96
    assert compare(emu_trace(c.scene, c.bundle, tc.R_MAX), c.res, 0.0, name)
    h = c.held
    print(h.line(name))
    print("   ratios: " + ", ".join("%s %.3g" % (q, r) for q, r in h.ratio.items() if r > 0))
    assert h.bounces >= 2 * c.bundle.n
    assert h.excluded <= (0 if name in tc.NO_EXCLUSIONS else 0.02 * h.bounces), (h.excluded, h.bounces)
    assert not h.over, h.over[:5]
    assert h.abs["t"] > 0.0 and h.abs["n"] > 0.0  # two different computations were compared
    assert 1e-4 < h.worst() <= 1.0                  # a bound that is never approached within four orders pins nothing


def test_singlet_reaches_its_edges(oracle):
    """The fans do what they are for: rays on the lens's axis, leaving hits, the barrel met from inside in total internal reflection."""
    for name in ("singlet-ray", "singlet-pol"):
        h = solved(oracle, name).held
        assert h.leaving >= 64 and h.barrel == 10 and h.tir == 10, (h.leaving, h.barrel, h.tir)
    c = solved(oracle, "singlet-ray")
    on_axis = [i for i in range(c.bundle.n) if abs(float(tr.exact_hit(c.exact[0], tr._v(c.bundle.planes[0:3, i]), tr._v(c.bundle.planes[3:6, i]),
                                                                      c.consts)["cos"])) > 1 - 1e-15]
    assert len(on_axis) == 2


def test_concave_scene_reaches_its_edges(oracle):
    """Hits 5 um, 24 um and 1 mm beside the concave apex, and the two rim rays: barrel to barrel in ONE recorded segment although the straight
    line leaves the glass through the concave face and enters it again (the inside march's last crossing, AbstractSDF.jl:132-159)."""
    c = solved(oracle, "concave-ray")
    n = c.bundle.n
    with mp.workdps(50):
        for i, r in zip(range(n - 14, n - 2), [5e-6] * 4 + [24e-6] * 4 + [1e-3] * 4):
            hit = tr.exact_trace(tc.root_of(c.bundle, i), c.exact, c.consts, 2)[0]["ex"]["hit"]
            assert hit["piece"] == "front" and abs(float(c.exact[0].d / 2 - hit["edge_dist"]) - r) < 0.02 * r + 1e-9
        for i in (n - 2, n - 1):
            trace = tr.exact_trace(tc.root_of(c.bundle, i), c.exact, c.consts, tc.R_MAX)
            assert [s["piece"] for s in trace[:2]] == ["barrel", "barrel"] and trace[1]["ex"]["hit"]["leaving"]
            between = [t for t in trace[1]["ex"]["hit"]["others"] if 1e-9 < t < trace[1]["ex"]["t"]]
            assert len(between) == 2, between  # out through the concave face and in again
            assert tc.sequence(c.res, i, c)[0][:2] == [(0, 0), (0, 0)] and c.res.node_nseg[i] >= 3


def test_l3_is_inflected_and_its_crest_is_a_seam(oracle):
    """What element L3 brings: both profiles rise and fall again (largest sag > 0 > edge sag), so lines cross the front profile twice, and
    the front leaf, closed by the plane at its largest sag (AsphericalLensSDF.jl:211-228), thins to nothing on the crest circle.  Within
    sqrt(2 grad_h / |sag''|) = 6.8 um of that circle the glass between the profile and that plane is thinner than the central-difference
    stencil (AsphericalLensSDF.jl:5, AbstractSDF.jl:81-88), the same thing as the wedge under a concave apex (rule ii), and
    no rule protects it: the exact hit lies within 1e-8 m of the seam between profile and plane, the one criterion by which a bounce is left
    out.  Eight rays aimed 0.5 um beside the crest: every one is such a bounce; the recorded hit DISTANCE still meets its bound, the recorded
    normal does not (printed, not asserted: it is the reference's algorithm that gives it)."""
    c = solved(oracle, "phone-l3")
    lens = c.exact[0]
    with mp.workdps(50):
        front = lens.regions[1]["lo"][1]
        crest = mp.findroot(lambda r: front.dsag(r)[0], (mp.mpf("0.5e-3"), mp.mpf("0.7e-3")), solver="anderson", tol=mp.mpf(10) ** -40, verify=False)
        edge = front.sag((mp.mpf(tc.L3["front"][1]) / 2) ** 2)
        assert abs(crest - tc.L3_CREST) < 1e-9 and front.sag(crest ** 2) > 2.2e-5 and edge < -1.8e-4
        assert abs(lens.regions[0]["lo"][1] - front.sag(crest ** 2)) < mp.mpf(10) ** -40  # the mid cylinder starts at the largest sag
        twice = 0
        for i in range(c.bundle.n):
            r = tc.root_of(c.bundle, i)
            cr = lens.crossings(lens.to_local(tr._v(r["pos"])), lens.vec_local(tr._v(r["dir"])))
            twice += len(cr) >= 4
        assert twice >= 1, "no line of the fan crosses the boundary more than twice"
        k = tc.SCENES["phone-l3"](crest=True)
        tc.compile_case(k)
        res = oracle.trace(k.scene, k.bundle, tc.R_MAX)
        worst_n = 0.0
        for i in range(k.bundle.n):
            seg = tr.segments_of(res, i)[0]
            ex = tr.exact_step(seg, k.exact[0], k.consts)
            assert ex["hit"]["piece"] == "asphere" and ex["hit"]["leaf"] < tr.SEAM and tr.excluded(ex)
            b = tr.step_bound(seg, ex, k.exact[0], k.consts)
            dt = tr._f(seg["t"]) - ex["t"]
            assert -b["t_lo"] <= dt <= b["t_hi"]
            worst_n = max(worst_n, tr.fdiff(seg["normal"], ex["normal"]) / float(b["n"]))
    print("phone-l3 crest: 8 hits on glass thinner than %.2g m; recorded t inside its bound, recorded normal up to %.3g bounds off" % (
        float(ex["hit"]["leaf"]), worst_n))


def test_fresnel_rhomb_gives_a_quarter_wave(oracle):
    """runtests.jl:2354-2361 on the exact evaluator and on the record: after two total internal reflections at 53.3 degrees in n = 1.5 the field
    of the axis ray is circular, arg(Ez) - arg(Ex) = pi / 2 (isapprox: to sqrt(eps)), |Ey| < 2e-14 of the field.  The evaluator's complex
    rs / rp are held to a known answer, not only to the record."""
    c = solved(oracle, "rhomb")
    assert c.held.tir == 2 * c.bundle.n
    with mp.workdps(50):
        trace = tr.exact_trace(tc.root_of(c.bundle, 0), c.exact, c.consts, tc.R_MAX)
        assert [bool(s["ex"] and s["ex"]["next"]["tir"]) for s in trace] == [False, True, True, False, False]
        E = trace[3]["ex"]["next"]["E0"]
        phi = mp.arg(E[2]) - mp.arg(E[0])
        assert abs(phi - mp.pi / 2) <= 2.0 ** -26 * mp.pi / 2 and abs(E[1]) < 2e-14
    last = tr.segments_of(c.res, 0)[-1]["E0"]
    assert abs(cmath.phase(last[2]) - cmath.phase(last[0]) - cmath.pi / 2) <= 2.0 ** -26 * cmath.pi / 2 and abs(last[1]) < 2e-14


@pytest.mark.parametrize("name", sorted(tc.SCENES))
def test_exact_trace_finds_the_recorded_sequence(oracle, name):
    """exact_trace picks the nearest object at every bounce by itself: the record's object sequence and its end (detected or lost)."""
    c = solved(oracle, name)
    skipped = 0
    roots = [int(n) for n in range(c.res.n_nodes) if c.res.node_parent[n] < 0]
    assert len(roots) == c.bundle.n
    with mp.workdps(50):
        for i in range(c.bundle.n):
            trace = tr.exact_trace(tc.root_of(c.bundle, i), c.exact, c.consts, tc.R_MAX)
            if tc.left_out(trace):
                skipped += 1
                continue
            tc.same_tree(trace, c.res, roots[i], c)
    print("%s: %d of %d roots left out (a hit within %g m of a seam or edge)" % (name, skipped, c.bundle.n, tr.SEAM))
    assert skipped <= (0 if name in tc.NO_EXCLUSIONS else 0.02 * c.bundle.n)


@pytest.mark.parametrize("name", ["singlet-ray", "asphere-curved-first", "miniscope"])
def test_end_to_end(oracle, name):
    """The one place where errors may accumulate: exact_trace from the root's doubles to the detector against the recorded row, within the sum
    over the bounces of the sensitivity of the row to that bounce's output times the bounce's bound."""
    c = solved(oracle, name)
    h = tc.end_to_end(c.res, c, c.consts, range(0, c.bundle.n, {"singlet-ray": 2, "miniscope": 14}.get(name, 6)))
    print("%s end to end: %d rows; worst |dpos| %.3g m, |ddir| %.3g, |dopl| %.3g m; worst recorded / bound %.3g" % (
        name, h.bounces, h.abs["row_pos"], h.abs["row_dir"], h.abs["opl"], h.worst()))
    assert h.bounces >= (4 if name == "miniscope" else 8) and not h.over, h.over[:5]
    assert 1e-4 < h.worst() <= 1.0


def test_doublet_via_air_changes_no_direction_below_the_critical_angle(oracle):
    """The issue's tenth switch, a cemented interface refracted glass -> air -> glass, is no mistake that a Ray's direction shows: n sin(theta)
    is kept across a gap of zero width.  Shown, not only argued: on the doublet scene the switched evaluator stays inside every bound and its
    directions equal the right ones to 50-digit rounding; beyond the critical angle glass -> air it reflects where the interface refracts."""
    c = solved(oracle, "doublet")
    h = tc.hold(c.res, c, c.consts, wrong=tc.SCENES["doublet"](planted=tr.VIA_AIR).exact, planted=tr.VIA_AIR, cache=c.cache)
    assert not h.over and h.bounces == c.held.bounces
    with mp.workdps(50):
        n1, n2 = mp.mpf("1.6456"), mp.mpf("1.7168")
        normal = [mp.mpf(0), mp.mpf(-1), mp.mpf(0)]
        for deg, same in ((10, True), (30, True), (37, True), (38, False), (50, False)):  # asin(1 / 1.6456) = 37.42 degrees
            d = [mp.sin(mp.radians(deg)), mp.cos(mp.radians(deg)), mp.mpf(0)]
            a, b = tr.interact_lens(d, normal, n1, n2), tr.interact_lens(d, normal, n1, n2, planted=tr.VIA_AIR)
            assert (tr._norm(tr._sub(a["dir"], b["dir"])) < mp.mpf(10) ** -45) == same and a["tir"] is False and b["tir"] == (not same)


def test_every_planted_mistake_has_a_scene():
    assert {p for p, _ in tc.PLANTED_ON} == set(tr.PLANTED)


@pytest.mark.parametrize("planted,name", tc.PLANTED_ON)
def test_the_bound_is_not_slack(oracle, planted, name):
    """The exact evaluator with one deliberate mistake is at least 1e4 bounds away from the record at some bounce."""
    c = solved(oracle, name)
    wrong = tc.SCENES[name](planted=planted).exact
    h = tc.hold(c.res, c, c.consts, wrong=wrong, planted=planted, cache=c.cache)
    q = max(h.ratio, key=h.ratio.get)
    print("%s on %s: recorded - planted is %.3g bounds at the worst bounce (%s); quantities with a bound of zero aside, %.3g" % (
        planted, name, h.worst(), q, h.worst_finite()))
    assert h.worst_finite() >= 1e4  # not the infinite ratio of a quantity whose bound is zero, nor that of a hit the planted evaluator lost

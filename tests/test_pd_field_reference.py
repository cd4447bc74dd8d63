"""The oracle's Photodetector field (bmo_cpu_photodetector_field) against a 50-digit evaluation of the reference's expression sequence
(Photodetector.jl:69-107, Gaussian.jl:298-392, Beam.jl:177-205; tests/pd_ref.py), inside a pointwise bound that is derived from the oracle's
arithmetic and not measured:

    |F_oracle - F_exact| <= sum_q |dE / dq| eps_q  +  u |E| (24 + 9 r^2 / w^2 + phases)  +  2 (H - 1) u sum_h |E_h|,    u = 2^-53,

q running over the intermediates that come out of a cancelling subtraction (pd_ref.py derives every eps_q and count).  The scenes enter
the branches no other Photodetector scene reaches: point_on_beam selecting an earlier segment, a child beamlet read at z < length(parent), a
grid across a focus (R and the Gouy phase change sign), and a sum over beamlets of different wavelength.  Each case prints its figures
("Read-outs", lists them).  tests/test_pd_field_edges_gpu.py then holds the GPU read-out to the oracle and to the
exact field on the same scenes."""
import numpy as np
import pytest

import pd_ref

mp = pytest.importorskip("mpmath")

FLOOR = 1e-290  # below it the field runs into subnormal numbers (TAIL_FLOOR of tests/test_photodetector.py)


def _check(c):
    """The assertions every case makes; returns the live mask."""
    ex, F = c.exact, c.oracle_field
    assert ex.bound.shape == F.shape == (len(c.xs), len(c.ys)) and F.size <= 441 and len(c.records) <= 3
    assert np.isfinite(F.view(np.float64)).all() and np.isfinite(ex.bound).all()
    live = ex.scale > FLOOR
    assert live.mean() >= 0.9, live.mean()
    err = ex.error(F)
    ratio, rel = err[live] / ex.bound[live], err[live] / ex.scale[live]
    print("%s: H = %d, %d points, %.0f %% live, min |E| / peak %.3g; worst error / bound %.3g, worst error / sum|E_h| %.3g, worst bound / sum|E_h| %.3g"
          % (c.name, len(c.records), F.size, 100 * live.mean(), ex.scale.min() / ex.scale.max(), ratio.max(), rel.max(), (ex.bound[live] / ex.scale[live]).max()))
    assert (err[live] <= ex.bound[live]).all(), (ratio.max(), np.unravel_index(np.argmax(err / np.maximum(ex.bound, 1e-300)), err.shape))
    assert err.max() > 0.0  # two different computations were compared: 3.5e5 rad of phase in doubles cannot be exact
    return live


def _share(index, k):
    return float((index == k).mean())


def test_earlier_segment(oracle):
    """The last chief segment is 1.47 mm long and the detector is tilted by 70 degrees: point_on_beam selects segment 2 (inside the glass)."""
    c = pd_ref.pd_case(oracle, "earlier_segment")
    assert len(c.records) == 1 and len(c.records[0]["segs"]) == 3 and c.records[0]["segs"][-1]["t"] < 1.5e-3
    live = _check(c)
    idx = c.exact.index[0]
    assert _share(idx, 2) >= 0.05 and _share(idx, 3) >= 0.5 and _share(idx, 1) == 0.0
    early = (idx == 2) & live
    assert c.exact.scale[early].max() > 1e-3 * c.exact.scale.max()  # the branch is entered where the field is not negligible


def test_all_three_segments(oracle):
    """Longer ys: the grid projects onto the path in front of the lens, inside it and behind it."""
    c = pd_ref.pd_case(oracle, "three_segments")
    assert len(c.records) == 1 and len(c.records[0]["segs"]) == 3
    _check(c)
    for k in (1, 2, 3):
        assert _share(c.exact.index[0], k) >= 0.05, (k, _share(c.exact.index[0], k))


def test_child_beamlet_in_front_of_its_parents_end(oracle):
    """The transmitted child of a thin splitter (one segment; the reflected child misses the detector): z < length(parent) on part of the grid,
    point_on_beam's last-ray rule with a negative z - temp."""
    c = pd_ref.pd_case(oracle, "child")
    assert c.res.n_nodes == 3 and len(c.records) == 1 and len(c.records[0]["segs"]) == 1 and len(c.records[0]["parents"]) == 1
    live = _check(c)
    ex = c.exact
    assert ex.l_parent[0] > 0.04 and (ex.index[0] == 1).all()
    before = (ex.z[0] < ex.l_parent[0]) & live
    assert 0.05 <= before.mean() <= 0.95, before.mean()
    err = ex.error(c.oracle_field)
    assert (err[before] <= ex.bound[before]).all()
    assert ex.scale[before].max() > 1e-3 * ex.scale.max()


def test_grid_across_a_focus(oracle):
    """A steep detector centred on the lens's focus: R passes zero on the grid and the rule R < 0 -> psi = -psi flips between neighbours."""
    c = pd_ref.pd_case(oracle, "focus")
    assert len(c.records) == 1
    live = _check(c)
    ex = c.exact
    assert ex.w[0].max() < 60e-6  # the focus: w = 54 um
    for name in ("R", "psi"):
        v = getattr(ex, name)[0][live]
        assert (v < 0).mean() >= 0.2 and (v > 0).mean() >= 0.2, (name, (v < 0).mean(), (v > 0).mean())
    assert ((ex.R[0] < 0) == (ex.psi[0] > 0)).all()


def test_three_beamlets_of_different_wavelength(oracle):
    c = pd_ref.pd_case(oracle, "three_wavelengths")
    assert len(c.records) == 3 and len({r["lam"] for r in c.records}) == 3
    _check(c)
    ex = c.exact
    assert ((ex.E_abs > 1e-3 * ex.E_abs.max()).sum(axis=0) >= 2).any()  # the spots overlap: the sum has more than one term that counts
    assert ex.terms["summation"].max() > 0.0


# Each planted mistake in the exact evaluator, and the scenes whose branch it changes.
PLANTED_ON = [("gouy_sign", "focus"), ("gouy_sign", "earlier_segment"), ("no_ref_phi", "earlier_segment"), ("proj_not_sqrt", "earlier_segment"),
              ("proj_not_sqrt", "child"), ("last_segment_rays", "earlier_segment"), ("last_segment_rays", "three_segments"),
              ("no_parent_length", "child"), ("curvature_reciprocal", "focus"), ("curvature_reciprocal", "child")]


def test_every_planted_mistake_has_a_scene():
    assert {p for p, _ in PLANTED_ON} == set(pd_ref.PLANTED)


@pytest.mark.parametrize("planted,scene", PLANTED_ON)
def test_the_bound_is_not_slack(oracle, planted, scene):
    """The exact evaluator with one deliberate mistake differs from the oracle by more than the bound, at a point that carries more than 1e-6
    of the peak and lies in the branch the mistake changes."""
    c = pd_ref.pd_case(oracle, scene)
    ex = c.exact
    wrong = pd_ref.pd_field_exact(c.records, c.position, c.orientation, c.xs, c.ys, planted=planted)
    where = ex.scale > 1e-6 * ex.scale.max()
    if planted == "last_segment_rays":
        where &= ex.index[0] < len(c.records[0]["segs"])
    assert where.any()
    ratio = wrong.error(c.oracle_field)[where] / ex.bound[where]
    print("%s on %s: %d points, largest |F_wrong - F_oracle| / bound %.3g, smallest %.3g" % (planted, scene, where.sum(), ratio.max(), ratio.min()))
    assert ratio.max() > 1.0

"""The engine's own records against the 50-digit evaluation of each bounce (tests/trace_ref.py, the scenes of tests/trace_cases.py).

Per scene, 1 024 rays through the HIP engine: the solve equals the oracle's bit for bit, and a strided sample of 64 beams of the ENGINE's
records is held to exact_step within step_bound, independently of the oracle - the record plus the derived bound, with no ulp allowance, since
traces are bit-exact.  The end-to-end row is checked on the detector rows as bmo_result_copy_hits returns them, and a retrace after a
kinematic move must meet the same per-bounce bounds against the moved prescription.

Host time, measured on a CPU: a closed-form bounce (sphere, plane, barrel, mesh) with its bound takes about 2.5 ms of mpmath, a bounce on an
aspheric profile (96-sample sign scan of the residual and refinement of the root) about 18 ms, a bounce of a lens with rings about 7 ms.  The
64 sampled beam trees are 130 - 600 bounces, so a scene's comparison takes 0.1 - 3 s (the slowest: acylinders, miniscope and its end-to-end
rows), inside the 10 s a test may take.  The scenes of the sdf and cuboid mirrors, the plano and thin lenses and the primitive bodies are
closed-form: 0.1 - 0.5 s each on the MI355X (the slowest, primitives-pol, 0.50 s).  The whole phone objective is eleven bounces per ray, ten
of them on aspheric profiles or plates: it samples 16 beam trees (176 bounces, 1.1 s on the MI355X), and its end-to-end test one row
(330 exact steps for the sensitivities of ten refractions, 1.2 s)."""
import ctypes as C
import math

import numpy as np
import pytest

import bmo_amd as bmo
import trace_cases as tc
from parity import compare

mp = pytest.importorskip("mpmath")

N_RAYS, SAMPLE = 1024, 64


def _solve(scene, bundle, prev=None):
    """One solve on the engine, created and closed inside: (TraceResult, solution to be freed)."""
    return bmo.system._engine_solve(scene, bundle, tc.R_MAX, prev)


def _wide(name, **kw):
    c = tc.SCENES[name](**kw)
    c.small = c.bundle
    c.bundle = tc.widen(c.small, N_RAYS)
    return tc.compile_case(c)


def _sample(c):
    """64 beams: every kind of ray of the fans (the first copy of the small bundle, strided) and copies further out; of the phone objective
    every fourth of them, 16."""
    first = list(range(0, c.small.n, 2))[:SAMPLE // 2]
    rest = list(range(c.small.n + 1, N_RAYS, (N_RAYS - c.small.n - 1) // (SAMPLE - len(first))))
    assert len(first + rest) >= SAMPLE
    return (first + rest)[:SAMPLE][::4 if c.name == "phone" else 1]


def _held(name, h, what="engine"):
    print(h.line("%s (%s)" % (name, what)))
    assert h.bounces >= 2 * SAMPLE * 0.9
    assert h.excluded <= (0 if name in tc.NO_EXCLUSIONS else 0.02 * h.bounces), (h.excluded, h.bounces)
    assert not h.over, h.over[:5]
    assert 1e-4 < h.worst() <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(tc.SCENES))
def test_engine_records_within_the_bound(oracle, name):
    c = _wide(name)
    got, sol = _solve(c.scene, c.bundle)
    try:
        compare(got, oracle.trace(c.scene, c.bundle, tc.R_MAX, threads=16), 0.0, name)
        _held(name, tc.hold(got, c, c.consts, nodes=tc.tree_nodes(got, _sample(c))))
    finally:
        sol.free()


@pytest.mark.gpu
@pytest.mark.parametrize("name,stride,rows_min", [("singlet-ray", 41, 20), ("miniscope", 255, 4), ("phone", 1024, 1)])
def test_engine_rows_end_to_end(name, stride, rows_min):
    """exact_trace from the root doubles to the detector against the rows bmo_result_copy_hits returns: through the singlet, and through the five
    lenses (eight refractions) of the miniscope's first three elements, and one row through the ten refractions of the phone objective."""
    c = _wide(name)
    got, sol = _solve(c.scene, c.bundle)
    try:
        n = int(got.det_count[0])
        rows = np.zeros((n, 9))
        bmo.abi.check(sol.lib, sol.lib.bmo_result_copy_hits(sol.handle, 0, rows.ctypes.data_as(C.c_void_p), n), "bmo_result_copy_hits")
        assert np.array_equal(rows, got.detector_hits(0))
        got.det_data = rows  # what end_to_end reads: the copied rows
        h = tc.end_to_end(got, c, c.consts, range(0, N_RAYS, stride))
    finally:
        sol.free()
    print("%s end to end (engine): %d rows; worst |dpos| %.3g m, |ddir| %.3g, |dopl| %.3g m; worst recorded / bound %.3g" % (
        name, h.bounces, h.abs["row_pos"], h.abs["row_dir"], h.abs["opl"], h.worst()))
    assert h.bounces >= rows_min and not h.over, h.over[:5]
    assert 1e-4 < h.worst() <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ray", "pol", "plate-ray", "cube-pol"])
def test_engine_retrace_after_a_move(oracle, kind):
    """The lens (ray, pol: the singlet; else the plate or cube splitter of that scene) translated by 0.3 mm and rotated by 0.5 degrees: the
    retraced records meet the per-bounce bounds of the MOVED prescription.  No beamlets through a moved splitter: there the reference computes
    a child's w0 over a stale tail, which the exact evaluator does not model."""
    move = ([0.3 * tc.mm, 0, 0], math.radians(0.5))
    scene = "singlet-" + kind if kind in ("ray", "pol") else kind
    c0, c1 = _wide(scene), _wide(scene, move=move)
    assert not np.array_equal(np.asarray(c0.lens.position()), np.asarray(c1.lens.position()))
    g0, s0 = _solve(c0.scene, c0.bundle)
    try:
        g1, s1 = _solve(c1.scene, c1.bundle, s0)
        try:
            a0, osol = oracle.trace(c0.scene, c0.bundle, tc.R_MAX, threads=16, keep=True)
            compare(g1, oracle.trace(c1.scene, c1.bundle, tc.R_MAX, threads=16, prev=osol), 0.0, "retrace")
            osol.free()
            _held(scene, tc.hold(g1, c1, c1.consts, nodes=tc.tree_nodes(g1, _sample(c1))), "retraced")
            assert g1.rec.shape != g0.rec.shape or not np.array_equal(g1.rec, g0.rec)  # the move shows in the records
        finally:
            s1.free()
    finally:
        s0.free()

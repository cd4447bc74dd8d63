"""The reference's Gaussian-beamlet known-answer tests (test/runtests.jl:1811-1932) against the code that SHIPS:
`gauss_parameters` of the oracle's C++ (oracle/bmo_oracle.cpp, exported as bmo_cpu_gauss_parameters — the function its splitter and
Photodetector code call) on the CPU, and `gauss_parameters_at` of the device lane code (csrc/bmo_lane.hpp, read out through
bmo_gauss_parameters — the code pd_field_kernel and the splitter path run) on the GPU.  Same inputs and tolerances as the reference's
tests; tests/test_oracle_kat2.py keeps the pure-Python helper as a third witness."""
import math

import numpy as np
import pytest

import bmo_amd as bmo

RTOL = math.sqrt(np.finfo(float).eps)


def _oracle_backend(oracle):
    def solve(system, g, r_max=100):
        bundle = bmo.RayBundle.from_beams([g])
        scene = bmo.CompiledScene(system, bundle.lambdas)
        res, sol = oracle.trace(scene, bundle, r_max, threads=1, keep=True)
        return res, sol
    return solve


def _engine_backend():
    def solve(system, g, r_max=100):
        bundle = bmo.RayBundle.from_beams([g])
        scene = bmo.CompiledScene(system, bundle.lambdas)
        return bmo.system._engine_solve(scene, bundle, r_max, None)
    return solve


def _free_space(solve):  # runtests.jl:1811-1871
    y = np.arange(-5, 5.0001, 0.01)
    far = bmo.IntersectableObject(bmo.QuadraticFlatMesh(1e-3))  # never reached: the beamlet stays one unbounded segment
    bmo.translate3d(far, [10.0, 0, 0])
    for lam, w0, M2 in ((500e-9, 1e-3, 1e-3), (1000e-9, 2e-3, 2e-3)):
        g = bmo.GaussianBeamlet([0.0, 0, 0], [0.0, 1, 0], lam, w0, M2=M2, P0=1, support=[1, 0, 0])
        res, sol = solve(bmo.System([far]), g)
        assert res.n_nodes == 1 and int(res.node_nseg[0]) == 1
        num = sol.gauss_parameters(0, y)
        sol.free()
        zr = math.pi * w0 ** 2 / lam / M2
        wa = w0 * np.sqrt(1 + (y / zr) ** 2)
        Ra = y / (y ** 2 + zr ** 2)
        pa = -np.arctan(y / zr)
        assert np.all(np.abs(wa - num[:, 0]) <= 1e-10)
        assert np.all(np.abs(Ra - num[:, 1]) <= 5e-9)
        assert np.all(np.abs(pa - num[:, 2]) <= 1e-7)
        assert np.all(np.abs(num[:, 3] - w0) <= RTOL * w0)


def _thin_lens_vs_abcd(solve):  # runtests.jl:1873-1932
    lam, w0 = 1000e-9, 1e-3
    zr = math.pi * w0 ** 2 / lam
    R1 = R2 = 1
    lens_y, nl = 0.1, 1.5
    f = 1 / ((nl - 1) * (1 / R1 + 1 / R2))
    dy = 0.001
    ys = np.arange(0, 1.5 + 1e-12, dy)
    w_ana, R_ana = np.zeros(len(ys)), np.zeros(len(ys))
    q0 = complex(0, zr)
    for i in range(1, len(ys) + 1):
        w_ana[i - 1] = math.sqrt(-lam / (math.pi * (1 / q0).imag))
        R_ana[i - 1] = (1 / q0).real
        if i * dy == lens_y:
            q0 = (1 * q0 + 0) / (-1 / f * q0 + 1)
            continue
        q0 = (q0 + dy) / 1
    lens = bmo.Lens(bmo.ThinLensSDF(R1, R2, 0.025), lambda x: nl)
    bmo.translate3d(lens, [0, lens_y, 0])
    g = bmo.GaussianBeamlet([0.0, 0, 0], [0.0, 1, 0], lam, w0, support=[1, 0, 0], M2=1)
    res, sol = solve(bmo.System([lens]), g)
    assert int(res.node_nseg[0]) == 3
    num = sol.gauss_parameters(0, ys)
    sol.free()
    assert np.all(np.abs(w_ana - num[:, 0]) <= 1e-6)
    ok = np.abs(R_ana - num[:, 1]) <= 1e-2
    assert ok.sum() / len(ok) > 0.95 and not np.any(np.isnan(num[:, 1]))
    i = int(np.argmin(w_ana))
    assert abs(num[0, 2]) <= 1e-3 and abs(num[i, 2]) <= 1e-3
    assert abs(num[i, 3] - w_ana[i]) <= 1e-7
    return num


def test_free_space_oracle_cpp(oracle):
    _free_space(_oracle_backend(oracle))


def test_thin_lens_vs_abcd_oracle_cpp(oracle):
    num = _thin_lens_vs_abcd(_oracle_backend(oracle))
    # the third witness: the pure-Python restatement used by tests/test_oracle_kat2.py agrees with the C++ to rounding
    lens = bmo.Lens(bmo.ThinLensSDF(1, 1, 0.025), lambda x: 1.5)
    bmo.translate3d(lens, [0, 0.1, 0])
    g = bmo.GaussianBeamlet([0.0, 0, 0], [0.0, 1, 0], 1000e-9, 1e-3, support=[1, 0, 0], M2=1)
    oracle.solve_system(bmo.System([lens]), g)
    ys = np.arange(0, 1.5 + 1e-12, 0.001)
    py = np.array([bmo.beams.gauss_parameters(g, yi) for yi in ys])
    assert np.allclose(py, num, rtol=1e-9, atol=1e-12)


@pytest.mark.gpu
def test_free_space_engine():
    _free_space(_engine_backend())


@pytest.mark.gpu
def test_thin_lens_vs_abcd_engine(oracle):
    num = _thin_lens_vs_abcd(_engine_backend())
    # and the device arithmetic against the oracle's: the same doubles.  No C library enters gauss_parameters_at: tan, acos and atan are the
    # restatements of Julia Base's on both sides (csrc/bmo_jlmath.hpp, oracle/jl_trig.hpp), the rest is +, -, *, / and sqrt without contraction
    lens = bmo.Lens(bmo.ThinLensSDF(1, 1, 0.025), lambda x: 1.5)
    bmo.translate3d(lens, [0, 0.1, 0])
    g = bmo.GaussianBeamlet([0.0, 0, 0], [0.0, 1, 0], 1000e-9, 1e-3, support=[1, 0, 0], M2=1)
    res, sol = _oracle_backend(oracle)(bmo.System([lens]), g)
    ref = sol.gauss_parameters(0, np.arange(0, 1.5 + 1e-12, 0.001))
    sol.free()
    assert np.array_equal(num, ref, equal_nan=True), np.argwhere(num != ref)[:5]


@pytest.mark.gpu
def test_children_of_a_splitter_engine(oracle):
    """gauss_parameters of a CHILD beamlet (z runs over parent + child: point_on_beam starts from length(parent)) — engine == oracle, the same
    doubles: what the ulp bound of the Photodetector field (TAIL_ULPS, tests/test_photodetector.py) takes for granted."""
    bs = bmo.ThinBeamsplitter(20e-3)
    bmo.xrotate3d(bs, math.radians(45))
    bmo.translate3d(bs, [0, 0.05, 0])
    lens = bmo.SphericalLens(0.1, -0.1, 5e-3, 25.4e-3, 1.5)
    bmo.translate3d(lens, [0, 0.12, 0])
    system = bmo.System([bs, lens])
    g = bmo.GaussianBeamlet([0.0, 0, 0], [0.0, 1, 0], 1064e-9, 0.5e-3, support=[1, 0, 0])
    zs = np.linspace(0.0, 0.4, 81)
    res_o, sol_o = _oracle_backend(oracle)(system, g)
    res_g, sol_g = _engine_backend()(system, g)
    assert res_o.n_nodes == res_g.n_nodes == 3
    for node in range(3):
        a, b = sol_o.gauss_parameters(node, zs), sol_g.gauss_parameters(node, zs)
        assert np.array_equal(a, b, equal_nan=True), (node, np.argwhere(a != b)[:5])
    sol_o.free()
    sol_g.free()

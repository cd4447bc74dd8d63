"""The union fast path of tracing_step's outside march (csrc/bmo_lane.hpp, BMO_MARCH_FASTPATH) on the CPU.

The device kernels take it only in the fresh EXT = 0 step kernels; the host emulator runs the EXT = 2 retrace-capable lane code, so
these tests build it twice, with the fast path forced on (2) and off (0), and require both to equal the oracle bit for bit on the
config-2 bundles, config 5 and a share of the random scenes of test_fuzz.py.  The forced build also counts its evaluations
(BMO_EMU_STATS) to show that the loop is really taken.
"""
import ctypes as C
import os
import subprocess

import pytest

import bmo_amd as bmo
import parity
import scenes
from bmo_amd import abi
from parity import compare, emu_trace
from test_fuzz import _case, _engine_first, _limit, R_MAX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_SRC = os.path.join(ROOT, "tests", "emu", "emu.cpp")
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-shared"]


def _load(path):
    lib = C.CDLL(path)
    lib.bmo_emu_trace.argtypes = [C.POINTER(abi.SceneDesc), C.POINTER(abi.RayBatch), C.POINTER(abi.TraceOpts), C.POINTER(C.c_void_p),
                                  C.POINTER(abi.ResultView)]
    lib.bmo_emu_free.argtypes = [C.c_void_p]
    lib.bmo_emu_retrace.argtypes = [C.POINTER(abi.SceneDesc), C.POINTER(abi.RayBatch), C.POINTER(abi.TraceOpts), C.POINTER(abi.ResultView),
                                    C.POINTER(C.c_void_p), C.POINTER(abi.ResultView)]
    return lib


@pytest.fixture(scope="module")
def emus(tmp_path_factory):
    d = tmp_path_factory.mktemp("emu_fastpath")
    libs = {}
    for mode, extra in (("on", ["-DBMO_MARCH_FASTPATH=2", "-DBMO_EMU_STATS"]), ("off", ["-DBMO_MARCH_FASTPATH=0"])):
        so = str(d / ("libemu_%s.so" % mode))
        subprocess.check_call(["g++"] + FLAGS + extra + ["-o", so, EMU_SRC])
        libs[mode] = _load(so)
    return libs


def _trace(lib, scene, bundle, r_max, **kw):
    saved = parity._emu
    parity._emu = lib
    try:
        return emu_trace(scene, bundle, r_max, **kw)
    finally:
        parity._emu = saved


def _loop_trips(lib):
    return C.c_long.in_dll(lib, "_ZN3bmo16g_emu_union_loopE").value


BUNDLES = {
    "c2s": lambda: (scenes.c2_scene()[0], scenes.c2_survey_bundle(2048)),
    "c2v": lambda: (scenes.c2_scene()[0], scenes.c2_vignetted_bundle(2048)),
    "c2": lambda: (scenes.c2_scene()[0], scenes.c2_bundle(1024)),
    "c5": lambda: (scenes.c5_scene()[0], scenes.c5_bundle(1024)),
}


@pytest.mark.parametrize("name", sorted(BUNDLES))
def test_fastpath_equals_oracle_on_configs(oracle, emus, name):
    system, bundle = BUNDLES[name]()
    scene = bmo.CompiledScene(system, bundle.lambdas)
    before = _loop_trips(emus["on"])
    on = _trace(emus["on"], scene, bundle, 20)
    assert _loop_trips(emus["on"]) > before, "the union fast path was never taken"
    off = _trace(emus["off"], scene, bundle, 20)
    ref = oracle.trace(scene, bundle, 20, threads=4)
    compare(on, ref, 0.0, name + " fast path on")
    compare(off, ref, 0.0, name + " fast path off")
    compare(on, off, 0.0, name + " on vs off")


def test_fastpath_equals_oracle_on_retrace(oracle, emus):
    system, bundle = BUNDLES["c2s"]()
    scene = bmo.CompiledScene(system, bundle.lambdas)
    first = _trace(emus["on"], scene, bundle, 20)
    on = _trace(emus["on"], scene, bundle, 20, prev=first)
    off = _trace(emus["off"], scene, bundle, 20, prev=first)
    compare(on, off, 0.0, "c2s retrace on vs off")


# (seed 119 draws a runaway beam tree: test_fuzz.py skips it)
CASES = [(seed, "ray") for seed in range(101, 125) if seed != 119] + [(seed, "pol") for seed in range(201, 207)] + [(seed, "gauss") for seed in range(301, 307)]


@pytest.mark.parametrize("seed,kind", CASES)
def test_fastpath_equals_oracle_on_random_scenes(oracle, emus, seed, kind):
    scene, bundle = _case(seed, kind, 128 if kind == "ray" else 64)
    on = _engine_first(lambda: _trace(emus["on"], scene, bundle, R_MAX, max_beams=_limit(bundle.n)))
    ref = oracle.trace(scene, bundle, R_MAX, threads=4)
    compare(on, ref, 0.0, "fuzz %d %s fast path on" % (seed, kind))
    off = _trace(emus["off"], scene, bundle, R_MAX, max_beams=_limit(bundle.n))
    compare(on, off, 0.0, "fuzz %d %s on vs off" % (seed, kind))

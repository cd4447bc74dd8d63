"""The scene builder (bmo_scene_blob.hpp: validation, mesh BVHs, blob layout, sweep merge) under AddressSanitizer and
UndefinedBehaviorSanitizer, in a stand-alone program of its own (tests/emu/scene_check.cpp lists what it checks): memory safety of the
builder's offset arithmetic and raw copies, which no test that loads the engine into Python can show."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "emu", "scene_check")


def test_scene_builder_under_sanitizers():
    if not os.path.exists(BIN):
        pytest.skip("tests/emu/scene_check was not built: the host tool chain has no static libasan / libubsan (-fsanitize=address,undefined -static-libasan -static-libubsan)")
    r = subprocess.run([BIN], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.rstrip().endswith("scene_check ok") and r.stdout.count("fnv1a") >= 14

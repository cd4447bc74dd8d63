"""The state-independence rule of DESIGN.md §2 for the entries of include/bmo_sweep_readout.h: what a case of
tests/sweep_readout_cases.py returns depends on its inputs alone.  The legs are those of tests/test_state_independence_gpu.py, whose
runner, comparison and sentinel filler are used here; everything is compared as uint64 words, never as values.

  deterministic   a case run twice, each time after abi.pool_release() (fresh device blocks), gives the same words
  unset outputs   the same words with abi._out handing out buffers of 0x7FF8DEAD words instead of zeros
  history         the same words after every other case, in list order and in reverse order, without a release in between
  poisoned pools  the same words in one fresh child process under BMO_POOL_POISON=1

Every leg compares with the same clean run (the first run of the deterministic leg)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import state_cases as sc
import sweep_readout_cases as sw
from bmo_amd import abi
from test_state_independence_gpu import ABNORMAL_CODES, sentinel_out

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [f.name for f in sw.CASES]
BY_NAME = {f.name: f for f in sw.CASES}
_clean = {}


def clean(name):
    """The clean run of a case: fresh device blocks, zeroed outputs.  Run once per process and never changed."""
    if name not in _clean:
        abi.pool_release()
        _clean[name] = sc.run(BY_NAME[name])
        for v in _clean[name].values():
            v.setflags(write=False)
    return _clean[name]


@pytest.mark.parametrize("name", NAMES)
def test_deterministic(name):
    first = clean(name)
    assert first
    abi.pool_release()
    assert sc.differences(sc.run(BY_NAME[name]), first) == []


def test_the_cases_read_what_they_say():
    """the middle configuration has no rows and reads like a single call without rows, the others have statistics and images"""
    st = clean("psf_focus_stats_sweep")["stats"]
    assert st.shape == (3, sw.M_PLANES, abi.FOCUS_STAT_N) and (st[[0, 2], :, 0] == [[300], [257]]).all() and np.isfinite(st[[0, 2]]).all()
    assert (st[1, :, 0] == 0).all() and np.isnan(st[1, :, 1:]).all()
    I = clean("psf_through_focus_sweep")["field/I"]
    assert I.shape == (3, sw.M_PLANES, 5, 5) and not I[1].any() and (I[[0, 2]].max(axis=(1, 2, 3)) > 0).all()
    for name, key in (("psf_geo_otf_sweep", "centers/"), ("psf_otf_sweep", "image/")):
        got = clean(name)
        assert np.isnan(got[key + "mtf"][1]).all() and not got[key + "otf"][1].any() and not got[key + "sums"][1].any()
        assert np.isfinite(got[key + "mtf"][[0, 2]]).all() and (got[key + "sums"][[0, 2]] > 0).all()


@pytest.mark.parametrize("name", NAMES)
def test_unset_outputs(name, monkeypatch):
    want = clean(name)
    handed = []

    def out(shape, dtype=float):
        handed.append(shape)
        return sentinel_out(shape, dtype)

    monkeypatch.setattr(abi, "_out", out)
    got = sc.run(BY_NAME[name])
    assert sc.differences(got, want) == []
    assert handed, name  # (the swapped helper is the one the wrappers call)


def test_history():
    """Every case after every other one's leftovers: list order, then reverse order, no release in between."""
    want = {name: clean(name) for name in NAMES}
    bad = {}
    for order in (NAMES, NAMES[::-1]):
        for name in order:
            d = sc.differences(sc.run(BY_NAME[name]), want[name])
            if d:
                bad.setdefault(name, []).append(d[:3])
    assert not bad, bad


def _child(out_path):
    """This file as a fresh child process with BMO_POOL_POISON=1 (the knob is read once per process), started the way
    test_state_independence_gpu._child starts its children: one at a time (subprocess.run waits), under a time limit, and an abnormal end
    is reported as it is, without another try."""
    path = os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")] + ([os.environ["PYTHONPATH"]] if os.environ.get("PYTHONPATH") else []))
    env = dict(os.environ, BMO_POOL_POISON="1", PYTHONPATH=path)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), out_path]
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
    except subprocess.TimeoutExpired as e:
        raise AssertionError("the poisoned child ran into its time limit: %s" % str(e.stderr)[-1500:])
    abnormal = r.returncode < 0 or r.returncode in ABNORMAL_CODES
    assert r.returncode == 0, ("abnormal end" if abnormal else "failed", r.returncode, r.stdout[-1500:] + r.stderr[-3000:])


def test_poisoned_pools(tmp_path):
    want = {name: clean(name) for name in NAMES}
    out_path = str(tmp_path / "focus_sweep.npz")
    _child(out_path)
    got = {name: {} for name in NAMES}
    with np.load(out_path) as z:
        for key in z.files:
            name, _, k = key.partition("::")
            got[name][k] = z[key]
    bad = {name: sc.differences(got[name], want[name])[:4] for name in NAMES if sc.differences(got[name], want[name])}
    assert not bad, bad


def _main(out_path):
    assert os.environ.get("BMO_POOL_POISON"), "the child runs under BMO_POOL_POISON"
    flat = {}
    for f in sw.CASES:
        for k, v in sc.run(f).items():
            flat[f.name + "::" + k] = v
    with open(out_path, "wb") as fh:
        np.savez(fh, **flat)


if __name__ == "__main__":
    _main(sys.argv[1])

"""What an entry returns depends on its inputs alone (DESIGN.md §2 "State independence"): not on what the recycled blocks of the device
and pinned pools hold, not on what the caller's output buffers hold, not on the calls before it.  The cases are tests/state_cases.py's;
everything is compared as uint64 / int32 words, never as values.

  deterministic   a case run twice, each time after abi.pool_release() (fresh device blocks), gives the same words
  anchored        the trace cases equal the oracle bit for bit, the spot image and the encircled-energy counts their numpy rules: the
                  file is not the engine compared with itself alone
  unset outputs   with abi._out handing out buffers of 0x7FF8DEAD words instead of zeros, as a caller with uninitialised memory does
  history         all cases in list order, then in reverse order, in one process without a release between them
  poisoned pools  a fresh child process per group with BMO_POOL_POISON=1: every block the pools hand out is filled with 0x7FF8DEAD
                  first (a NaN as FP64 and FP32, a huge index as int32, neither of the engine's own 0 / 0xFF markers)

Every leg compares with the same clean run (the first run of the deterministic leg)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import state_cases as sc
from bmo_amd import abi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x7FF8DEAD
NAMES = [f.name for f in sc.CASES]
BY_NAME = {f.name: f for f in sc.CASES}
_clean = {}


def clean(name):
    """The clean run of a case: fresh device blocks, zeroed outputs.  Run once per process and never changed."""
    if name not in _clean:
        abi.pool_release()
        _clean[name] = sc.run(BY_NAME[name])
        for v in _clean[name].values():
            v.setflags(write=False)
    return _clean[name]


def sentinel_out(shape, dtype=float):
    """abi._out with every 32-bit word 0x7FF8DEAD: 0x7FF8DEAD7FF8DEAD in an FP64 or int64 element, 0x7FF8DEAD in an int32 one"""
    a = np.empty(shape, dtype=dtype)
    assert a.dtype.itemsize in (4, 8)
    a.reshape(-1).view(np.uint32)[:] = SENTINEL
    return a


def test_the_sentinel_is_what_it_is_said_to_be():
    assert np.isnan(sentinel_out(3)).all() and (sentinel_out(3).view(np.uint64) == 0x7FF8DEAD7FF8DEAD).all()
    assert (sentinel_out((2, 2), dtype=np.int64) == 0x7FF8DEAD7FF8DEAD).all() and (sentinel_out(2, dtype=np.int32) == 2147016365).all()
    assert np.isnan(np.array([SENTINEL], dtype=np.uint32).view(np.float32)).all() and sentinel_out(0).shape == (0,)


@pytest.mark.parametrize("name", NAMES)
def test_deterministic(name):
    first = clean(name)
    assert first
    abi.pool_release()
    again = sc.run(BY_NAME[name])
    assert sc.differences(again, first) == []


# ------------------------------------------------------------------------------------------------ anchored
@pytest.mark.parametrize("name", ["trace_ray", "trace_polarized", "trace_gaussian", "retrace_after_a_move", "retrace_device_after_a_move"])
def test_trace_cases_equal_the_oracle(oracle, name):
    from parity import compare

    keep = []
    abi.pool_release()
    got = {k: np.ascontiguousarray(v) for k, v in BY_NAME[name](keep=keep).items()}
    assert sc.differences(got, clean(name)) == []
    assert keep
    for label, res, scene, bundle, r_max, prev_scenes in keep:
        if prev_scenes is None:
            ref = oracle.trace(scene, bundle, r_max, threads=8)
        else:
            _, sol = oracle.trace(prev_scenes[0], bundle, r_max, threads=8, keep=True)
            ref = oracle.trace(scene, bundle, r_max, threads=8, prev=sol)
            sol.free()
        compare(res, ref, 0.0, "%s: %s" % (name, label))
        assert res.n_nodes > res.n_roots  # the splitters made children


def test_device_solves_equal_the_anchored_host_solve():
    """trace_device_views solves trace_ray's scene and bundle from an uploaded batch, with and without the segment log: the whole view of the
    first equals trace_ray's (which the oracle anchors) word for word, and so do the detector tables of the second.  (trace_sweep is not
    anchored here: tests/test_sweep_gpu.py holds a sweep's slices to separate solves.)"""
    got, want = clean("trace_device_views"), clean("trace_ray")
    with_log = {k[len("log/all/"):]: v for k, v in got.items() if k.startswith("log/all/")}
    assert sc.differences(with_log, want) == []
    for k in ("det_count", "det_offset", "det_node", "det_data", "node_root", "node_parent", "node_status"):
        assert sc.differences({k: got["nolog/all/" + k]}, {k: want[k]}) == [], k
    n = int(got["log/count"][0])
    assert n == int(want["det_count"][0]) > 0
    assert sc.differences({"h": got["log/copy_hits"], "c": got["log/copy_hit_columns"]}, {"h": want["det_data"][:n], "c": want["det_data"][:n, :2]}) == []


def test_spot_image_equals_the_binning_rule():
    import spot_ref as sr

    got = clean("spot_image")
    for H in sc.ROW_COUNTS:
        for nx, nz in sc.SPOT_SHAPES:
            want, want_out = sr.bin_rule(sc.spot_rows(H), sc.SPOT_WINDOW, nx, nz)
            img, outside = got["H%d/%dx%d/image" % (H, nx, nz)], got["H%d/%dx%d/outside" % (H, nx, nz)]
            assert img.dtype == np.int64 and np.array_equal(img, want) and int(outside[0]) == want_out, (H, nx, nz)
            assert img.sum() + want_out == H and (H == 0 or img.any())


def test_encircled_counts_equal_the_numpy_rule():
    from test_ee_gpu import _spot_numpy

    got = clean("spot_ee")
    for H in sc.ROW_COUNTS:
        for shape in ("circle", "square"):
            want = _spot_numpy(sc.spot_rows(H), (0.1e-3, -0.05e-3), sc.RADII * 50, shape)
            assert got["H%d/%s" % (H, shape)].dtype == np.int64 and np.array_equal(got["H%d/%s" % (H, shape)], want), (H, shape)
        assert H == 0 or 0 < got["H%d/circle" % H][0] < got["H%d/circle" % H][3]


# ------------------------------------------------------------------------------------------------ unset outputs
# Cases that hand a C entry no output buffer through abi._out: the solves return views of the library's own tables (copied by abi._np), the
# Photodetector sweep's only buffer is field_inout (read and written: zeros by contract), the self-test returns a code.  For these the leg
# is a repeat of the clean run.
NO_OUTPUT_BUFFER = {"trace_ray", "trace_polarized", "trace_gaussian", "retrace_after_a_move", "retrace_device_after_a_move", "trace_sweep",
                    "photodetector_field_sweep", "selftest"}


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
    assert bool(handed) == (name not in NO_OUTPUT_BUFFER), (name, len(handed))  # (the swapped helper is the one the wrappers call)


# ------------------------------------------------------------------------------------------------ history
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


# ------------------------------------------------------------------------------------------------ poisoned pools
_abnormal = []  # the first child that ended abnormally: the remaining poisoned tests fail without starting a process
ABNORMAL_CODES = (134, 139, 124, 137)
LIVE = "__row_behind_the_hits__"


def _child(group, out_path):
    """This file as a fresh child process with BMO_POOL_POISON=1 (the knob is read once per process): it runs the group's cases and writes
    them to out_path.  Never more than one child at a time: subprocess.run waits."""
    path = os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")] + ([os.environ["PYTHONPATH"]] if os.environ.get("PYTHONPATH") else []))
    env = dict(os.environ, BMO_POOL_POISON="1", PYTHONPATH=path)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), group, out_path]
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
    except subprocess.TimeoutExpired as e:
        _abnormal.append((group, "timeout"))
        raise AssertionError("the poisoned child of group %s ran into its time limit: %s" % (group, str(e.stderr)[-1500:]))
    if r.returncode < 0 or r.returncode in ABNORMAL_CODES:
        _abnormal.append((group, r.returncode))
    assert r.returncode == 0, (group, r.returncode, r.stdout[-1500:] + r.stderr[-3000:])


@pytest.mark.parametrize("group", sc.GROUPS)
def test_poisoned_pools(group, tmp_path):
    assert not _abnormal, "not started: the poisoned child %r ended abnormally" % (_abnormal[0],)
    names = [f.name for f in sc.CASES if f.group == group]
    want = {name: clean(name) for name in names}
    out_path = str(tmp_path / (group + ".npz"))
    _child(group, out_path)
    with np.load(out_path) as z:
        got = {name: {} for name in names}
        if group == sc.GROUPS[0]:  # the knob is live: memory no kernel writes holds the poison word, so a child that passes has run on poison
            assert (z[LIVE] == SENTINEL).all(), ["%08X" % w for w in z[LIVE]]
        for key in z.files:
            if key == LIVE:
                continue
            name, _, k = key.partition("::")
            got[name][k] = z[key]
    bad = {name: sc.differences(got[name], want[name])[:4] for name in names if sc.differences(got[name], want[name])}
    assert not bad, bad


def _row_behind_the_hits():
    """The 18 words behind the last written row of a solve's device hit table.  The table is sized by a bound before the counts are known
    (count_and_gather_hits: (beams + roots) / 2 + 1 rows for Rays), only det_count rows of it are ever written: the next row holds what the
    pool handed out."""
    import ctypes as C

    import bmo_amd as bmo
    from test_splitter_chain import _bundle, _chain

    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    bundle = _bundle("ray", 96)
    eng = bmo.Engine(bmo.CompiledScene(_chain(2), bundle.lambdas), 0)
    try:
        batch = eng.upload(bundle)
        h = eng.trace_device(batch, 50)
        try:
            ptr, cnt = eng.result_device_hits(h, 0)
            n_nodes = eng.result_size(h)[2]
            assert 0 < cnt and cnt + 1 <= (n_nodes + bundle.n) // 2 + 1, (cnt, n_nodes)  # the row read lies inside the table
            row = np.zeros(18, dtype=np.uint32)
            assert hip.hipMemcpy(row.ctypes.data, C.c_void_p(ptr + 72 * cnt), 72, 2) == 0  # (2: device to host)
        finally:
            eng.free_result(h)
            eng.free_batch(batch)
    finally:
        eng.close()
    return row


def _main(group, out_path):
    assert os.environ.get("BMO_POOL_POISON"), "the child runs under BMO_POOL_POISON"
    flat = {}
    if group == sc.GROUPS[0]:
        flat[LIVE] = _row_behind_the_hits()
    for f in sc.CASES:
        if f.group == group:
            for k, v in sc.run(f).items():
                flat[f.name + "::" + k] = v
    with open(out_path, "wb") as fh:
        np.savez(fh, **flat)


if __name__ == "__main__":
    _main(sys.argv[1], sys.argv[2])

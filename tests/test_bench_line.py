"""The bench line's contract: `cpu_baseline` and `roofline` are JSON OBJECTS — the driver's parser keeps
nothing else —, the headline workload is SURVEY §8(d)'s literal config-2 bundle, and the per-solve kernel time rides next to the
per-launch average."""
import json
import os
import subprocess
import sys
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    sys.path.insert(0, ROOT)
    import bench

    return bench


def test_cpu_baseline_is_one_object_with_the_contract_keys():
    """bench.cpu_baseline on a small sample of config 1 (CPU only: the oracle and the host build of the lane code)."""
    import bmo_amd as bmo
    from scenes import c1_scene, disc_bundle

    bench = _bench()
    system, _ = c1_scene()
    bundle = disc_bundle(512, center=[0, -0.05, 0], direction=[0, 1, 0], diameter=0.01, lam=1.064e-6)
    case = types.SimpleNamespace(bmo=bmo, scene=bmo.CompiledScene(system, bundle.lambdas), bundle=bundle)
    cb = bench.cpu_baseline(case, 64, 100)
    assert isinstance(cb, dict)
    for rec in (cb, cb["all_cores"], cb["lane_code_all_cores"]):
        assert isinstance(rec, dict)
        assert rec["value"] > 0 and rec["unit"] == "intersections/s" and rec["kind"] == "port"
        assert isinstance(rec["cores"], int) and rec["cores"] >= 1 and isinstance(rec["sample"], str)
        assert rec["nproc"] >= 1 and rec["cpu"]
    assert cb["cores"] == 1  # the headline baseline: the reference's serial trace loop (System.jl:463-468)
    json.dumps(cb)


def test_default_workload_is_the_survey_bundle():
    bench = _bench()
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert 'name = args.workload or ("c5" if multi else "c2s")' in src
    assert bench.CONFIG_KEY["c2"] == "c2_cone" and bench.DEFAULT_RAYS["c2s"] == 1 << 20


@pytest.mark.gpu
def test_bench_line_objects_on_the_gpu():
    """One short run of bench.py itself (small bundle, small CPU sample): the printed line parses and carries the objects."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--rays", "16384", "--cpu-sample", "128", "--no-extras", "--full"]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln][-1]
    out = json.loads(line)
    assert out["metric"] == "ray-surface intersections/s" and out["n_gpus"] == 1 and out["steps"] == 2
    assert out["config"]["name"] == "c2s" and "SURVEY 8(d)" in out["config"]["workload"]
    rl, cb = out["roofline"], out["cpu_baseline"]
    assert isinstance(rl, dict) and isinstance(cb, dict)
    assert rl["bound"] == "hbm" and rl["peak"] == 8000.0 and abs(rl["frac"] - rl["achieved"] / rl["peak"]) < 1e-12
    assert rl["kernel_ms_per_solve"] > 0 and rl["kernel_ms_per_solve"] >= rl["avg_launch_ms"]
    assert rl["valu_issue"] is None  # the committed counter pass is of the default size only: no VALU figure for another bundle size
    assert cb["value"] > 0 and cb["cores"] == 1 and cb["kind"] == "port" and "all_cores" in cb and "lane_code_all_cores" in cb
    assert abs(out["vs_baseline"] - out["value"] / cb["value"]) <= 1e-9 * out["vs_baseline"]


def test_dump_sample_rows_are_fixed_and_bounded():
    """--dump-outputs keeps a short table whole and a long one as the same seeded, ascending sample every time."""
    import numpy as np

    bench = _bench()
    assert np.array_equal(bench._dump_rows(7, 10), np.arange(7))
    a, b = bench._dump_rows(1 << 20, 1000), bench._dump_rows(1 << 20, 1000)
    assert np.array_equal(a, b) and len(a) == 1000 and np.all(np.diff(a) > 0) and a[-1] < 1 << 20


def _join_nonfinite(values, codes):
    """Inverse of bench._split_nonfinite."""
    import numpy as np

    out = values.copy()
    for j in range(values.shape[1]):
        c = (codes[:, j // 26].astype(np.int64) >> (2 * (j % 26))) & 3
        out[c == 1, j], out[c == 2, j], out[c == 3, j] = np.nan, np.inf, -np.inf
    return out


def test_dump_tables_are_finite_and_keep_their_nonfinite_entries():
    """A dumped table holds finite numbers only; NaN / +Inf / -Inf (the engine's t = +Inf of a segment without intersection) come back
    from the code columns, in tables wider than one code column too."""
    import numpy as np

    bench = _bench()
    t = np.random.Generator(np.random.PCG64(1)).normal(size=(50, 35))
    t[3, 0], t[4, 9], t[5, 25], t[6, 26], t[7, 34], t[8, 9] = np.nan, np.inf, -np.inf, np.inf, np.nan, -0.0
    values, codes = bench._split_nonfinite(t)
    assert values.shape == t.shape and codes.shape == (50, 2) and values.dtype == codes.dtype == np.float64
    assert np.isfinite(values).all() and np.isfinite(codes).all() and (codes < 2.0 ** 53).all()
    assert np.array_equal(_join_nonfinite(values, codes), t, equal_nan=True) and np.signbit(values[8, 9])
    assert not codes[np.setdiff1d(np.arange(50), [3, 4, 5, 6, 7])].any()


def _plain_run(dump_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--rays", "16384", "--dump-outputs", str(dump_dir)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln][-1])


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_same_outputs_twice(tmp_path):
    """Without --full the line holds the headline only; --dump-outputs writes the last step's solution, bounded, and a second run
    with the same arguments writes the same arrays."""
    import numpy as np

    out = _plain_run(tmp_path / "a")
    assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["value"] > 0 and out["dtype"] == "f64" and out["higher_is_better"] is True
    assert out["metric"] == "ray-surface intersections/s" and out["unit"] == "intersections/s"
    assert not {"cpu_baseline", "configs", "pcie", "one_gpu_same_workload"} & set(out) and out["vs_baseline"] is None
    names = sorted(os.listdir(tmp_path / "a"))
    assert {"counts.npy", "nodes.npy", "segments.npy", "det0_hits.npy"} <= set(names)
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64 << 20
    counts = np.load(tmp_path / "a" / "counts.npy")
    cfg = out["config"]
    assert counts[0] == cfg["intersect3d_calls_per_step"] and counts[1] == cfg["segments_per_step"] and counts[2] == cfg["beam_nodes"]
    assert counts[3:].sum() == cfg["detector_hits"]
    assert all(np.isfinite(np.load(tmp_path / "a" / n)).all() for n in names)
    seg = np.load(tmp_path / "a" / "segments.npy")
    assert seg.dtype == np.float64 and seg.shape == (cfg["segments_per_step"], 2 + 11)
    # the record's length t (column 2 + 7) is +Inf exactly on the segments without intersection (object id -1)
    full = _join_nonfinite(seg, np.load(tmp_path / "a" / "segments_nonfinite.npy"))
    assert np.array_equal(np.isposinf(full[:, 9]), seg[:, 0] == -1) and (seg[:, 0] == -1).any()
    assert np.isfinite(np.delete(full, 9, axis=1)).all()
    _plain_run(tmp_path / "b")
    assert sorted(os.listdir(tmp_path / "b")) == names
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b, equal_nan=True), n


def test_valu_issue_figure_reads_the_committed_counter_pass():
    """roofline.valu_issue: vector instructions per solve from the committed SQ pass over the live kernel time, against 256 CUs x 4 SIMDs x 2.4 GHz / 4."""
    bench = _bench()
    tj = json.load(open(os.path.join(ROOT, "profiles", "r04_traffic.json")))["c2s"]
    v = bench.valu_issue("c2s", 1 << 20, 100, 3.0)
    assert v["peak"] == 256 * 4 * 2.4e9 / 4 and v["wave_instructions_per_solve"] == tj["valu_wave_instructions"]
    assert abs(v["achieved"] - tj["valu_wave_instructions"] / 3.0e-3) <= 1e-6 * v["achieved"] and abs(v["frac"] - v["achieved"] / v["peak"]) < 1e-12
    assert 0.2 < v["fp64_arithmetic_share"] < 0.8
    assert bench.valu_issue("c2s", 1 << 16, 100, 3.0) is None and bench.valu_issue("c2s", 1 << 20, 50, 3.0) is None

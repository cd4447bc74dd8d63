"""What a solve costs outside its step kernels: total_ms - kernel_ms of Engine.result_timing (device time between the events around the
whole solve and around the step launches) for one bench workload, min / median / max over the solves; library from BMO_ENGINE_LIB.
    python tools/finish_pass_times.py c2s [rays [solves]]"""
import os, statistics, sys
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import bmo_amd as bmo
import bench

name = sys.argv[1] if len(sys.argv) > 1 else "c2s"
n = int(sys.argv[2]) if len(sys.argv) > 2 and int(sys.argv[2]) else bench.DEFAULT_RAYS[name]
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 12
system, bundle, _ = bench.workload(name, n)
scene = bmo.CompiledScene(system, bundle.lambdas)
eng = bmo.Engine(scene, 0)
dev = eng.upload(bundle)
k, t = [], []
for rep in range(reps + 2):
    res = eng.trace_device(dev, 100)
    kms, tms, nl = eng.result_timing(res)
    eng.free_result(res)
    if rep >= 2:  # (the first solves size the pools and have no tile costs yet)
        k.append(kms); t.append(tms)
eng.free_batch(dev); eng.close()
o = [b - a for a, b in zip(k, t)]
f = lambda v: "%.4f / %.4f / %.4f" % (min(v), statistics.median(v), max(v))
print("%-20s %-4s rays %8d  kernel_ms %s  total_ms %s  total - kernel %s  (min / median / max of %d solves, %d launches)" % (
    os.environ.get("BMO_ENGINE_LIB", "default")[-20:], name, n, f(k), f(t), f(o), reps, nl), flush=True)

"""Resource usage (VGPRs, SGPRs, scratch, LDS, occupancy, the compiler's SGPR / VGPR spill counts) of the step and read-out kernels and of the
ordering / finish-pass helpers (tree_*, hit_*):
    python tools/kernel_resources.py [extra hipcc flags]          (-DBMO_DEV_RAY_LDS_ONLY: the Ray kernels of the plain-shapes level only, ~2 min)
    python tools/kernel_resources.py --log <file>                 (reads the remarks of a build made with -Rpass-analysis=kernel-resource-usage)"""
import os, re, subprocess, sys
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # the compiler, its flags and the sources are the build script's

cmd = [g.HIPCC] + g.HIP_FLAGS + ["-I", os.path.join(ROOT, "include"), "-o", "/tmp/kr_lib.so", g.engine_sources()[0],
                                 "-Rpass-analysis=kernel-resource-usage"] + sys.argv[1:]
if sys.argv[1:2] == ["--log"]:
    out = open(sys.argv[2]).read()
else:
    out = subprocess.run(cmd, capture_output=True, text=True).stderr
cur = None
rows = {}
for line in out.splitlines():
    m = re.search(r"Function Name: (\S+)", line)
    if m:
        cur = m.group(1); rows[cur] = {}
        continue
    m = re.search(r"\s(TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]|SGPRs Spill|VGPRs Spill): (\d+)", line)
    if m and cur:
        rows[cur][m.group(1).replace("s Spill", "spill").split()[0]] = int(m.group(2))
    if "error" in line:
        print(line)
for k, v in rows.items():
    if "step_kernel" in k or "psf" in k or "spot" in k or "sum_reduce" in k or "hit_" in k or "tree_" in k:
        name = subprocess.run(["c++filt", k], capture_output=True, text=True).stdout.strip().replace("(anonymous namespace)::", "")
        print("%-58s VGPR %3d SGPR %3d scratch %4d LDS %5d occ %d  spilled SGPR %3d VGPR %3d" % (name[:58], v.get("VGPRs", -1), v.get("TotalSGPRs", -1), v.get("ScratchSize", -1),
                                                                                                   v.get("LDS", -1), v.get("Occupancy", -1), v.get("SGPRspill", -1), v.get("VGPRspill", -1)))

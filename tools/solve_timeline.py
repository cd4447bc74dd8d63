"""What one solve queues on the device, read from a `rocprofv3 --kernel-trace --memory-copy-trace --stats --output-format csv -d DIR` run of
bench.py: every kernel and copy from the init_roots_kernel of the last but one solve in the trace (or of the solve numbered by the second
argument, 0 = first) to the init_roots_kernel of the next solve, with start, own time and the idle gap in front of it; then the totals.
Copies from and to pinned memory are kernels here (__amd_rocclr_copyBuffer), a memset is __amd_rocclr_fillBufferAligned.
    python tools/solve_timeline.py DIR [solve]"""
import csv, glob, os, re, sys

d = sys.argv[1]
ops = []  # (start ns, end ns, name)


def rows(pattern):
    for path in glob.glob(os.path.join(d, "**", pattern), recursive=True):
        with open(path, newline="") as f:
            yield from csv.DictReader(f)


def short(name):
    name = name.replace("(anonymous namespace)::", "")
    m = re.search(r"rocprim::\w+::detail::(\w+?)<", name)
    if m and "trampoline" in name:  # rocprim's kernels go through one trampoline: name the algorithm's configuration
        inner = re.search(r"wrapped_(\w+?)_config", name)
        return "rocprim " + (inner.group(1) if inner else m.group(1)) + " " + str(len(name))  # (the length tells the instantiations apart)
    m = re.search(r"rocprim::\w+::detail::(\w+)", name)
    if m:
        return "rocprim " + m.group(1)
    name = re.sub(r"^void ", "", name)
    return name.split("(")[0][:60]


for r in rows("*kernel_trace.csv"):
    ops.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])))
for r in rows("*memory_copy_trace.csv"):
    ops.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "copy " + r.get("Direction", "?").replace("MEMORY_COPY_", "")))
ops.sort()
starts = [i for i, o in enumerate(ops) if o[2].startswith("init_roots_kernel")]
if not starts:
    raise SystemExit("no init_roots_kernel in the trace")
if len(starts) < 2:
    raise SystemExit("the trace holds fewer than two solves")
which = int(sys.argv[2]) if len(sys.argv) > 2 else len(starts) - 2
# one period of the steady state: from the init_roots_kernel of a solve to that of the next one, so the fill and the copy the NEXT solve
# queues in front of its init_roots_kernel stand at the end of the list (the bench frees the result in between)
lo, hi = starts[which], starts[which + 1]
sel = ops[lo:hi]
t0 = sel[0][0]
print("solve %d of %d: %d operations (%d kernels, %d copies)" % (which, len(starts), len(sel), sum(not o[2].startswith("copy") for o in sel),
                                                                 sum(o[2].startswith("copy") for o in sel)))
print("%10s %9s %9s  %s" % ("start us", "own us", "gap us", "operation"))
prev_end = None
busy = gaps = 0
for s, e, name in sel:
    gap = 0 if prev_end is None else s - prev_end
    print("%10.1f %9.1f %9.1f  %s" % ((s - t0) / 1e3, (e - s) / 1e3, gap / 1e3, name))
    busy += e - s
    gaps += max(gap, 0)
    prev_end = e if prev_end is None else max(prev_end, e)
step = [o for o in sel if o[2].startswith("step_kernel")]
print("span %.1f us: operations %.1f us (step kernels %.1f us), idle gaps %.1f us" % ((prev_end - t0) / 1e3, busy / 1e3, sum(e - s for s, e, _ in step) / 1e3, gaps / 1e3))

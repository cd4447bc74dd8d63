"""Share of the union evaluations per bounce level that the union fast path of tracing_step can take (csrc/bmo_lane.hpp), counted by the
host emulator with the fast path forced on (CPU only): python tools/fastpath_stats.py [N] [c2|c2s|c2v|c5].  Prints emu_stats.py's lines, each
followed by the level's union evaluations, those decided by the one `others_lb` compare, and those run in the specialised loop, and by the
level's outside-march trips on single plain shapes, generic and in the loop (BMO_LEAF_MARCH=0 in the environment: the loop without them).
The last two lines: how the SDF marches ended, and how those ended that the box cull takes (they run all the same here, to be tallied)."""
import ctypes as C, os, subprocess, sys, tempfile
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import bmo_amd as bmo, parity, scenes
from bmo_amd import abi
so = os.path.join(tempfile.mkdtemp(), "libbmo_emu_fastpath.so")
subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-DBMO_EMU_STATS", "-DBMO_EMU_BOX_SHADOW", "-DBMO_MARCH_FASTPATH=2",
                       "-DBMO_LEAF_MARCH=" + os.environ.get("BMO_LEAF_MARCH", "1"), "-shared", "-o", so,
                       os.path.join(ROOT, "tools/fastpath_stats.cpp")])
emu = C.CDLL(so)
emu.bmo_emu_trace.argtypes = [C.POINTER(abi.SceneDesc), C.POINTER(abi.RayBatch), C.POINTER(abi.TraceOpts), C.POINTER(C.c_void_p), C.POINTER(abi.ResultView)]
emu.bmo_emu_free.argtypes = [C.c_void_p]
emu.bmo_fastpath_totals.argtypes = []
parity._emu = emu
n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
which = sys.argv[2] if len(sys.argv) > 2 else "c2s"
system, _ = scenes.c5_scene() if which == "c5" else scenes.c2_scene()
b = {"c2v": scenes.c2_vignetted_bundle, "c2s": scenes.c2_survey_bundle, "c5": scenes.c5_bundle}.get(which, scenes.c2_bundle)(n)
parity.emu_trace(bmo.CompiledScene(system, b.lambdas), b, 20)
sys.stderr.flush()
emu.bmo_fastpath_totals()

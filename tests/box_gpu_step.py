"""One GPU step of tests/test_box_cull_gpu.py, run as a process of its own under that test's time limit:
    python tests/box_gpu_step.py baseline <c2s|c5|c3|c4> <rays> | retrace | sweep | directed <name>
Prints "equal" and exits 0 when the engine's result equals the oracle's at zero tolerance."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE, os.path.join(os.path.dirname(HERE), "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import bmo_amd as bmo  # noqa: E402
import box_scenes as bx  # noqa: E402
import pyoracle  # noqa: E402
import scenes  # noqa: E402
from parity import compare  # noqa: E402

mm = 1e-3


def engine_vs_oracle(scene, bundle, r_max, label):
    eng = bmo.Engine(scene, 0)
    try:
        got = eng.trace(bundle, r_max)
    finally:
        eng.close()
    ref = pyoracle.trace(scene, bundle, r_max, threads=16)
    compare(got, ref, 0.0, label)
    bx.hits_inside_boxes(scene, ref)


def main(argv):
    what = argv[0]
    if what == "baseline":
        scene_fn, bundle_fn = {"c2s": (scenes.c2_scene, scenes.c2_survey_bundle), "c5": (scenes.c5_scene, scenes.c5_bundle),
                               "c3": (scenes.c2_scene, scenes.c3_bundle), "c4": (scenes.c4_scene, scenes.c4_bundle)}[argv[1]]
        bundle = bundle_fn(int(argv[2]))
        engine_vs_oracle(bmo.CompiledScene(scene_fn()[0], bundle.lambdas), bundle, 100, argv[1])
    elif what == "retrace":
        from test_fuzz import R_MAX, _retrace_case

        scene0, scene1, bundle = _retrace_case(401, "ray", 2048)
        g0, h0 = bmo.system._engine_solve(scene0, bundle, R_MAX, None)
        g1, h1 = bmo.system._engine_solve(scene1, bundle, R_MAX, h0)
        a0, sol = pyoracle.trace(scene0, bundle, R_MAX, threads=16, keep=True)
        a1 = pyoracle.trace(scene1, bundle, R_MAX, threads=16, prev=sol)
        compare(g0, a0, 0.0, "first solve")
        compare(g1, a1, 0.0, "retrace")
        h0.free()
        h1.free()
    elif what == "sweep":
        from test_sweep_gpu import _sweep_vs_separate

        system, a, b = bx.two_lenses()
        bundle = scenes.disc_bundle(512, [0, -10 * mm, 0], [0, 1, 0], 11 * mm, lam=bx.LAM, seed=21, cone=0.1)
        # configuration 1 moves the second lens 9 mm sideways: rays that went through it now pass its box, and the other way round
        snaps = bmo.sweep_snapshots(system, bundle.lambdas, 2, lambda c: bmo.translate3d(b, [9 * mm * c, 0, 0]))[0]
        t0, t1 = bx.box_table(snaps[0])[0], bx.box_table(snaps[1])[0]
        sid = snaps[0].shape_id(b.shape)
        assert abs((t1[sid, 0] - t0[sid, 0]) - 9 * mm) < 1e-12 and (t0[snaps[0].shape_id(a.shape)] == t1[snaps[0].shape_id(a.shape)]).all()
        res = _sweep_vs_separate(snaps, [bundle, bundle], bx.R_MAX, label="box sweep", oracle=pyoracle, oracle_every=1)
        assert res.n_roots == 2 * bundle.n
    elif what == "directed":
        scene, bundle = bx.DIRECTED[argv[1]]()
        engine_vs_oracle(scene, bundle, bx.R_MAX, argv[1])
    else:
        raise SystemExit("unknown step %r" % what)
    print("equal")


if __name__ == "__main__":
    main(sys.argv[1:])

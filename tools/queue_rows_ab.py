"""GPU box: what the row windows of the traversal queue (RT_TRAVQ_ROWS, csrc/rt_qrows.h) remove from the headline frame, and what that buys.

  1. the frame's counters with the windows on and off, through both counting instantiations (the binary32 pairs, and with RT_TRAVQ_QW_COUNT=1 the production kernel's):
     queue fetches, and the rays, box tests, nodes and triangle tests that must not move;
  2. bench.py, interleaved, at least three runs each in a fresh process: this build, this build with RT_TRAVQ_ROWS=0 and, with --parent-lib, the parent commit's library
     (RT_LIB); with --dump-dir the first run of this build and of the parent also write --dump-outputs, and frame.npy of the two is compared bit for bit.

usage: python tools/queue_rows_ab.py [--parent-lib PATH] [--runs 3] [--dump-dir DIR] > profiles/queue_rows/ab_bench.txt"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", default="")
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--dump-dir", default="")
ap.add_argument("--no-counters", action="store_true")
args = ap.parse_args()

if not args.no_counters:
    import raytracinggpu_amd as rt
    from raytracinggpu_amd import hostlib
    v, t = rt.scenes.load_cat_arrays()
    mesh = hostlib.build_mesh(v, t, albedo=rt.scenes.CAT_ALBEDO, object_slot=rt.scenes.mesh_slot("cpu"))
    for qw in ("0", "1"):
        os.environ["RT_TRAVQ_QW_COUNT"] = qw
        per = {}
        for rows in ("1", "0"):
            os.environ["RT_TRAVQ_ROWS"] = rows
            c = rt.Context(0)
            c.scene_upload(rt.scenes.spheres("cpu"), mesh)
            per[rows] = c.count_work(rt.make_params(1920, 1080, 1, 3, **rt.scenes.CPU_LAUNCHER), detail=True)
            print("RT_TRAVQ_QW_COUNT=%s RT_TRAVQ_ROWS=%s headline frame: %s" % (qw, rows, json.dumps(per[rows])), flush=True)
            c.close()
        on, off = per["1"], per["0"]
        print("RT_TRAVQ_QW_COUNT=%s: fetches %d -> %d (%.1f %% fewer); rays / box tests / nodes / triangle tests %s" % (
            qw, off["steps"]["fetches"], on["steps"]["fetches"], 100 * (1 - on["steps"]["fetches"] / off["steps"]["fetches"]),
            "the same" if all(on[k] == off[k] for k in ("rays", "box_tests", "nodes", "tri_tests")) else "DIFFER"), flush=True)
    os.environ.pop("RT_TRAVQ_ROWS")
    os.environ.pop("RT_TRAVQ_QW_COUNT")

builds = [("branch", {}), ("branch RT_TRAVQ_ROWS=0", {"RT_TRAVQ_ROWS": "0"})]
if args.parent_lib:
    builds.insert(1, ("parent", {"RT_LIB": os.path.abspath(args.parent_lib)}))
ms = {name: [] for name, _ in builds}
for r in range(args.runs):
    for name, extra in builds:
        env = dict(os.environ, **extra)
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "60", "--warmup", "5"]
        if args.dump_dir and r == 0 and name in ("branch", "parent"):
            cmd += ["--dump-outputs", os.path.join(args.dump_dir, name)]
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, cwd=ROOT, timeout=170)
        if p.returncode != 0:
            print("bench %s failed (%d): %s" % (name, p.returncode, p.stderr[-400:]), flush=True)
            sys.exit(1)
        d = json.loads(p.stdout.strip().splitlines()[-1])
        ms[name].append(d["ms_per_step"])
        print("bench %-24s %.4f ms per frame, %.0f Mrays/s" % (name + ":", d["ms_per_step"], d["value"]), flush=True)
med = {}
for name, _ in builds:
    x = sorted(ms[name])
    med[name] = x[len(x) // 2]
    print("%-24s median %.4f ms (min %.4f, max %.4f, spread %.4f)" % (name + ":", med[name], x[0], x[-1], x[-1] - x[0]))
if args.parent_lib:
    sp = max(ms["parent"]) - min(ms["parent"])
    print("branch - parent: %+.4f ms (%+.2f %%); three times the parent's spread: %.4f ms" % (med["branch"] - med["parent"], 100 * (med["branch"] / med["parent"] - 1), 3 * sp))
print("the row windows alone (branch - branch RT_TRAVQ_ROWS=0): %+.4f ms" % (med["branch"] - med["branch RT_TRAVQ_ROWS=0"]))
if args.parent_lib:
    if args.dump_dir:
        import numpy as np
        a, b = (np.load(os.path.join(args.dump_dir, n, "frame.npy")) for n in ("branch", "parent"))
        print("frame.npy of branch and parent: %s" % ("bit-identical" if a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)) else "DIFFERENT"))

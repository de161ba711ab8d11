"""GPU box: what the dead-channel rule (RT_DEAD_CHANNELS, rt_wavefront.hip.h wf_dead_channels) removes from the headline frame, and what that buys.

  1. the frame's counters with the rule on and off (RT_TRAVQ_QW_COUNT=1: the production kernels' counting instantiation): BOX and TRI steps, rays handed to the traversal,
     rays elided, paths outside the rule's guarantee;
  2. the share of shadow rays elided per segment: frames of 0 .. 3 bounces trace the same paths one segment further each, so the difference of two consecutive frames'
     counters is one segment's; set against the walls-only model of the issue (67 / 79 / 92 % for segments 1 / 2 / 3);
  3. bench.py, interleaved, at least three runs each: this build, this build with RT_DEAD_CHANNELS=0 and, with --parent-lib, the parent commit's library (RT_LIB).

usage: python tools/dead_channels_ab.py [--parent-lib PATH] [--runs 3] > profiles/dead_channels/ab_bench.txt"""
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
ap.add_argument("--no-counters", action="store_true")
args = ap.parse_args()

if not args.no_counters:
    os.environ["RT_TRAVQ_QW_COUNT"] = "1"
    import raytracinggpu_amd as rt
    from raytracinggpu_amd import hostlib
    v, t = rt.scenes.load_cat_arrays()
    mesh = hostlib.build_mesh(v, t, albedo=rt.scenes.CAT_ALBEDO, object_slot=rt.scenes.mesh_slot("cpu"))
    per = {}
    for rule in ("1", "0"):
        os.environ["RT_DEAD_CHANNELS"] = rule
        c = rt.Context(0)
        c.scene_upload(rt.scenes.spheres("cpu"), mesh)
        for b in (3, 0, 1, 2):
            w = c.count_work(rt.make_params(1920, 1080, 1, b, **rt.scenes.CPU_LAUNCHER), detail=True)
            per[rule, b] = w
            if b == 3:
                print("RT_DEAD_CHANNELS=%s headline frame: %s" % (rule, json.dumps(w)), flush=True)
        c.close()
    os.environ.pop("RT_DEAD_CHANNELS")
    os.environ.pop("RT_TRAVQ_QW_COUNT")
    on, off = per["1", 3], per["0", 3]
    tr = lambda w: w["dead_channels"]["trav_continuation"] + w["dead_channels"]["trav_shadow"]
    print("rays handed to the traversal: %d -> %d (%.1f %% fewer); BOX steps %d -> %d (%.1f %%), TRI steps %d -> %d (%.1f %%)" % (
        tr(off), tr(on), 100 * (1 - tr(on) / tr(off)), off["steps"]["box_steps"], on["steps"]["box_steps"], 100 * (1 - on["steps"]["box_steps"] / off["steps"]["box_steps"]),
        off["steps"]["tri_steps"], on["steps"]["tri_steps"], 100 * (1 - on["steps"]["tri_steps"] / off["steps"]["tri_steps"])))
    print("shadow rays that reach the traversal with the rule off (they pass the root box, their direct term is not +0 and no sphere shades them), and of those the ones the rule elides:")
    model = {1: 67, 2: 79, 3: 92}
    for d in range(4):
        sh = lambda rule: per[rule, d]["dead_channels"]["trav_shadow"] - (per[rule, d - 1]["dead_channels"]["trav_shadow"] if d else 0)
        el = per["1", d]["dead_channels"]["elided"] - (per["1", d - 1]["dead_channels"]["elided"] if d else 0)
        print("  segment %d: %9d, elided %9d = %5.1f %%  (walls-only model: %s); elided before the root test, all of the segment: %d" % (
            d, sh("0"), sh("0") - sh("1"), 100.0 * (sh("0") - sh("1")) / max(sh("0"), 1), ("%d %%" % model[d]) if d in model else "-", el), flush=True)

builds = [("branch", {}), ("branch RT_DEAD_CHANNELS=0", {"RT_DEAD_CHANNELS": "0"})]
if args.parent_lib:
    builds.insert(1, ("parent", {"RT_LIB": os.path.abspath(args.parent_lib)}))
ms = {name: [] for name, _ in builds}
for r in range(args.runs):
    for name, extra in builds:
        env = dict(os.environ, **extra)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "60", "--warmup", "5"], env=env, capture_output=True, text=True, cwd=ROOT, timeout=170)
        if p.returncode != 0:
            print("bench %s failed (%d): %s" % (name, p.returncode, p.stderr[-400:]), flush=True)
            sys.exit(1)
        d = json.loads(p.stdout.strip().splitlines()[-1])
        ms[name].append(d["ms_per_step"])
        print("bench %-26s %.4f ms per frame, %.0f Mrays/s" % (name + ":", d["ms_per_step"], d["value"]), flush=True)
for name, _ in builds:
    x = sorted(ms[name])
    print("%-26s median %.4f ms (min %.4f, max %.4f)" % (name + ":", x[len(x) // 2], x[0], x[-1]))

"""GPU box: what the first-hit cache (RT_FIRST_HIT_CACHE, rt_ctx::FirstHit) takes off a frame of a still camera.

  1. the cache's counters over four frames of the workload on one context (one fill per sub-frame, then skips), so that the figures below are known to be a cached frame's;
     then, in one process, frames of a still camera against frames that each miss (a cold frame every time), with the knob on and off;
  2. bench.py, interleaved, at least three runs each in a fresh process: this build, the parent commit's library (--parent-lib, through RT_LIB) and this build with
     RT_FIRST_HIT_CACHE=0 -- the figure of a moving camera; with --dump-dir the first run of this build and of the parent also write --dump-outputs, and frame.npy of the
     two is compared bit for bit.

usage: python tools/first_hit_cache_ab.py [--parent-lib PATH] [--runs 3] [--dump-dir DIR] [--width 1920 --height 1080 --spp 1 --bounces 3] > profiles/first_hit_cache/ab_bench.txt"""
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
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--spp", type=int, default=1)
ap.add_argument("--bounces", type=int, default=3)
args = ap.parse_args()
shape = ["--width", str(args.width), "--height", str(args.height), "--spp", str(args.spp), "--bounces", str(args.bounces)]
print("workload: cat %dx%d, %d sample(s), %d bounces; bench.py --gpus 1 --steps 60 --warmup 5" % (args.width, args.height, args.spp, args.bounces), flush=True)

if not args.no_counters:
    import raytracinggpu_amd as rt
    from raytracinggpu_amd import hostlib
    v, t = rt.scenes.load_cat_arrays()
    mesh = hostlib.build_mesh(v, t, albedo=rt.scenes.CAT_ALBEDO, object_slot=rt.scenes.mesh_slot("cpu"))
    c = rt.Context(0)
    c.scene_upload(rt.scenes.spheres("cpu"), mesh)
    p = rt.make_params(args.width, args.height, args.spp, args.bounces, **rt.scenes.CPU_LAUNCHER)
    for k in range(4):
        c.render(p)
        print("frame %d on one context: %s" % (k, json.dumps(c.first_hit_cache_counts())), flush=True)
    c.close()

    # 1b. in one process, pipelined into two buffers as bench.py renders: a still camera, and a camera that no frame shares with the one before it (tri_tmin alternates
    #     between two neighbouring floats: every frame a key miss and a refill -- a COLD frame each time), on a default context and on one with the knob off
    import numpy as np
    import torch
    from raytracinggpu_amd._capi import Rows

    def per_frame(ctx, frames, warm=10, n=40):
        rows = Rows(0, args.height, args.height, 1)
        bufs = [torch.zeros((args.height, args.width, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
        stream = torch.cuda.Stream()
        ctx.set_pipelining(True)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for k in range(warm + n):
            if k == warm:
                t0.record(stream)
            ctx.render_device(frames[k % len(frames)], rows, bufs[k % 2].data_ptr(), stream.cuda_stream)
        t1.record(stream)
        t1.synchronize()
        ctx.set_pipelining(False)
        return t0.elapsed_time(t1) / n

    t_a = 1e-4
    t_b = float(np.nextafter(np.float32(t_a), np.float32(1.0)))
    still = [p]
    moving = [rt.make_params(args.width, args.height, args.spp, args.bounces, **dict(rt.scenes.CPU_LAUNCHER, tri_tmin=t)) for t in (t_a, t_b)]
    for knob in ("1", "0"):
        os.environ["RT_FIRST_HIT_CACHE"] = knob
        c = rt.Context(0)
        c.scene_upload(rt.scenes.spheres("cpu"), mesh)
        for rep in range(3):
            a, b = per_frame(c, still), per_frame(c, moving)
            print("RT_FIRST_HIT_CACHE=%s in one process, 40 pipelined frames: still camera %.4f ms per frame, every frame cold %.4f ms" % (knob, a, b), flush=True)
        print("RT_FIRST_HIT_CACHE=%s counters: %s" % (knob, json.dumps(c.first_hit_cache_counts())), flush=True)
        c.close()
    os.environ.pop("RT_FIRST_HIT_CACHE")

builds = [("branch", {}), ("branch RT_FIRST_HIT_CACHE=0", {"RT_FIRST_HIT_CACHE": "0"})]
if args.parent_lib:
    builds.insert(1, ("parent", {"RT_LIB": os.path.abspath(args.parent_lib)}))
ms = {name: [] for name, _ in builds}
for r in range(args.runs):
    for name, extra in builds:
        env = dict(os.environ, **extra)
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "60", "--warmup", "5"] + shape
        if args.dump_dir and r == 0 and name in ("branch", "parent"):
            cmd += ["--dump-outputs", os.path.join(args.dump_dir, name)]
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, cwd=ROOT, timeout=170)
        if p.returncode != 0:
            print("bench %s failed (%d): %s" % (name, p.returncode, p.stderr[-400:]), flush=True)
            sys.exit(1)
        d = json.loads(p.stdout.strip().splitlines()[-1])
        ms[name].append(d["ms_per_step"])
        print("bench %-28s %.4f ms per frame, %.0f Mrays/s" % (name + ":", d["ms_per_step"], d["value"]), flush=True)
med = {}
for name, _ in builds:
    x = sorted(ms[name])
    med[name] = x[len(x) // 2]
    print("%-28s median %.4f ms (min %.4f, max %.4f, spread %.4f)" % (name + ":", med[name], x[0], x[-1], x[-1] - x[0]))
off = "branch RT_FIRST_HIT_CACHE=0"
if args.parent_lib:
    sp = max(ms["parent"]) - min(ms["parent"])
    print("branch - parent: %+.4f ms (%+.2f %%); three times the parent's spread: %.4f ms; every run of the branch below every run of the parent: %s" % (
        med["branch"] - med["parent"], 100 * (med["branch"] / med["parent"] - 1), 3 * sp, max(ms["branch"]) < min(ms["parent"])))
    print("knob off - parent: %+.4f ms (%+.2f %%); the parent's spread: %.4f ms" % (med[off] - med["parent"], 100 * (med[off] / med["parent"] - 1), sp))
print("the cache alone (branch - branch RT_FIRST_HIT_CACHE=0): %+.4f ms (%+.2f %%)" % (med["branch"] - med[off], 100 * (med["branch"] / med[off] - 1)))
if args.parent_lib and args.dump_dir:
    import numpy as np
    a, b = (np.load(os.path.join(args.dump_dir, n, "frame.npy")) for n in ("branch", "parent"))
    print("frame.npy of branch and parent: %s" % ("bit-identical" if a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)) else "DIFFERENT"))

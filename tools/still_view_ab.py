"""GPU box: what one level of the still view (csrc/rt_still.h) takes off a frame -- --knob RT_FIRST_HIT_CACHE (a still camera),
RT_FIRST_SHADOW_CACHE or RT_FIRST_SHADE_CACHE (a still view under a still light) -- and whether a change of the host code moved a frame at all.  --knob RT_CHAIN_ENDS:
the same steps for the kernel of a plain chain's last launch (csrc/rt_wavefront.hip.h CLOSE), which every frame runs, a still view or not.  --knob RT_STREAM_POLICY: the
same steps for the cache policy of wf_advance's use-once streams (kPol*), on = both groups (the default), --also 1,2 each group alone.  --knob RT_DEAD_LAST: the same
steps for the rule that leaves a dead path's last continuation ray out of the traversal (csrc/rt_deadlast.h), which every frame of a permitted scene runs.  --also V[,V] adds this
build with the knob at each further value to the interleaved runs (an experimental build that knows more than on and off).

For the headline frame and then for BASELINE config 2 (--width 512 --height 512 --spp 8), each step a process of its own under its own time limit, the first failure
ending the run:
  1. (--stage inproc) the counters of the three levels over five frames of the workload on one context (fill, read and store, then every chain resumes), so that the
     figures below are known to be a resumed frame's; then, in one process, 40 pipelined frames of a still view against 40 frames that each miss the knob's level and
     nothing below it -- tri_tmin (first-hit) or the light's x (the other two) alternates between two neighbouring floats -- with the knob on and off, three times;
     the same stage once more on the parent commit's library (--parent-lib, through RT_LIB);
  2. bench.py --gpus 1 --steps 60 --warmup 5, interleaved, --runs (at least five) each in a fresh process: this build, the parent commit's library and this build with
     the knob off; with --dump-dir the first run of this build and of the parent also write --dump-outputs, and frame.npy of the two is compared bit for bit.

usage: python tools/still_view_ab.py --knob RT_FIRST_SHADE_CACHE --parent-lib PATH [--runs 5] [--dump-dir DIR] [--only headline|spp8] > profiles/still_view/ab_bench.txt"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CACHES = ["RT_FIRST_HIT_CACHE", "RT_FIRST_SHADOW_CACHE", "RT_FIRST_SHADE_CACHE"]
KNOBS = CACHES + ["RT_CHAIN_ENDS", "RT_STREAM_POLICY", "RT_DEAD_LAST"]
ap = argparse.ArgumentParser()
ap.add_argument("--knob", required=True, choices=KNOBS)
ap.add_argument("--parent-lib", default="")
ap.add_argument("--also", default="", help="further values of the knob, comma separated: a build each in the interleaved runs")
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--dump-dir", default="")
ap.add_argument("--only", default="", choices=["", "headline", "spp8"])
ap.add_argument("--stage", default="", choices=["", "inproc"])
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--spp", type=int, default=1)
ap.add_argument("--bounces", type=int, default=3)
args = ap.parse_args()
KNOB = args.knob
ON = "3" if KNOB == "RT_STREAM_POLICY" else "1"                       # the knob's value that turns on all there is


def inproc():
    import numpy as np
    import torch
    import raytracinggpu_amd as rt
    from raytracinggpu_amd import hostlib
    from raytracinggpu_amd._capi import Rows
    v, t = rt.scenes.load_cat_arrays()
    mesh = hostlib.build_mesh(v, t, albedo=rt.scenes.CAT_ALBEDO, object_slot=rt.scenes.mesh_slot("cpu"))
    params = lambda **kw: rt.make_params(args.width, args.height, args.spp, args.bounces, **dict(rt.scenes.CPU_LAUNCHER, **kw))
    p = params()
    c = rt.Context(0)
    c.scene_upload(rt.scenes.spheres("cpu"), mesh)
    which = "parent library" if os.environ.get("RT_LIB") else "this build"

    def counters(ctx):
        return ", ".join("%s %s" % (k[3:-6].lower().replace("_", "-"), json.dumps(getattr(ctx, k[3:].lower() + "_counts")())) for k in reversed(CACHES))
    for k in range(5):
        c.render(p)
        print("%s, frame %d on one context: %s" % (which, k, counters(c)), flush=True)
    c.close()
    (lx, ly, lz), intensity = (-10.0, 20.0, 40.0), 3e10                # scene_upload's light
    lx1 = float(np.nextafter(np.float32(lx), np.float32(0.0)))
    t_a = 1e-4
    t_b = float(np.nextafter(np.float32(t_a), np.float32(1.0)))
    # what a frame that misses alternates: (params, light x) of frame k
    miss = [(params(tri_tmin=t_a), lx), (params(tri_tmin=t_b), lx)] if KNOB == KNOBS[0] else [(p, lx), (p, lx1)]

    def per_frame(ctx, frames, warm=10, n=40):
        rows = Rows(0, args.height, args.height, 1)
        bufs = [torch.zeros((args.height, args.width, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
        stream = torch.cuda.Stream()
        ctx.set_pipelining(True)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for k in range(warm + n):
            if k == warm:
                t0.record(stream)
            q, x = frames[k % len(frames)]
            ctx.set_light((x, ly, lz), intensity)       # (a host-side edit of the scene the next frame's launches carry: the still view sets the same light again)
            ctx.render_device(q, rows, bufs[k % 2].data_ptr(), stream.cuda_stream)
        t1.record(stream)
        t1.synchronize()
        ctx.set_pipelining(False)
        return t0.elapsed_time(t1) / n

    for knob in (ON, "0") if not os.environ.get("RT_LIB") else (ON,):
        os.environ[KNOB] = knob
        c = rt.Context(0)
        c.scene_upload(rt.scenes.spheres("cpu"), mesh)
        for rep in range(3):
            a, b = per_frame(c, [(p, lx)]), per_frame(c, miss)
            print("%s, %s=%s in one process, 40 pipelined frames: still view %.4f ms per frame, every frame a miss %.4f ms" % (which, KNOB, knob, a, b), flush=True)
        print("%s, %s=%s counters: %s" % (which, KNOB, knob, counters(c)), flush=True)
        c.close()


def step(cmd, env, limit):
    """one GPU step: a process of its own under its own time limit; the first failure ends the run"""
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, cwd=ROOT, timeout=limit)
    except subprocess.TimeoutExpired:
        print("step ran into its time limit of %d s: %s" % (limit, " ".join(cmd[1:])), flush=True)
        sys.exit(1)
    if r.returncode != 0:
        print("step failed (%d): %s\n%s" % (r.returncode, " ".join(cmd[1:]), r.stderr[-600:]), flush=True)
        sys.exit(1)
    return r.stdout


def workload(width, height, spp, bounces, dump_dir):
    shape = ["--width", str(width), "--height", str(height), "--spp", str(spp), "--bounces", str(bounces)]
    print("workload: cat %dx%d, %d sample(s), %d bounces; bench.py --gpus 1 --steps 60 --warmup 5" % (width, height, spp, bounces), flush=True)
    stage = [sys.executable, os.path.abspath(__file__), "--knob", KNOB, "--stage", "inproc"] + shape
    print(step(stage, dict(os.environ), 240), end="", flush=True)
    if args.parent_lib:
        print(step(stage, dict(os.environ, RT_LIB=os.path.abspath(args.parent_lib)), 240), end="", flush=True)
    off = "branch %s=0" % KNOB
    builds = [("branch", {}), (off, {KNOB: "0"})] + [("branch %s=%s" % (KNOB, v), {KNOB: v}) for v in args.also.split(",") if v]
    if args.parent_lib:
        builds.insert(1, ("parent", {"RT_LIB": os.path.abspath(args.parent_lib)}))
    ms = {name: [] for name, _ in builds}
    for r in range(args.runs):
        for name, extra in builds:
            cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "60", "--warmup", "5"] + shape
            if dump_dir and r == 0 and name in ("branch", "parent"):
                cmd += ["--dump-outputs", os.path.join(dump_dir, name)]
            d = json.loads(step(cmd, dict(os.environ, **extra), 170).strip().splitlines()[-1])
            ms[name].append(d["ms_per_step"])
            print("bench %-32s %.4f ms per frame, %.0f Mrays/s" % (name + ":", d["ms_per_step"], d["value"]), flush=True)
    med = {}
    for name, _ in builds:
        x = sorted(ms[name])
        med[name] = x[len(x) // 2]
        print("%-32s median %.4f ms (min %.4f, max %.4f, spread %.4f)" % (name + ":", med[name], x[0], x[-1], x[-1] - x[0]))
    if args.parent_lib:
        sp = max(ms["parent"]) - min(ms["parent"])
        print("branch - parent: %+.4f ms (%+.2f %%); the parent's spread: %.4f ms, three times the parent's spread: %.4f ms; every run of the branch below every run of the "
              "parent: %s" % (med["branch"] - med["parent"], 100 * (med["branch"] / med["parent"] - 1), sp, 3 * sp, max(ms["branch"]) < min(ms["parent"])))
        print("knob off - parent: %+.4f ms (%+.2f %%)" % (med[off] - med["parent"], 100 * (med[off] / med["parent"] - 1)))
    print("the level alone (branch - %s): %+.4f ms (%+.2f %%)" % (off, med["branch"] - med[off], 100 * (med["branch"] / med[off] - 1)))
    for name, _ in builds[3 if args.parent_lib else 2:]:
        print("branch - %s: %+.4f ms (%+.2f %%); every run of the branch below every run of it: %s" % (
            name, med["branch"] - med[name], 100 * (med["branch"] / med[name] - 1), max(ms["branch"]) < min(ms[name])))
    if args.parent_lib and dump_dir:
        import numpy as np
        a, b = (np.load(os.path.join(dump_dir, n, "frame.npy")) for n in ("branch", "parent"))
        print("frame.npy of branch and parent: %s" % ("bit-identical" if a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)) else "DIFFERENT"), flush=True)


if args.stage == "inproc":
    inproc()
else:
    if args.only in ("", "headline"):
        workload(1920, 1080, 1, 3, os.path.join(args.dump_dir, "headline") if args.dump_dir else "")
    if args.only in ("", "spp8"):
        workload(512, 512, 8, 3, os.path.join(args.dump_dir, "spp8") if args.dump_dir else "")

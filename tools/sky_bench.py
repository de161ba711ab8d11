"""GPU box: what an environment map costs and what it looks like (rt_scene_set_environment).

  headline  python3 bench.py --gpus 1 --steps 20 --warmup 5 on this tree's library and, through RT_LIB, on the parent commit's (--parent-lib PATH), ROUNDS interleaved
            rounds, the parent first in every round; medians, spreads, and whether this tree's median lies inside the parent's own spread.  No headline kernel changed.
  frame     two scenes at 1920 x 1080, one sample, three bounces: the cat without its walls, and the cat in its room with the wall in front of the camera removed.  Each with a
            map beside the same scene without one, both on ONE context created with RT_FIRST_HIT_CACHE=0 -- the chain a sky frame is comparable to: under a map no chain keeps
            anything of a still view -- the map switched between windows.  Then, on a context of its own, the frame without a map with the caches on: the share of the price
            that is the lost still view.  And the headline scene cached, to put both in its units.  Host clock around windows of CALLS frames and one wait, ROUNDS
            interleaved rounds, medians and the spread.
  quality   the open cat at 640 x 360, b = 3, lit by gradient_sky alone (the point light dark): RMSE in the tonemap's [0, 1] scale against a 1024-sample frame -- of 1, 4, 16
            and 64 samples, and of the default SvgfSequence over eight frames, overall, on the pixels that see the sky directly (no object: the filters' guides are empty
            there) and on the rest.
  launches  frames for a kernel trace: 30 frames each with and without the map of the room with a wall removed -- plain, with a light list (the soft route), textured, textured
            with a light list -- all under RT_FIRST_HIT_CACHE=0 and RT_CHAIN_ENDS=0, so that both sides run the same launches at the same positions of the chain.  Run under
                rocprofv3 --kernel-trace --output-format csv -d DIR -o trace -- python tools/sky_bench.py --only launches
            and reduce the trace with  python tools/sky_bench.py --trace DIR/.../trace_kernel_trace.csv: the four sky forms against their counterparts, in us.

usage: python tools/sky_bench.py [--only headline|frame|quality|launches] [--parent-lib PATH] [--trace CSV] > profiles/sky/sky_bench.txt"""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--only", default="")
ap.add_argument("--trace", default="")
ap.add_argument("--parent-lib", default="")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--calls", type=int, default=40)
ap.add_argument("--windows", type=int, default=5)
args = ap.parse_args()


def spread(xs):
    xs = sorted(xs)
    return "median %.4f (min %.4f, max %.4f, spread %.4f)" % (statistics.median(xs), xs[0], xs[-1], xs[-1] - xs[0])


def reduce_trace(path):
    """mean / median duration of the four sky forms and of the forms they stand in for, from a rocprofv3 kernel trace"""
    from advance_forms import describe, form, form_of
    pairs = [(form("sky"), 0), (form("soft", "sky"), form("lights")), (form("tex", "sky"), form("tex")), (form("tex", "soft", "sky"), form("tex", "lights"))]
    dur = {f: [] for pair in pairs for f in pair}
    for r in csv.DictReader(open(path)):
        f = form_of(r["Kernel_Name"].replace(" ", ""))
        if f in dur:
            dur[f].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    print("wf_advance launches of one of two sub-frames of 1920 x 1080 (the room with a wall removed, b = 3, RT_FIRST_HIT_CACHE=0, RT_CHAIN_ENDS=0), us, from a rocprofv3 kernel")
    print("trace; the same rays with and without the map, so the same live paths at every position; a launch's time is the mean over the chain's positions.  A light list")
    print("without a radius runs the soft forms under a map (radii 0: the shell draw is skipped) and the lights forms without one: that pair also holds the radius test.")
    for a, b in pairs:
        for f in (a, b):
            v = dur[f]
            if v:
                v = sorted(v)[len(v) // 10: len(v) - len(v) // 10 or None]  # (the first launches of a process run cold)
                print(f"  {describe(f):40s} mean {statistics.mean(v):.1f}, median {statistics.median(v):.1f}, min {v[0]:.1f}, max {v[-1]:.1f} ({len(v)} launches)")


def headline():
    if not args.parent_lib:
        raise SystemExit("headline: --parent-lib PATH (the parent commit's libraytrace_hip.so)")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"]
    runs = {"parent": [], "this": []}
    print("python3 bench.py --gpus 1 --steps 20 --warmup 5; this tree's library and, through RT_LIB, the parent commit's; interleaved (parent first in every round); one MI355X", flush=True)
    for r in range(args.rounds):
        for who in ("parent", "this"):
            env = dict(os.environ)
            env.pop("RT_LIB", None)
            if who == "parent":
                env["RT_LIB"] = os.path.abspath(args.parent_lib)
            out = subprocess.run(cmd, env=env, check=True, stdout=subprocess.PIPE, text=True, timeout=300).stdout
            res = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
            runs[who].append(res["ms_per_step"])
            print(f"round {r + 1} {who:6s} {res['value']:.2f} Mrays/s  {res['ms_per_step']:.4f} ms per frame", flush=True)
    for who in ("parent", "this"):
        print(f"{who}: {spread(runs[who])}")
    lo, hi, m = min(runs["parent"]), max(runs["parent"]), statistics.median(runs["this"])
    print(f"this tree's median lies {'inside' if lo <= m <= hi else 'OUTSIDE'} the parent's own spread [{lo:.4f}, {hi:.4f}]")


if args.trace:
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    reduce_trace(args.trace)
    sys.exit(0)
if args.only == "headline":
    headline()
    sys.exit(0)

import numpy as np
import torch

import raytracinggpu_amd as rt
from raytracinggpu_amd import environment, hostlib
from raytracinggpu_amd._capi import Rows

B = 3
THREE = [((-10.0, 20.0, 40.0), 1e10), ((15.0, 25.0, 30.0), 2e10), ((0.0, 35.0, 5.0), 5e10)]
SKY = environment.gradient_sky((0.25, 0.45, 1.0), (1.0, 1.0, 1.0), (0.25, 0.2, 0.15), 256)


def context(**env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return rt.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def cat_mesh(slot):
    v, t = rt.scenes.load_cat_arrays()
    return hostlib.build_mesh(v, t, albedo=rt.scenes.CAT_ALBEDO, object_slot=slot)


SCENES = {"the cat without its walls": [], "the room with the wall in front of the camera removed": rt.scenes.WALLS[1:], "the headline scene": rt.scenes.WALLS}


def upload(c, name, mesh_cache={}):
    sph = list(SCENES[name])
    if len(sph) not in mesh_cache:
        mesh_cache[len(sph)] = cat_mesh(len(sph))
    c.scene_upload(sph, mesh_cache[len(sph)])
    return mesh_cache[len(sph)]


def params(seed, w, h, spp=1):
    return rt.make_params(w, h, spp, B, seed=seed, **rt.scenes.CPU_LAUNCHER)


def frame():
    W, H = 1920, 1080
    rows = Rows(0, H, H, 1)
    buf = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    p = params(123456, W, H)

    def window(c):
        c.render_device(p, rows, buf.data_ptr())
        c.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            c.render_device(p, rows, buf.data_ptr())
        c.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.calls

    c = context()
    upload(c, "the headline scene")
    head = [statistics.median(window(c) for _ in range(args.windows)) for _ in range(args.rounds)]
    c.close()
    print(f"cat 1920x1080, one sample, b = {B}; ms per frame, host clock around {args.calls} frames and one wait, median of {args.windows} windows, {args.rounds} interleaved rounds", flush=True)
    print(f"  {'the headline scene, caches on':44s} per round {' / '.join('%.4f' % x for x in head)} -> {spread(head)}", flush=True)
    h = statistics.median(head)
    for name in list(SCENES)[:2]:
        c = context(RT_FIRST_HIT_CACHE="0")
        upload(c, name)
        on, off = "with the map", "without a map, RT_FIRST_HIT_CACHE=0"
        modes = {on: lambda: c.set_environment(SKY), off: lambda: c.set_environment()}
        runs = {k: [] for k in modes}
        for _ in range(args.rounds):
            for k, set_up in modes.items():
                set_up()
                runs[k].append(statistics.median(window(c) for _ in range(args.windows)))
        c.close()
        c = context()
        upload(c, name)
        cached = [statistics.median(window(c) for _ in range(args.windows)) for _ in range(args.rounds)]
        c.close()
        print(f"{name}:", flush=True)
        for k, r in runs.items():
            print(f"  {k:44s} per round {' / '.join('%.4f' % x for x in r)} -> {spread(r)}", flush=True)
        print(f"  {'without a map, caches on':44s} per round {' / '.join('%.4f' % x for x in cached)} -> {spread(cached)}", flush=True)
        a, b, cc = statistics.median(runs[on]), statistics.median(runs[off]), statistics.median(cached)
        print(f"  the map against no map without caches: {a / b:.4f}; the lost still-view caches: {b / cc:.4f}; together {a / cc:.4f}; "
              f"against the cached headline frame: {a / h:.4f} (of which this scene without a map, cached: {cc / h:.4f})", flush=True)


def textured(c, mesh):
    v = np.asarray(mesh["vertices"], np.float32)
    lo, hi = v.min(0), v.max(0)
    uv = ((v[:, :2] - lo[:2]) / (hi[:2] - lo[:2])).astype(np.float32)
    texels = np.random.default_rng(21).integers(0, 256, size=(64, 64, 3), dtype=np.uint8)
    c.mesh_set_texture(uv, np.asarray(mesh["indices"])[:, :3], texels, filter="bilinear")


def launches():
    W, H = 1920, 1080
    c = context(RT_FIRST_HIT_CACHE="0", RT_CHAIN_ENDS="0")
    rows = Rows(0, H, H, 1)
    buf = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    p = params(123456, W, H)

    def both():
        for env in (SKY, None):
            c.set_environment(env)
            for _ in range(30):
                c.render_device(p, rows, buf.data_ptr())
            c.synchronize()

    name = "the room with the wall in front of the camera removed"
    mesh = upload(c, name)
    both()                                                             # sky against 0
    c.set_lights(THREE)
    both()                                                             # soft | sky against lights
    upload(c, name)
    textured(c, mesh)
    both()                                                             # tex | sky against tex
    c.set_lights(THREE)
    both()                                                             # tex | soft | sky against tex | lights
    c.close()


def tonemap(a):
    """min(pow(c, 1 / 2.2), 255) / 255: the tonemap's scale (cpu:714-716)"""
    return np.minimum(np.power(np.maximum(a[..., :3].astype(np.float64), 0.0), 1 / 2.2), 255.0) / 255.0


def quality():
    w, h, frames = 640, 360, 8
    ctx = context()
    upload(ctx, "the cat without its walls")
    ctx.set_light((-10.0, 20.0, 40.0), 0.0)                            # the sky alone lights the cat
    # radiances in the tonemap's units: pow(c, 1 / 2.2) / 255 puts 255^2.2 = 1.97e5 at white
    ctx.set_environment((SKY * np.float32(1.2e5)).astype(np.float32))
    ref4 = ctx.render(params(7000, w, h, 1024))
    ref = tonemap(ref4)
    sky_px = ref4[..., 3] == 1024                                      # every sample's camera ray left the scene: no object in the feature buffers
    rm = lambda a, m=slice(None): float(np.sqrt(np.mean((a[m] - ref[m]) ** 2)))
    print(f"quality: the open cat {w}x{h}, b = {B}, lit by gradient_sky alone (n = 256); RMSE in the tonemap's [0, 1] scale against a 1024-sample frame; {int(sky_px.sum())} of "
          f"{sky_px.size} pixels see the sky directly", flush=True)
    for spp in (1, 4, 16, 64):
        fr = [tonemap(ctx.render(params(100 + i, w, h, spp))) for i in range(4)]
        e = [rm(f) for f in fr]
        print(f"  {spp:3d} sample{'s' if spp > 1 else ' '}: {np.mean(e):.5f} (mean of 4 seeds, min {min(e):.5f}, max {max(e):.5f}); on the cat {rm(fr[0], ~sky_px):.5f}, on the sky "
              f"{rm(fr[0], sky_px):.5f}", flush=True)
    outs = []
    with rt.SvgfSequence(ctx, w, h) as seq:
        for i in range(frames):
            out = seq.frame(params(100 + i, w, h))
            ctx.synchronize()
            outs.append(tonemap(ctx.device_to_host(out, (h, w, 4))))
    print("  SvgfSequence (one sample per frame) per frame: " + " ".join(f"{rm(o):.5f}" for o in outs), flush=True)
    print(f"  after {frames} frames: overall {rm(outs[-1]):.5f}; on the cat {rm(outs[-1], ~sky_px):.5f}, on the sky {rm(outs[-1], sky_px):.5f}; "
          f"mean signed error there {float(np.mean(outs[-1][~sky_px] - ref[~sky_px])):+.5f} / {float(np.mean(outs[-1][sky_px] - ref[sky_px])):+.5f}; "
          f"largest error on a sky pixel {float(np.abs(outs[-1][sky_px] - ref[sky_px]).max()):.5f}", flush=True)
    ctx.close()


if args.only in ("", "frame"):
    frame()
if args.only in ("", "quality"):
    quality()
if args.only == "launches":
    launches()

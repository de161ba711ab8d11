"""GPU box: what several point lights cost and what they look like (rt_scene_set_lights).

  frame     the headline frame (cat, 1920 x 1080, one sample, three bounces) under FOUR lights beside the same build's ONE-light frame, both on ONE context created
            with RT_FIRST_SHADOW_CACHE=0 -- the chain it is comparable to: a still view of several lights keeps the camera rays' hits and nothing above them.  (One
            context: a second one's streams can share a hardware queue with the first one's, and its sub-frames then run one after the other.)  Host clock
            around windows of CALLS frames and one wait, ROUNDS interleaved rounds, medians and the spread; then, under rt_stats_enable (every launch of the chain is
            enqueued and bracketed by events), the mean time of a wf_advance launch and of a traversal launch of both.
  quality   the four-light cat scene at 640 x 360, b = 3: RMSE in the tonemap's [0, 1] scale against a 1024-sample frame -- of a one-sample frame, and of the default
            SvgfSequence after eight frames; beside the same for ONE light of the total intensity at the first light's place.

usage: python tools/lights_bench.py [--only frame|quality] > profiles/lights/lights_bench.txt"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--only", default="")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--calls", type=int, default=40)
ap.add_argument("--windows", type=int, default=5)
args = ap.parse_args()

import numpy as np
import torch

import raytracinggpu_amd as rt
from raytracinggpu_amd import hostlib
from raytracinggpu_amd._capi import Rows

SLOT = rt.scenes.mesh_slot("cpu")
B = 3
# four lamps in the room (walls at +-60): the uploaded light's place and three more, intensities 3 : 2 : 2 : 1 of 4e10 in all
FOUR = [((-10.0, 20.0, 40.0), 1.5e10), ((25.0, 30.0, 20.0), 1.0e10), ((-30.0, 35.0, -10.0), 1.0e10), ((10.0, 15.0, 50.0), 0.5e10)]
TOTAL = float(sum(np.float32(i) for _, i in FOUR))


def spread(xs):
    xs = sorted(xs)
    return "median %.4f (min %.4f, max %.4f, spread %.4f)" % (statistics.median(xs), xs[0], xs[-1], xs[-1] - xs[0])


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


def cat_mesh():
    v, t = rt.scenes.load_cat_arrays()
    return hostlib.build_mesh(v, t, albedo=rt.scenes.CAT_ALBEDO, object_slot=SLOT)


def params(seed, w, h, spp=1):
    return rt.make_params(w, h, spp, B, seed=seed, **rt.scenes.CPU_LAUNCHER)


def frame():
    W, H = 1920, 1080
    mesh = cat_mesh()
    c = context(RT_FIRST_SHADOW_CACHE="0")
    c.scene_upload(rt.scenes.spheres("cpu"), mesh)
    lights = {"four lights": lambda: c.set_lights(FOUR), "one light, RT_FIRST_SHADOW_CACHE=0": lambda: c.set_light(FOUR[0][0], TOTAL)}
    rows = Rows(0, H, H, 1)
    buf = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    p = params(123456, W, H)

    def window():
        c.render_device(p, rows, buf.data_ptr())
        c.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            c.render_device(p, rows, buf.data_ptr())
        c.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.calls

    runs = {name: [] for name in lights}
    for _ in range(args.rounds):
        for name, set_up in lights.items():
            set_up()
            runs[name].append(statistics.median(window() for _ in range(args.windows)))
    print(f"{c.device_name}; cat {W}x{H}, one sample, b = {B}; ms per frame, host clock around {args.calls} frames and one wait, median of {args.windows} windows, "
          f"{args.rounds} interleaved rounds (a still view: both chains use the camera rays' hits and nothing above them)", flush=True)
    for name, r in runs.items():
        print(f"  {name:36s} per round {' / '.join('%.4f' % x for x in r)} -> {spread(r)}", flush=True)
    a, b = statistics.median(runs["four lights"]), statistics.median(runs["one light, RT_FIRST_SHADOW_CACHE=0"])
    print(f"  four lights / one light: {a / b:.4f}", flush=True)
    print("per launch, under rt_stats_enable (the whole chain enqueued, part 0's launches bracketed by events); mean over 20 frames:", flush=True)
    for name, set_up in lights.items():
        set_up()
        c.stats_enable(True)
        adv, trav, ker = [], [], []
        for _ in range(20):
            c.render_device(p, rows, buf.data_ptr())
            c.synchronize()
            s = c.stats()
            adv.append(s["adv_ms"] / max(s["adv_launches"], 1))
            trav.append(s["trav_ms"] / max(s["trav_launches"], 1))
            ker.append(s["kernel_ms"])
        c.stats_enable(False)
        print(f"  {name.split(',')[0]:12s} wf_advance {statistics.median(adv) * 1e3:.1f} us per launch ({s['adv_launches']} launches, {s['adv_paths']} paths, min {min(adv) * 1e3:.1f}, max {max(adv) * 1e3:.1f}); "
              f"traversal {statistics.median(trav) * 1e3:.1f} us per launch ({s['trav_launches']}); kernel_ms {statistics.median(ker):.4f}", flush=True)
    c.close()


def tonemap(a):
    """min(pow(c, 1 / 2.2), 255) / 255: the tonemap's scale (cpu:714-716)"""
    return np.minimum(np.power(np.maximum(a[..., :3].astype(np.float64), 0.0), 1 / 2.2), 255.0) / 255.0


def quality():
    w, h, frames = 640, 360, 8
    mesh = cat_mesh()
    ctx = context()
    print(f"quality: cat scene {w}x{h}, b = {B}; RMSE in the tonemap's [0, 1] scale against a 1024-sample frame of the same lights", flush=True)
    for name, set_up in (("four lights", lambda: ctx.set_lights(FOUR)), ("one light of the total", lambda: ctx.set_light(FOUR[0][0], TOTAL))):
        ctx.scene_upload(rt.scenes.spheres("cpu"), mesh)
        set_up()
        ref = tonemap(ctx.render(params(7000, w, h, 1024)))
        one = [float(np.sqrt(np.mean((tonemap(ctx.render(params(100 + i, w, h))) - ref) ** 2))) for i in range(frames)]
        errs = []
        with rt.SvgfSequence(ctx, w, h) as seq:
            for i in range(frames):
                out = seq.frame(params(100 + i, w, h))
                ctx.synchronize()
                errs.append(float(np.sqrt(np.mean((tonemap(ctx.device_to_host(out, (h, w, 4))) - ref) ** 2))))
        print(f"  {name:24s} one sample: {np.mean(one):.5f} (mean of {frames} seeds, min {min(one):.5f}, max {max(one):.5f});  SvgfSequence after {frames} frames: {errs[-1]:.5f}  "
              "per frame " + " ".join(f"{e:.5f}" for e in errs), flush=True)
    ctx.close()


if args.only in ("", "frame"):
    frame()
if args.only in ("", "quality"):
    quality()

"""GPU box: what several point lights cost and what they look like (rt_scene_set_lights).

  frame     the headline frame (cat, 1920 x 1080, one sample, three bounces) under FOUR lights beside the same build's ONE-light frame, both on ONE context created
            with RT_FIRST_SHADOW_CACHE=0 -- the chain it is comparable to: a still view of several lights keeps the camera rays' hits and nothing above them.  (One
            context: a second one's streams can share a hardware queue with the first one's, and its sub-frames then run one after the other.)  Host clock
            around windows of CALLS frames and one wait, ROUNDS interleaved rounds, medians and the spread; then, under rt_stats_enable (every launch of the chain is
            enqueued and bracketed by events), the mean time of a wf_advance launch and of a traversal launch of both.
  quality   the four-light cat scene at 640 x 360, b = 3: RMSE in the tonemap's [0, 1] scale against a 1024-sample frame -- of a one-sample frame, and of the default
            SvgfSequence after eight frames; beside the same for ONE light of the total intensity at the first light's place.

  --radius R   (R > 0) lights with a radius (rt_scene_set_light_radii): `frame` gains the four lights at radius R -- the SAME context, the radii
            switched between windows -- and its wf_advance_soft / traversal launches; `quality` gains the four soft lights against their own 1024-sample frame, with
            the SvgfSequence's error after the first and after the last frame.

usage: python tools/lights_bench.py [--only frame|quality] [--radius R] > profiles/lights/lights_bench.txt"""
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
ap.add_argument("--radius", type=float, default=0.0)
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
    soft = f"four lights of radius {args.radius:g}"
    if args.radius > 0:
        lights[soft] = lambda: (c.set_lights(FOUR), c.set_light_radii([args.radius] * len(FOUR)))
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
    if args.radius > 0:
        print(f"  {soft} / four lights: {statistics.median(runs[soft]) / a:.4f}", flush=True)
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
        print(f"  {name.split(', RT')[0]:12s} wf_advance {statistics.median(adv) * 1e3:.1f} us per launch ({s['adv_launches']} launches, {s['adv_paths']} paths, min {min(adv) * 1e3:.1f}, max {max(adv) * 1e3:.1f}); "
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
    cases = [("four lights", lambda: ctx.set_lights(FOUR)), ("one light of the total", lambda: ctx.set_light(FOUR[0][0], TOTAL))]
    if args.radius > 0:
        cases.append((f"four lights of radius {args.radius:g}", lambda: (ctx.set_lights(FOUR), ctx.set_light_radii([args.radius] * len(FOUR)))))
    kept = {}
    for name, set_up in cases:
        ctx.scene_upload(rt.scenes.spheres("cpu"), mesh)
        set_up()
        ref = tonemap(ctx.render(params(7000, w, h, 1024)))
        ones = [tonemap(ctx.render(params(100 + i, w, h))) for i in range(frames)]
        one = [float(np.sqrt(np.mean((f - ref) ** 2))) for f in ones]
        errs, outs = [], []
        with rt.SvgfSequence(ctx, w, h) as seq:
            for i in range(frames):
                out = seq.frame(params(100 + i, w, h))
                ctx.synchronize()
                outs.append(tonemap(ctx.device_to_host(out, (h, w, 4))))
                errs.append(float(np.sqrt(np.mean((outs[-1] - ref) ** 2))))
        kept[name] = (ref, ones, outs)
        print(f"  {name:24s} one sample: {np.mean(one):.5f} (mean of {frames} seeds, min {min(one):.5f}, max {max(one):.5f});  SvgfSequence after the first frame: {errs[0]:.5f}, after {frames} frames: {errs[-1]:.5f}  "
              "per frame " + " ".join(f"{e:.5f}" for e in errs), flush=True)
    if args.radius > 0:
        # the penumbrae alone: the pixels where the soft lights' 1024-sample frame departs from the point lights' by more than 0.02 in some channel
        (ref, ones, outs), point = kept[cases[-1][0]], kept["four lights"][0]
        mask = np.abs(ref - point).max(-1) > 0.02
        rm = lambda a, m: float(np.sqrt(np.mean((a[m] - ref[m]) ** 2)))
        print(f"  penumbra pixels (soft and point 1024-sample frames more than 0.02 apart): {int(mask.sum())} of {mask.size}; there the two references differ by "
              f"{float(np.sqrt(np.mean((ref[mask] - point[mask]) ** 2))):.5f} RMS -- what a hard-edged answer would miss", flush=True)
        for what, m in (("inside", mask), ("outside", ~mask)):
            print(f"  {what:8s} one sample: {np.mean([rm(f, m) for f in ones]):.5f};  SvgfSequence after the first frame: {rm(outs[0], m):.5f}, after {frames} frames: {rm(outs[-1], m):.5f};  "
                  f"mean signed error after {frames} frames: {float(np.mean(outs[-1][m] - ref[m])):+.5f}", flush=True)
    ctx.close()


if args.only in ("", "frame"):
    frame()
if args.only in ("", "quality"):
    quality()

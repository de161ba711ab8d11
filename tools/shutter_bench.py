"""GPU box: what the shutter costs and what it looks like (rt_scene_set_shutter).

  frame     the headline frame (cat, 1920 x 1080, one sample, three bounces) with the shutter on beside the same build's closed-shutter frame, both on ONE context created
            with RT_FIRST_HIT_CACHE=0 -- the chain a shutter frame is comparable to: with the shutter on no chain keeps anything of a still view.  Then, on a context of its
            own, the closed frame with the caches on -- the headline's chain: the price of losing them.  Host clock around windows of CALLS frames and one wait, ROUNDS
            interleaved rounds, medians and the spread; then, under rt_stats_enable, the mean time of a wf_advance launch (the launches after the opening one) and of a
            traversal launch of both.
  quality   the cat scene at 640 x 360, b = 3, with one fast sphere in front of the cat: RMSE in the tonemap's [0, 1] scale against a 1024-sample shutter frame -- of 1, 4,
            16 and 64 samples, and of the default SvgfSequence after eight frames, overall and where the sphere's streak is (where the shutter's and the closed shutter's
            1024-sample frames are more than 0.02 apart).  The sequence's guides see the start-of-exposure pose.
  launches  frames for a kernel trace: 30 frames each of the cat with the shutter on and closed, the same behind the lens, the same with a texture, all under
            RT_FIRST_HIT_CACHE=0.  Run under
                rocprofv3 --kernel-trace --output-format csv -d DIR -o trace -- python tools/shutter_bench.py --only launches
            and reduce the trace with  python tools/shutter_bench.py --trace DIR/.../trace_kernel_trace.csv: the four shutter forms against their counterparts, in us.

usage: python tools/shutter_bench.py [--only frame|quality|launches] [--trace CSV] > profiles/shutter/shutter_bench.txt"""
import argparse
import csv
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--only", default="")
ap.add_argument("--trace", default="")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--calls", type=int, default=40)
ap.add_argument("--windows", type=int, default=5)
args = ap.parse_args()


def reduce_trace(path):
    """mean / median duration of the four shutter forms and of the forms they stand in for, from a rocprofv3 kernel trace"""
    from advance_forms import describe, form, form_of
    pairs = [(form("first", "shutter"), form("first")), (form("first", "lens", "shutter"), form("first", "lens")), (form("shutter"), 0), (form("tex", "shutter"), form("tex"))]
    dur = {f: [] for pair in pairs for f in pair}
    for r in csv.DictReader(open(path)):
        f = form_of(r["Kernel_Name"].replace(" ", ""))
        if f in dur:
            dur[f].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    print("wf_advance launches of one of two sub-frames of 1920 x 1080 (cat, b = 3, RT_FIRST_HIT_CACHE=0), us, from a rocprofv3 kernel trace; a later launch's time is the mean over")
    print("the chain's positions, whose live paths differ:")
    for a, b in pairs:
        for f in (a, b):
            v = dur[f]
            if v:
                v = sorted(v)[len(v) // 10: len(v) - len(v) // 10 or None]  # (the first launches of a process run cold)
                print(f"  {describe(f):40s} mean {statistics.mean(v):.1f}, median {statistics.median(v):.1f}, min {v[0]:.1f}, max {v[-1]:.1f} ({len(v)} launches)")


if args.trace:
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    reduce_trace(args.trace)
    sys.exit(0)

import numpy as np
import torch

import raytracinggpu_amd as rt
from raytracinggpu_amd import hostlib
from raytracinggpu_amd._capi import Rows

SLOT = rt.scenes.mesh_slot("cpu")
B = 3
LENS = (1.5, 45.0)
# the headline scene in motion: the light travels and the floor (slot 1) rises, as in tests/test_gpu_shutter.py
MOTION = dict(light=(6.0, 0.0, -4.0), objects={1: (0.0, 0.75, 0.0)})
# quality: a ball in front of the cat (slot 7, behind the cat's slot 6) that crosses a third of the view during the exposure
BALL = ((-8.0, 0.0, 25.0), 3.0, (0.7, 0.3, 0.2))
BALL_MOTION = dict(light=(0.0, 0.0, 0.0), objects={7: (16.0, 0.0, 0.0)})


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

    c = context(RT_FIRST_HIT_CACHE="0")
    c.scene_upload(rt.scenes.spheres("cpu"), mesh)
    on, off = "shutter on (light and floor move)", "shutter closed, RT_FIRST_HIT_CACHE=0"
    modes = {on: lambda: c.set_shutter(**MOTION), off: lambda: c.set_shutter()}
    runs = {name: [] for name in modes}
    for _ in range(args.rounds):
        for name, set_up in modes.items():
            set_up()
            runs[name].append(statistics.median(window(c) for _ in range(args.windows)))
    print(f"{c.device_name}; cat {W}x{H}, one sample, b = {B}; ms per frame, host clock around {args.calls} frames and one wait, median of {args.windows} windows, "
          f"{args.rounds} interleaved rounds", flush=True)
    for name, r in runs.items():
        print(f"  {name:40s} per round {' / '.join('%.4f' % x for x in r)} -> {spread(r)}", flush=True)
    a, b = statistics.median(runs[on]), statistics.median(runs[off])
    print(f"  shutter on / closed without caches: {a / b:.4f}", flush=True)
    print("per launch, under rt_stats_enable (part 0's launches after the opening one bracketed by events); median over 20 frames:", flush=True)
    for name, set_up in modes.items():
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
        print(f"  {name.split(' (')[0].split(',')[0]:16s} wf_advance {statistics.median(adv) * 1e3:.1f} us per launch ({s['adv_launches']} launches, {s['adv_paths']} paths); "
              f"traversal {statistics.median(trav) * 1e3:.1f} us per launch ({s['trav_launches']}); kernel_ms {statistics.median(ker):.4f}", flush=True)
    c.close()
    c = context()                                                      # the headline's chain: a still view with its three caches
    c.scene_upload(rt.scenes.spheres("cpu"), mesh)
    cached = [statistics.median(window(c) for _ in range(args.windows)) for _ in range(args.rounds)]
    print(f"  {'shutter closed, caches on (the headline)':40s} per round {' / '.join('%.4f' % x for x in cached)} -> {spread(cached)}", flush=True)
    print(f"  shutter on / cached headline: {a / statistics.median(cached):.4f}", flush=True)
    c.close()


def launches():
    W, H = 1920, 1080
    c = context(RT_FIRST_HIT_CACHE="0")
    mesh = cat_mesh()
    rows = Rows(0, H, H, 1)
    buf = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    p = params(123456, W, H)

    def both():
        for motion in (MOTION, None):
            if motion:
                c.set_shutter(**motion)
            else:
                c.set_shutter()
            for _ in range(30):
                c.render_device(p, rows, buf.data_ptr())
            c.synchronize()

    c.scene_upload(rt.scenes.spheres("cpu"), mesh)
    both()                                                             # first | shutter, shutter against first, 0
    c.set_lens(*LENS)
    both()                                                             # first | lens | shutter against first | lens
    c.set_lens(0.0, 1.0)
    v = np.asarray(mesh["vertices"], np.float32)
    lo, hi = v.min(0), v.max(0)
    uv = ((v[:, :2] - lo[:2]) / (hi[:2] - lo[:2])).astype(np.float32)
    texels = np.random.default_rng(21).integers(0, 256, size=(64, 64, 3), dtype=np.uint8)
    c.mesh_set_texture(uv, np.asarray(mesh["indices"])[:, :3], texels, filter="bilinear")
    both()                                                             # tex | shutter against tex
    c.close()


def tonemap(a):
    """min(pow(c, 1 / 2.2), 255) / 255: the tonemap's scale (cpu:714-716)"""
    return np.minimum(np.power(np.maximum(a[..., :3].astype(np.float64), 0.0), 1 / 2.2), 255.0) / 255.0


def quality():
    w, h, frames = 640, 360, 8
    ctx = context()
    ctx.scene_upload(rt.scenes.spheres("cpu") + [BALL], cat_mesh())
    closed = tonemap(ctx.render(params(7000, w, h, 1024)))
    ctx.set_shutter(**BALL_MOTION)
    ref = tonemap(ctx.render(params(7000, w, h, 1024)))
    rm = lambda a, m=slice(None): float(np.sqrt(np.mean((a[m] - ref[m]) ** 2)))
    mask = np.abs(ref - closed).max(-1) > 0.02
    print(f"quality: cat scene {w}x{h}, b = {B}, a ball of radius {BALL[1]:g} at {BALL[0]} travelling {BALL_MOTION['objects'][7]}; RMSE in the tonemap's [0, 1] scale against a "
          f"1024-sample shutter frame", flush=True)
    print(f"  streak pixels (shutter and closed-shutter 1024-sample frames more than 0.02 apart): {int(mask.sum())} of {mask.size}; there the two references differ by "
          f"{float(np.sqrt(np.mean((ref[mask] - closed[mask]) ** 2))):.5f} RMS -- what an instantaneous answer would miss", flush=True)
    for spp in (1, 4, 16, 64):
        e = [rm(tonemap(ctx.render(params(100 + i, w, h, spp)))) for i in range(4)]
        m = [rm(tonemap(ctx.render(params(100 + i, w, h, spp))), mask) for i in range(1)]
        print(f"  {spp:3d} sample{'s' if spp > 1 else ' '}: {np.mean(e):.5f} (mean of 4 seeds, min {min(e):.5f}, max {max(e):.5f}); in the streak {m[0]:.5f}", flush=True)
    outs = []
    with rt.SvgfSequence(ctx, w, h) as seq:
        for i in range(frames):
            out = seq.frame(params(100 + i, w, h))
            ctx.synchronize()
            outs.append(tonemap(ctx.device_to_host(out, (h, w, 4))))
    print("  SvgfSequence (one sample per frame, guides at the start-of-exposure pose) per frame: " + " ".join(f"{rm(o):.5f}" for o in outs), flush=True)
    print(f"  after {frames} frames: overall {rm(outs[-1]):.5f}; in the streak {rm(outs[-1], mask):.5f}, elsewhere {rm(outs[-1], ~mask):.5f}; "
          f"mean signed error there {float(np.mean(outs[-1][mask] - ref[mask])):+.5f} / {float(np.mean(outs[-1][~mask] - ref[~mask])):+.5f}", flush=True)
    ctx.set_shutter()
    outs = []
    with rt.SvgfSequence(ctx, w, h) as seq:
        for i in range(frames):
            out = seq.frame(params(100 + i, w, h))
            ctx.synchronize()
            outs.append(tonemap(ctx.device_to_host(out, (h, w, 4))))
    print(f"  the closed shutter's own sequence against its 1024-sample frame after {frames} frames: {float(np.sqrt(np.mean((outs[-1] - closed) ** 2))):.5f}", flush=True)
    ctx.close()


if args.only in ("", "frame"):
    frame()
if args.only in ("", "quality"):
    quality()
if args.only == "launches":
    launches()

"""GPU box: what the thin lens costs and what it looks like (rt_camera_set_lens).

  frame     the headline frame (cat, 1920 x 1080, one sample, three bounces) with the lens on beside the same build's pinhole frame, both on ONE context created with
            RT_FIRST_HIT_CACHE=0 -- the chain a lens frame is comparable to: with a lens no chain keeps anything of a still view.  (The pinhole chain of this build is the
            parent commit's, kernel for kernel: profiles/lens/asm_compare.txt.)  Then, on a context of its own, the pinhole frame with the caches on -- the headline's
            chain: the price of losing them.  Host clock around windows of CALLS frames and one wait, ROUNDS interleaved rounds, medians and the spread; then, under
            rt_stats_enable, the mean time of a wf_advance launch (the launches after the opening one) and of a traversal launch of both.
  quality   the cat scene at 640 x 360, b = 3, with the lens on: RMSE in the tonemap's [0, 1] scale against a 1024-sample lens frame -- of 1, 4, 16 and 64 samples, and of
            the default SvgfSequence after eight frames, overall and in the defocused region alone (where the lens's and the pinhole's 1024-sample frames are more than
            0.02 apart).  The sequence's guides are the pinhole's.
  opening   frames for a kernel trace: 30 lens frames and 30 pinhole frames under RT_FIRST_HIT_CACHE=0.  Run under
                rocprofv3 --kernel-trace --output-format csv -d DIR -o trace -- python tools/lens_bench.py --only opening
            and reduce the trace with  python tools/lens_bench.py --trace DIR/.../trace_kernel_trace.csv: the opening launch, wf_advance_lens against
            wf_advance<false, true>, in us.
  pinhole   the pinhole line of `frame` alone, without a call of rt_camera_set_lens: what a library that lacks the entry (RT_LIB = the parent commit's build) can run.

usage: python tools/lens_bench.py [--only frame|quality|opening|pinhole] [--trace CSV] > profiles/lens/lens_bench.txt"""
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
ap.add_argument("--radius", type=float, default=1.5)
ap.add_argument("--focus", type=float, default=45.0)
args = ap.parse_args()


def reduce_trace(path):
    """mean / median duration of the two opening kernels in a rocprofv3 kernel trace (printed under the names they had as kernels of their own: profiles/lens)"""
    from advance_forms import form, form_of
    dur = {"wf_advance_lens": [], "wf_advance<false, true>": []}
    for r in csv.DictReader(open(path)):
        name = r["Kernel_Name"].replace(" ", "")
        d = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        f = form_of(name)
        if f == form("first", "lens"):
            dur["wf_advance_lens"].append(d)
        elif f == form("first"):
            dur["wf_advance<false, true>"].append(d)
    print("the opening launch of a chain (one of two sub-frames of 1920 x 1080), us, from a rocprofv3 kernel trace:")
    for k, v in dur.items():
        if v:
            v = sorted(v)[len(v) // 10: len(v) - len(v) // 10 or None]  # (the first launches of a process run cold)
            print(f"  {k:24s} mean {statistics.mean(v):.1f}, median {statistics.median(v):.1f}, min {v[0]:.1f}, max {v[-1]:.1f} ({len(v)} launches)")


if args.trace:
    reduce_trace(args.trace)
    sys.exit(0)

import numpy as np
import torch

import raytracinggpu_amd as rt
from raytracinggpu_amd import hostlib
from raytracinggpu_amd._capi import Rows

SLOT = rt.scenes.mesh_slot("cpu")
B = 3
LENS = (args.radius, args.focus)


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
    on, off = f"lens on (R {LENS[0]:g}, f {LENS[1]:g})", "pinhole, RT_FIRST_HIT_CACHE=0"
    modes = {on: lambda: c.set_lens(*LENS), off: lambda: c.set_lens(0.0, LENS[1])}
    if args.only == "pinhole":
        modes = {off: lambda: None}
    runs = {name: [] for name in modes}
    for _ in range(args.rounds):
        for name, set_up in modes.items():
            set_up()
            runs[name].append(statistics.median(window(c) for _ in range(args.windows)))
    print(f"{c.device_name}; cat {W}x{H}, one sample, b = {B}; ms per frame, host clock around {args.calls} frames and one wait, median of {args.windows} windows, "
          f"{args.rounds} interleaved rounds", flush=True)
    for name, r in runs.items():
        print(f"  {name:36s} per round {' / '.join('%.4f' % x for x in r)} -> {spread(r)}", flush=True)
    if args.only == "pinhole":
        c.close()
        return
    a, b = statistics.median(runs[on]), statistics.median(runs[off])
    print(f"  lens on / pinhole without caches: {a / b:.4f}", flush=True)
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
        print(f"  {name.split(' (')[0].split(',')[0]:12s} wf_advance {statistics.median(adv) * 1e3:.1f} us per launch ({s['adv_launches']} launches, {s['adv_paths']} paths); "
              f"traversal {statistics.median(trav) * 1e3:.1f} us per launch ({s['trav_launches']}); kernel_ms {statistics.median(ker):.4f}", flush=True)
    c.close()
    c = context()                                                      # the headline's chain: a still pinhole view with its three caches
    c.scene_upload(rt.scenes.spheres("cpu"), mesh)
    cached = [statistics.median(window(c) for _ in range(args.windows)) for _ in range(args.rounds)]
    print(f"  {'pinhole, caches on (the headline)':36s} per round {' / '.join('%.4f' % x for x in cached)} -> {spread(cached)}", flush=True)
    print(f"  lens on / cached headline: {a / statistics.median(cached):.4f}", flush=True)
    c.close()


def opening():
    W, H = 1920, 1080
    c = context(RT_FIRST_HIT_CACHE="0")
    c.scene_upload(rt.scenes.spheres("cpu"), cat_mesh())
    rows = Rows(0, H, H, 1)
    buf = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    p = params(123456, W, H)
    for lens in (LENS, (0.0, LENS[1])):
        c.set_lens(*lens)
        for _ in range(30):
            c.render_device(p, rows, buf.data_ptr())
        c.synchronize()
    c.close()


def tonemap(a):
    """min(pow(c, 1 / 2.2), 255) / 255: the tonemap's scale (cpu:714-716)"""
    return np.minimum(np.power(np.maximum(a[..., :3].astype(np.float64), 0.0), 1 / 2.2), 255.0) / 255.0


def quality():
    w, h, frames = 640, 360, 8
    ctx = context()
    ctx.scene_upload(rt.scenes.spheres("cpu"), cat_mesh())
    pin = tonemap(ctx.render(params(7000, w, h, 1024)))
    ctx.set_lens(*LENS)
    ref = tonemap(ctx.render(params(7000, w, h, 1024)))
    rm = lambda a, m=slice(None): float(np.sqrt(np.mean((a[m] - ref[m]) ** 2)))
    mask = np.abs(ref - pin).max(-1) > 0.02
    print(f"quality: cat scene {w}x{h}, b = {B}, lens R {LENS[0]:g} f {LENS[1]:g}; RMSE in the tonemap's [0, 1] scale against a 1024-sample lens frame", flush=True)
    print(f"  defocused pixels (lens and pinhole 1024-sample frames more than 0.02 apart): {int(mask.sum())} of {mask.size}; there the two references differ by "
          f"{float(np.sqrt(np.mean((ref[mask] - pin[mask]) ** 2))):.5f} RMS -- what a sharp answer would miss", flush=True)
    for spp in (1, 4, 16, 64):
        e = [rm(tonemap(ctx.render(params(100 + i, w, h, spp)))) for i in range(4)]
        print(f"  {spp:3d} sample{'s' if spp > 1 else ' '}: {np.mean(e):.5f} (mean of 4 seeds, min {min(e):.5f}, max {max(e):.5f})", flush=True)
    outs = []
    with rt.SvgfSequence(ctx, w, h) as seq:
        for i in range(frames):
            out = seq.frame(params(100 + i, w, h))
            ctx.synchronize()
            outs.append(tonemap(ctx.device_to_host(out, (h, w, 4))))
    print(f"  SvgfSequence (one sample per frame, pinhole guides) per frame: " + " ".join(f"{rm(o):.5f}" for o in outs), flush=True)
    print(f"  after {frames} frames: overall {rm(outs[-1]):.5f}; defocused region {rm(outs[-1], mask):.5f}, elsewhere {rm(outs[-1], ~mask):.5f}; "
          f"mean signed error there {float(np.mean(outs[-1][mask] - ref[mask])):+.5f} / {float(np.mean(outs[-1][~mask] - ref[~mask])):+.5f}", flush=True)
    ctx.set_lens(0.0, LENS[1])
    outs = []
    with rt.SvgfSequence(ctx, w, h) as seq:
        for i in range(frames):
            out = seq.frame(params(100 + i, w, h))
            ctx.synchronize()
            outs.append(tonemap(ctx.device_to_host(out, (h, w, 4))))
    print(f"  the pinhole's own sequence against the pinhole's 1024-sample frame after {frames} frames: {float(np.sqrt(np.mean((outs[-1] - pin) ** 2))):.5f}", flush=True)
    ctx.close()


if args.only in ("", "frame", "pinhole"):
    frame()
if args.only in ("", "quality"):
    quality()
if args.only == "opening":
    opening()

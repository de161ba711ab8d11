#!/usr/bin/env python3
"""Tinted mirrors and glass, measured (the output is profiles/tint/tint_bench.txt).

  frame   the room (five walls) with the mirror cat and a mirror ball, 1920 x 1080, one sample, b = 3, in up to four configurations, windows of 20 frames and one
          wait, interleaved, each behind one untimed frame; ms per frame and the rays per frame (the sum of .w):
            smooth        nothing flagged: the scene's own form of wf_advance (the plain chain with its closing kernel; with RT_FIRST_HIT_CACHE=0 the still view is off
                          and every ray is traced, without it the still view is on)
            tinted        both mirrors flagged: the tint forms with an empty roughness mask
            rough         both mirrors at --alpha: the gloss forms
            rough_tinted  both at --alpha and flagged: the tint forms with the mask filled
          A tint changes no ray, so the rays of smooth and tinted, and of rough and rough_tinted, are the same number: the ratio of the times is what the forms cost.
          rough_tinted against rough is the price of the mask test and the two stores; tinted against smooth is the price a tint-only scene pays for leaving the plain
          chain (and, without RT_FIRST_HIT_CACHE=0, the still view).
          The library is RT_LIB's or this tree's: the sides that are to be measured on the parent commit (smooth, rough) are run with RT_LIB set to its library and
          --configs smooth,rough, in processes interleaved with this tree's.

usage: [RT_LIB=<parent's library>] [RT_FIRST_HIT_CACHE=0] python tools/tint_bench.py [--rounds N] [--alpha A] [--configs smooth,tinted,rough,rough_tinted] [--tag NAME]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import raytracinggpu_amd as rt  # noqa: E402

ALL = {"smooth": (False, False), "tinted": (False, True), "rough": (True, False), "rough_tinted": (True, True)}
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--alpha", type=float, default=0.25)
ap.add_argument("--configs", default="smooth,tinted,rough,rough_tinted")
ap.add_argument("--tag", default="this tree", help="which library this is, for the output's lines")
args = ap.parse_args()
names = [n for n in args.configs.split(",") if n]
for n in names:
    if n not in ALL:
        raise SystemExit(f"tint_bench: no configuration {n!r} (one of {', '.join(ALL)})")


def spread(v):
    return f"median {statistics.median(v):.3f} ms (min {min(v):.3f}, max {max(v):.3f})"


def timed(f):
    t = time.perf_counter()
    f()
    return (time.perf_counter() - t) * 1e3


c = rt.Context(0)
print(f"{c.device_name}; {args.tag}; {args.rounds} rounds; alpha {args.alpha}; RT_FIRST_HIT_CACHE={os.environ.get('RT_FIRST_HIT_CACHE', '(unset)')}", flush=True)
g = np.load(rt.scenes.CAT_FIXTURE, allow_pickle=False)
copper = (0.72, 0.45, 0.2)
cat = dict(vertices=g["vertices"], indices=g["tri_bvh_order"], bvh_arr10=g["bvh_arr10"], albedo=copper, object_slot=6, mirror=1)
ball = ((24.0, 0.0, 10.0), 10.0, (0.83, 0.61, 0.23), 1, 1.0, 1.0)
c.scene_upload(list(rt.scenes.WALLS[1:]) + [ball], cat)
import torch  # noqa: E402
p = rt.make_params(1920, 1080, 1, 3, **rt.scenes.CPU_LAUNCHER)
rows = rt._capi.Rows(0, 1080, 1080, 1)
buf = torch.zeros((1080, 1920, 4), dtype=torch.float32, device="cuda")


def window():
    for _ in range(20):
        c.render_device(p, rows, buf.data_ptr())
    c.synchronize()


any_tinted = any(ALL[n][1] for n in names)
per = {n: [] for n in names}
rays = {}
for k in range(args.rounds + 1):
    for n in names:
        rough, tinted = ALL[n]
        for slot in (5, 6):
            c.set_roughness(slot, args.alpha if rough else 0.0)
            if any_tinted:                                              # (a library without the entry -- the parent's, through RT_LIB -- is asked for nothing)
                c.set_tint(slot, tinted)
                assert c.tint(slot) == tinted
        c.render_device(p, rows, buf.data_ptr())                        # one untimed frame of this configuration
        c.synchronize()
        if n not in rays:
            rays[n] = int(buf[..., 3].sum(dtype=torch.float64).item())
        per[n].append(timed(window) / 20)
for n, v in per.items():
    print(f"{args.tag}: the room with the mirror cat and a mirror ball, 1920 x 1080, b = 3, {n}: {spread(v[1:])} per frame, {rays[n]} rays per frame", flush=True)
c.close()

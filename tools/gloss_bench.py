#!/usr/bin/env python3
"""Rough mirrors, measured (the output is profiles/gloss/gloss_bench.txt).

  frame   the room (five walls) with the mirror cat and a mirror ball, 1920 x 1080, one sample, b = 3: both smooth (the scene's own form of wf_advance, the still
          view off through RT_FIRST_HIT_CACHE=0 so that both sides trace every ray) against both rough (the gloss form), windows of 20 frames and one wait,
          interleaved, each behind one untimed frame; ms per frame and the rays per frame (the sum of .w) of either side: a rough path leaves its mirror in another
          direction, so the two sides do not trace the same rays -- the ratio of the times over the ratio of the rays is what a ray costs more.

usage: RT_FIRST_HIT_CACHE=0 python tools/gloss_bench.py [--rounds N] [--alpha A] [--only smooth|rough] > profiles/gloss/gloss_bench.txt"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import raytracinggpu_amd as rt  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--alpha", type=float, default=0.25)
ap.add_argument("--only", default="", help="smooth or rough: that side alone (a run under a kernel trace, whose per-kernel sums then belong to one side)")
args = ap.parse_args()


def spread(v):
    return f"median {statistics.median(v):.3f} ms (min {min(v):.3f}, max {max(v):.3f})"


def timed(f):
    t = time.perf_counter()
    f()
    return (time.perf_counter() - t) * 1e3


c = rt.Context(0)
print(f"{c.device_name}; {args.rounds} rounds; alpha {args.alpha}; RT_FIRST_HIT_CACHE={os.environ.get('RT_FIRST_HIT_CACHE', '(unset)')}", flush=True)
g = np.load(rt.scenes.CAT_FIXTURE, allow_pickle=False)
cat = dict(vertices=g["vertices"], indices=g["tri_bvh_order"], bvh_arr10=g["bvh_arr10"], albedo=rt.scenes.CAT_ALBEDO, object_slot=6, mirror=1)
ball = ((24.0, 0.0, 10.0), 10.0, (0.0, 0.0, 0.0), 1, 1.0, 1.0)
c.scene_upload(list(rt.scenes.WALLS[1:]) + [ball], cat)
import torch  # noqa: E402
p = rt.make_params(1920, 1080, 1, 3, **rt.scenes.CPU_LAUNCHER)
rows = rt._capi.Rows(0, 1080, 1080, 1)
buf = torch.zeros((1080, 1920, 4), dtype=torch.float32, device="cuda")


def window():
    for _ in range(20):
        c.render_device(p, rows, buf.data_ptr())
    c.synchronize()


configs = [(name, a) for name, a in (("smooth", 0.0), ("rough", args.alpha)) if args.only in ("", name)]
per = {name: [] for name, _ in configs}
rays = {}
for k in range(args.rounds + 1):
    for name, a in configs:
        c.set_roughness(5, a)
        c.set_roughness(6, a)
        c.render_device(p, rows, buf.data_ptr())                        # one untimed frame of this configuration
        c.synchronize()
        if name not in rays:
            rays[name] = int(buf[..., 3].sum(dtype=torch.float64).item())
        per[name].append(timed(window) / 20)
for name, v in per.items():
    line = f"the room with the mirror cat and a mirror ball, 1920 x 1080, b = 3, {name}: {spread(v[1:])} per frame, {rays[name]} rays per frame"
    if "smooth" in per:
        line += f"; against smooth: time {statistics.median(v[1:]) / statistics.median(per['smooth'][1:]):.4f}, rays {rays[name] / rays['smooth']:.4f}"
    print(line, flush=True)
c.close()

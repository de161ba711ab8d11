#!/usr/bin/env python3
"""Sky sampling, measured (the output is profiles/sky_sample/sky_sample_bench.txt).

  build   rt_scene_set_environment of an n x n map with the share at 0.5 against the same call with the share at 0: the difference is the table's build (four launches,
          two read-backs, one device-wide wait and one allocation), n = 64 and n = 1024.  Host clock, ROUNDS calls each, interleaved; medians and spreads.
  draw    rt_kat_environment_sample on 2^20 keys (upload, one launch of sky_draw + sky_weight, read-back), per map: what one draw costs through the known-answer
          entry, an upper bound on the search (the copies are in it).

  frame   the cat without its walls, 1920 x 1080, one sample, b = 3, under a 256 x 256 gradient sky plus a 0.5 degree sun: share 0 (the sky forms of wf_advance)
          against shares 0.5 and 1 (the sampling forms), windows of 20 frames and one wait, interleaved; ms per frame.  A sky chain uses no still-view cache either way.

usage: python tools/sky_sample_bench.py [--rounds N] > profiles/sky_sample/sky_sample_bench.txt"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import raytracinggpu_amd as rt  # noqa: E402
from raytracinggpu_amd import environment as envm  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
args = ap.parse_args()


def spread(v):
    return f"median {statistics.median(v):.3f} ms (min {min(v):.3f}, max {max(v):.3f})"


def timed(f):
    t = time.perf_counter()
    f()
    return (time.perf_counter() - t) * 1e3


c = rt.Context(0)
c.scene_upload(rt.scenes.spheres("demo10"), None)
print(f"{c.device_name}; {args.rounds} rounds", flush=True)
for n in (64, 1024):
    sky = envm.add_sun(envm.gradient_sky((0.2, 0.5, 2.0), (1.5, 1.5, 1.5), (0.3, 0.2, 0.1), n), (0.3, 0.8, -0.5), np.radians(0.5), 5000.0)
    off, on = [], []
    for _ in range(args.rounds + 1):
        c.set_environment_sampling(0.0)
        off.append(timed(lambda: c.set_environment(sky)))
        c.set_environment_sampling(0.5)
        on.append(timed(lambda: c.set_environment(sky)))
    off, on = off[1:], on[1:]                                            # (the first round loads the code objects)
    print(f"n = {n:4d}: rt_scene_set_environment at share 0: {spread(off)}; at share 0.5: {spread(on)}; the table's build: {statistics.median(on) - statistics.median(off):.3f} ms", flush=True)
    hs = np.arange(1 << 20, dtype=np.uint32) * np.uint32(2654435761)
    draw = [timed(lambda: c.kat_environment_sample(hs, 1)) for _ in range(args.rounds + 1)][1:]
    print(f"n = {n:4d}: rt_kat_environment_sample on 2^20 keys: {spread(draw)}", flush=True)

g = np.load(rt.scenes.CAT_FIXTURE, allow_pickle=False)
c.scene_upload([], dict(vertices=g["vertices"], indices=g["tri_bvh_order"], bvh_arr10=g["bvh_arr10"], albedo=rt.scenes.CAT_ALBEDO, object_slot=0))
c.set_environment(envm.add_sun(envm.gradient_sky((0.2, 0.5, 2.0), (1.5, 1.5, 1.5), (0.3, 0.2, 0.1), 256), (0.3, 0.8, -0.5), np.radians(0.5), 5000.0))
import torch  # noqa: E402
p = rt.make_params(1920, 1080, 1, 3, **rt.scenes.CPU_LAUNCHER)
rows = rt._capi.Rows(0, 1080, 1080, 1)
buf = torch.zeros((1080, 1920, 4), dtype=torch.float32, device="cuda")


def window():
    for _ in range(20):
        c.render_device(p, rows, buf.data_ptr())
    c.synchronize()


per = {0.0: [], 0.5: [], 1.0: []}
for k in range(args.rounds + 1):
    for share in per:
        c.set_environment_sampling(share)
        per[share].append(timed(window) / 20)
for share, v in per.items():
    print(f"open cat 1920 x 1080, b = 3, share {share}: {spread(v[1:])} per frame; against share 0: {statistics.median(v[1:]) / statistics.median(per[0.0][1:]):.4f}", flush=True)
c.close()

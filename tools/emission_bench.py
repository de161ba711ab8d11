#!/usr/bin/env python3
"""Emissive meshes, measured (the output is profiles/emission/emission_bench.txt).

  build   rt_scene_set_emission of a mesh followed by Context.kat_emission_table (the call that brings the table up to date, then reads it back): the table's build --
          four launches, two read-backs, one allocation and one device-wide wait -- for a panel of 2 triangles and a sheet of 5 000, and the same call again with
          nothing to rebuild: the difference is the build.  Host clock, ROUNDS calls each, the radiance changing so that every call rebuilds; medians and spreads.
  frame   the room (five walls) with the cat under a ceiling panel, 1920 x 1080, one sample, b = 3: the panel not emitting (the scene's own forms of wf_advance,
          the still view off through RT_FIRST_HIT_CACHE=0 so that both sides trace every ray) against the panel emitting at shares 0, 0.5 and 1 (the emission forms),
          windows of 20 frames and one wait, interleaved, each behind a refresh of the table and one untimed frame; ms per frame.

usage: RT_FIRST_HIT_CACHE=0 python tools/emission_bench.py [--rounds N] > profiles/emission/emission_bench.txt"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import raytracinggpu_amd as rt  # noqa: E402
from oracle import oracle_py as orc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
args = ap.parse_args()


def spread(v):
    return f"median {statistics.median(v):.3f} ms (min {min(v):.3f}, max {max(v):.3f})"


def timed(f):
    t = time.perf_counter()
    f()
    return (time.perf_counter() - t) * 1e3


def mesh_dict(vertices, triangles, slot):
    m = orc.Mesh.from_arrays(vertices, triangles).build_bvh()
    return dict(vertices=m.vertices, indices=m.triangles, bvh_arr10=m.bvh_array(), albedo=(0.5, 0.5, 0.5), object_slot=slot)


def sheet(n):
    """a bumpy sheet of 2 n n triangles"""
    rng = np.random.default_rng(n)
    x, z = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="xy")
    v = np.stack([x - n / 2, 30 + rng.uniform(-0.3, 0.3, x.shape), z - n / 2], axis=-1).reshape(-1, 3).astype(np.float32)
    i = (z[:-1, :-1] * (n + 1) + x[:-1, :-1]).ravel()
    return v, np.concatenate([np.stack([i, i + 1, i + n + 2], axis=1), np.stack([i, i + n + 2, i + n + 1], axis=1)]).astype(np.int32)


c = rt.Context(0)
print(f"{c.device_name}; {args.rounds} rounds", flush=True)
for name, (v, t) in (("a panel of 2 triangles", rt.scenes.panel((-20, 30, -20), (40, 1, 0), (0, 0.5, 40))), ("a sheet of 5 000 triangles", sheet(50))):
    c.scene_upload(rt.scenes.spheres("cpu"), mesh_dict(v, t, 6))
    build = []
    for k in range(args.rounds + 1):
        c.set_emission(6, (1.0 + k, 2.0, 3.0))
        build.append(timed(c.kat_emission_table))
    print(f"{name}: the table's build with its read-back: {spread(build[1:])}", flush=True)     # (the first round loads the code objects)
    idle = [timed(c.kat_emission_table) for _ in range(args.rounds)]
    print(f"{name}: the read-back alone (nothing to rebuild): {spread(idle)}", flush=True)

g = np.load(rt.scenes.CAT_FIXTURE, allow_pickle=False)
cat = dict(vertices=g["vertices"], indices=g["tri_bvh_order"], bvh_arr10=g["bvh_arr10"], albedo=rt.scenes.CAT_ALBEDO, object_slot=5)
panel = mesh_dict(*rt.scenes.panel((-30, 45, -30), (60, 2, 0), (0, 1, 60)), 6)
c.scene_upload(rt.scenes.WALLS[1:], [cat, panel])
import torch  # noqa: E402
p = rt.make_params(1920, 1080, 1, 3, **rt.scenes.CPU_LAUNCHER)
rows = rt._capi.Rows(0, 1080, 1080, 1)
buf = torch.zeros((1080, 1920, 4), dtype=torch.float32, device="cuda")


def window():
    for _ in range(20):
        c.render_device(p, rows, buf.data_ptr())
    c.synchronize()


configs = [("not emitting", None), ("share 0", 0.0), ("share 0.5", 0.5), ("share 1", 1.0)]
per = {name: [] for name, _ in configs}
for k in range(args.rounds + 1):
    for name, share in configs:
        c.set_emission(6, (0, 0, 0) if share is None else (3e5, 3e5, 2.5e5))
        if share is not None:
            c.set_emission_sampling(share)
        c.kat_emission_table()                                          # the table up to date before the clock starts: the window holds frames alone
        c.render_device(p, rows, buf.data_ptr())                        # ... and one untimed frame of this configuration
        c.synchronize()
        per[name].append(timed(window) / 20)
base = statistics.median(per["not emitting"][1:])
for name, v in per.items():
    print(f"the room with the cat under a panel, 1920 x 1080, b = 3, {name}: {spread(v[1:])} per frame; against not emitting: {statistics.median(v[1:]) / base:.4f}", flush=True)
c.close()

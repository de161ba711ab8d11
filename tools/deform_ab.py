"""GPU box: what a per-frame change of a mesh's shape costs (rt_mesh_set_vertices_device), and what the refit across the chip
(rt_meshops.hip.h refit_up_kernel) saves against the one-workgroup refit_kernel that rt_mesh_transform keeps.  Three runs of everything, with the spread.

  calls    time per call, host wall clock (each entry waits on its stream once, for the root box): rt_mesh_set_vertices_device with the vertices the mesh already has,
           beside rt_mesh_transform with the identity on the SAME context and mesh -- the same retri and requantize around the other refit, so the difference is the refit
           -- and beside rt_mesh_set_vertices_device on a context created under RT_REFIT_WIDE=0 (the same entry through refit_kernel).  Meshes: the cat on the reference's
           tree (2 019 nodes) and the displaced grids of 524 288 and 2 097 152 triangles after an LBVH rebuild.
  kernels  the two refits alone: run `calls` under `rocprofv3 --kernel-trace --output-format csv` (a run of its own), then `--summarise kernel_trace.csv` groups the
           launches of refit_kernel and of refit_parent / refit_up / refit_copy by tree (node count = grid size) and by run.
  frames   steady state of "deform, then render" on the cat at 1920 x 1080, one sample, three bounces: per frame rt_mesh_set_vertices_device (two shapes alternating)
           + rt_render_device, beside the frame of a still mesh on a context under RT_FIRST_HIT_CACHE=0 (every deformed frame is a cache miss by construction) and
           beside the cached still frame.

usage: python tools/deform_ab.py [--only calls|frames] [--meshes cat,g513,g1025] [--runs 3] [--calls 20] > profiles/deform/deform_ab.txt
       python tools/deform_ab.py --summarise kernel_trace.csv [--runs 3] >> profiles/deform/refit_kernels.txt"""
import argparse
import csv
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--only", default="")
ap.add_argument("--meshes", default="cat,g513,g1025")
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--summarise", default="")
args = ap.parse_args()


def spread(xs):
    xs = sorted(xs)
    return "median %.4f (min %.4f, max %.4f, spread %.4f)" % (xs[len(xs) // 2], xs[0], xs[-1], xs[-1] - xs[0])


if args.summarise:
    # per kernel and grid size (= tree), the launches in order, cut into --runs equal parts: the median of each part, then the spread over the parts
    by = {}
    for r in csv.DictReader(open(args.summarise)):
        name = r["Kernel_Name"]
        short = next((k for k in ("refit_kernel", "refit_parent_kernel", "refit_up_kernel", "refit_copy_kernel", "retri_kernel", "repack_vertices_kernel") if k in name), None)
        if short is None:
            continue
        grid = int(r.get("Grid_Size_X", r.get("Grid_Size", 0)) or 0)
        by.setdefault((short, grid), []).append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    print("kernel times from %s (us; launches in order, cut into %d runs)" % (os.path.basename(args.summarise), args.runs))
    for (short, grid), ev in sorted(by.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        d = [x[1] for x in sorted(ev)]
        n = len(d) // args.runs
        if n == 0:
            continue
        meds = [sorted(d[k * n:(k + 1) * n])[n // 2] for k in range(args.runs)]
        print("  %-24s grid %9d threads, %4d launches: per run %s -> %s" % (short, grid, len(d), " / ".join("%.2f" % m for m in meds), spread(meds)))
    sys.exit(0)

import numpy as np
import torch

import raytracinggpu_amd as rt
from raytracinggpu_amd import hostlib
from raytracinggpu_amd._capi import Rows

sys.path.insert(0, os.path.join(ROOT, "tests"))
from lbvh_fixtures import displaced_grid  # noqa: E402

EYE, ZERO = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)


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


def load(name):
    if name == "cat":
        v, t = rt.scenes.load_cat_arrays()
        return np.asarray(v, np.float32), hostlib.build_mesh(v, t, albedo=rt.scenes.CAT_ALBEDO, object_slot=rt.scenes.mesh_slot("cpu")), False
    v, t = displaced_grid(int(name[1:]))
    return v, hostlib.build_mesh(v, t, albedo=rt.scenes.CAT_ALBEDO, object_slot=rt.scenes.mesh_slot("cpu")), True


def per_call(fn, n):
    fn(); fn()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    return (time.perf_counter() - t0) * 1e3 / n


if args.only in ("", "calls"):
    for name in args.meshes.split(","):
        v, mesh, lbvh = load(name)
        dev = torch.from_numpy(np.ascontiguousarray(v)).to("cuda")
        torch.cuda.synchronize()
        wide, serial = context(), context(RT_REFIT_WIDE="0")
        for c in (wide, serial):
            c.scene_upload(rt.scenes.spheres("cpu"), mesh)
            if lbvh:
                c.mesh_rebuild(len(mesh["indices"]), mode="lbvh")
        n_nodes = wide.build_stats()["n_nodes"] if lbvh else len(np.asarray(mesh["bvh_arr10"]).reshape(-1, 10))
        h0 = wide.layout_hash()
        res = {"set_vertices_device (climb)": [], "mesh_transform(identity) (refit_kernel)": [], "set_vertices_device, RT_REFIT_WIDE=0 (refit_kernel)": []}
        for r in range(args.runs):
            res["set_vertices_device (climb)"].append(per_call(lambda: wide.mesh_set_vertices(device_ptr=dev.data_ptr(), stride=3, n_vertices=len(v)), args.calls))
            res["mesh_transform(identity) (refit_kernel)"].append(per_call(lambda: wide.mesh_transform(EYE, ZERO), args.calls))
            res["set_vertices_device, RT_REFIT_WIDE=0 (refit_kernel)"].append(per_call(lambda: serial.mesh_set_vertices(device_ptr=dev.data_ptr(), stride=3, n_vertices=len(v)), args.calls))
        same = wide.layout_hash() == h0 == serial.layout_hash()
        print("%s: %d triangles, %d nodes%s; ms per call over %d calls, %d runs; layouts unchanged and equal: %s" % (
            name, len(mesh["indices"]), n_nodes, " (LBVH)" if lbvh else "", args.calls, args.runs, same), flush=True)
        for k, xs in res.items():
            print("  %-56s %s" % (k, spread(xs)), flush=True)
        a, b = sorted(res["set_vertices_device (climb)"]), sorted(res["mesh_transform(identity) (refit_kernel)"])
        print("  climb - refit_kernel, same context: %+.4f ms per call; refit_kernel's own spread %.4f ms" % (a[len(a) // 2] - b[len(b) // 2], b[-1] - b[0]), flush=True)
        wide.close(); serial.close()

if args.only in ("", "frames"):
    Wd, Ht = 1920, 1080
    v, mesh, _ = load("cat")
    ext = v.max(0) - v.min(0)
    shapes = []
    for ph in (0.0, 1.0):
        w = v.copy()
        w[:, 1] = (v[:, 1] + 0.04 * ext[1] * np.sin(2 * np.pi * 2.5 * (v[:, 0] - v[:, 0].min()) / ext[0] + ph)).astype(np.float32)
        shapes.append(torch.from_numpy(w).to("cuda"))
    torch.cuda.synchronize()
    p = rt.make_params(Wd, Ht, 1, 3, **rt.scenes.CPU_LAUNCHER)
    rows = Rows(0, Ht, Ht, 1)
    bufs = [torch.zeros((Ht, Wd, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
    stream = torch.cuda.Stream()

    def frames(c, deform, n=40, warm=8):
        for k in range(warm + n):
            if k == warm:
                stream.synchronize()
                t0 = time.perf_counter()
            if deform:
                c.mesh_set_vertices(device_ptr=shapes[k % 2].data_ptr(), stride=3, n_vertices=len(v))
            c.render_device(p, rows, bufs[k % 2].data_ptr(), stream.cuda_stream)
            stream.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    on, off = context(), context(RT_FIRST_HIT_CACHE="0")
    for c in (on, off):
        c.scene_upload(rt.scenes.spheres("cpu"), mesh)
    res = {"deform + render": [], "deform + render, RT_FIRST_HIT_CACHE=0": [], "still mesh, RT_FIRST_HIT_CACHE=0": [], "still mesh, cached": []}
    for r in range(args.runs):
        res["deform + render"].append(frames(on, True))
        res["deform + render, RT_FIRST_HIT_CACHE=0"].append(frames(off, True))
        res["still mesh, RT_FIRST_HIT_CACHE=0"].append(frames(off, False))
        res["still mesh, cached"].append(frames(on, False))
    print("cat %dx%d, 1 sample, 3 bounces, one frame in flight (host wall clock, ms per frame over 40 frames, %d runs); cache counters of the deforming context: %s" % (
        Wd, Ht, args.runs, on.first_hit_cache_counts()), flush=True)
    for k, xs in res.items():
        print("  %-40s %s" % (k, spread(xs)), flush=True)
    on.close(); off.close()

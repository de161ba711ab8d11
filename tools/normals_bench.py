"""GPU box: what vertex normals on the device and the normal snapshot cost (rt_mesh_compute_normals*, rt_mesh_snapshot_normals).
Three interleaved rounds of everything, medians of windows, the spread stated.

  calls     rt_mesh_compute_normals per call, host clock around CALLS calls and one wait, on the cat and on the displaced grids of 524 288 and 2 097 152 triangles after
            an LBVH rebuild -- beside its byte floor (adjacency + triangle records + per-vertex buffer + tidx + nrm) and beside THE ONLY WAY THERE WAS: the vertices
            read back from device memory, the same formula in numpy on the host, rt_mesh_set_normals (HOST_CALLS calls per window: it is slow).  The first call (the
            adjacency built on the host and uploaded) separately: the mesh made flat, rebuilt (which drops the adjacency), then one call and a wait.
  kernels   run `--only calls` under `rocprofv3 --kernel-trace --output-format csv` (a run of its own), then `--summarise kernel_trace.csv`.
  planes    rt_render_aov_motion_device at 1920 x 1080 on the smooth cat with its vertices snapshotted, without and with the normal snapshot (HIP events, windows of
            CALLS calls on one stream).
  snapshot  rt_mesh_snapshot_normals per call beside a plain device-to-device copy of the same bytes.
  frames    steady state of deform + render and of deform + compute_normals + render on the headline frame (cat, 1920 x 1080, one sample, three bounces; the mesh
            smooth in both), one frame in flight, host clock.

usage: python tools/normals_bench.py [--only calls|planes|snapshot|frames] [--meshes cat,g513,g1025] > profiles/normals/normals_bench.txt
       python tools/normals_bench.py --summarise kernel_trace.csv >> profiles/normals/normals_kernels.txt"""
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
ap.add_argument("--meshes", default="cat,g513,g1025")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--calls", type=int, default=40)
ap.add_argument("--host-calls", type=int, default=3)
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--no-host", action="store_true", help="skip the host path (the kernel-trace run)")
ap.add_argument("--summarise", default="")
args = ap.parse_args()


def spread(xs):
    xs = sorted(xs)
    return "median %.4f (min %.4f, max %.4f, spread %.4f)" % (xs[len(xs) // 2], xs[0], xs[-1], xs[-1] - xs[0])


if args.summarise:
    by = {}
    for r in csv.DictReader(open(args.summarise)):
        short = next((k for k in ("vertex_normals_kernel", "corner_normals_kernel") if k in r["Kernel_Name"]), None)
        if short is None:
            continue
        grid = int(r.get("Grid_Size_X", r.get("Grid_Size", 0)) or 0)
        by.setdefault((short, grid), []).append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    print("kernel times from %s (us; launches in order, cut into %d runs)" % (os.path.basename(args.summarise), args.rounds))
    for (short, grid), ev in sorted(by.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        d = [x[1] for x in sorted(ev)]
        n = len(d) // args.rounds
        if n == 0:
            continue
        meds = [sorted(d[k * n:(k + 1) * n])[n // 2] for k in range(args.rounds)]
        print("  %-24s grid %9d threads, %4d launches: per run %s -> %s" % (short, grid, len(d), " / ".join("%.2f" % m for m in meds), spread(meds)))
    sys.exit(0)

import numpy as np
import torch

import raytracinggpu_amd as rt
from raytracinggpu_amd import hostlib
from raytracinggpu_amd._capi import Rows

sys.path.insert(0, os.path.join(ROOT, "tests"))
from lbvh_fixtures import displaced_grid  # noqa: E402

SLOT = rt.scenes.mesh_slot("cpu")
HBM = 6.29e12                                                          # bytes / s DESIGN.md calls achievable


def load(name):
    if name == "cat":
        v, t = rt.scenes.load_cat_arrays()
        return np.asarray(v, np.float32), hostlib.build_mesh(v, t, albedo=rt.scenes.CAT_ALBEDO, object_slot=SLOT), False
    v, t = displaced_grid(int(name[1:]))
    return np.asarray(v, np.float32), hostlib.build_mesh(v, t, albedo=rt.scenes.CAT_ALBEDO, object_slot=SLOT), True


def host_normals(v, t):
    """the same formula in numpy, as a caller without the entry would write it: binary32 face normals, summed per vertex, normalised"""
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    n = np.cross(b - a, c - a)
    s = np.zeros_like(v)
    for k in range(3):
        np.add.at(s, t[:, k], n)
    d = (s * s).sum(1, dtype=np.float32)
    with np.errstate(all="ignore"):
        return np.where((d > 0)[:, None], s / np.sqrt(d)[:, None], np.float32(0)).astype(np.float32)


def host_window(fn, sync, n):
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    sync()
    return (time.perf_counter() - t0) * 1e3 / n


def tris_of(mesh, order=None):
    t = np.ascontiguousarray(np.asarray(mesh["indices"])[:, :3], np.int32)
    return t if order is None else t[order]


if args.only in ("", "calls"):
    for name in args.meshes.split(","):
        print("%s: building the mesh ..." % name, file=sys.stderr, flush=True)
        v, mesh, lbvh = load(name)
        print("%s: built" % name, file=sys.stderr, flush=True)
        t = tris_of(mesh)
        ctx = rt.Context(0)
        ctx.scene_upload(rt.scenes.spheres("cpu"), mesh)
        if lbvh:
            _, order = ctx.mesh_rebuild(len(t), mode="lbvh")
            t = t[order]
        dev = torch.from_numpy(np.ascontiguousarray(v)).to("cuda")
        torch.cuda.synchronize()
        nv, nt = len(v), len(t)
        first = []
        for r in range(args.rounds):                                   # the first call: flat, rebuilt (the adjacency is dropped), one call and a wait
            ctx.mesh_set_normals(None, None)
            _, order = ctx.mesh_rebuild(nt, mode="lbvh" if lbvh else "reference")
            t = t[order]
            ctx.synchronize()
            first.append(host_window(ctx.mesh_compute_normals, ctx.synchronize, 1))

        def parent_way():
            vh = dev.cpu().numpy()                                       # the vertices live on the device: read them back
            ctx.mesh_set_normals(host_normals(vh, t), t)

        ctx.mesh_compute_normals()
        got = ctx.mesh_vertex_normals()
        err = float(np.abs(got.astype(np.float64) - host_normals(v, t).astype(np.float64)).max())
        res = {"device": [], "host": []}
        for r in range(args.rounds):
            for _ in range(3):
                ctx.mesh_compute_normals()
            ctx.synchronize()
            res["device"].append(statistics.median(host_window(ctx.mesh_compute_normals, ctx.synchronize, args.calls) for _ in range(args.windows)))
            if args.no_host:
                continue
            parent_way()
            res["host"].append(statistics.median(host_window(parent_way, ctx.synchronize, args.host_calls) for _ in range(3)))
            print("%s: round %d done" % (name, r), file=sys.stderr, flush=True)
        floor = 4 * (nv + 1) + 12 * nt + 48 * nt + 2 * 16 * nv + 16 * nt + 48 * nt
        print("%s: %d vertices, %d triangles%s; ms per call, %d rounds; largest difference between the device's normals and the host formula's %.3g" % (
            name, nv, nt, " (LBVH)" if lbvh else "", args.rounds, err), flush=True)
        print("  %-72s %s" % ("mesh_compute_normals (median of %d windows of %d calls and one wait)" % (args.windows, args.calls), spread(res["device"])), flush=True)
        if not args.no_host:
            print("  %-72s %s" % ("vertices read back + numpy + mesh_set_normals (median of 3 windows of %d calls)" % args.host_calls, spread(res["host"])), flush=True)
        print("  %-72s %s" % ("first call after a rebuild (adjacency built and uploaded), one call", spread(first)), flush=True)
        print("  byte floor: adjacency %.2f + triangle records %.2f + per-vertex buffer %.2f + tidx %.2f + nrm %.2f = %.2f MB = %.2f us at %.2f TB/s" % (
            (4 * (nv + 1) + 12 * nt) / 1e6, 48 * nt / 1e6, 32 * nv / 1e6, 16 * nt / 1e6, 48 * nt / 1e6, floor / 1e6, floor / HBM * 1e6, HBM / 1e12), flush=True)
        h = sorted(res["host"])
        if h:
            print("  host - device: %.4f ms per call; the host path's own spread %.4f ms" % (h[len(h) // 2] - sorted(res["device"])[len(h) // 2], h[-1] - h[0]), flush=True)
        ctx.close()

W, H = 1920, 1080
if args.only in ("", "planes", "snapshot", "frames"):
    v, mesh, _ = load("cat")
    t = tris_of(mesh)
    ext = v.max(0) - v.min(0)
    shapes = []
    for ph in (0.0, 1.0):
        w = v.copy()
        w[:, 1] = (v[:, 1] + 0.04 * ext[1] * np.sin(2 * np.pi * 2.5 * (v[:, 0] - v[:, 0].min()) / ext[0] + ph)).astype(np.float32)
        shapes.append(torch.from_numpy(w).to("cuda"))
    st = torch.cuda.Stream()
    torch.cuda.synchronize()

if args.only in ("", "planes"):
    ctx = rt.Context(0)
    ctx.scene_upload(rt.scenes.spheres("cpu"), mesh)
    ctx.mesh_compute_normals()
    ctx.mesh_snapshot_vertices()
    ctx.mesh_set_vertices(device_ptr=shapes[1].data_ptr(), stride=3, n_vertices=len(v))
    p = rt.make_params(W, H, 1, 3, **rt.scenes.CPU_LAUNCHER)
    planes = torch.zeros((3, H, W, 4), dtype=torch.float32, device="cuda:0")
    prev = torch.zeros((2, H, W, 4), dtype=torch.float32, device="cuda:0")
    table = rt.static_motion()
    call = lambda: ctx.render_aov_motion_device(p, planes.data_ptr(), prev.data_ptr(), motion=table, stream=st.cuda_stream)

    def window():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        for _ in range(args.calls):
            call()
        b.record(st)
        b.synchronize()
        return a.elapsed_time(b) / args.calls * 1e3

    def measure():
        for _ in range(5):
            call()
        torch.cuda.synchronize()
        return statistics.median(window() for _ in range(args.windows))

    call()
    torch.cuda.synchronize()
    on_cat = int((planes[0, ..., 3] == SLOT).sum().item())
    res = {"without": [], "with": []}
    for r in range(args.rounds):
        ctx.mesh_snapshot_normals(keep=False)
        res["without"].append(measure())
        ctx.mesh_snapshot_normals()
        ctx.synchronize()
        res["with"].append(measure())
    print("rt_render_aov_motion_device, smooth cat %dx%d, vertices snapshotted, %d pixels on the cat; us per call (median of %d windows of %d calls), %d rounds" % (
        W, H, on_cat, args.windows, args.calls, args.rounds), flush=True)
    for k, xs in res.items():
        print("  %-28s %s" % (k + " the normal snapshot", spread(xs)), flush=True)
    print("  with - without: %+.2f us; 48 B x %d hits = %.2f MB gathered" % (
        sorted(res["with"])[args.rounds // 2] - sorted(res["without"])[args.rounds // 2], on_cat, on_cat * 48 / 1e6), flush=True)
    ctx.close()

if args.only in ("", "snapshot"):
    ctx = rt.Context(0)
    ctx.scene_upload(rt.scenes.spheres("cpu"), mesh)
    ctx.mesh_compute_normals()
    n4 = 3 * len(t)
    src, dst = torch.zeros((n4, 4), dtype=torch.float32, device="cuda:0"), torch.zeros((n4, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    res = {"rt_mesh_snapshot_normals": [], "a device-to-device copy of the same bytes": []}
    for r in range(args.rounds):
        for name, fn, sync in (("rt_mesh_snapshot_normals", ctx.mesh_snapshot_normals, ctx.synchronize),
                               ("a device-to-device copy of the same bytes", lambda: dst.copy_(src), torch.cuda.synchronize)):
            for _ in range(5):
                fn()
            sync()
            res[name].append(statistics.median(host_window(fn, sync, args.calls) for _ in range(args.windows)) * 1e3)
    print("the cat's normal snapshot: %d float4, %.0f kB; us per call (host clock around %d calls and one wait, median of %d windows), %d rounds" % (
        n4, n4 * 16 / 1e3, args.calls, args.windows, args.rounds), flush=True)
    for k, xs in res.items():
        print("  %-44s %s" % (k, spread(xs)), flush=True)
    ctx.close()

if args.only in ("", "frames"):
    ctx = rt.Context(0)
    ctx.scene_upload(rt.scenes.spheres("cpu"), mesh)
    ctx.mesh_compute_normals()                                           # smooth in both: the frames differ by the recomputation alone
    p = rt.make_params(W, H, 1, 3, **rt.scenes.CPU_LAUNCHER)
    rows = Rows(0, H, H, 1)
    bufs = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(2)]

    def frames(recompute, n=40, warm=8):
        for k in range(warm + n):
            if k == warm:
                st.synchronize()
                t0 = time.perf_counter()
            ctx.mesh_set_vertices(device_ptr=shapes[k % 2].data_ptr(), stride=3, n_vertices=len(v))
            if recompute:
                ctx.mesh_compute_normals()
            ctx.synchronize()                                            # (the frame is issued on another stream: the edits are the caller's to finish first)
            ctx.render_device(p, rows, bufs[k % 2].data_ptr(), st.cuda_stream)
            st.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    res = {"deform + render (stale normals)": [], "deform + compute_normals + render": []}
    for r in range(args.rounds):
        res["deform + render (stale normals)"].append(frames(False))
        res["deform + compute_normals + render"].append(frames(True))
    print("smooth cat %dx%d, 1 sample, 3 bounces, one frame in flight (host wall clock, ms per frame over 40 frames), %d rounds" % (W, H, args.rounds), flush=True)
    for k, xs in res.items():
        print("  %-40s %s" % (k, spread(xs)), flush=True)
    ctx.close()

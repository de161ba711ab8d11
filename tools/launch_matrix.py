#!/usr/bin/env python3
"""What the host launch code does, as text: a fixed list of render / count / trace scenarios through the C-ABI, one line each with the return code, the error text,
every non-timing field of rt_get_stats and the SHA-256 of the output bytes.  Two builds whose lines are equal launched the same work and computed the same frames;
under `rocprofv3 --kernel-trace -- python tools/launch_matrix.py` the trace's ordered kernel list (name, grid, workgroup, LDS) says the same of every launch.
The scenarios reach every renderer, every traversal form, the sub-frame cuts, chunking, sample chains, pipelining, the async slots, batches and the refusals.
usage: [RT_LIB=other/libraytrace_hip.so] [RT_DEBUG_LIB=.../libraytrace_hip_debug.so] python tools/launch_matrix.py [--groups variants,knobs] [--only SUBSTRING] > matrix.txt"""
import argparse
import ctypes as C
import hashlib
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import raytracinggpu_amd as rt
from raytracinggpu_amd import _capi, hostlib

STAT_FIELDS = ("variant", "travq_mode", "grid_blocks", "block_threads", "lds_bytes", "parts", "pixels", "trav_launches", "adv_launches", "adv_paths")
V, T = rt.scenes.load_cat_arrays()
CAT = hostlib.build_mesh(V, T, object_slot=6)
ONLY = ""


def context(env=None, mesh=CAT, spheres="cpu"):
    """a context created under `env` (the knobs are read once, at creation) with the scene uploaded"""
    env = env or {}
    old = {n: os.environ.get(n) for n in env}
    os.environ.update(env)
    try:
        ctx = rt.Context(0)
    finally:
        for n, val in old.items():
            os.environ.pop(n, None) if val is None else os.environ.__setitem__(n, val)
    ctx.scene_upload(rt.scenes.spheres(spheres), mesh)
    return ctx


def params(w=1920, h=1080, spp=1, bounces=3, variant="auto"):
    return rt.make_params(w, h, spp, bounces, variant=variant, **rt.scenes.CPU_LAUNCHER)


def sha(x):
    if isinstance(x, torch.Tensor):
        torch.cuda.synchronize()
        x = x.cpu().numpy()
    return hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()[:24]


def line(name, ctx, fn):
    """run fn() -> output (array / tensor / dict / None); print the scenario's line"""
    if ONLY and ONLY not in name:
        return
    rc, err, out = 0, "", None
    try:
        out = fn()
    except _capi.RtError as e:
        rc, err = e.code, str(e)
        torch.cuda.synchronize()                                      # what the call had enqueued before it was refused
    st = ctx.stats()
    fields = " ".join(f"{k}={st[k]}" for k in STAT_FIELDS)
    res = "-" if out is None else (" ".join(f"{k}={v}" for k, v in out.items()) if isinstance(out, dict) else sha(out))
    print(f"{name} | rc={rc} | {err or '-'} | {fields} | {res}", flush=True)


def dev_frame(rows_n, w, n=1):
    return [torch.zeros((max(rows_n, 1), w, 4), dtype=torch.float32, device="cuda:0") for _ in range(n)]


def device_render(ctx, p, rows=None, pose=None):
    rows = rows or _capi.Rows(0, p.height, p.height, 1)
    buf = dev_frame(rows.n_rows, p.width)[0]
    if pose is None:
        ctx.render_device(p, rows, buf.data_ptr())
    else:
        ctx._check(ctx._L.rt_render_pose_device(ctx._h, C.byref(p), C.byref(pose), C.byref(rows), C.c_void_p(buf.data_ptr()), None))
    ctx.synchronize()
    return buf


def variants():
    ctx = context()
    for v in _capi.VARIANTS:
        line(f"cat 1080p {v}", ctx, lambda: ctx.render(params(variant=v)))
    ctx.stats_enable(True)                                            # the timed launches of part 0's last chain
    for v, spp in (("auto", 1), ("wavefront", 1), ("auto", 4), ("path", 1)):
        line(f"cat 1080p {v} num_rays {spp}, rt_stats_enable", ctx, lambda: ctx.render(params(spp=spp, variant=v)))
    ctx.stats_enable(False)
    for spp in (1, 8, 64):
        for v in ("auto", "path"):
            c2 = context({"RT_PATH_SAMP_MB": "64"})
            line(f"cat 512x512 num_rays {spp} RT_PATH_SAMP_MB=64 {v}", c2, lambda: c2.render(params(512, 512, spp, 3, v)))
    for env in ({}, {"RT_AUTO_LOCKSTEP": "0"}):
        c2 = context(env, mesh=None)
        line(f"spheres only auto {env}", c2, lambda: c2.render(params()))
    for tr, ts, n in ((8, 3, 100), (4, 3, 40), (8, 1, 0)):
        rows = _capi.Rows(8 if ts > 1 else 0, n, tr, ts)
        for v in ("auto", "path"):
            line(f"rows tile_rows {tr} tile_step {ts} n_rows {n} {v}", ctx, lambda: device_render(ctx, params(variant=v), rows))
    for prio in ("0", "1"):
        c2 = context({"RT_PART_PRIO": prio})
        line(f"cat 3840x2160 auto RT_PART_PRIO={prio}", c2, lambda: c2.render(params(3840, 2160)))


def pipelining():
    ctx = context()
    p = params()
    rows = _capi.Rows(0, p.height, p.height, 1)
    a, b = dev_frame(p.height, p.width, 2)
    rgb = torch.zeros((p.height, p.width, 3), dtype=torch.uint8, device="cuda:0")
    s = torch.cuda.Stream()
    ctx.set_pipelining(True)

    def frames():
        for k in range(6):
            ctx.render_device(p, rows, (a, b)[k & 1].data_ptr(), s.cuda_stream)
        for k in range(2):
            ctx.render_device(p, rows, a.data_ptr(), s.cuda_stream)
        ctx.tonemap_device(b.data_ptr(), p.height * p.width, rgb.data_ptr(), s.cuda_stream)
        ctx.render_device(p, rows, b.data_ptr(), s.cuda_stream)         # the hazard: the product takes the full fork
        torch.cuda.synchronize()
        return torch.cat([a.flatten(), b.flatten()])
    line("pipelining: 6 alternating, 2 same buffer, tonemap then its buffer", ctx, frames)
    line("... the image", ctx, lambda: rgb)
    dbg = os.environ.get("RT_DEBUG_LIB")
    if dbg and os.environ.get("RT_LIB") != dbg:                          # the same sequence on the -DRT_DEBUG build: refused
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--groups", "pipelining", "--only", "pipelining: 6"], env=dict(os.environ, RT_LIB=dbg),
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        print("debug build: " + r.stdout.strip().replace("\n", " // "), flush=True)


def asynchronous():
    ctx = context()
    p = params()
    for rgb8 in (False, True):
        outs = [_capi.PinnedArray((p.height, p.width, 3 if rgb8 else 4), np.uint8 if rgb8 else np.float32) for _ in range(2)]

        def run():
            for k in range(4):
                if k >= 2:
                    ctx.wait(k & 1)
                ctx.render_async(p, outs[k & 1].array, slot=k & 1, rgb8=rgb8)
            ctx.wait(0), ctx.wait(1)
            return np.concatenate([o.array.reshape(-1) for o in outs])
        line(f"render_async both slots rgb8={rgb8}", ctx, run)


def batches():
    ctx = context()
    p = params()
    rows, _ = rt.interleaved_rows(p.height, 8, 0, 8)
    for n in (8, 5, 1):
        bufs = dev_frame(rows.n_rows, p.width, n)
        fr = [(bf.data_ptr(), (0.0, 0.0, 55.0 - k), None, 100 + k) for k, bf in enumerate(bufs)]
        line(f"batch of {n} frames, 1/8 share", ctx, lambda: (ctx.render_device_batch(p, rows, fr), ctx.synchronize(), torch.cat([x.flatten() for x in bufs]))[2])
    for v in ("path", "lockstep"):
        bufs = dev_frame(rows.n_rows, p.width, 2)
        fr = [(bf.data_ptr(), (0.0, 0.0, 55.0), None, 1) for bf in bufs]
        line(f"batch refused for {v}", ctx, lambda: ctx.render_device_batch(params(variant=v), rows, fr))


def counting():
    for env, vs in (({}, ("auto", "wavefront", "wavefront_lds", "path", "lockstep", "global")), ({"RT_TRAVQ_QW_COUNT": "1"}, ("auto",))):
        ctx = context(env)
        for v in vs:
            line(f"count_work {v} {env}", ctx, lambda: {k: val for k, val in ctx.count_work(params(640, 360, 1, 3, v), detail=True).items() if k != "steps"})


def knobs():
    for env in ({"RT_TRAVQ_QW": "0"}, {"RT_TRAVQ_Q16": "1", "RT_TRAVQ_QW": "0"}, {"RT_TRAVQ_LDS": "8"}, {"RT_TRAVQ_R": "32"}, {"RT_TRAVQ_CAP": "128"}, {"RT_PARTS": "1"},
                {"RT_PARTS": "3"}, {"RT_TRAVQ_ANYHIT": "0"}):
        ctx = context(env)
        line(f"cat 1080p auto {env}", ctx, lambda: ctx.render(params()))
        if "RT_TRAVQ_LDS" in env or "RT_TRAVQ_CAP" in env:
            line(f"cat 1080p path {env}", ctx, lambda: ctx.render(params(variant="path")))


def scenes():
    ctx = context()
    pose = _capi.make_pose((0.0, 5.0, 50.0), 0.2, 0.25)
    for v in ("auto", "path", "lockstep"):
        line(f"posed camera {v}", ctx, lambda: device_render(ctx, params(variant=v), pose=pose))
    # smooth shading: area-weighted vertex normals of the cat
    fn = np.cross(V[T[:, 1]] - V[T[:, 0]], V[T[:, 2]] - V[T[:, 0]])
    vn = np.zeros_like(V)
    for k in range(3):
        np.add.at(vn, T[:, k], fn)
    vn /= np.maximum(np.linalg.norm(vn, axis=1, keepdims=True), 1e-30)
    ctx.mesh_set_normals(vn, T)
    for v in ("auto", "path", "lockstep"):
        line(f"smooth cat {v}", ctx, lambda: ctx.render(params(variant=v)))
    ctx.mesh_set_normals(None, None)
    rng = np.random.default_rng(7)
    ctx.mesh_set_texture(rng.random((len(V), 2), dtype=np.float32), T, rng.integers(0, 256, (64, 64, 3), dtype=np.uint8), filter="bilinear")
    for v in ("auto", "wavefront", "path", "lockstep"):
        line(f"textured cat {v}", ctx, lambda: ctx.render(params(variant=v)))
    two = [hostlib.build_mesh(V, T, object_slot=3), dict(hostlib.build_mesh(V * 0.5 + np.float32([18, 0, 5]), T, object_slot=7), mirror=1)]
    c2 = context(mesh=two)
    for v in ("auto", "wavefront", "path", "global"):
        line(f"two cats {v}", c2, lambda: c2.render(params(variant=v)))


def tracing():
    rng = np.random.default_rng(11)
    n = 100003
    o = np.float32([0, 0, 55]) + rng.normal(0, 2, (n, 3)).astype(np.float32)
    u = np.float32([0, -5, 0]) + rng.normal(0, 12, (n, 3)).astype(np.float32) - o
    rays = np.concatenate([o, u / np.linalg.norm(u, axis=1, keepdims=True)], axis=1).astype(np.float32)
    for env in ({}, {"RT_TRAVQ_LDS": "8"}, {"RT_TRAVQ_QW": "0"}):
        ctx = context(env)
        for v in ("wavefront_queue", "wavefront", "path"):
            line(f"trace_rays {v} {env}", ctx, lambda: ctx.trace_rays(rays, variant=v))
        line(f"kat_surface {env}", ctx, lambda: ctx.kat_surface(rays[:20001]))
        line(f"... a frame after it {env}", ctx, lambda: ctx.render(params(640, 360)))


def main():
    global ONLY
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", default="", help="comma-separated: variants, pipelining, asynchronous, batches, counting, knobs, scenes, tracing (default: all)")
    ap.add_argument("--only", default="", help="print the scenarios whose name contains this")
    args = ap.parse_args()
    ONLY = args.only
    for group in (variants, pipelining, asynchronous, batches, counting, knobs, scenes, tracing):
        if not args.groups or group.__name__ in args.groups.split(","):
            group()


if __name__ == "__main__":
    main()

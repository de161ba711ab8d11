#!/usr/bin/env python3
"""Cost of a textured mesh: ms per frame of the 1920x1080 cat (spp 1, b 3, the cpu preset) untextured, textured with nearest and with bilinear filtering.

The texture is procedural (a 512 x 1024 RGBA8 image, the size of the reference asset's map_Kd; its pixels are not used), the UVs planar over the cat's x / y.
Frames are rendered back to back into one device buffer on one stream and timed with HIP events over the whole window after a warm-up; the three forms
alternate round by round, and the table gives each form's median over the rounds.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    import torch
    import raytracinggpu_amd as rt
    W, H = 1920, 1080
    g = np.load(rt.scenes.CAT_FIXTURE, allow_pickle=False)
    v, tv = g["vertices"], np.asarray(g["tri_bvh_order"])[:, :3]
    mesh = dict(vertices=v, indices=g["tri_bvh_order"], bvh_arr10=g["bvh_arr10"], albedo=rt.scenes.CAT_ALBEDO, object_slot=6)
    lo, hi = v.min(0), v.max(0)
    uvs = ((v[:, :2] - lo[:2]) / (hi[:2] - lo[:2])).astype(np.float32)
    yy, xx = np.mgrid[0:1024, 0:512]
    px = np.stack([(xx * 255) // 511, (yy * 255) // 1023, ((xx // 32 + yy // 32) % 2) * 255, np.full_like(xx, 255)], -1).astype(np.uint8)
    ctx = rt.Context(0)
    ctx.scene_upload(rt.scenes.spheres("cpu"), mesh)
    p = rt.make_params(W, H, 1, 3, **rt.scenes.CPU_LAUNCHER)
    rows = rt._capi.Rows(0, H, H, 1)
    out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def use(form):
        if form == "untextured":
            ctx.mesh_set_texture(None, None, None)
        else:
            ctx.mesh_set_texture(uvs, tv, px, filter=form)

    def window(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            ctx.render_device(p, rows, out.data_ptr(), stream)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    forms = ("untextured", "nearest", "bilinear")
    ms = {f: [] for f in forms}
    for f in forms:
        use(f)
        window(a.warmup)
    for _ in range(a.rounds):
        for f in forms:
            use(f)
            window(2)
            ms[f].append(window(a.frames))
    res = {f: round(float(np.median(ms[f])), 4) for f in forms}
    res.update(workload="cat_1920x1080_spp1_b3", texture="512x1024 RGBA8", device=ctx.device_name, frames=a.frames, rounds=a.rounds,
               spread={f: [round(min(ms[f]), 4), round(max(ms[f]), 4)] for f in forms})
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()

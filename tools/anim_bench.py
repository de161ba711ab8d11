"""GPU box: what an animated sequence costs, four ways.  A K-frame sequence on the cat scene in which the light orbits (MoveLightSource steps) and the floor sphere moves
(MoveObject steps), b = 3, one sample:
  (a) rt_scene_upload + a lone frame          -- the only way before the in-place edits: every mesh re-sent and re-laid out per frame
  (b) rt_scene_set_light / set_sphere + a lone frame
  (c) rt_render_device_batch of K frames      -- the static scene: what a batch costs without per-frame tables
  (d) rt_render_device_batch_scenes           -- the batch with every frame's own light and sphere poses: (d0) every frame holding the uploaded scene -- the pixels of (c), so
                                                 the difference is the tables alone -- and (d) the moving sequence (other pixels: other rays)
(a) and (b) on a full 1920x1080 frame and on the share of rank 3 of 8 (interleaved 8-row tiles); (c) and (d) on that share.  ms per frame: the median of RUNS timed runs in
this one process, each a host clock around N frames that ends in a synchronise; (c) and (d) alternate run by run.  (b) against (a) is what the edit saves, (d0) against (c) what the
tables cost; the spread of (c)'s runs says how small a difference this output can show.
usage: python tools/anim_bench.py [> profiles/anim/anim_bench.txt]"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np
import torch
import raytracinggpu_amd as rt

K = int(os.environ.get("K", "8"))
RUNS = int(os.environ.get("RUNS", "7"))
N = int(os.environ.get("FRAMES", "96"))
W, H, B = 1920, 1080, 3

g = np.load(rt.scenes.CAT_FIXTURE, allow_pickle=False)
mesh = dict(vertices=g["vertices"], indices=g["tri_bvh_order"], bvh_arr10=g["bvh_arr10"], albedo=rt.scenes.CAT_ALBEDO, object_slot=6)
base = [(tuple(float(x) for x in s[0]), float(s[1]), tuple(float(x) for x in s[2]), 0, 1.0, 1.0) for s in rt.scenes.spheres("cpu")]

# the sequence: frame k's light and floor
lights, floors = [], []
light, c = rt.scenes.LIGHT, np.float32(base[1][0])
for k in range(K):
    light = rt.light_orbit(light, 4.0, 0.1)
    c = (c + (np.float32([0.0, -1.5, 0.0]) * np.float32(0.2)).astype(np.float32)).astype(np.float32)
    lights.append(light)
    floors.append((tuple(float(x) for x in c),) + base[1][1:])
static = [(rt.scenes.LIGHT, [(s[0], s[1]) for s in base]) for k in range(K)]
scenes = [(lights[k], [(s[0], s[1]) if j != 1 else (floors[k][0], floors[k][1]) for j, s in enumerate(base)]) for k in range(K)]

ctx = rt.Context(0)
ctx.scene_upload(base, mesh)
st = torch.cuda.Stream()
p = rt.make_params(W, H, 1, B, **rt.scenes.CPU_LAUNCHER)


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(n):
        fn(k)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def report(name, runs):
    print(f"{name}: {statistics.median(runs):.4f} ms per frame (median of {len(runs)} runs, min {min(runs):.4f}, max {max(runs):.4f})", flush=True)
    return statistics.median(runs)


print(f"{ctx.device_name}; cat scene {W}x{H} b={B}, one sample; a sequence of {K} frames (light orbit + one moving sphere); {RUNS} runs of {N} lone frames / {4 * N} batched frames each", flush=True)
for what, rows in (("full frame", rt.interleaved_rows(H, 8, 0, 1)[0]), ("share of rank 3 of 8", rt.interleaved_rows(H, 8, 3, 8)[0])):
    bufs = [torch.zeros((rows.n_rows, W, 4), dtype=torch.float32, device="cuda:0") for _ in range(2 * K)]

    def upload_frame(k):
        j = k % K
        ctx.scene_upload([s if i != 1 else floors[j] for i, s in enumerate(base)], mesh, light=lights[j])
        ctx.render_device(p, rows, bufs[k & 1].data_ptr(), st.cuda_stream)

    def edit_frame(k):
        j = k % K
        ctx.set_light(*lights[j])
        ctx.set_sphere(1, floors[j])
        ctx.render_device(p, rows, bufs[k & 1].data_ptr(), st.cuda_stream)

    def plain_frame(k):
        ctx.render_device(p, rows, bufs[k & 1].data_ptr(), st.cuda_stream)

    res = {}
    for name, fn in (("(a) upload + lone frame", upload_frame), ("(b) set_light / set_sphere + lone frame", edit_frame), ("    lone frame of the static scene", plain_frame)):
        ctx.scene_upload(base, mesh)
        timed(fn, 6)
        res[name] = report(f"{what}: {name}", [timed(fn, N) / N for _ in range(RUNS)])
    a, b = res["(a) upload + lone frame"], res["(b) set_light / set_sphere + lone frame"]
    print(f"{what}: the edit saves {a - b:.4f} ms per frame ({a / b:.2f}x)", flush=True)
    if rows.tile_step == 1:
        continue
    ctx.scene_upload(base, mesh)
    descs = [[(bufs[h * K + k].data_ptr(), (0.0, 0.0, 55.0), None, 1000 + k) for k in range(K)] for h in range(2)]
    nb = max(4, 4 * N // K)                                         # calls per run: as long a window as the lone frames get
    plain = lambda k: ctx.render_device_batch(p, rows, descs[k & 1], st.cuda_stream)
    same = lambda k: ctx.render_device_batch(p, rows, descs[k & 1], st.cuda_stream, scenes=static)
    anim = lambda k: ctx.render_device_batch(p, rows, descs[k & 1], st.cuda_stream, scenes=scenes)
    timed(plain, 3), timed(same, 3), timed(anim, 3)
    rc, r0, rd = [], [], []
    for _ in range(RUNS):                                             # alternating: all three see the same machine
        rc.append(timed(plain, nb) / (nb * K))
        r0.append(timed(same, nb) / (nb * K))
        rd.append(timed(anim, nb) / (nb * K))
    mc = report(f"{what}: (c) rt_render_device_batch of {K} frames", rc)
    m0 = report(f"{what}: (d0) rt_render_device_batch_scenes of {K} frames, the uploaded scene in each", r0)
    report(f"{what}: (d) rt_render_device_batch_scenes of {K} frames, the moving sequence", rd)
    print(f"{what}: the per-frame tables cost {m0 - mc:+.4f} ms per frame ({(m0 / mc - 1) * 100:+.2f} %); spread of (c)'s runs {max(rc) - min(rc):.4f} ms", flush=True)
    del bufs
ctx.close()

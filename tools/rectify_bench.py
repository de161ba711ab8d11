"""GPU box: what the responsive history costs on the headline frame -- cat scene, 1920x1080, b = 3, one sample.
In one process, alternating:
  accumulate                   rt_temporal_accumulate_device in steady state (a previous frame, every pixel reprojected)
  accumulate, fast             rt_temporal_accumulate_fast_device on the same inputs: + 16 B read (the previous fast plane at the accepted tap) and 16 B written per pixel
  rectify, radius 1 / 2 / 3    rt_history_rectify_device on a history longer than the fast one (every window runs; out of place, so that the input stays what it is), beside its byte floor: 64 B read (history
                               32, fast 16, plane 0 16) and 32 B written per pixel at the 6.29 TB/s DESIGN.md calls achievable
  rectify, all copies          the same call on a history no longer than the fast one: every pixel a copy (a first frame)
  frame, frame + rectify       one whole SvgfSequence.frame, without and with rectify=
Each figure is the median of RUNS windows of N calls on one stream between two HIP events (torch.cuda.Event), after a warm-up of every call.
usage: python tools/rectify_bench.py [> profiles/rectify/rectify_bench.txt]"""
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import numpy as np
import torch
import raytracinggpu_amd as rt

RUNS = int(os.environ.get("RUNS", "7"))
N = int(os.environ.get("N", "40"))
W, H, B = 1920, 1080, 3
HBM = 6.29e12                                                        # bytes / s DESIGN.md calls achievable

g = np.load(rt.scenes.CAT_FIXTURE, allow_pickle=False)
ctx = rt.Context(0)
ctx.scene_upload(rt.scenes.spheres("cpu"), dict(vertices=g["vertices"], indices=g["tri_bvh_order"], bvh_arr10=g["bvh_arr10"], albedo=rt.scenes.CAT_ALBEDO, object_slot=6))
st = torch.cuda.Stream()
s = st.cuda_stream
rows = rt.interleaved_rows(H, 8, 0, 1)[0]
zeros = lambda *shape: torch.zeros(shape, dtype=torch.float32, device="cuda:0")
color, planes = zeros(H, W, 4), zeros(3, H, W, 4)
hist, fast, out, out_fast = [zeros(2, H, W, 4), zeros(2, H, W, 4)], [zeros(H, W, 4), zeros(H, W, 4)], zeros(2, H, W, 4), zeros(H, W, 4)
rp = rt.make_reproject(motion=rt.static_motion())
torch.cuda.synchronize()


def params(seed):
    return rt.make_params(W, H, 1, B, **dict(rt.scenes.CPU_LAUNCHER, seed=seed))


def window(fn, n=N):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    for _ in range(n):
        fn()
    b.record(st)
    b.synchronize()
    return a.elapsed_time(b) / n


print(f"{ctx.device_name}; cat scene {W}x{H}, one sample; fast_history {rt.FAST_HISTORY_DEFAULT}, {rt.RECTIFY_DEFAULTS}", flush=True)
# a static sequence of eight frames: hist[1] and fast[1] end as histories of length 8 and 4
ctx.render_aov_device(params(1), planes.data_ptr(), stream=s)
for f in range(8):
    ctx.render_device(params(1 + f), rows, color.data_ptr(), s)
    first = f == 0
    ctx.temporal_accumulate_fast_device(color.data_ptr(), planes.data_ptr(), 0 if first else planes.data_ptr(), 0 if first else hist[1 - f % 2].data_ptr(),
                                        0 if first else fast[1 - f % 2].data_ptr(), W, H, hist[f % 2].data_ptr(), fast[f % 2].data_ptr(), reproject=None if first else rp, stream=s)
torch.cuda.synchronize()
n, nf = hist[1][1, ..., 2], fast[1][..., 3]
print(f"history length 8 on {float((n == 8).float().mean()):.3f} of the frame, fast length 4 on {float((nf == 4).float().mean()):.3f}, misses {float((nf == 0).float().mean()):.3f}", flush=True)
PH, PF = hist[1].data_ptr(), fast[1].data_ptr()


def rectify(radius, source):
    rc = rt.make_rectify_params(radius=radius, k_clamp=rt.RECTIFY_DEFAULTS["k_clamp"])
    return lambda: ctx.history_rectify_device(source.data_ptr(), PF, planes.data_ptr(), W, H, out.data_ptr(), params=rc, stream=s)


short = hist[1].clone()
short[1, ..., 2] = torch.minimum(short[1, ..., 2], fast[1][..., 3])   # a history no longer than the fast one
calls = [("accumulate", lambda: ctx.temporal_accumulate_device(color.data_ptr(), planes.data_ptr(), planes.data_ptr(), PH, W, H, out.data_ptr(), reproject=rp, stream=s)),
         ("accumulate, fast", lambda: ctx.temporal_accumulate_fast_device(color.data_ptr(), planes.data_ptr(), planes.data_ptr(), PH, PF, W, H, out.data_ptr(), out_fast.data_ptr(),
                                                                          reproject=rp, stream=s))]
calls += [(f"rectify, radius {r}", rectify(r, hist[1])) for r in (1, 2, 3)] + [("rectify, all copies (radius 1)", rectify(1, short))]
seqs = {"frame": rt.SvgfSequence(ctx, W, H, stream=s), "frame + rectify": rt.SvgfSequence(ctx, W, H, stream=s, rectify=rt.make_rectify_params())}
seed = [100]


def frame(seq):
    def fn():
        seed[0] += 1
        seq.frame(params(seed[0]))
    return fn


calls += [(name, frame(seq)) for name, seq in seqs.items()]
for _, fn in calls:
    for _ in range(5):
        fn()
torch.cuda.synchronize()
runs = {name: [] for name, _ in calls}
for _ in range(RUNS):                                                # alternating: one window of every call per round
    for name, fn in calls:
        runs[name].append(window(fn, 10 if name.startswith("frame") else N))
med = {name: statistics.median(r) for name, r in runs.items()}
for name, r in runs.items():
    print(f"{name}: {med[name] * 1e3:.1f} us per call (median of {RUNS} windows, min {min(r) * 1e3:.1f}, max {max(r) * 1e3:.1f})", flush=True)
px = W * H
print(f"accumulate, fast: +{(med['accumulate, fast'] - med['accumulate']) * 1e3:.1f} us = {med['accumulate, fast'] / med['accumulate']:.3f} x; its added traffic (16 B read + 16 B written "
      f"per pixel) is {px * 32 / HBM * 1e6:.1f} us at {HBM / 1e12:.2f} TB/s", flush=True)
floor = px * 96 / HBM * 1e6
for r in (1, 2, 3):
    t = med[f"rectify, radius {r}"] * 1e3
    print(f"rectify, radius {r}: {t:.1f} us = {t / floor:.2f} x the floor of {floor:.1f} us (64 B read + 32 B written per pixel = {px * 96 / 1e6:.0f} MB at {HBM / 1e12:.2f} TB/s)", flush=True)
print(f"SvgfSequence.frame: {med['frame'] * 1e3:.1f} us without, {med['frame + rectify'] * 1e3:.1f} us with rectification: +{(med['frame + rectify'] - med['frame']) * 1e3:.1f} us", flush=True)
for seq in seqs.values():
    seq.close()
ctx.close()

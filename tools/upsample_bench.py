"""GPU box: what rt_upsample_device costs beside its byte floor, and what the chain gains from it, on the headline frame -- cat scene, 1920x1080, b = 3, one sample.
In one process, alternating:
  (a) the kernel            rt_upsample_device for f = 2 and 4, one plane (a colour frame) and two (a history), rendered planes at both resolutions; beside each the
                            traffic it cannot avoid -- 32 B of planes read and 16 n_planes B written per pixel, (32 + 16 n_planes) / f^2 B of low-resolution data
  (b) the chain             SvgfSequence.frame at full resolution (today's) against upsample=2 with filter_at="low" (pipeline A) and "full" (pipeline B): render,
                            planes, accumulation, filter, upsample, all on one stream
Each figure is the median of RUNS windows of N calls on one stream between two HIP events (torch.cuda.Event), after a warm-up of every call.
usage: python tools/upsample_bench.py [> profiles/upsample/upsample_bench.txt]"""
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
zeros = lambda *shape: torch.zeros(shape, dtype=torch.float32, device="cuda:0")


def params(w, h, seed):
    return rt.make_params(w, h, 1, B, **dict(rt.scenes.CPU_LAUNCHER, seed=seed))


def window(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    for _ in range(N):
        fn()
    b.record(st)
    b.synchronize()
    return a.elapsed_time(b) / N


def measure(calls):
    for _, fn in calls:
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    runs = {name: [] for name, _ in calls}
    for _ in range(RUNS):                                            # alternating: one window of every call per round
        for name, fn in calls:
            runs[name].append(window(fn))
    return runs


print(f"{ctx.device_name}; cat scene {W}x{H}, one sample, b = {B}; {rt.UPSAMPLE_DEFAULTS}", flush=True)
planes, out = zeros(3, H, W, 4), zeros(2, H, W, 4)
ctx.render_aov_device(params(W, H, 1), planes.data_ptr(), stream=s)
calls, floors, keep = [], {}, []
for f in (2, 4):
    w, h = W // f, H // f
    low_planes, hist, color = zeros(3, h, w, 4), zeros(2, h, w, 4), zeros(h, w, 4)
    ctx.render_aov_device(params(w, h, 1), low_planes.data_ptr(), stream=s)
    ctx.render_device(params(w, h, 1), rt.interleaved_rows(h, 8, 0, 1)[0], color.data_ptr(), s)
    ctx.temporal_accumulate_device(color.data_ptr(), low_planes.data_ptr(), 0, 0, w, h, hist.data_ptr(), stream=s)
    keep.append((low_planes, hist, color))
    for n in (1, 2):
        name = f"upsample f = {f}, {n} plane{'s' * (n - 1)}"
        calls.append((name, lambda f=f, n=n, lp=low_planes, hs=hist: ctx.upsample_device(hs.data_ptr(), lp.data_ptr(), planes.data_ptr(), W, H, f, out.data_ptr(), n_planes=n, stream=s)))
        floors[name] = W * H * (32 + 16 * n) * (1 + 1 / (f * f))
torch.cuda.synchronize()
for name, r in measure(calls).items():
    med, floor = statistics.median(r), floors[name] / HBM * 1e6
    print(f"{name}: {med * 1e3:.1f} us per call (median of {RUNS} windows of {N} calls, min {min(r) * 1e3:.1f}, max {max(r) * 1e3:.1f}); "
          f"{floors[name] / 1e6:.0f} MB = {floor:.1f} us at {HBM / 1e12:.2f} TB/s: {med * 1e3 / floor:.2f} x the floor", flush=True)

# (b) the chain, end to end: every sequence gets its own seeds; the first frames fill the histories
seqs = [("full resolution (today)", rt.SvgfSequence(ctx, W, H, stream=s)), ("A: upsample=2, filter_at='low'", rt.SvgfSequence(ctx, W, H, stream=s, upsample=2, filter_at="low")),
        ("B: upsample=2, filter_at='full'", rt.SvgfSequence(ctx, W, H, stream=s, upsample=2, filter_at="full"))]
seed = [0]


def frame(seq):
    seed[0] += 1
    seq.frame(params(W, H, seed[0]))


chain = measure([(name, lambda q=q: frame(q)) for name, q in seqs])
med = {name: statistics.median(r) for name, r in chain.items()}
for name, r in chain.items():
    print(f"chain, {name}: {med[name] * 1e3:.1f} us per frame (median of {RUNS} windows of {N} frames, min {min(r) * 1e3:.1f}, max {max(r) * 1e3:.1f}); "
          f"{med[name] / med['full resolution (today)']:.3f} x today's", flush=True)
torch.cuda.synchronize()
for _, q in seqs:
    q.close()
ctx.close()

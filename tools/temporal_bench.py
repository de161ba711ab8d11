"""GPU box: what temporal accumulation and the variance-guided filter cost on the headline frame -- cat scene, 1920x1080, b = 3, one sample.
  render b=3, aov            the frame and its first-hit planes (as tools/denoise_bench.py)
  accumulate, steady state   rt_temporal_accumulate_device on a static sequence whose history is longer than 4 frames: no pixel takes the spatial-variance tail
  accumulate, first frame    the same call without a previous frame: every pixel takes the tail (25 direct loads)
  denoise / denoise_var n    rt_denoise_device and rt_denoise_var_device with their default weights, n = 1 .. 5; pass k's time is the difference of consecutive n
  chain                      render + planes + accumulate + denoise_var (default passes) on one stream: the whole per-frame chain beside the frame alone
Each figure is the median of RUNS windows of N calls on one stream between two HIP events (torch.cuda.Event), after a warm-up of every call.  Compulsory traffic of an
accumulation: 16 B colour + 32 B planes + 32 B previous planes + 32 B history read, 32 B written = 144 B per pixel.
usage: python tools/temporal_bench.py [> profiles/temporal/temporal_bench.txt]; ONLY=temporal|denoise|render|chain (with N, RUNS) narrows the run, for a kernel trace."""
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import numpy as np
import torch
import raytracinggpu_amd as rt

RUNS = int(os.environ.get("RUNS", "7"))
N = int(os.environ.get("N", "40"))
ONLY = os.environ.get("ONLY", "")
W, H, B = 1920, 1080, 3
HBM = 6.29e12                                                        # bytes / s DESIGN.md calls achievable

g = np.load(rt.scenes.CAT_FIXTURE, allow_pickle=False)
ctx = rt.Context(0)
ctx.scene_upload(rt.scenes.spheres("cpu"), dict(vertices=g["vertices"], indices=g["tri_bvh_order"], bvh_arr10=g["bvh_arr10"], albedo=rt.scenes.CAT_ALBEDO, object_slot=6))
st = torch.cuda.Stream()
rows = rt.interleaved_rows(H, 8, 0, 1)[0]
zeros = lambda *shape: torch.zeros(shape, dtype=torch.float32, device="cuda:0")
color, planes, prev_planes, out = zeros(H, W, 4), zeros(3, H, W, 4), zeros(3, H, W, 4), zeros(H, W, 4)
hist = [zeros(2, H, W, 4), zeros(2, H, W, 4)]
rp = rt.make_reproject(motion=rt.static_motion())                    # the table is read although nothing moves: the general case
torch.cuda.synchronize()


def params(seed):
    return rt.make_params(W, H, 1, B, **dict(rt.scenes.CPU_LAUNCHER, seed=seed))


def window(fn):
    """ms per call: N calls on the stream between two events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    for _ in range(N):
        fn()
    b.record(st)
    b.synchronize()
    return a.elapsed_time(b) / N


def measure(name, fn):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    runs = [window(fn) for _ in range(RUNS)]
    m = statistics.median(runs)
    print(f"{name}: {m * 1e3:.1f} us per call (median of {RUNS} windows of {N} calls, min {min(runs) * 1e3:.1f}, max {max(runs) * 1e3:.1f})", flush=True)
    return m


def accumulate(src, dst, first=False):
    ctx.temporal_accumulate_device(color.data_ptr(), planes.data_ptr(), 0 if first else prev_planes.data_ptr(), 0 if first else hist[src].data_ptr(), W, H, hist[dst].data_ptr(),
                                   reproject=None if first else rp, stream=st.cuda_stream)


print(f"{ctx.device_name}; cat scene {W}x{H}, one sample; {rt._capi.TEMPORAL_DEFAULTS}; {rt._capi.DENOISE_VAR_DEFAULTS}", flush=True)
# a static sequence of six frames: hist[1] ends as a history of length 6, hist[0] of length 5
ctx.render_aov_device(params(1), planes.data_ptr(), stream=st.cuda_stream)
ctx.render_aov_device(params(1), prev_planes.data_ptr(), stream=st.cuda_stream)
for f in range(6):
    ctx.render_device(params(1 + f), rows, color.data_ptr(), st.cuda_stream)
    accumulate(1 - f % 2, f % 2, first=f == 0)
torch.cuda.synchronize()
n = hist[1][1, ..., 2]
print(f"history lengths after six static frames: min {n.min().item():.0f}, max {n.max().item():.0f}; pixels with a first hit: {(planes[0, ..., 3] >= 0).float().mean().item():.4f}", flush=True)
frame = None
if ONLY in ("", "render"):
    frame = measure("render b=3", lambda: ctx.render_device(params(7), rows, color.data_ptr(), st.cuda_stream))
    measure("aov", lambda: ctx.render_aov_device(params(7), planes.data_ptr(), stream=st.cuda_stream))
if ONLY in ("", "temporal"):
    floor = W * H * 144 / HBM * 1e3
    for name, first in (("accumulate, steady state", False), ("accumulate, first frame", True)):
        m = measure(name, lambda: accumulate(1, 0, first))
        print(f"    compulsory traffic {W * H * (144 if not first else 80) / 1e6:.0f} MB; the steady-state floor is {floor * 1e3:.1f} us at {HBM / 1e12:.2f} TB/s: {m / floor:.1f} x", flush=True)
if ONLY in ("", "denoise"):
    prev = prev_v = 0.0
    for k in range(1, 6):
        m = measure(f"denoise n_passes={k}", lambda: ctx.denoise_device(color.data_ptr(), planes.data_ptr(), W, H, out.data_ptr(), n_passes=k, stream=st.cuda_stream))
        v = measure(f"denoise_var n_passes={k}", lambda: ctx.denoise_var_device(hist[1].data_ptr(), planes.data_ptr(), W, H, out.data_ptr(), n_passes=k, stream=st.cuda_stream))
        print(f"    pass {k - 1} (step {1 << (k - 1)}): plain {(m - prev) * 1e3:.1f} us, variance-guided {(v - prev_v) * 1e3:.1f} us ({(v - prev_v) / (m - prev):.2f} x)", flush=True)
        prev, prev_v = m, v
if ONLY in ("", "chain"):
    def chain():
        ctx.render_device(params(7), rows, color.data_ptr(), st.cuda_stream)
        ctx.render_aov_device(params(7), planes.data_ptr(), stream=st.cuda_stream)
        accumulate(1, 0)
        ctx.denoise_var_device(hist[0].data_ptr(), planes.data_ptr(), W, H, out.data_ptr(), stream=st.cuda_stream)
    m = measure("chain: render + aov + accumulate + denoise_var (defaults)", chain)
    if frame:
        print(f"    {m / frame:.2f} x the b = 3 frame alone", flush=True)
ctx.close()

"""GPU box: what the first-hit planes and the a-trous filter cost on the headline frame -- cat scene, 1920x1080, b = 3, one sample.
  render b=3 / b=0   the frame itself, and the same frame with direct light only (one camera ray and one shadow ray per pixel: the traversal work nearest the planes')
  aov                rt_render_aov_device: emit + wf_travq + close, one ray per pixel
  denoise n = 1..5   rt_denoise_device with the default weights; pass k's time is the difference of consecutive n, beside its compulsory traffic: 64 B read + 16 B
                     written per pixel
Each figure is the median of RUNS windows of N calls on one stream between two HIP events (torch.cuda.Event), after a warm-up of every call.
usage: python tools/denoise_bench.py [> profiles/denoise/denoise_bench.txt]; ONLY=denoise|aov|render (with N, RUNS) narrows the run to one kind of call, for a kernel trace."""
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
p3 = rt.make_params(W, H, 1, B, **rt.scenes.CPU_LAUNCHER)
p0 = rt.make_params(W, H, 1, 0, **rt.scenes.CPU_LAUNCHER)
color = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
direct = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
planes = torch.zeros((3, H, W, 4), dtype=torch.float32, device="cuda:0")
out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
torch.cuda.synchronize()


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


print(f"{ctx.device_name}; cat scene {W}x{H}, one sample; weights {rt._capi.DENOISE_DEFAULTS}", flush=True)
ctx.render_device(p3, rows, color.data_ptr(), st.cuda_stream)
ctx.render_aov_device(p3, planes.data_ptr(), stream=st.cuda_stream)
torch.cuda.synchronize()
if ONLY in ("", "render"):
    measure("render b=3", lambda: ctx.render_device(p3, rows, color.data_ptr(), st.cuda_stream))
    measure("render b=0", lambda: ctx.render_device(p0, rows, direct.data_ptr(), st.cuda_stream))
if ONLY in ("", "aov"):
    measure("aov", lambda: ctx.render_aov_device(p3, planes.data_ptr(), stream=st.cuda_stream))
if ONLY in ("", "denoise"):
    floor = W * H * 80 / HBM * 1e3
    prev = 0.0
    for n in range(1, 6):
        m = measure(f"denoise n_passes={n}", lambda: ctx.denoise_device(color.data_ptr(), planes.data_ptr(), W, H, out.data_ptr(), n_passes=n, stream=st.cuda_stream))
        print(f"    pass {n - 1} (step {1 << (n - 1)}): {(m - prev) * 1e3:.1f} us; compulsory traffic {W * H * 80 / 1e6:.0f} MB = "
              f"{floor * 1e3:.1f} us at {HBM / 1e12:.2f} TB/s: {(m - prev) / floor:.1f} x the floor", flush=True)
        prev = m
    hit = (planes[0, ..., 3] >= 0).float().mean().item()
    print(f"pixels with a first hit: {hit:.4f}", flush=True)
ctx.close()

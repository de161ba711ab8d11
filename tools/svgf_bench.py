"""GPU box: what rt_svgf_filter_device costs beside rt_denoise_var_device on the headline frame -- cat scene, 1920x1080, b = 3, one sample, 3 passes.
In one process, alternating:
  denoise_var                  rt_denoise_var_device (the second instantiation of the pass kernel)
  svgf, both switches off      rt_svgf_filter_device: the third instantiation doing the same work -- what the two uniform branches and the wider argument cost
  svgf, pre-filter             + the 3 x 3 Gaussian of the variance: nine LDS reads and one quotient per pixel and pass
  svgf, feedback (pass f)      + the second history: pass f writes its colour there instead of the ping-pong frame (nothing added) and copies plane 1 (16 B read +
                               16 B written per pixel -- the traffic it cannot avoid); f = the last pass writes the colour twice
  svgf, both
  copy of plane 1              one device-to-device copy of a plane on the stream: the other way to move plane 1
Each figure is the median of RUNS windows of N calls on one stream between two HIP events (torch.cuda.Event), after a warm-up of every call.
usage: python tools/svgf_bench.py [> profiles/svgf/svgf_bench.txt]"""
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import numpy as np
import torch
import raytracinggpu_amd as rt

RUNS = int(os.environ.get("RUNS", "7"))
N = int(os.environ.get("N", "40"))
W, H, B, PASSES = 1920, 1080, 3, 3
HBM = 6.29e12                                                        # bytes / s DESIGN.md calls achievable

g = np.load(rt.scenes.CAT_FIXTURE, allow_pickle=False)
ctx = rt.Context(0)
ctx.scene_upload(rt.scenes.spheres("cpu"), dict(vertices=g["vertices"], indices=g["tri_bvh_order"], bvh_arr10=g["bvh_arr10"], albedo=rt.scenes.CAT_ALBEDO, object_slot=6))
st = torch.cuda.Stream()
rows = rt.interleaved_rows(H, 8, 0, 1)[0]
zeros = lambda *shape: torch.zeros(shape, dtype=torch.float32, device="cuda:0")
color, planes, out = zeros(H, W, 4), zeros(3, H, W, 4), zeros(H, W, 4)
hist, fed = [zeros(2, H, W, 4), zeros(2, H, W, 4)], zeros(2, H, W, 4)
rp = rt.make_reproject(motion=rt.static_motion())
torch.cuda.synchronize()


def params(seed):
    return rt.make_params(W, H, 1, B, **dict(rt.scenes.CPU_LAUNCHER, seed=seed))


def window(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    for _ in range(N):
        fn()
    b.record(st)
    b.synchronize()
    return a.elapsed_time(b) / N


print(f"{ctx.device_name}; cat scene {W}x{H}, one sample, {PASSES} passes; {rt._capi.DENOISE_VAR_DEFAULTS}", flush=True)
# a static sequence of six frames: hist[1] ends as a history of length 6
ctx.render_aov_device(params(1), planes.data_ptr(), stream=st.cuda_stream)
for f in range(6):
    ctx.render_device(params(1 + f), rows, color.data_ptr(), st.cuda_stream)
    ctx.temporal_accumulate_device(color.data_ptr(), planes.data_ptr(), 0 if f == 0 else planes.data_ptr(), 0 if f == 0 else hist[1 - f % 2].data_ptr(), W, H, hist[f % 2].data_ptr(),
                                   reproject=None if f == 0 else rp, stream=st.cuda_stream)
torch.cuda.synchronize()
H1 = hist[1].data_ptr()


def svgf(f, pre):
    sp = rt.make_svgf_params(n_passes=PASSES, feedback_pass=f, prefilter=pre)
    return lambda: ctx.svgf_filter_device(H1, planes.data_ptr(), W, H, out.data_ptr(), fed.data_ptr() if f >= 0 else None, params=sp, stream=st.cuda_stream)


def plane_copy():
    with torch.cuda.stream(st):
        fed[1].copy_(hist[1][1], non_blocking=True)


calls = [("denoise_var", lambda: ctx.denoise_var_device(H1, planes.data_ptr(), W, H, out.data_ptr(), n_passes=PASSES, stream=st.cuda_stream)),
         ("svgf, both switches off", svgf(-1, 0)), ("svgf, pre-filter", svgf(-1, 1)), ("svgf, feedback (pass 0)", svgf(0, 0)), ("svgf, feedback (pass 1)", svgf(1, 0)),
         (f"svgf, feedback (pass {PASSES - 1}, the last)", svgf(PASSES - 1, 0)), ("svgf, both (pass 0)", svgf(0, 1)), ("copy of plane 1 (device to device)", plane_copy)]
for _, fn in calls:
    for _ in range(5):
        fn()
torch.cuda.synchronize()
runs = {name: [] for name, _ in calls}
for _ in range(RUNS):                                                # alternating: one window of every call per round
    for name, fn in calls:
        runs[name].append(window(fn))
med = {name: statistics.median(r) for name, r in runs.items()}
for name, r in runs.items():
    print(f"{name}: {med[name] * 1e3:.1f} us per call (median of {RUNS} windows of {N} calls, min {min(r) * 1e3:.1f}, max {max(r) * 1e3:.1f})", flush=True)
base, off = med["denoise_var"], med["svgf, both switches off"]
floor = W * H * 32 / HBM * 1e3
print(f"both switches off: {off / base:.3f} x rt_denoise_var_device", flush=True)
print(f"pre-filter: +{(med['svgf, pre-filter'] - off) * 1e3:.1f} us = {(med['svgf, pre-filter'] - off) / PASSES * 1e3:.1f} us per pass, {med['svgf, pre-filter'] / off:.3f} x", flush=True)
for f in range(PASSES):
    name = [n for n in med if n.startswith(f"svgf, feedback (pass {f}")][0]
    print(f"feedback from pass {f}: +{(med[name] - off) * 1e3:.1f} us; plane 1's traffic (16 B read + 16 B written per pixel = {W * H * 32 / 1e6:.0f} MB) is {floor * 1e3:.1f} us at "
          f"{HBM / 1e12:.2f} TB/s; one pass is {off / PASSES * 1e3:.1f} us", flush=True)
print(f"the copy of plane 1 as a call of its own: {med['copy of plane 1 (device to device)'] * 1e3:.1f} us", flush=True)
ctx.close()

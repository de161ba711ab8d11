"""GPU box: what reprojecting a deforming mesh costs on the headline frame -- cat scene, 1920x1080.
  aov / aov_motion             rt_render_aov_device beside rt_render_aov_motion_device, without a snapshot (the rigid table) and with the cat snapshotted, interleaved
                               ROUNDS times; the added time against the added compulsory bytes: 32 B written per pixel, at most 112 B gathered per snapshot-mesh hit
  snapshot                     rt_mesh_snapshot_vertices per call on the cat and on a 524 288-triangle LBVH mesh, beside a plain device-to-device copy of the same bytes
  accumulate                   rt_temporal_accumulate_device fed the previous-frame planes (no table) beside the same call fed the current planes and the table: the
                               same kernel and the same bytes
Each figure is the median of RUNS windows of N calls on one stream between two HIP events (torch.cuda.Event), after a warm-up; the snapshot, which runs on the
context's own stream, is timed on the host around N calls and one rt_synchronize.
usage: python tools/motion_bench.py [> profiles/motion/motion_bench.txt]; BIG_N=0 skips the large mesh."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np
import torch
import raytracinggpu_amd as rt
from raytracinggpu_amd import hostlib

RUNS = int(os.environ.get("RUNS", "7"))
N = int(os.environ.get("N", "40"))
ROUNDS = int(os.environ.get("ROUNDS", "3"))
BIG_N = int(os.environ.get("BIG_N", "513"))
W, H = 1920, 1080
HBM = 6.29e12                                                        # bytes / s DESIGN.md calls achievable

g = np.load(rt.scenes.CAT_FIXTURE, allow_pickle=False)
cat = dict(vertices=g["vertices"], indices=g["tri_bvh_order"], bvh_arr10=g["bvh_arr10"], albedo=rt.scenes.CAT_ALBEDO, object_slot=6)
ctx = rt.Context(0)
ctx.scene_upload(rt.scenes.spheres("cpu"), cat)
st = torch.cuda.Stream()
rows = rt.interleaved_rows(H, 8, 0, 1)[0]
zeros = lambda *shape: torch.zeros(shape, dtype=torch.float32, device="cuda:0")
color, planes, prev, prev_planes = zeros(H, W, 4), zeros(3, H, W, 4), zeros(2, H, W, 4), zeros(3, H, W, 4)
hist = [zeros(2, H, W, 4), zeros(2, H, W, 4)]
table = rt.static_motion()
p = rt.make_params(W, H, 1, 3, **rt.scenes.CPU_LAUNCHER)
torch.cuda.synchronize()


def window(fn):
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


def host_timed(name, fn, sync):
    for _ in range(5):
        fn()
    sync()
    runs = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        for _ in range(N):
            fn()
        sync()
        runs.append((time.perf_counter() - t0) / N * 1e3)
    m = statistics.median(runs)
    print(f"{name}: {m * 1e3:.1f} us per call (host clock around {N} calls and one wait; median of {RUNS}, min {min(runs) * 1e3:.1f}, max {max(runs) * 1e3:.1f})", flush=True)
    return m


print(f"{ctx.device_name}; cat scene {W}x{H}", flush=True)
aov = lambda: ctx.render_aov_device(p, planes.data_ptr(), stream=st.cuda_stream)
motion = lambda: ctx.render_aov_motion_device(p, planes.data_ptr(), prev.data_ptr(), motion=table, stream=st.cuda_stream)
aov()
torch.cuda.synchronize()
on_cat = int((planes[0, ..., 3] == 6).sum().item())
print(f"pixels on the cat: {on_cat} of {W * H}", flush=True)
for r in range(ROUNDS):
    ctx.mesh_snapshot_vertices(keep=False)
    a = measure(f"round {r}: aov", aov)
    m = measure(f"round {r}: aov_motion, no snapshot (table)", motion)
    ctx.mesh_snapshot_vertices()
    s = measure(f"round {r}: aov_motion, cat snapshotted", motion)
    floor = W * H * 32 / HBM * 1e3
    print(f"    added: {(m - a) * 1e3:.1f} us without, {(s - a) * 1e3:.1f} us with the snapshot; 32 B per pixel = {W * H * 32 / 1e6:.0f} MB = {floor * 1e3:.1f} us at {HBM / 1e12:.2f} TB/s; "
          f"at most 112 B x {on_cat} hits = {on_cat * 112 / 1e6:.1f} MB gathered", flush=True)

# the accumulation: previous-frame planes without a table beside the planes with the table (a static scene: the same taps)
ctx.mesh_snapshot_vertices(keep=False)
ctx.render_device(p, rows, color.data_ptr(), st.cuda_stream)
motion()
ctx.render_aov_device(p, prev_planes.data_ptr(), stream=st.cuda_stream)
rp_table, rp_none = rt.make_reproject(motion=table), rt.make_reproject()
for f in range(6):
    ctx.temporal_accumulate_device(color.data_ptr(), planes.data_ptr(), 0 if f == 0 else prev_planes.data_ptr(), 0 if f == 0 else hist[1 - f % 2].data_ptr(), W, H,
                                   hist[f % 2].data_ptr(), reproject=None if f == 0 else rp_table, stream=st.cuda_stream)
torch.cuda.synchronize()
for r in range(ROUNDS):
    measure(f"round {r}: accumulate, current planes + table", lambda: ctx.temporal_accumulate_device(
        color.data_ptr(), planes.data_ptr(), prev_planes.data_ptr(), hist[1].data_ptr(), W, H, hist[0].data_ptr(), reproject=rp_table, stream=st.cuda_stream))
    measure(f"round {r}: accumulate, previous-frame planes, no table", lambda: ctx.temporal_accumulate_device(
        color.data_ptr(), prev.data_ptr(), prev_planes.data_ptr(), hist[1].data_ptr(), W, H, hist[0].data_ptr(), reproject=rp_none, stream=st.cuda_stream))


def snapshot_bench(name, n_vertices):
    src, dst = zeros(n_vertices, 4), zeros(n_vertices, 4)
    torch.cuda.synchronize()
    for r in range(ROUNDS):
        host_timed(f"round {r}: {name}: rt_mesh_snapshot_vertices ({n_vertices} vertices, {n_vertices * 16 / 1e3:.0f} kB)", ctx.mesh_snapshot_vertices, ctx.synchronize)
        host_timed(f"round {r}: {name}: a device-to-device copy of the same bytes", lambda: dst.copy_(src), torch.cuda.synchronize)


snapshot_bench("cat", len(cat["vertices"]))
if BIG_N > 1:
    n = BIG_N
    rng = np.random.default_rng(11)
    gx, gz = np.meshgrid(np.linspace(-18, 18, n), np.linspace(-14, 22, n), indexing="ij")
    gy = -9.0 + 3.0 * np.sin(gx * 0.45) * np.cos(gz * 0.38) + 0.15 * rng.standard_normal((n, n))
    v = np.stack([gx, gy, gz], -1).reshape(-1, 3).astype(np.float32)
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    a = (i * n + j).reshape(-1)
    t = np.concatenate([np.stack([a, a + 1, a + n], 1), np.stack([a + 1, a + n + 1, a + n], 1)]).astype(np.int32)
    ctx.scene_upload(rt.scenes.spheres("cpu"), hostlib.build_mesh(v, t, albedo=rt.scenes.CAT_ALBEDO, object_slot=6))
    ctx.mesh_rebuild(len(t), mode="lbvh")
    snapshot_bench(f"{len(t)} triangles (LBVH)", len(v))
    ctx.mesh_snapshot_vertices()
    measure("aov_motion on that mesh, snapshotted", motion)
    ctx.mesh_snapshot_vertices(keep=False)
    measure("aov on that mesh", aov)
ctx.close()

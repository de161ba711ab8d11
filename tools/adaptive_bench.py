"""GPU box: what adaptive sampling (rt_render_counts*, rt_sample_counts*, SvgfSequence(adaptive=...)) costs and what it buys.  DESIGN.md section 5.13 quotes this output.

Part 1, cost -- cat scene, 1920x1080, b = 3.  rt_render_counts_device waits on its stream once, so a call cannot be bracketed by two events without the wait inside;
every figure is host wall clock around `calls, then one synchronize` (median of RUNS windows of N calls), and the kernels' own times come from a rocprofv3 kernel trace
of this program (profiles/adaptive/kernel_stats.csv):
  dense frame                       rt_render_device, one sample: W x H items
  list, all ones                    rt_render_counts_device with a count of 1 everywhere: the same items as a list (plan + wait + chain + fold)
  list, zeros                       ... with a count of 0 everywhere: plan + wait + fold, no chain
  list, 5 % at 4 (band / scattered) ... with base: 5 % of the pixels trace samples 1 .. 3, as one vertical band / as scattered single pixels
  uniform 2, uniform 4              rt_render_device with num_rays = 2, 4
  sample_counts                     rt_sample_counts_device
  frame ...                         one whole SvgfSequence.frame: plain, adaptive in steady state, adaptive on a cut (every hit pixel newly revealed), uniform 2 / 4
Part 2, quality -- 640x360, b = 3, three sequences of eight frames (a new seed each): a yawing camera with a cut to another view at frame 4; a still camera with a cut at
frame 6; a still camera under a light that stands for four frames and then orbits (rt_scene_move_light).  RMSE of the filtered frame in the tonemap's [0, 1] scale against
a 256-sample frame of the frame's own scene, per frame, for the plain chain, the adaptive chain (rows of parameters) and uniform num_rays = 2 and 4.
usage: python tools/adaptive_bench.py [> profiles/adaptive/adaptive_bench.txt]     (QUALITY=0 / COST=0 skips a part)"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np
import torch
import raytracinggpu_amd as rt

RUNS = int(os.environ.get("RUNS", "7"))
N = int(os.environ.get("N", "10"))
W, H, B = 1920, 1080, 3

g = np.load(rt.scenes.CAT_FIXTURE, allow_pickle=False)
ctx = rt.Context(0)
CAT = dict(vertices=g["vertices"], indices=g["tri_bvh_order"], bvh_arr10=g["bvh_arr10"], albedo=rt.scenes.CAT_ALBEDO, object_slot=6)
ctx.scene_upload(rt.scenes.spheres("cpu"), CAT)
st = torch.cuda.Stream()
s = st.cuda_stream


def params(seed, w=W, h=H, spp=1):
    return rt.make_params(w, h, spp, B, **dict(rt.scenes.CPU_LAUNCHER, seed=seed))


def window(fn, n=N):
    st.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    st.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def cost():
    rows = rt.interleaved_rows(H, 8, 0, 1)[0]
    color, base = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0"), torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    hist = torch.rand((2, H, W, 4), dtype=torch.float32, device="cuda:0")
    dcounts = torch.zeros((H, W), dtype=torch.uint8, device="cuda:0")
    ctx.render_device(params(1), rows, base.data_ptr(), s)
    rng = np.random.default_rng(1)
    band = np.ones((H, W), np.uint8)
    band[:, W // 2: W // 2 + W // 20] = 4
    scattered = np.where(rng.random((H, W)) < 0.05, 4, 1).astype(np.uint8)
    pats = {k: torch.from_numpy(v).to("cuda:0") for k, v in dict(ones=np.ones((H, W), np.uint8), zeros=np.zeros((H, W), np.uint8), band=band, scattered=scattered).items()}
    torch.cuda.synchronize()
    seed = [10]

    def dense(spp):
        def fn():
            seed[0] += 1
            ctx.render_device(params(seed[0], spp=spp), rows, color.data_ptr(), s)
        return fn

    def listed(name, with_base):
        def fn():
            seed[0] += 1
            ctx.render_counts_device(params(seed[0]), pats[name].data_ptr(), color.data_ptr(), base_ptr=base.data_ptr() if with_base else None, stream=s)
        return fn
    calls = [("dense frame", dense(1)), ("list, all ones", listed("ones", False)), ("list, zeros", listed("zeros", False)), ("list, 5 % at 4 (band)", listed("band", True)),
             ("list, 5 % at 4 (scattered)", listed("scattered", True)), ("uniform 2", dense(2)), ("uniform 4", dense(4)),
             ("sample_counts", lambda: ctx.sample_counts_device(hist.data_ptr(), W, H, dcounts.data_ptr(), stream=s))]
    seqs = {"frame, plain": (rt.SvgfSequence(ctx, W, H, stream=s), 1, False), "frame, adaptive (steady)": (rt.SvgfSequence(ctx, W, H, stream=s, adaptive=rt.make_sample_count_params()), 1, False),
            "frame, adaptive (every frame a cut)": (rt.SvgfSequence(ctx, W, H, stream=s, adaptive=rt.make_sample_count_params()), 1, True),
            "frame, uniform 2": (rt.SvgfSequence(ctx, W, H, stream=s), 2, False), "frame, uniform 4": (rt.SvgfSequence(ctx, W, H, stream=s), 4, False)}

    def frame(seq, spp, cut):
        def fn():
            seed[0] += 1
            seq.frame(params(seed[0], spp=spp), cut=cut)
        return fn
    calls += [(name, frame(*v)) for name, v in seqs.items()]
    info = {}
    for name, fn in calls:
        for _ in range(3):
            fn()
        if name.startswith("list"):
            st.synchronize()
            info[name] = ctx.render_counts_info()
    runs = {name: [] for name, _ in calls}
    for _ in range(RUNS):                                              # alternating: one window of every call per round
        for name, fn in calls:
            runs[name].append(window(fn))
    med = {name: statistics.median(r) for name, r in runs.items()}
    print(f"{ctx.device_name}; cat scene {W}x{H}, b = {B}; host wall clock per call, median of {RUNS} windows of {N} calls", flush=True)
    for name, r in runs.items():
        extra = f"; {info[name]['items']} items, {info[name]['chains']} chain(s)" if name in info else ""
        print(f"{name}: {med[name] * 1e3:.1f} us (min {min(r) * 1e3:.1f}, max {max(r) * 1e3:.1f}){extra}", flush=True)
    px = W * H
    zero = med["list, zeros"]
    print(f"dense chain: {med['dense frame'] * 1e6 / px:.3f} ns per item; list chain (all ones, plan + wait + fold taken off): {(med['list, all ones'] - zero) * 1e6 / px:.3f} ns per item", flush=True)
    for k in ("band", "scattered"):
        name = f"list, 5 % at 4 ({k})"
        it = info[name]["items"]
        print(f"{name}: {(med[name] - zero) * 1e6 / it:.3f} ns per item over {it} items ({it / px:.3f} frames' worth of paths); whole call {med[name] / med['dense frame']:.3f} x a dense frame", flush=True)
    print(f"plan + read-back wait + fold (no chain): {zero * 1e3:.1f} us", flush=True)
    for k in ("adaptive (steady)", "adaptive (every frame a cut)", "uniform 2", "uniform 4"):
        print(f"frame, {k}: {med['frame, ' + k] / med['frame, plain']:.3f} x the plain frame ({med['frame, ' + k] * 1e3:.0f} vs {med['frame, plain'] * 1e3:.0f} us)", flush=True)
    for seq, _, _ in seqs.values():
        seq.close()


def tonemap(a):
    """min(pow(c, 1 / 2.2), 255) / 255: the tonemap's scale (cpu:714-716)"""
    return np.minimum(np.power(np.maximum(a[..., :3].astype(np.float64), 0.0), 1 / 2.2), 255.0) / 255.0


def quality():
    w, h, frames = 640, 360, 8
    views = [dict(position=(0.0, 2.0, 55.0), yaw=0.0, pitch=0.05), dict(position=(14.0, 4.0, 48.0), yaw=0.4, pitch=0.1)]

    def yawing(i):
        v = dict(views[0 if i < 4 else 1])
        v["yaw"] += 0.02 * (i % 4)
        return rt.make_pose(**v), i == 4, 0.0
    sequences = {"yawing camera, cut at 4": yawing, "still camera, cut at 6": lambda i: (rt.make_pose(**views[0 if i < 6 else 1]), i == 6, 0.0),
                 "still camera, light orbits from 4": lambda i: (rt.make_pose(**views[0]), False, 3.0 if i >= 4 else 0.0)}
    rows = {"plain": (None, 1), "uniform 2": (None, 2), "uniform 4": (None, 4)}
    for ns in (2, 4):
        for k in (0.0, 0.25, 1.0):
            rows[f"adaptive new {ns} k_rel {k:g}"] = (rt.make_sample_count_params(max_samples=4, short_history=2, new_surface_samples=ns, k_rel=k), 1)
    rows["adaptive new 4 short 4"] = (rt.make_sample_count_params(max_samples=4, short_history=4, new_surface_samples=4, k_rel=0.0), 1)
    print(f"quality: cat scene {w}x{h}, b = {B}, {frames} frames; RMSE in the tonemap's [0, 1] scale against 256 samples; samples = traced per pixel and frame, mean over the sequence", flush=True)
    for sname, step in sequences.items():
        refs = []
        ctx.scene_upload(rt.scenes.spheres("cpu"), CAT)
        for i in range(frames):
            pose, _, speed = step(i)
            if speed:
                ctx.move_light(speed)
            refs.append(tonemap(ctx.render_pose(params(7000 + i, w, h, 256), pose)))
        for rname, (ad, spp) in rows.items():
            ctx.scene_upload(rt.scenes.spheres("cpu"), CAT)
            errs, traced = [], []
            with rt.SvgfSequence(ctx, w, h, adaptive=ad) as seq:
                for i in range(frames):
                    pose, cut, speed = step(i)
                    if speed:
                        ctx.move_light(speed)
                    out = seq.frame(params(100 + i, w, h, spp), pose=pose, cut=cut)
                    ctx.synchronize()
                    errs.append(float(np.sqrt(np.mean((tonemap(ctx.device_to_host(out, (h, w, 4))) - refs[i]) ** 2))))
                    traced.append(spp if ad is None else 1 + ctx.render_counts_info()["items"] / (w * h))
            print(f"{sname:34s} {rname:28s} samples {np.mean(traced):.3f}  last {errs[-1]:.5f}  mean {np.mean(errs):.5f}  per frame " + " ".join(f"{e:.5f}" for e in errs), flush=True)


if os.environ.get("COST", "1") != "0":
    cost()
if os.environ.get("QUALITY", "1") != "0":
    quality()
ctx.close()

"""GPU box: what the planes of the first diffuse surface and the demodulate / modulate pair cost at 1920x1080, and what they buy.
  planes      rt_render_aov_surface_device at max_specular 0, 4 and 8 beside rt_render_aov_device of the same run, on the config-1 sphere scene (demo10: a glass
              sphere, a mirror, a nested glass pair) and on the glass cat: max_specular + 1 rounds of (wf_travq, step kernel) whatever the scene
  elementwise rt_demodulate_device / rt_modulate_device beside their compulsory 48 B per pixel (colour and plane 2 read, colour written)
  quality     the measure of DESIGN.md section 5.7 -- RMSE in the tonemap's [0, 1] scale of a one-sample b = 3 frame against a many-sample one -- for the first-hit
              pipeline (rt_render_aov -> rt_denoise, default weights) and the surface + irradiance pipeline (rt_render_aov_surface -> rt_demodulate -> rt_denoise
              with k_albedo = 0 -> rt_modulate), over the whole frame and over the pixels whose first hit is specular (demo10) or textured (the cat), seeds 1 to 5;
              three more columns take the result apart: the surface planes alone, and either pipeline with a colour tolerance scaled to irradiance
Each time is the median of RUNS windows of N calls on one stream between two HIP events (torch.cuda.Event), after a warm-up of every call.
usage: python tools/surface_bench.py [> profiles/surface/surface_bench.txt]; ONLY=planes|elementwise|quality narrows the run; REF_SPP sets the reference's samples."""
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
REF_SPP = int(os.environ.get("REF_SPP", "1024"))
W, H, B = 1920, 1080, 3
HBM = 6.29e12                                                        # bytes / s DESIGN.md calls achievable
MAX_SPECULAR = 8
FLOOR = 1e-3
KC_DIV = 16.0

g = np.load(rt.scenes.CAT_FIXTURE, allow_pickle=False)
ctx = rt.Context(0)
st = torch.cuda.Stream()
p = rt.make_params(W, H, 1, B, **rt.scenes.CPU_LAUNCHER)
color = torch.rand((H, W, 4), dtype=torch.float32, device="cuda:0")
planes = torch.zeros((3, H, W, 4), dtype=torch.float32, device="cuda:0")
out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
torch.cuda.synchronize()


def cat(albedo=rt.scenes.CAT_ALBEDO, **material):
    d = dict(vertices=g["vertices"], indices=g["tri_bvh_order"], bvh_arr10=g["bvh_arr10"], albedo=albedo, object_slot=6)
    d.update(material)
    return d


def upload(name):
    if name == "demo10":
        ctx.scene_upload(rt.scenes.spheres("demo10"))
    elif name == "glass cat":
        ctx.scene_upload(rt.scenes.spheres("cpu"), cat(in_refraction_index=1.5, out_refraction_index=1.0))
    else:                                                            # the textured cat: blocks of random colour, bilinear, repeated 2.6 times across the mesh
        ctx.scene_upload(rt.scenes.spheres("cpu"), cat(albedo=(0.75, 0.5, 0.3)))
        v, tv = np.asarray(g["vertices"]), np.asarray(g["tri_bvh_order"])[:, :3]
        lo, hi = v.min(0), v.max(0)
        uvs = (((v[:, :2] - lo[:2]) / (hi[:2] - lo[:2])) * np.float32(2.6) - np.float32(0.8)).astype(np.float32)
        ctx.mesh_set_texture(uvs, tv, np.random.default_rng(5).integers(0, 256, size=(23, 37, 3), dtype=np.uint8), filter="bilinear", wrap="repeat")


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


def gamma_unit(c):
    with np.errstate(invalid="ignore"):
        return np.minimum(np.power(np.asarray(c, np.float64), 1 / 2.2), 255.0) / 255.0


def rmse(a, b, mask=None):
    d = (gamma_unit(a[..., :3]) - gamma_unit(b[..., :3])) ** 2
    return float(np.sqrt(np.mean(d if mask is None else d[mask])))


print(f"{ctx.device_name}; {W}x{H}; weights {rt._capi.DENOISE_DEFAULTS}", flush=True)
if ONLY in ("", "planes"):
    for scene in ("demo10", "glass cat"):
        upload(scene)
        print(f"-- planes, {scene}", flush=True)
        base = measure("rt_render_aov_device", lambda: ctx.render_aov_device(p, planes.data_ptr(), stream=st.cuda_stream))
        for m in (0, 4, 8):
            t = measure(f"rt_render_aov_surface_device max_specular={m}", lambda: ctx.render_aov_surface_device(p, m, planes.data_ptr(), stream=st.cuda_stream))
            print(f"    {t / base:.2f} x rt_render_aov_device", flush=True)
        torch.cuda.synchronize()
        code = planes[0, ..., 3]
        k = torch.where(code >= 0, torch.floor(code / 256), torch.zeros_like(code))
        print(f"    at max_specular 8: pixels behind a chain {(k >= 1).float().mean().item():.4f}, longest chain {int(k.max().item())}, "
              f"exhausted {((planes[2, ..., 3] == 0) & (code >= 0)).float().mean().item():.5f}, misses {(code < 0).float().mean().item():.5f}", flush=True)
if ONLY in ("", "elementwise"):
    upload("demo10")
    ctx.render_aov_surface_device(p, MAX_SPECULAR, planes.data_ptr(), stream=st.cuda_stream)
    torch.cuda.synchronize()
    floor = W * H * 48 / HBM * 1e3
    print(f"-- demodulate / modulate, demo10 planes; compulsory traffic {W * H * 48 / 1e6:.0f} MB = {floor * 1e3:.1f} us at {HBM / 1e12:.2f} TB/s", flush=True)
    for name, fn in (("rt_demodulate_device", ctx.demodulate_device), ("rt_modulate_device", ctx.modulate_device)):
        t = measure(name, lambda: fn(color.data_ptr(), planes.data_ptr(), W * H, out.data_ptr(), albedo_floor=FLOOR, stream=st.cuda_stream))
        print(f"    {t / floor:.2f} x the floor", flush=True)
    t = measure("rt_demodulate_device in place", lambda: ctx.demodulate_device(out.data_ptr(), planes.data_ptr(), W * H, out.data_ptr(), albedo_floor=FLOOR, stream=st.cuda_stream))
    t3 = measure("rt_denoise_device, 3 passes, k_albedo=0", lambda: ctx.denoise_device(color.data_ptr(), planes.data_ptr(), W, H, out.data_ptr(), k_albedo=0.0, stream=st.cuda_stream))
    print(f"    one filter pass is {t3 / 3 * 1e3:.1f} us", flush=True)
if ONLY in ("", "quality"):
    for scene, what in (("demo10", "first hit specular"), ("textured cat", "first hit textured")):
        upload(scene)
        ref = ctx.render(rt.make_params(W, H, REF_SPP, B, seed=99, **rt.scenes.CPU_LAUNCHER))
        first = ctx.render_aov(p)
        surf = ctx.render_aov_surface(p, MAX_SPECULAR)
        mask = np.isin(first[0, ..., 3], [0, 1, 2, 3]) if scene == "demo10" else first[0, ..., 3] == 6
        print(f"-- quality, {scene}, b = {B}, one sample against {REF_SPP}; '{what}' is {mask.mean():.4f} of the frame; albedo_floor {FLOOR}", flush=True)
        print("   each pair: whole frame, masked.  A = first-hit pipeline; B = surface + irradiance pipeline; C = surface planes guiding the filter over the COLOUR (default", flush=True)
        print(f"   k_albedo, nothing divided out); D = B with k_color / {KC_DIV:g} (the colour term weighs absolute differences, and irradiance is colour / albedo); E = A with that k_color", flush=True)
        print("   seed | noisy | A | B | C | D | E", flush=True)
        kc = rt._capi.DENOISE_DEFAULTS["k_color"] / KC_DIV
        for seed in range(1, 6):
            noisy = ctx.render(rt.make_params(W, H, 1, B, seed=seed, **rt.scenes.CPU_LAUNCHER))
            irr = ctx.demodulate(noisy, surf, FLOOR)
            a = ctx.denoise(noisy, first)
            b = ctx.modulate(ctx.denoise(irr, surf, k_albedo=0.0), surf, FLOOR)
            c = ctx.denoise(noisy, surf)
            d = ctx.modulate(ctx.denoise(irr, surf, k_albedo=0.0, k_color=kc), surf, FLOOR)
            e = ctx.denoise(noisy, first, k_color=kc)
            print(f"   {seed} | " + " | ".join(f"{rmse(x, ref):.5f} {rmse(x, ref, mask):.5f}" for x in (noisy, a, b, c, d, e)), flush=True)
ctx.close()

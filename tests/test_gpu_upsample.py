"""rt_upsample[_device] and SvgfSequence(upsample=...) on the device against the numpy model of tests/upsample_model.py: every channel of every pixel, as uint32.  -m gpu.

tests/test_upsample_model.py proves on the CPU that the synthetic pairs used here reach every branch (1 .. 4 counted taps, taps dropped for each single reason, the
fallback, both sides of rt_div.h's range) and that the listed faults would change their bits.  Here: every case of tests/upsample_fixtures.py with one and two planes;
a rendered pair of the cat through the device entry on a second stream, and the host form; pipeline A with rt_demodulate / rt_modulate on a textured mesh against the
models' composition; SvgfSequence(upsample=2) in both filter_at modes against the same chain issued call by call, and upsample=1 against today's sequence; every
refusal; planted NaN and Inf.  (The pipelining note is in tests/test_gpu_upsample_between.py.)"""
import ctypes as C

import numpy as np
import pytest

import raytracinggpu_amd as rt
from raytracinggpu_amd import _capi
from . import denoise_model as dm
from . import surface_model as surf_model
from . import upsample_fixtures as uf
from . import upsample_model as um

pytestmark = pytest.mark.gpu

KN, KP = (float(np.float32(_capi.UPSAMPLE_DEFAULTS[n])) for n in ("k_normal", "k_position"))


@pytest.fixture(scope="module")
def ctx():
    c_ = rt.Context(0)
    yield c_
    c_.close()


def _same(got, exp, msg, finite=True):
    got, exp = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(exp, np.float32)
    assert got.shape == exp.shape                                      # no pixel is left out of the comparison
    nan = np.isnan(exp)
    assert not (finite and nan.any()), msg
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=msg + ": NaN in other places than the model's")
    np.testing.assert_array_equal(np.where(nan, 0, got.view(np.uint32)), np.where(nan, 0, exp.view(np.uint32)), err_msg=msg)


def _cat(cat_golden, **kw):
    return dict(dict(vertices=cat_golden["vertices"], indices=cat_golden["tri_bvh_order"], bvh_arr10=cat_golden["bvh_arr10"], albedo=rt.scenes.CAT_ALBEDO, object_slot=6), **kw)


# ---------------------------------------------------------------- the synthetic pairs ----------------------------------------------------------------
@pytest.mark.parametrize("n_planes", [1, 2])
@pytest.mark.parametrize("name", sorted(uf.CASES))
def test_synthetic_pairs_equal_the_model(ctx, name, n_planes):
    """2 x 2 and 4 x 4 from one low-resolution pixel; 66 x 18 from 33 x 9 crosses the seams of the 32 x 8 tile and is no multiple of it; 140 x 40 at f = 2 and 4 (the
    case the CPU minimums are asserted on), 99 x 27 at f = 3 (fractions of 0, 1/3 and 2/3: a tap of weight 0 inside the fallback)."""
    p = uf.case(name)
    low = p["low"] if n_planes == 2 else p["low"][0]
    got = ctx.upsample(low, p["low_aov"], p["aov"], p["factor"])
    _same(got, um.upsample(low, p["low_aov"], p["aov"], p["factor"], KN, KP), f"{name}, {n_planes} plane(s)")
    if name == uf.MAIN:                                                # other weights, and each term switched off (a k of exactly 0)
        for kn, kp in ((0.0, KP), (KN, 0.0), (0.0, 0.0), (7.5, 30.0)):
            _same(ctx.upsample(low, p["low_aov"], p["aov"], p["factor"], k_normal=kn, k_position=kp), um.upsample(low, p["low_aov"], p["aov"], p["factor"], kn, kp),
                  f"{name}, k_normal {kn}, k_position {kp}")


# ---------------------------------------------------------------- a rendered pair ----------------------------------------------------------------
RW = RH = 128
POSES = [dict(), dict(position=(1.5, 0.5, 54.0), yaw=0.04), dict(position=(3.0, 1.0, 53.0), yaw=0.08, pitch=0.28), dict(position=(4.5, 1.0, 52.5), yaw=0.12, pitch=0.28)]


def _params(w, h, i=0):
    return rt.make_params(w, h, 1, 3, **dict(rt.scenes.CPU_LAUNCHER, seed=500 + i))


def test_a_rendered_pair_on_a_second_stream_and_the_host_form(ctx, cat_golden):
    import torch
    ctx.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden))
    st = torch.cuda.Stream()
    s = st.cuda_stream
    w, h = RW // 2, RH // 2
    buf = lambda n, hh, ww: torch.full((n, hh, ww, 4), -7.0, dtype=torch.float32, device="cuda:0")
    color, low_planes, planes, out = buf(1, h, w), buf(3, h, w), buf(3, RH, RW), buf(1, RH, RW)
    torch.cuda.synchronize()
    ctx.render_device(_params(w, h), rt.interleaved_rows(h, 8, 0, 1)[0], color.data_ptr(), s)
    ctx.render_aov_device(_params(w, h), low_planes.data_ptr(), stream=s)
    ctx.render_aov_device(_params(RW, RH), planes.data_ptr(), stream=s)
    ctx.upsample_device(color.data_ptr(), low_planes.data_ptr(), planes.data_ptr(), RW, RH, 2, out.data_ptr(), stream=s)
    torch.cuda.synchronize()
    c, la, a = color.cpu().numpy()[0], low_planes.cpu().numpy(), planes.cpu().numpy()
    st_ = {}
    exp = um.upsample(c, la, a, 2, KN, KP, stats=st_)
    assert np.isfinite(exp).all()
    _same(out.cpu().numpy()[0], exp, "rt_upsample_device on rendered planes")
    _same(ctx.upsample(c, la, a, 2), exp, "the host form")
    _same(ctx.render_aov(_params(w, h)), la, "the low-resolution planes")
    fb = st_["fallback"].mean()
    print(f"rendered cat 128 x 128 from 64 x 64: {100 * fb:.2f} % fallback pixels, counted taps {np.bincount(st_['counted'].ravel(), minlength=5)}")
    assert 0 < fb <= 0.02
    assert (exp.view(np.uint32) != um.bilinear(c, la, a, 2).view(np.uint32)).any()


def test_pipeline_a_with_demodulated_irradiance_on_a_textured_mesh(ctx, cat_golden):
    """surface planes at both resolutions -> rt_demodulate at the low one -> rt_denoise -> rt_upsample -> rt_modulate at the full one: every stage's model composed."""
    ctx.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden, albedo=(0.75, 0.5, 0.3)))
    rng = np.random.default_rng(5)
    v, tv = np.asarray(cat_golden["vertices"]), np.asarray(cat_golden["tri_bvh_order"])[:, :3]
    lo, hi = v.min(0), v.max(0)
    uvs = (((v[:, :2] - lo[:2]) / (hi[:2] - lo[:2])) * np.float32(2.6) - np.float32(0.8)).astype(np.float32)
    ctx.mesh_set_texture(uvs, tv, rng.integers(0, 256, size=(23, 37, 3), dtype=np.uint8), filter="bilinear", wrap="repeat")
    try:
        W, H, f, floor = 120, 96, 2, 1e-3
        pl, pf = _params(W // f, H // f), _params(W, H)
        color = ctx.render(pl)
        low_surf, surf = ctx.render_aov_surface(pl, 2), ctx.render_aov_surface(pf, 2)
        irr = ctx.demodulate(color, low_surf, floor)
        filtered = ctx.denoise(irr, low_surf, k_albedo=0.0)
        out = ctx.modulate(ctx.upsample(filtered, low_surf, surf, f), surf, floor)
        dp = rt.make_denoise_params(k_albedo=0.0)
        e = dm.denoise(surf_model.demodulate(color, low_surf, floor), low_surf, dp.n_passes, dp.k_normal, dp.k_position, 0.0, dp.k_color)
        exp = surf_model.modulate(um.upsample(e, low_surf, surf, f, KN, KP), surf, floor)
        _same(out, exp, "demodulate -> denoise -> upsample -> modulate")
        # the texture comes back at full resolution: on the cat the result is not what upsampling the low-resolution MODULATED frame gives
        cat = (surf[0, ..., 3] == 6) & (surf[2, ..., 3] == 1)
        blurred = um.upsample(surf_model.modulate(e, low_surf, floor), low_surf, surf, f, KN, KP)
        assert cat.sum() > 500 and (out[cat][:, :3] != blurred[cat][:, :3]).any(-1).mean() > 0.5
    finally:
        ctx.mesh_set_texture(None, None, None)


# ---------------------------------------------------------------- SvgfSequence ----------------------------------------------------------------
def _explicit_chain(ctx, f, filter_at, svgf, n_frames=4):
    """The chain of SvgfSequence(upsample=f, filter_at=...) issued call by call through the host forms -> every frame's full-resolution output"""
    w, h = RW // f, RH // f
    outs, prev = [], None
    for i in range(n_frames):
        pose = rt.make_pose(**POSES[i])
        pl, pf = _params(w, h, i), _params(RW, RH, i)
        color, aov = ctx.render_pose(pl, pose), ctx.render_aov(pl, pose=pose)
        if prev is None:
            acc = ctx.temporal_accumulate(color, aov)
        else:
            acc = ctx.temporal_accumulate(color, aov, prev[0], prev[1], reproject=rt.make_reproject(pose=rt.make_pose(**POSES[i - 1])))
        if f == 1:
            out, fed = ctx.svgf_filter(acc, aov, params=svgf)
        else:
            full = ctx.render_aov(pf, pose=pose)
            if filter_at == "low":
                low_out, fed = ctx.svgf_filter(acc, aov, params=svgf)
                out = ctx.upsample(low_out, aov, full, f)
            else:
                out, fed = ctx.svgf_filter(ctx.upsample(acc, aov, full, f), full, params=svgf)
                assert fed is None
        prev = (aov, acc if fed is None else fed)
        outs.append(out)
    return outs


def _sequence(ctx, n_frames=4, **kw):
    with rt.SvgfSequence(ctx, RW, RH, **kw) as seq:
        outs = []
        for i in range(n_frames):
            ptr = seq.frame(_params(RW, RH, i), pose=rt.make_pose(**POSES[i]))
            ctx.synchronize()
            outs.append(ctx.device_to_host(ptr, (RH, RW, 4)))
        n_buffers = len(seq._ptrs)
    assert seq._ptrs == []
    return outs, n_buffers


@pytest.mark.parametrize("filter_at,feedback", [("low", -1), ("low", 0), ("full", -1)])
def test_sequence_with_upsample_equals_the_chain_call_by_call(ctx, cat_golden, filter_at, feedback):
    ctx.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden))
    svgf = rt.make_svgf_params(feedback_pass=feedback)
    exp = _explicit_chain(ctx, 2, filter_at, svgf)
    got, n_buffers = _sequence(ctx, svgf=svgf, upsample=2, filter_at=filter_at)
    assert n_buffers == 8
    for i, (g, e) in enumerate(zip(got, exp)):
        assert np.isfinite(e).all()
        _same(g, e, f"SvgfSequence(upsample=2, filter_at={filter_at!r}), feedback_pass {feedback}, frame {i}")
    assert (got[3].view(np.uint32) != got[0].view(np.uint32)).any()


def test_upsample_1_is_todays_sequence(ctx, cat_golden):
    ctx.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden))
    svgf = rt.make_svgf_params(feedback_pass=0)
    today = _explicit_chain(ctx, 1, "low", svgf, n_frames=3)
    plain, n_plain = _sequence(ctx, n_frames=3, svgf=svgf)
    for filter_at in ("low", "full"):                                  # (with upsample=1 filter_at says nothing)
        got, n_buffers = _sequence(ctx, n_frames=3, svgf=svgf, upsample=1, filter_at=filter_at)
        assert n_buffers == n_plain == 6
        for i in range(3):
            _same(got[i], today[i], f"upsample=1, frame {i}")
            _same(got[i], plain[i], f"upsample=1 against the sequence without the keyword, frame {i}")
    with pytest.raises(rt.RtError):
        rt.SvgfSequence(ctx, RW + 1, RH, upsample=2)
    with rt.SvgfSequence(ctx, RW, RH, upsample=2) as seq:
        with pytest.raises(rt.RtError):                                # frame() takes the FULL-resolution parameters
            seq.frame(_params(RW // 2, RH // 2))


# ---------------------------------------------------------------- refusals ----------------------------------------------------------------
def test_refusals_leave_the_output_untouched(ctx):
    import torch
    p = uf.case("66x18")
    W, H, f = uf.CASES["66x18"]
    full, low = W * H * 16, W * H * 16 // (f * f)
    dl, dla, da = (torch.from_numpy(p[k]).to("cuda:0") for k in ("low", "low_aov", "aov"))
    out = torch.full((2, H, W, 4), -7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    ok = dict(low_ptr=dl.data_ptr(), low_aov_ptr=dla.data_ptr(), aov_ptr=da.data_ptr(), width=W, height=H, factor=f, out_ptr=out.data_ptr(), n_planes=2)
    ctx.upsample_device(**ok)                                          # the call these are variations of is accepted
    ctx.synchronize()
    _same(out.cpu().numpy(), um.upsample(p["low"], p["low_aov"], p["aov"], f, KN, KP), "the accepted call")
    out.fill_(-7.0)
    torch.cuda.synchronize()
    refused = [dict(low_ptr=0), dict(low_aov_ptr=0), dict(aov_ptr=0), dict(out_ptr=0),
               dict(factor=1), dict(factor=5), dict(factor=0), dict(factor=-2), dict(n_planes=0), dict(n_planes=3),
               dict(width=0), dict(height=-2), dict(width=W + 1), dict(height=H - 1), dict(factor=4), dict(factor=3, width=W, height=H + 1),   # 66 = 3 * 22 but 19 is no multiple
               dict(width=2 ** 14, height=2 ** 14),                    # 2^28 pixels
               dict(out_ptr=dl.data_ptr()), dict(out_ptr=dl.data_ptr() + 2 * low - 16), dict(out_ptr=dla.data_ptr() + 3 * low - 16),        # over an input's last bytes
               dict(out_ptr=da.data_ptr() + 3 * full - 16), dict(out_ptr=da.data_ptr() + 2 * full + 32),                                     # (plane 2, which is not read, counts)
               dict(low_ptr=out.data_ptr() + 2 * full - 16), dict(aov_ptr=out.data_ptr() + full)]
    for kw in refused:
        with pytest.raises(rt.RtError) as e:
            ctx.upsample_device(**dict(ok, **kw))
        assert e.value.code == -1, kw
    L = _capi.load()                                                   # NULL parameters: below the Python layer, which always builds them
    vp = lambda t: t.data_ptr()
    assert L.rt_upsample_device(ctx._h, vp(dl), vp(dla), vp(da), W, H, None, vp(out), None) == -1
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all()
    for t, k in ((dl, "low"), (dla, "low_aov"), (da, "aov")):
        _same(t.cpu().numpy(), p[k], "an input")
    # the host form
    ho = np.full((2, H, W, 4), -7, np.float32)
    fp = C.POINTER(C.c_float)
    ptr = lambda a: a.ctypes.data_as(fp)
    for up in (rt.make_upsample_params(5, 2), rt.make_upsample_params(2, 3), rt.make_upsample_params(4, 2)):
        assert L.rt_upsample(ctx._h, ptr(p["low"]), ptr(p["low_aov"]), ptr(p["aov"]), W, H, C.byref(up), ptr(ho)) == -1
    up = rt.make_upsample_params(f, 2)
    assert L.rt_upsample(ctx._h, ptr(p["low"]), ptr(p["low_aov"]), ptr(p["aov"]), W, H, C.byref(up), ptr(p["aov"])) == -1   # the planes as the output
    assert L.rt_upsample(ctx._h, ptr(p["low"]), ptr(p["low_aov"]), None, W, H, C.byref(up), ptr(ho)) == -1
    assert (ho == -7).all()
    _same(ctx.upsample(p["low"], p["low_aov"], p["aov"], f, out=ho), um.upsample(p["low"], p["low_aov"], p["aov"], f, KN, KP), "and the context still works")


# ---------------------------------------------------------------- non-finite values ----------------------------------------------------------------
def _footprint(W, H, f, qx, qy):
    """the full-resolution pixels one of whose four taps is the low-resolution pixel (qx, qy)"""
    ix, _ = um.coords(W, f)
    iy, _ = um.coords(H, f)
    return ((iy[:, None] == qy) | (iy[:, None] + 1 == qy)) & ((ix[None, :] == qx) | (ix[None, :] + 1 == qx))


def test_planted_nan_and_inf_change_their_footprint_and_nothing_else(ctx):
    p = uf.case(uf.MAIN)
    W, H, f = uf.CASES[uf.MAIN]
    clean_stats = {}
    clean = um.upsample(p["low"], p["low_aov"], p["aov"], f, KN, KP, stats=clean_stats)
    low, low_aov, aov = p["low"].copy(), p["low_aov"].copy(), p["aov"].copy()
    NAN, INF = np.float32(np.nan), np.float32(np.inf)
    # low-resolution guides: a normal, a position, an id; low-resolution values: NaN and Inf; full-resolution guides: a normal and a position
    low_guides = {(10, 5): (0, 1, NAN), (30, 12): (1, 0, NAN), (50, 7): (0, 3, NAN), (60, 15): (1, 2, INF)}
    low_values = {(20, 3): (0, 1, NAN), (40, 16): (1, 2, INF), (64, 4): (0, 0, -INF)}
    full_guides = {(25, 30): (0, 0, NAN), (90, 9): (1, 1, NAN), (120, 33): (0, 3, NAN)}
    for (x, y), (plane, c, v) in low_guides.items():
        assert p["low_ids"][y, x] != -1
        low_aov[plane, y, x, c] = v
    for (x, y), (plane, c, v) in low_values.items():
        low[plane, y, x, c] = v
    for (x, y), (plane, c, v) in full_guides.items():
        assert p["ids"][y, x] != -1 and clean_stats["counted"][y, x] > 0
        aov[plane, y, x, c] = v
    st = {}
    exp = um.upsample(low, low_aov, aov, f, KN, KP, stats=st)
    got = ctx.upsample(low, low_aov, aov, f)
    _same(got, exp, "planted NaN and Inf", finite=False)
    assert 0 < np.isnan(exp).sum() < 0.02 * exp.size
    changed = ((got.view(np.uint32) != clean.view(np.uint32)) & ~(np.isnan(got) & np.isnan(clean))).any(axis=(0, 3))
    allowed = np.zeros((H, W), bool)
    for (x, y) in list(low_guides) + list(low_values):
        allowed |= _footprint(W, H, f, x, y)
    for (x, y) in full_guides:
        allowed[y, x] = True
    assert changed.sum() >= len(low_guides) + len(low_values) + len(full_guides) and not (changed & ~allowed).any()
    for (x, y) in full_guides:                                         # a pixel whose own guide is NaN counts no tap: plain bilinear, finite
        assert st["fallback"][y, x] and st["counted"][y, x] == 0 and changed[y, x]
        assert np.isfinite(got[:, y, x]).all()
        _same(got[:, y, x], um.bilinear(low, low_aov, aov, f)[:, y, x], "a NaN-guided pixel takes the fallback")
    for (x, y) in low_guides:                                          # a tap with a NaN guide weighs nothing: no NaN comes out of its footprint
        assert np.isfinite(got[:, _footprint(W, H, f, x, y)]).all()

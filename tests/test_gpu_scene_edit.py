"""Animated scenes on the device: the light and the spheres of the uploaded scene edited in place (rt_scene_set_* / rt_scene_move_*), and per frame of a batch
(rt_render_device_batch_scenes).  -m gpu.

Every comparison is on uint32 views, no tolerance: an edited scene renders what rt_scene_upload* of the same meshes with the edited light and spheres renders, and frame k of an
animated batch is the lone frame of frame k's scene.  Two contexts: `ctx` is edited, `ref` is uploaded afresh."""
import numpy as np
import pytest

import raytracinggpu_amd as rt

pytestmark = pytest.mark.gpu

ALL_VARIANTS = ["auto", "global", "lds_verts", "lds_top", "lds_all", "lockstep", "wavefront", "wavefront_lds", "wavefront_queue", "path"]
SLOT = 6                                                              # the cat in the `cpu` preset
LIGHT = rt.scenes.LIGHT
W, H = 333, 77                                                        # partial 8 x 8 tiles in both directions


@pytest.fixture(scope="module")
def ctx():
    c_ = rt.Context(0)
    yield c_
    c_.close()


@pytest.fixture(scope="module")
def ref():
    c_ = rt.Context(0)
    yield c_
    c_.close()


def _bits_equal(a, b, msg=""):
    np.testing.assert_array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32), err_msg=msg)


def _differ(a, b):
    """pixels whose colour differs"""
    return int((np.ascontiguousarray(a[..., :3], np.float32).view(np.uint32) != np.ascontiguousarray(b[..., :3], np.float32).view(np.uint32)).any(-1).sum())


def _cat(cat_golden):
    return dict(vertices=cat_golden["vertices"], indices=cat_golden["tri_bvh_order"], bvh_arr10=cat_golden["bvh_arr10"], albedo=rt.scenes.CAT_ALBEDO, object_slot=SLOT)


def _full(s):
    """a sphere of rt.scenes as the six-field tuple"""
    return (tuple(float(x) for x in s[0]), float(s[1]), tuple(float(x) for x in s[2]), int(s[3]) if len(s) > 3 else 0, float(s[4]) if len(s) > 4 else 1.0,
            float(s[5]) if len(s) > 5 else 1.0)


def _params(b, spp=1, variant="auto", w=W, h=H, **kw):
    d = dict(rt.scenes.CPU_LAUNCHER)
    d.update(kw)
    return rt.make_params(w, h, spp, b, variant=variant, **d)


# ---- the edits of test 1 (and what the other tests start from) -----------------------------------------------------------------------------------------------------------
# cat scene: six wall spheres and the cat.  The light moves and dims; the floor (slot 1) and the back wall (slot 0) get a new centre and radius; the right wall (slot 4) turns mirror
CAT_LIGHT = ((15.0, 25.0, 30.0), 2e10)


def cat_edits():
    s = [_full(x) for x in rt.scenes.spheres("cpu")]
    return {1: ((0.0, -1002.0, 0.0), 991.5) + s[1][2:], 0: ((3.0, 0.0, -1010.0), 945.0) + s[0][2:], 4: s[4][:3] + (1,) + s[4][4:]}


# demo10: glass sphere at the origin (slot 0), mirror sphere (slot 1), a hollow glass sphere (slots 2, 3), six walls (slots 4..9).  Three stages: the glass sphere and the
# mirror sphere move, the glass sphere shrinks, the mirror sphere turns diffuse; then it is a mirror again, bigger; then glass
DEMO_LIGHT = ((5.0, 30.0, 35.0), 4e10)


def demo_stages():
    s = [_full(x) for x in rt.scenes.spheres("demo10")]
    moved = ((-22.0, 2.0, -5.0),)
    return [{0: ((2.0, 3.0, 5.0), 8.0) + s[0][2:], 1: moved + (10.0, (0.8, 0.3, 0.3), 0, 1.0, 1.0)},
            {1: moved + (11.5, (0.0, 0.0, 0.0), 1, 1.0, 1.0)},
            {1: moved + (11.5, (0.0, 0.0, 0.0), 0, 1.5, 1.0)}]


def _apply(spheres, edits):
    out = [_full(x) for x in spheres]
    for slot, s in edits.items():
        out[slot] = s
    return out


def _frames(c, variants, bs=(0, 3)):
    """every variant x b: the frame, or the refusal's code"""
    out = {}
    for v in variants:
        for b in bs:
            try:
                out[(v, b)] = c.render(_params(b, variant=v))
            except rt.RtError as e:
                out[(v, b)] = e.code
    return out


def _same_frames(got, exp, what):
    assert got.keys() == exp.keys()
    n = 0
    for k in got:
        if isinstance(exp[k], int):
            assert got[k] == exp[k], (what, k)
        else:
            _bits_equal(got[k], exp[k], f"{what} {k}")
            n += 1
    return n


def test_edit_equals_upload_cat(ctx, ref, oracle, oracle_cat, cat_golden):
    """1. cat scene: light, floor, back wall, a wall turned mirror -- every variant, b 0 and 3: the frame after the edits is the frame after the upload of the edited scene,
    count_work too; one case against the oracle; the edited frame is not the unedited one"""
    base = [_full(x) for x in rt.scenes.spheres("cpu")]
    mesh = _cat(cat_golden)
    ctx.scene_upload(base, mesh)
    before = _frames(ctx, ["auto"])
    h0 = ctx.layout_hash()
    ctx.set_light(*CAT_LIGHT)
    for slot, s in cat_edits().items():
        ctx.set_sphere(slot, s)
    assert ctx.layout_hash() == h0
    assert ctx.light() == (CAT_LIGHT[0], float(np.float32(CAT_LIGHT[1])))
    for slot, s in cat_edits().items():
        assert ctx.sphere(slot) == tuple(s)
    edited = _apply(base, cat_edits())
    ref.scene_upload(edited, mesh, light=CAT_LIGHT)
    got, exp = _frames(ctx, ALL_VARIANTS), _frames(ref, ALL_VARIANTS)
    assert _same_frames(got, exp, "cat") == 2 * len(ALL_VARIANTS)       # every variant renders this scene
    for b in (0, 3):
        assert _differ(got[("auto", b)], before[("auto", b)]) > 1000   # (the oracle: 22 158 of the 25 641 pixels for b 0, 24 206 for b 3)
        for v in ("auto", "wavefront", "lockstep"):
            assert ctx.count_work(_params(b, variant=v)) == ref.count_work(_params(b, variant=v)), (v, b)
    osc = oracle.Scene()
    for s in edited:
        osc.add_sphere(*s)
    osc.add_mesh(oracle_cat)
    osc.set_light(*CAT_LIGHT)
    want, _, cnt = osc.render(W, H, 1, 3, want_rgb8=False)
    _bits_equal(got[("auto", 3)], want)
    assert ctx.count_work(_params(3)) == {k: cnt[k] for k in ("rays", "box_tests", "nodes", "tri_tests")}
    # more than one sample, a posed camera, progressive frames, explicit rays: the same scene everywhere
    pose = rt.make_pose(yaw=0.2, pitch=0.1)
    _bits_equal(ctx.render(_params(2, spp=3)), ref.render(_params(2, spp=3)))
    _bits_equal(ctx.render_pose(_params(2), pose), ref.render_pose(_params(2), pose))
    for c_ in (ctx, ref):
        c_.progressive_reset()
    for _ in range(2):
        a, b = ctx.progressive_frame(_params(1), pose), ref.progressive_frame(_params(1), pose)
    _bits_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    rays = np.concatenate([np.tile(np.float32([0, 0, 55]), (64, 1)), np.random.default_rng(3).normal(0, 1, (64, 3)).astype(np.float32) * 0.2 + np.float32([0, -0.1, -1])], 1)
    _bits_equal(ctx.trace_rays(rays), ref.trace_rays(rays))


def test_edit_equals_upload_demo10(ctx, ref, oracle):
    """1. demo10 without a mesh: the glass and the mirror sphere move, one changes radius, the material of one goes diffuse -> mirror -> glass; each stage against the upload"""
    base = [_full(x) for x in rt.scenes.spheres("demo10")]
    ctx.scene_upload(base, None)
    prev = _frames(ctx, ["auto", "wavefront"])
    ctx.set_light(*DEMO_LIGHT)
    cur = base
    for n, edits in enumerate(demo_stages()):
        for slot, s in edits.items():
            ctx.set_sphere(slot, s)
        cur = _apply(cur, edits)
        ref.scene_upload(cur, None, light=DEMO_LIGHT)
        got, exp = _frames(ctx, ALL_VARIANTS), _frames(ref, ALL_VARIANTS)
        assert _same_frames(got, exp, f"demo10 stage {n}") == 2 * len(ALL_VARIANTS)
        for b in (0, 3):
            # the oracle: stage 0 changes 11 282 (b 0) / 18 534 (b 3) pixels, stage 1 7 176 / 8 542, stage 2 none / 8 312 -- with one segment a mirror and a glass
            # sphere are the same black
            assert _differ(got[("auto", b)], prev[("auto", b)]) > (1000 if (b, n) != (0, 2) else -1), (n, b)
            assert ctx.count_work(_params(b, variant="wavefront")) == ref.count_work(_params(b, variant="wavefront"))
            assert ctx.count_work(_params(b)) == ref.count_work(_params(b))
        prev = got
    osc = oracle.Scene()
    for s in cur:
        osc.add_sphere(*s)
    osc.set_light(*DEMO_LIGHT)
    want, _, _ = osc.render(W, H, 1, 3, want_rgb8=False)
    _bits_equal(got[("auto", 3)], want)
    _bits_equal(got[("wavefront_queue", 3)], want)


def _vertex_normals(v, tv):
    vn = np.zeros_like(np.asarray(v, np.float64))
    fn = np.cross(v[tv[:, 1]] - v[tv[:, 0]], v[tv[:, 2]] - v[tv[:, 0]])
    for k in range(3):
        np.add.at(vn, tv[:, k], fn)
    return (vn / np.maximum(np.linalg.norm(vn, axis=1, keepdims=True), 1e-20)).astype(np.float32)


def _planar_uv(v):
    v = np.asarray(v, np.float32)
    lo, hi = v.min(0), v.max(0)
    return (((v[:, :2] - lo[:2]) / (hi[:2] - lo[:2])) * np.float32(2.6) - np.float32(0.8)).astype(np.float32)


def _rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.float32([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def _dress(c, cat_golden, px, dec):
    """smooth normals and a texture on the cat"""
    v, tv = cat_golden["vertices"], np.asarray(cat_golden["tri_bvh_order"])[:, :3]
    c.mesh_set_normals(_vertex_normals(v, tv), tv)
    c.mesh_set_texture(_planar_uv(v), tv, px, filter="bilinear", decode=dec)


def test_mesh_state_survives_the_edits(ctx, ref, cat_golden):
    """2. smooth normals, a texture, a device-side transform and an LBVH rebuild stay through the edits (the layout hashes too); and edits made first are still there after a
    transform and a rebuild in either mode (the rebuilds start from a copy of the scene in use)"""
    rng = np.random.default_rng(21)
    px, dec = rng.integers(0, 256, size=(23, 37, 3), dtype=np.uint8), rng.random(256).astype(np.float32)
    base = [_full(x) for x in rt.scenes.spheres("cpu")]
    edited = _apply(base, cat_edits())
    mesh = _cat(cat_golden)
    nt = len(np.asarray(mesh["indices"]))
    R, t = _rot_y(0.4), (2.0, 1.5, -3.0)

    def four_ops(c):
        _dress(c, cat_golden, px, dec)
        c.mesh_transform(R, t)
        c.mesh_rebuild(nt, mode="lbvh")

    def shots(c):
        return [c.render(_params(3)), c.render(_params(2, spp=2, sigma=0.2, seed=9)), c.render(_params(0, variant="wavefront"))]

    ctx.scene_upload(base, mesh)
    four_ops(ctx)
    h0 = ctx.layout_hash()
    plain = shots(ctx)
    ctx.set_light(*CAT_LIGHT)
    for slot, s in cat_edits().items():
        ctx.set_sphere(slot, s)
    assert ctx.layout_hash() == h0
    ref.scene_upload(edited, mesh, light=CAT_LIGHT)
    four_ops(ref)
    assert ref.layout_hash() == h0
    got = shots(ctx)
    for g, e, p in zip(got, shots(ref), plain):
        _bits_equal(g, e)
        assert _differ(g, p) > 1000
    # the other order
    for mode in ("reference", "lbvh"):
        ctx.scene_upload(base, mesh)
        ctx.set_light(*CAT_LIGHT)
        for slot, s in cat_edits().items():
            ctx.set_sphere(slot, s)
        ref.scene_upload(edited, mesh, light=CAT_LIGHT)
        for c_ in (ctx, ref):
            c_.mesh_transform(R, t)
            c_.mesh_rebuild(nt, mode=mode)
        assert ctx.layout_hash() == ref.layout_hash()
        assert ctx.light() == ref.light() and all(ctx.sphere(k) == ref.sphere(k) == tuple(edited[k]) for k in range(6))
        _bits_equal(ctx.render(_params(3)), ref.render(_params(3)), mode)
        _bits_equal(ctx.render(_params(1, variant="path")), ref.render(_params(1, variant="path")), mode)


def test_the_reference_motions_and_refusals(ctx, ref, cat_golden):
    """3. MoveObject three times is the upload with the centre numpy forms as c + v * dt in float32 three times; MoveLightSource is set_light(rt_light_orbit); a mesh's slot and a
    slot outside the scene are refused with the scene unchanged; a context without a scene answers RT_ERR_NO_SCENE"""
    base = [_full(x) for x in rt.scenes.spheres("demo10")]
    ctx.scene_upload(base, None)
    v, dt = np.float32([1.7, -0.3, 2.9]), np.float32(0.2)
    c = np.float32(base[0][0])
    for _ in range(3):
        ctx.move_sphere(0, v, float(dt))
        c = (c + (v * dt).astype(np.float32)).astype(np.float32)
    assert np.float32(ctx.sphere(0)[0]).tolist() == c.tolist()
    light = LIGHT
    for _ in range(4):
        ctx.move_light(2.5)
        light = rt.light_orbit(light, 2.5, 2e-2)
    assert ctx.light() == light
    assert light[0][1] == LIGHT[0][1] and light[0][0] != LIGHT[0][0]
    moved = _apply(base, {0: (tuple(float(x) for x in c),) + base[0][1:]})
    ref.scene_upload(moved, None, light=light)
    for variant in ("auto", "wavefront_queue", "path"):
        _bits_equal(ctx.render(_params(3, variant=variant)), ref.render(_params(3, variant=variant)), variant)
    ref.scene_upload(base, None)
    ref.set_light(*light)
    assert ref.light() == light
    # refusals
    ctx.scene_upload(rt.scenes.spheres("cpu"), _cat(cat_golden))
    frame = ctx.render(_params(1))
    for call in (lambda: ctx.move_sphere(SLOT, v), lambda: ctx.move_sphere(7, v), lambda: ctx.move_sphere(-1, v), lambda: ctx.set_sphere(SLOT, base[0]),
                 lambda: ctx.set_sphere(16, base[0]), lambda: ctx.sphere(SLOT), lambda: ctx.sphere(99)):
        with pytest.raises(rt.RtError) as e:
            call()
        assert e.value.code == -1
        _bits_equal(ctx.render(_params(1)), frame)
    fresh = rt.Context(0)
    try:
        for call in (lambda: fresh.light(), lambda: fresh.set_light(*LIGHT), lambda: fresh.sphere(0), lambda: fresh.set_sphere(0, base[0]), lambda: fresh.move_light(1.0),
                     lambda: fresh.move_sphere(0, v)):
            with pytest.raises(rt.RtError) as e:
                call()
            assert e.value.code == -4
    finally:
        fresh.close()


def test_edits_between_frames_in_flight(ctx, ref, cat_golden):
    """4. pipelining on, two alternating buffers, an edit between the calls and no synchronisation: frame k is the lone frame of the scene as it was at call k -- the kernels'
    arguments are captured at launch.  The same through render_async / wait."""
    import torch
    mesh = _cat(cat_golden)
    base = [_full(x) for x in rt.scenes.spheres("cpu")]
    w, h, n = 640, 360, 6
    p = _params(3, w=w, h=h)
    rows, _ = rt.interleaved_rows(h, 8, 0, 1)
    v = np.float32([0.0, -3.0, 0.0])
    # the scenes, frame by frame: the light orbits, the floor sinks (MoveObject), the back wall grows every other frame
    ref.scene_upload(base, mesh)
    want = []
    for k in range(n):
        ref.move_light(6.0, 0.1)
        ref.move_sphere(1, v, 0.25)
        if k % 2:
            s = ref.sphere(0)
            ref.set_sphere(0, (s[0], s[1] + 2.0) + s[2:])
        want.append(ref.render(p))
    assert all(_differ(want[k], want[k - 1]) > 1000 for k in range(1, n))
    st = torch.cuda.Stream()
    bufs = [torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0") for _ in range(2)]
    keep = [torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0") for _ in range(n)]
    torch.cuda.synchronize()
    ctx.scene_upload(base, mesh)
    try:
        ctx.set_pipelining(True)
        for k in range(n):
            ctx.move_light(6.0, 0.1)
            ctx.move_sphere(1, v, 0.25)
            if k % 2:
                s = ctx.sphere(0)
                ctx.set_sphere(0, (s[0], s[1] + 2.0) + s[2:])
            ctx.render_device(p, rows, bufs[k % 2].data_ptr(), st.cuda_stream)
            with torch.cuda.stream(st):                                  # a consumer of frame k, submitted after its call: sees it complete
                keep[k].copy_(bufs[k % 2], non_blocking=True)
        torch.cuda.synchronize()
    finally:
        ctx.set_pipelining(False)
    for k in range(n):
        _bits_equal(keep[k].cpu().numpy(), want[k], f"frame {k}")
    # render_async: slots alternate, the edit for frame k + 1 is made while frame k is in flight
    ctx.scene_upload(base, mesh)
    outs = [rt.PinnedArray((h, w, 4)).array for _ in range(n)]
    for k in range(n):
        ctx.move_light(6.0, 0.1)
        ctx.move_sphere(1, v, 0.25)
        if k % 2:
            s = ctx.sphere(0)
            ctx.set_sphere(0, (s[0], s[1] + 2.0) + s[2:])
        if k >= 2:
            ctx.wait(k % 2)
        ctx.render_async(p, outs[k], slot=k % 2)
    ctx.wait(0)
    ctx.wait(1)
    for k in range(n):
        _bits_equal(outs[k], want[k], f"async frame {k}")


# ---- animated batches ----------------------------------------------------------------------------------------------------------------------------------------------------
def _sequence(base, n, light=LIGHT):
    """frame k of a sequence over the spheres `base`: (camera position, fov, seed), light, sphere poses -- the light orbits (MoveLightSource steps) and changes intensity once,
    the first sphere drifts and grows, the second sinks and shrinks"""
    out = []
    for k in range(n):
        if k:
            light = rt.light_orbit(light, 4.0, 0.1)
        if k == 3:
            light = (light[0], 2e10)
        poses = [(s[0], s[1]) for s in base]
        c0, c1 = base[0][0], base[1][0]
        poses[0] = ((c0[0] + 0.5 * k, c0[1], c0[2] - 1.25 * k), base[0][1] + 0.5 * k)
        poses[1] = ((c1[0], c1[1] - 0.75 * k, c1[2] + 0.25 * k), base[1][1] - 0.125 * k)
        cam = ((0.5 * k - 1.0, 0.25 * (k % 3), 55.0 - 0.75 * k), None if k != 2 else 1.2, 1000 + 17 * k)
        out.append((cam, light, poses))
    return out


def _posed(base, poses):
    return [(tuple(float(x) for x in c), float(r)) + tuple(s[2:]) for s, (c, r) in zip(base, poses)]


def _batch(c, p, rows, seq, outs, st, animated=True):
    frames = [(o.data_ptr(), cam[0], cam[1], cam[2]) for o, (cam, _, _) in zip(outs, seq)]
    c.render_device_batch(p, rows, frames, st.cuda_stream, scenes=[(light, poses) for _, light, poses in seq] if animated else None)
    st.synchronize()
    return [o.cpu().numpy() for o in outs]


def _lone(c, base, mesh, p_of, rows, frame, buf, st, dress=None):
    cam, light, poses = frame
    c.scene_upload(_posed(base, poses), mesh, light=light, camera=(cam[0], cam[1]))
    if dress:
        dress(c)
    c.render_device(p_of(cam[2]), rows, buf.data_ptr(), st.cuda_stream)
    st.synchronize()
    return buf.cpu().numpy()


def test_animated_batch_is_the_lone_frames(ctx, ref, oracle, oracle_cat, cat_golden):
    """5. rows of rank 3 of 8 at 1920 x 1080, b 3, five frames each with its own camera, seed, light and sphere poses: every buffer is what render_device writes after the upload
    of that frame's scene (ray counts included); frame 2 is the oracle's.  Then the by-frames cut with jitter, 16 whole small frames, the spheres-only scene, the cat textured and
    smooth-shaded, scenes=None, and a plain batch right after an animated one."""
    import torch
    mesh = _cat(cat_golden)
    base = [_full(x) for x in rt.scenes.spheres("cpu")]
    w, h, b = 1920, 1080, 3
    rows, _ = rt.interleaved_rows(h, 8, 3, 8)
    st = torch.cuda.Stream()
    seq = _sequence(base, 5)
    outs = [torch.zeros((rows.n_rows, w, 4), dtype=torch.float32, device="cuda:0") for _ in range(5)]
    lone = torch.zeros_like(outs[0])
    torch.cuda.synchronize()
    ctx.scene_upload(base, mesh)
    got = _batch(ctx, _params(b, w=w, h=h), rows, seq, outs, st)
    assert ctx.stats()["travq_mode"] == 2
    assert ctx.light() == (LIGHT[0], float(np.float32(LIGHT[1])))      # the uploaded scene is not touched
    for k, fr in enumerate(seq):
        _bits_equal(got[k], _lone(ref, base, mesh, lambda seed: _params(b, w=w, h=h, seed=seed), rows, fr, lone, st), f"frame {k}")
        assert k == 0 or _differ(got[k], got[k - 1]) > 1000
    cam, light, poses = seq[2]
    osc = oracle.Scene()
    for s in _posed(base, poses):
        osc.add_sphere(*s)
    osc.add_mesh(oracle_cat)
    osc.set_light(*light)
    exp, _, _ = osc.render(w, h, 1, b, rows=(3 * 8, h), tile_rows=8, tile_step=8, cam=cam[0], fov=cam[1], seed=cam[2], want_rgb8=False)
    _bits_equal(got[2], exp)                                            # colours and the rays traced per pixel
    # a plain batch right after: the uploaded scene in every frame, nothing of the animated one left behind; scenes=None is that batch
    plain = _batch(ctx, _params(b, w=w, h=h), rows, seq[:2], outs[:2], st, animated=False)
    ref.scene_upload(base, mesh)
    again = _batch(ref, _params(b, w=w, h=h), rows, seq[:2], [lone, outs[4]], st, animated=False)
    for k in range(2):
        _bits_equal(plain[k], again[k], f"plain frame {k}")
        assert _differ(plain[k], got[k]) > 1000 or k == 0
    static = [(cam_, LIGHT, [(s[0], s[1]) for s in base]) for cam_, _, _ in seq[:2]]   # an animated batch whose frames all hold the uploaded scene
    for k, g in enumerate(_batch(ctx, _params(b, w=w, h=h), rows, static, outs[2:4], st)):
        _bits_equal(g, plain[k], f"static frame {k}")
    # four frames: the two sub-frames take two frames each (the by-frames cut); pixel jitter
    pj = lambda seed=0: _params(2, w=w, h=h, sigma=0.2, seed=seed)
    ctx.scene_upload(base, mesh)
    got = _batch(ctx, pj(), rows, seq[1:5], outs[:4], st)
    for k, fr in enumerate(seq[1:5]):
        _bits_equal(got[k], _lone(ref, base, mesh, pj, rows, fr, lone, st), f"jittered frame {k}")
    # the spheres-only scene (its lone frames: the lock-step kernel)
    demo = [_full(x) for x in rt.scenes.spheres("demo10")]
    dseq = _sequence(demo, 3, light=DEMO_LIGHT)
    ctx.scene_upload(demo, None)
    got = _batch(ctx, _params(5, w=w, h=h), rows, dseq, outs[:3], st)
    for k, fr in enumerate(dseq):
        _bits_equal(got[k], _lone(ref, demo, None, lambda seed: _params(5, w=w, h=h, seed=seed), rows, fr, lone, st), f"demo10 frame {k}")
    assert ref.stats()["variant"] == 5
    # 16 whole frames of 256 x 144
    w2, h2 = 256, 144
    rows2, _ = rt.interleaved_rows(h2, 8, 0, 1)
    seq16 = _sequence(base, 16)
    bufs = [torch.zeros((h2, w2, 4), dtype=torch.float32, device="cuda:0") for _ in range(16)]
    one = torch.zeros_like(bufs[0])
    torch.cuda.synchronize()
    ctx.scene_upload(base, mesh)
    got = _batch(ctx, _params(2, w=w2, h=h2), rows2, seq16, bufs, st)
    for k in (0, 7, 15):
        _bits_equal(got[k], _lone(ref, base, mesh, lambda seed: _params(2, w=w2, h=h2, seed=seed), rows2, seq16[k], one, st), f"frame {k} of 16")
    # the cat textured and smooth-shaded (wf_advance<kFormTex>'s animated form), against lone frames with the same texture and normals applied again
    rng = np.random.default_rng(22)
    px, dec = rng.integers(0, 256, size=(23, 37, 4), dtype=np.uint8), rng.random(256).astype(np.float32)
    dress = lambda c_: _dress(c_, cat_golden, px, dec)
    ctx.scene_upload(base, mesh)
    dress(ctx)
    got = _batch(ctx, _params(3, w=w2, h=h2), rows2, seq16[4:7], bufs[:3], st)
    for k, fr in enumerate(seq16[4:7]):
        _bits_equal(got[k], _lone(ref, base, mesh, lambda seed: _params(3, w=w2, h=h2, seed=seed), rows2, fr, one, st, dress=dress), f"textured frame {k}")
    ctx.mesh_set_texture(None, None, None)                              # smooth normals alone: the untextured kernel's animated form reads them too
    got = _batch(ctx, _params(3, w=w2, h=h2), rows2, seq16[4:6], bufs[:2], st)
    v, tv = cat_golden["vertices"], np.asarray(cat_golden["tri_bvh_order"])[:, :3]
    smooth = lambda c_: c_.mesh_set_normals(_vertex_normals(v, tv), tv)
    for k, fr in enumerate(seq16[4:6]):
        _bits_equal(got[k], _lone(ref, base, mesh, lambda seed: _params(3, w=w2, h=h2, seed=seed), rows2, fr, one, st, dress=smooth), f"smooth frame {k}")
    ctx.selfcheck()


def test_animated_batch_refusals(ctx, cat_golden):
    """6. what an animated batch cannot be: another sphere count, a variant without wf_advance, more than one sample, 17 frames -- nothing is rendered"""
    import torch
    base = [_full(x) for x in rt.scenes.spheres("cpu")]
    ctx.scene_upload(base, _cat(cat_golden))
    w, h = 256, 144
    rows, _ = rt.interleaved_rows(h, 8, 0, 1)
    st = torch.cuda.Stream()
    bufs = [torch.full((h, w, 4), -7.0, dtype=torch.float32, device="cuda:0") for _ in range(17)]
    torch.cuda.synchronize()
    seq = _sequence(base, 16)
    seq17 = seq + [seq[0]]

    def refused(p, frames_seq, code):
        with pytest.raises(rt.RtError) as e:
            _batch(ctx, p, rows, frames_seq, bufs[:len(frames_seq)], st)
        assert e.value.code == code
        torch.cuda.synchronize()
        assert all(bool((bf == -7.0).all()) for bf in bufs)

    short = [(cam, light, poses[:5]) for cam, light, poses in seq[:2]]
    refused(_params(2, w=w, h=h), short, -1)
    long_ = [(cam, light, poses + [poses[0]]) for cam, light, poses in seq[:2]]
    refused(_params(2, w=w, h=h), long_, -1)
    refused(_params(2, w=w, h=h, variant="lockstep"), seq[:2], -5)
    refused(_params(2, w=w, h=h, variant="path"), seq[:2], -5)
    refused(_params(2, spp=2, w=w, h=h), seq[:2], -5)
    refused(_params(2, w=w, h=h), seq17, -1)
    got = _batch(ctx, _params(2, w=w, h=h), rows, seq[:2], bufs[:2], st)          # and the context still renders
    assert all((g[..., 3] >= 1).all() for g in got)

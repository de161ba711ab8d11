"""Frames of scenes in which a mirror or a glass object is tinted (rt_material_set_tint: every wf_advance launch after the opening one is a kFormTint form; a specular
hit on the object is folded with the object's albedo).  -m gpu.  Every case fails on a library without the entries.

Every comparison is on uint32 views, .w (the ray count) included.  References, none of them the code under test:
  what exists   no flag, a flag set and removed, and an ineffective flag on a diffuse object, against a context that never heard of the calls: frames and the twelve
                still-view counters; flagged objects whose albedo is (1, 1, 1) against the unflagged frame;
  the model     tests/tint_model.py Walker (held to the closed forms and to gloss_model.Walker by tests/test_tint_model.py), its intersections the oracle's: a gold
                mirror ball over a floor; the tinted mirror cat in the open room, with flat and with smooth normals; a tinted rough ball beside a smooth untinted
                mirror; a tinted glass ball beside an unflagged one; a tinted ball beside the textured diffuse cat; a tint with a zero channel.
Frames are 67 x 45, 96 x 64 and 1 x 1."""
import ctypes as C

import numpy as np
import pytest

import raytracinggpu_amd as rt
from raytracinggpu_amd import _capi
from . import lens_model as lnm
from . import lights_model as lm
from . import still_view as sv
from . import texture_model as tm
from . import tint_model as tn
from .test_gpu_sky import FLOOR, LENS, NEAR, ROOM, WAVEFRONTS
from .test_gpu_soft_lights import COUNTS, POSE, THREE, _bits_equal, _differ, _moved, _params, _planar_uv, _texture, _vertex_normals

pytestmark = pytest.mark.gpu

f32 = np.float32
FP = C.POINTER(C.c_float)
RADII = [0.0, 2.0, 5.0]
GOLD, COPPER, BOTTLE, CYAN, WHITE = (0.83, 0.61, 0.23), (0.72, 0.45, 0.2), (0.3, 0.8, 0.35), (0.0, 0.6, 0.9), (1.0, 1.0, 1.0)
DIFFUSE_BALL = ((-22.0, -2.0, 10.0), 8.0, (0.7, 0.6, 0.3))


def _mirror(centre, radius, albedo):
    return (centre, radius, albedo, 1, 1.0, 1.0)


def _glass(centre, radius, albedo):
    return (centre, radius, albedo, 0, 1.5, 1.0)


# name -> (spheres, the mesh or None: (textured, mirror, smooth, albedo), {object position: alpha}, the flagged object positions); the mesh takes the position after the spheres
SCENES = {
    "gold ball": ([FLOOR, DIFFUSE_BALL, _mirror((2.0, 0.0, 12.0), 10.0, GOLD)], None, {}, (2,)),
    "mirror cat": (ROOM, (False, 1, False, COPPER), {}, (5,)),
    "smooth mirror cat": (ROOM, (False, 1, True, COPPER), {}, (5,)),
    "rough beside": ([FLOOR, _mirror((-14.0, 0.0, 10.0), 9.0, GOLD), _mirror((8.0, 0.0, 0.0), 9.0, COPPER)], None, {1: 0.25}, (1,)),   # the right one keeps the reference's mirror
    "glass pair": ([FLOOR, _glass((-12.0, 0.0, 14.0), 9.0, BOTTLE), _glass((12.0, 0.0, 14.0), 9.0, GOLD)], None, {}, (1,)),            # ... and the right one its clear glass
    "textured": ([FLOOR, _mirror((22.0, 0.0, 20.0), 10.0, GOLD)], (True, 0, False, rt.scenes.CAT_ALBEDO), {}, (1,)),                   # a tinted ball beside the textured diffuse cat
    "zero channel": ([FLOOR, DIFFUSE_BALL, _mirror((2.0, 0.0, 12.0), 10.0, CYAN)], None, {}, (2,)),
    "white": ([FLOOR, _mirror((-20.0, 0.0, 10.0), 9.0, WHITE), _mirror((0.0, 0.0, 0.0), 9.0, WHITE), _glass((20.0, 0.0, 10.0), 9.0, WHITE)], None, {2: 0.25}, (1, 2, 3)),
}


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


_CACHE = {}


def _built(oracle, g, name):
    """-> (spheres, upload dicts, oracle meshes, vertex normals or None), built once"""
    if ("built", name) not in _CACHE:
        spheres, mesh, _, _ = SCENES[name]
        dicts, oms, normals = [], [], None
        if mesh is not None:
            _, mirror, smooth, albedo = mesh
            m = oracle.Mesh.from_arrays(g["vertices"], g["tri_obj_order"]).build_bvh()
            oms.append(m)
            dicts.append(dict(vertices=m.vertices, indices=m.triangles, bvh_arr10=m.bvh_array(), albedo=albedo, object_slot=len(spheres), mirror=mirror))
            if smooth:
                normals = _vertex_normals(np.asarray(m.vertices), np.asarray(m.triangles)[:, :3])
                m.set_normals(normals, np.asarray(m.triangles)[:, :3])
        _CACHE[("built", name)] = (spheres, dicts, oms, normals)
    return _CACHE[("built", name)]


def _up(c, oracle, g, name, tinted=None, rough=None, **kw):
    spheres, dicts, _, normals = _built(oracle, g, name)
    c.scene_upload(spheres, dicts[0] if dicts else None, **kw)
    if normals is not None:
        c.mesh_set_normals(normals, np.asarray(dicts[0]["indices"])[:, :3])
    if SCENES[name][1] is not None and SCENES[name][1][0]:
        texels, decode = _texture()
        c.mesh_set_texture(_planar_uv(g["vertices"]), np.asarray(dicts[0]["indices"])[:, :3], texels, filter="bilinear", decode=decode, object_slot=dicts[0]["object_slot"])
    for slot, alpha in (SCENES[name][2] if rough is None else rough).items():
        c.set_roughness(slot, alpha)
    for slot in (SCENES[name][3] if tinted is None else tinted):
        c.set_tint(slot)


def _oracle_scene(oracle, g, name):
    """-> (oracle scene, materials, surface hook or None), built once"""
    if ("scene", name) not in _CACHE:
        spheres, dicts, oms, _ = _built(oracle, g, name)
        osc = oracle.Scene()
        for s in spheres:
            osc.add_sphere(s[0], s[1], s[2], *(s[3:] if len(s) > 3 else ()))
        for m in oms:
            osc.add_mesh(m)
        surface = None
        if SCENES[name][1] is not None and SCENES[name][1][0]:
            texels, decode = _texture()
            mesh, slot = oms[0], dicts[0]["object_slot"]
            verts, tris, uvs = mesh.vertices, mesh.triangles, _planar_uv(g["vertices"])

            def surface(oid, O, u, alb):
                if oid != slot:
                    return alb
                found, _, _, tri = mesh.intersect_tri(O, u, 1e-4)
                assert found and tri >= 0
                return tm.surface(verts, tris, tris, uvs, texels, decode, tm.BILINEAR, tm.REPEAT, alb, [tri], np.asarray(O, f32)[None], np.asarray(u, f32)[None])[1][0]
        _CACHE[("scene", name)] = (osc, lm.materials(spheres, dicts), surface)
    return _CACHE[("scene", name)]


class _LensWalker(tn.Walker, lnm.Walker):
    """the tint walker's path behind the lens walker's camera rays"""


def _model(oracle, g, name, b, spp=1, w=67, h=45, pose=None, rows=None, lights=(rt.scenes.LIGHT,), radii=None, lens=None, cam=(0, 0, 55), seed=123456, tinted=None):
    """the model's frame, computed once and left unchanged"""
    tinted = tuple(SCENES[name][3] if tinted is None else tinted)
    key = ("frame", name, b, spp, w, h, pose, None if rows is None else tuple(rows), repr(lights), repr(radii), lens, cam, seed, tinted)
    if key not in _CACHE:
        osc, mats, surface = _oracle_scene(oracle, g, name)
        kw = dict(fov=np.pi / 2) if pose is not None else {}
        if lens is not None:
            kw["lens"] = lens
        wk = (_LensWalker if lens is not None else tn.Walker)(osc, mats, list(lights), radii, rough=SCENES[name][2], tinted=tinted, cam=cam, seed=seed, **kw)
        wk.surface = surface
        fr = wk.render(w, h, spp, b, pose=pose, rows=rows)
        fr.setflags(write=False)
        _CACHE[key] = fr
        assert not tinted or wk.tints > 0 or w * h == 1, key             # the frame holds what it is there for
    return _CACHE[key]


# ---- exact against what exists ----------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scene", ["mirror cat", "textured"])
def test_no_flag_one_removed_and_an_ineffective_one_are_the_context_that_never_heard_of_the_calls(oracle, cat_golden, scene):
    """frames and the twelve still-view counters, on new contexts"""
    a, b = rt.Context(0), rt.Context(0)
    try:
        _up(a, oracle, cat_golden, scene, tinted=())
        _up(b, oracle, cat_golden, scene, tinted=())                    # b: not one call about a tint
        slot = SCENES[scene][3][0]
        a.set_tint(0)                                                   # the diffuse floor or wall: ineffective
        a.set_tint(slot, False)                                         # removing a flag that is not set
        p = _params(2, w=96, h=64)
        before = [[getattr(c_, n)() for n in COUNTS] for c_ in (a, b)]
        for _ in range(4):                                              # fill, use, store the records, resume
            plain = b.render(p)
            _bits_equal(a.render(p), plain)
        assert _moved(a, before[0]) == _moved(b, before[1])
        # set, rendered twice, and removed: a tinted chain keeps out of the still view, so the levels a holds are the ones it stored -- from here on a's frames AND its
        # counters move as b's do, which rendered nothing in between (a refill would show as misses and fills that b does not have)
        a.set_tint(slot)
        before = [getattr(a, n)() for n in COUNTS]
        lit = a.render(p)
        assert _differ(lit, plain) > 20
        _bits_equal(lit[..., 3], plain[..., 3])                         # .w counts what it counted
        _bits_equal(a.render(p), lit)
        assert all(all(v == 0 for v in d.values()) for d in _moved(a, before))                 # no counter moves under an effective tint
        a.set_tint(slot, False)
        assert not a.tint(slot) and a.tint(0)
        before = [[getattr(c_, n)() for n in COUNTS] for c_ in (a, b)]
        for q in (p, p, _params(2, spp=4, w=96, h=64), p, _params(0, w=1, h=1)):
            _bits_equal(a.render(q), b.render(q))
        assert _moved(a, before[0]) == _moved(b, before[1])
        _bits_equal(a.render_pose(_params(2), rt.make_pose(**POSE)), b.render_pose(_params(2), rt.make_pose(**POSE)))
    finally:
        a.close()
        b.close()


def test_a_flag_on_a_diffuse_sphere_and_a_material_changed_under_it(ctx, ref, oracle, cat_golden):
    """the materials are read when a chain is planned: a flagged diffuse sphere renders as ever, and becomes a tinted mirror the moment rt_scene_set_sphere makes it one"""
    _up(ctx, oracle, cat_golden, "gold ball", tinted=(0, 1))            # the floor and the diffuse ball
    _up(ref, oracle, cat_golden, "gold ball", tinted=())
    p = _params(2)
    before = [[getattr(c_, n)() for n in COUNTS] for c_ in (ctx, ref)]
    _bits_equal(ctx.render(p), ref.render(p))
    _bits_equal(ctx.render(p), ref.render(p))
    assert _moved(ctx, before[0]) == _moved(ref, before[1])
    mirror = _mirror(DIFFUSE_BALL[0], DIFFUSE_BALL[1], COPPER)
    ctx.set_sphere(1, mirror)
    osc = oracle.Scene()
    spheres = [FLOOR, mirror, SCENES["gold ball"][0][2]]
    for s in spheres:
        osc.add_sphere(s[0], s[1], s[2], *(s[3:] if len(s) > 3 else ()))
    wk = tn.Walker(osc, lm.materials(spheres), [rt.scenes.LIGHT], tinted=(0, 1))
    _bits_equal(ctx.render(p), wk.render(67, 45, 1, 2), "the diffuse ball made a mirror under its flag: tinted by the albedo rt_scene_set_sphere gave it")
    assert wk.tinted == {1} and wk.tints > 0


@pytest.mark.parametrize("b,spp", [(2, 1), (5, 1), (2, 4)])
def test_flagged_white_mirror_rough_mirror_and_glass_render_the_unflagged_frame(ctx, ref, oracle, cat_golden, b, spp):
    """fl(1 x) is x and +0 + x is x: the tint forms with a full mask against the gloss forms, word for word"""
    _up(ctx, oracle, cat_golden, "white")
    _up(ref, oracle, cat_golden, "white", tinted=())
    assert [ctx.tint(k) for k in range(4)] == [False, True, True, True]
    for w, h in ((67, 45), (96, 64)):
        _bits_equal(ctx.render(_params(b, spp=spp, w=w, h=h)), ref.render(_params(b, spp=spp, w=w, h=h)), f"b={b} spp={spp} {w}x{h}")


# ---- against the model, word for word --------------------------------------------------------------------------------------------------------------------------------------

MODELLED = ["gold ball", "mirror cat", "smooth mirror cat", "rough beside", "glass pair", "textured", "zero channel"]
CASES = [(s, b, spp) for s in MODELLED for b, spp in ((0, 1), (2, 1), (5, 1), (2, 4))]


@pytest.mark.parametrize("scene,b,spp", CASES)
def test_scenes_with_a_tint_equal_the_model(ctx, oracle, cat_golden, scene, b, spp):
    _up(ctx, oracle, cat_golden, scene)
    _bits_equal(ctx.render(_params(b, spp=spp)), _model(oracle, cat_golden, scene, b, spp), f"{scene} b={b} spp={spp}")


def test_the_tinted_frame_is_not_the_plain_one_and_w_is(ctx, ref, oracle, cat_golden):
    for scene in ("glass pair", "rough beside"):
        _up(ctx, oracle, cat_golden, scene)
        _up(ref, oracle, cat_golden, scene, tinted=())
        a, b = ctx.render(_params(2, spp=4, w=96, h=64)), ref.render(_params(2, spp=4, w=96, h=64))
        assert _differ(a, b) > 100, scene
        _bits_equal(a[..., 3], b[..., 3], scene)                        # the same rays, counted the same
        same = ~(a.view(np.uint32) != b.view(np.uint32)).any(-1)        # (a pixel whose paths never meet the tinted ball keeps every word)
        assert same.sum() > 100, scene


def test_three_lights_and_radii_equal_the_model(ctx, oracle, cat_golden):
    """soft | gloss | tint and tex | soft | gloss | tint: a light list takes the soft route with radii 0, then with radii"""
    for scene in ("gold ball", "textured"):
        _up(ctx, oracle, cat_golden, scene)
        ctx.set_lights(THREE)
        _bits_equal(ctx.render(_params(2)), _model(oracle, cat_golden, scene, 2, lights=THREE), f"{scene}: three lights")
        ctx.set_light_radii(RADII)
        _bits_equal(ctx.render(_params(2)), _model(oracle, cat_golden, scene, 2, lights=THREE, radii=RADII), f"{scene}: radii")
        ctx.set_light(*rt.scenes.LIGHT)
        ctx.set_light_radii([3.0])
        _bits_equal(ctx.render(_params(2)), _model(oracle, cat_golden, scene, 2, radii=[3.0]), f"{scene}: one light with a radius")


def test_lens_posed_camera_row_shares_one_pixel_and_every_wavefront_variant_equal_the_model(ctx, oracle, cat_golden):
    import torch
    _up(ctx, oracle, cat_golden, "textured")
    p = _params(2)
    whole = _model(oracle, cat_golden, "textured", 2)
    ctx.set_lens(*LENS)
    _bits_equal(ctx.render(p), _model(oracle, cat_golden, "textured", 2, lens=LENS), "lens")
    ctx.set_lens(0.0, 1.0)
    near = ctx.render_pose(p, rt.make_pose(position=NEAR, **POSE))
    _bits_equal(near, _model(oracle, cat_golden, "textured", 2, pose=(POSE["yaw"], POSE["pitch"]), cam=NEAR), "posed")
    share, image_rows = rt.interleaved_rows(45, 8, 1, 3)
    buf = torch.zeros((share.n_rows, 67, 4), dtype=torch.float32, device="cuda")
    ctx.render_device(p, share, buf.data_ptr())
    ctx.synchronize()
    _bits_equal(buf.cpu().numpy(), whole[list(image_rows)], "row share")
    _up(ctx, oracle, cat_golden, "gold ball")
    _bits_equal(ctx.render(_params(2, w=1, h=1, spp=4)), _model(oracle, cat_golden, "gold ball", 2, spp=4, w=1, h=1), "1 x 1")
    # with a mesh: all seven; spheres alone (auto would take the lock-step kernel without the tint): the three that stage nothing
    for scene, variants in (("textured", WAVEFRONTS), ("glass pair", ("auto", "wavefront", "wavefront_queue"))):
        _up(ctx, oracle, cat_golden, scene)
        for v in variants:
            _bits_equal(ctx.render(_params(2, variant=v)), _model(oracle, cat_golden, scene, 2), f"{scene} {v}")


@pytest.mark.parametrize("knobs", [dict(RT_PARTS="1"), dict(RT_PARTS="3"), dict(RT_DEAD_CHANNELS="0"), dict(RT_TRAVQ_ANYHIT="0")])
def test_other_cuts_and_knobs_render_the_same_words(oracle, cat_golden, knobs):
    """(RT_DEAD_CHANNELS=0: the model knows no dead channel, and the default's frames are the model's too -- the two are the same words)"""
    c_ = sv.context(**knobs)
    try:
        for scene, b, spp in (("mirror cat", 2, 1), ("zero channel", 5, 1), ("zero channel", 2, 4), ("textured", 2, 1)):
            _up(c_, oracle, cat_golden, scene)
            _bits_equal(c_.render(_params(b, spp=spp)), _model(oracle, cat_golden, scene, b, spp), f"{knobs} {scene}")
    finally:
        c_.close()


def test_a_batch_of_three_async_and_the_flag_toggled_between_pipelined_frames(ctx, ref, oracle, cat_golden):
    import torch
    W, H = 67, 45
    _up(ctx, oracle, cat_golden, "gold ball")
    rows = _capi.Rows(0, H, H, 1)
    cams = [((0.5 * k, 0.0, 55.0 - 3 * k), 40 + k) for k in range(3)]
    bufs = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in cams]
    ctx.render_device_batch(_params(2), rows, [(bf.data_ptr(), cam, None, seed) for bf, (cam, seed) in zip(bufs, cams)])
    ctx.synchronize()
    for bf, (cam, seed) in zip(bufs, cams):
        _up(ref, oracle, cat_golden, "gold ball", camera=(cam, None))
        _bits_equal(bf.cpu().numpy(), ref.render(_params(2, seed=seed)), str(cam))
    cam, seed = cams[1]
    _bits_equal(bufs[1].cpu().numpy(), _model(oracle, cat_golden, "gold ball", 2, cam=cam, seed=seed), "the batch's second frame")
    out = rt.PinnedArray((H, W, 4), np.float32)
    try:
        ctx.render_async(_params(2), out.array, slot=0)
        ctx.wait(0)
        _bits_equal(out.array, _model(oracle, cat_golden, "gold ball", 2), "async")
    finally:
        out.close()
    # four pipelined frames, the flag toggled between them: on, off, on, off
    flags = [True, False, True, False]
    want = [_model(oracle, cat_golden, "gold ball", 2, tinted=(2,) if f else ()) for f in flags]
    assert _differ(want[0], want[1]) > 20
    pair = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
    got = []
    ctx.set_pipelining(True)
    try:
        for k in range(4):
            ctx.set_tint(2, flags[k])
            ctx.render_device(_params(2), rows, pair[k % 2].data_ptr())
            if k % 2 == 1:
                ctx.synchronize()
                got.extend(b.cpu().numpy() for b in pair)
    finally:
        ctx.set_pipelining(False)
    for k, fr in enumerate(got):
        _bits_equal(fr, want[k], f"pipelined frame {k}")


# ---- what refuses ----------------------------------------------------------------------------------------------------------------------------------------------------------------

def test_what_cannot_render_a_tint_refuses(ctx, oracle, cat_golden):
    """RT_ERR_UNSUPPORTED (-5), outputs as they were (filled with -7), "tint" in the error text"""
    import torch
    W, H = 67, 45
    _up(ctx, oracle, cat_golden, "textured")
    ctx.mesh_set_texture(None, None, None, object_slot=2)               # (the variants below refuse a texture before they ask about the lights)
    p = _params(2)
    frame = ctx.render(p)
    lib, h = ctx._L, ctx._h
    counts = np.full((H, W), 2, np.uint8)

    def refused():
        for v in ("path", "lockstep", "global"):
            out = np.full((H, W, 4), -7.0, f32)
            pv = _params(2, variant=v)
            yield v, lib.rt_render(h, C.byref(pv), 0, H, out.ctypes.data_as(FP)), bool((out == -7.0).all())
        work = _capi.Work()
        C.memset(C.byref(work), 7, C.sizeof(work))
        yield "rt_count_work", lib.rt_count_work(h, C.byref(p), 0, H, C.byref(work)), bytes(work) == b"\x07" * C.sizeof(work)
        out = np.full((H, W, 4), -7.0, f32)
        yield "rt_render_counts", lib.rt_render_counts(h, C.byref(p), None, counts.ctypes.data_as(C.POINTER(C.c_uint8)), None, out.ctypes.data_as(FP)), bool((out == -7.0).all())
        dcounts = torch.full((H, W), 2, dtype=torch.uint8, device="cuda")
        dout = torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda")
        rc = lib.rt_render_counts_device(h, C.byref(p), None, C.c_void_p(dcounts.data_ptr()), None, C.c_void_p(dout.data_ptr()), None)
        ctx.synchronize()
        yield "rt_render_counts_device", rc, bool((dout == -7.0).all())
        buf = torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda")
        poses = [(s[0], s[1]) for s in SCENES["textured"][0]]
        try:
            ctx.render_device_batch(p, _capi.Rows(0, H, H, 1), [(buf.data_ptr(), (0.0, 0.0, 55.0), None, 1)], scenes=[(rt.scenes.LIGHT, poses)])
            rc = 0
        except rt.RtError as e:
            rc = e.code
        ctx.synchronize()
        yield "rt_render_device_batch_scenes", rc, bool((buf.cpu().numpy() == -7.0).all())

    seen = 0
    for what, rc, untouched in refused():
        assert rc == -5 and untouched, (what, rc, untouched)
        assert b"tint" in lib.rt_last_error(h), what
        seen += 1
    assert seen == 7
    for turn_on, turn_off in ((lambda: ctx.set_shutter(light=(6.0, 0.0, -4.0)), lambda: ctx.set_shutter()),
                              (lambda: ctx.set_environment(np.ones((2, 2, 3), f32)), lambda: ctx.set_environment()),
                              (lambda: ctx.set_emission(2, (1.0, 1.0, 1.0)), lambda: ctx.set_emission(2, (0.0, 0.0, 0.0)))):
        turn_on()
        out = np.full((H, W, 4), -7.0, f32)
        assert lib.rt_render(h, C.byref(p), 0, H, out.ctypes.data_as(FP)) == -5 and (out == -7.0).all()
        assert b"tint" in lib.rt_last_error(h)
        turn_off()
    _bits_equal(ctx.render(p), frame)
    # the feature-buffer entries are unchanged under an effective tint
    ctx.set_tint(1, False)
    planes = ctx.render_aov(p)
    ctx.set_tint(1)
    _bits_equal(ctx.render_aov(p), planes)
    # the flag removed: everything renders again
    ctx.set_tint(1, False)
    assert ctx.count_work(p)["rays"] > 0
    assert ctx.render(_params(2, variant="path"))[..., 3].sum() > 0
    # ... and beside an effective Fresnel flag: the unflagged glass ball of "glass pair" made a Fresnel dielectric; and a roughness beside the tint still says "tint"
    _up(ctx, oracle, cat_golden, "glass pair")
    p = _params(2)
    frame = ctx.render(p)
    ctx.set_fresnel(0)                                                  # a Fresnel flag on the diffuse floor is not effective: the frame is what it was
    _bits_equal(ctx.render(p), frame)
    ctx.set_fresnel(2)
    out = np.full((H, W, 4), -7.0, f32)
    assert lib.rt_render(h, C.byref(p), 0, H, out.ctypes.data_as(FP)) == -5 and (out == -7.0).all()
    assert b"tint" in lib.rt_last_error(h)
    ctx.set_fresnel(2, False)
    _bits_equal(ctx.render(p), frame)
    _up(ctx, oracle, cat_golden, "rough beside")
    out = np.full((H, W, 4), -7.0, f32)
    pv = _params(2, variant="path")
    assert lib.rt_render(h, C.byref(pv), 0, H, out.ctypes.data_as(FP)) == -5 and (out == -7.0).all()
    assert b"tint" in lib.rt_last_error(h)

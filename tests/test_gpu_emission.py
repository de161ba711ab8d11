"""Emissive meshes on the device (rt_scene_set_emission: the table over the scene's triangles, built by emit_dist_weights and the sky table's three kernels, and the draw
emit_draw of rt_shade.hip.h).  -m gpu.  Every case fails on a library without the entries.

Every comparison is on integer views, against tests/emission_model.py (held to the mathematics by tests/test_emission_model.py): the table for one triangle, a panel,
300 triangles with zero-area ones among them, about 5 000 triangles (several workgroups of 256) and three meshes of which two emit; the draw on 2^16 keys per scene.
The stored order is the one the upload's tree gives (emission_model.stored_order), the meshes one after the other in object order."""
import ctypes as C

import numpy as np
import pytest

import raytracinggpu_amd as rt
from . import emission_model as em
from .sky_sample_model import mix32

pytestmark = pytest.mark.gpu

f32 = np.float32
FLOOR = ((0, -1000, 0), 990, (0.5, 0.5, 0.5))
R1 = np.array([[0.9553365, 0, 0.29552022], [0, 1, 0], [-0.29552022, 0, 0.9553365]], np.float32)
T1 = (0.5, 0.25, -0.5)


def _grid(nx, nz, origin, step, seed, flat=0):
    """a bumpy sheet of 2 nx nz triangles; `flat` of them are made zero-area by naming one vertex twice"""
    rng = np.random.default_rng(seed)
    x, z = np.meshgrid(np.arange(nx + 1), np.arange(nz + 1), indexing="xy")
    v = np.stack([origin[0] + step * x, origin[1] + rng.uniform(-0.3, 0.3, x.shape), origin[2] + step * z], axis=-1).reshape(-1, 3).astype(f32)
    i = (z[:-1, :-1] * (nx + 1) + x[:-1, :-1]).ravel()
    t = np.concatenate([np.stack([i, i + 1, i + nx + 2], axis=1), np.stack([i, i + nx + 2, i + nx + 1], axis=1)]).astype(np.int32)
    t = t[rng.permutation(len(t))]
    t[:flat, 2] = t[:flat, 1]
    return v, t


def _one_triangle():
    return np.array([[-3, 12, 1], [4, 12, 2], [0, 13, -5]], f32), np.array([[0, 1, 2]], np.int32)


MESHES = {
    "triangle": [(_one_triangle(), (3.0, 2.0, 1.0))],
    "panel": [(rt.scenes.panel((-6, 14, -6), (12, 0.5, 0), (0, 0.25, 12)), (10.0, 9.0, 8.0))],
    "300": [(_grid(15, 10, (-8, 10, -5), 1.0, 300, flat=17), (0.5, 0.0, 2.0))],
    "5000": [(_grid(50, 50, (-25, 12, -25), 1.0, 5000, flat=3), (1.0, 1.0, 1.0))],
    # three meshes of which two emit, with different radiance; the one in the middle does not
    "three": [(_grid(6, 5, (-9, 11, -3), 1.0, 31), (4.0, 0.0, 0.0)), (_grid(7, 4, (-2, 9, -3), 1.0, 32, flat=2), (0.0, 0.0, 0.0)),
              (rt.scenes.panel((5, 13, -4), (3, 0, 0), (0, 1, 5)), (0.25, 0.5, 40.0))],
}


@pytest.fixture(scope="module")
def ctx():
    c_ = rt.Context(0)
    yield c_
    c_.close()


_BUILT = {}


def _built(oracle, name):
    """-> (oracle meshes, upload dicts): the meshes of MESHES[name] behind one floor sphere, at object positions 1, 2, ..."""
    if name not in _BUILT:
        oms, dicts = [], []
        for k, ((v, t), _) in enumerate(MESHES[name]):
            m = oracle.Mesh.from_arrays(v, t).build_bvh()
            oms.append(m)
            dicts.append(dict(vertices=m.vertices, indices=m.triangles, bvh_arr10=m.bvh_array(), albedo=(0.5, 0.5, 0.5), object_slot=1 + k))
        _BUILT[name] = (oms, dicts)
    return _BUILT[name]


def _upload(ctx, oracle, name, emit=True):
    oms, dicts = _built(oracle, name)
    ctx.scene_upload([FLOOR], dicts if len(dicts) > 1 else dicts[0])
    if emit:
        for k, (_, le) in enumerate(MESHES[name]):
            ctx.set_emission(1 + k, le)
    return dicts


def _model(dicts, les):
    """the table of the uploaded meshes `dicts` (object order) under the radiances `les`"""
    tris = [em.corners(d["vertices"], d["indices"], em.stored_order(d["bvh_arr10"])) for d in dicts]
    le = [np.broadcast_to(np.asarray(l, f32), (len(t), 3)) for t, l in zip(tris, les)]
    return em.TriTable(np.concatenate(tris), np.concatenate(le))


def _same_table(ctx, tb):
    c, prefix, total = ctx.kat_emission_table()
    assert total == tb.total
    assert len(c) == tb.nt
    assert (c == tb.c).all()
    assert (prefix == tb.prefix).all()


def _bits_equal(a, b):
    np.testing.assert_array_equal(np.ascontiguousarray(a, f32).view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32))


def _keys(salt, n=1 << 16):
    hs = mix32(np.arange(n, dtype=np.uint64) ^ np.uint64(salt)).astype(np.uint32)
    hs[:4] = (0, 1, 0xFFFFFFFF, 0x80000000)
    return hs, (np.arange(n) % 7).astype(np.int32)


@pytest.mark.parametrize("name", list(MESHES))
def test_the_table_and_the_draw_equal_the_model(ctx, oracle, name):
    dicts = _upload(ctx, oracle, name)
    tb = _model(dicts, [le for _, le in MESHES[name]])
    assert tb.total > 0
    _same_table(ctx, tb)
    hs, seg = _keys(0x2545F491)
    tri, point = ctx.kat_emission_sample(hs, seg)
    t, Q = tb.sample(hs, seg)
    assert (tri == t).all()
    _bits_equal(point, Q)
    assert (tb.c[tri] > 0).all()                                        # a draw never lands on a triangle without area or without radiance
    if name == "5000":
        assert tb.nt == 5000 and len(np.unique(tri)) > 4000
    if name == "three":
        assert (tb.c[30 * 2:30 * 2 + 56] == 0).all() and (tb.c[:60] > 0).all() and (tb.c[-2:] > 0).all()
    if name in ("300", "three"):
        assert ((tb.A2 == 0) & (tb.c == 0)).sum() >= 2


def test_a_transform_and_a_rebuild_of_the_emitter_rebuild_the_table(ctx, oracle):
    oms, dicts = _built(oracle, "three")
    les = [le for _, le in MESHES["three"]]
    _upload(ctx, oracle, "three")
    _same_table(ctx, _model(dicts, les))
    ctx.mesh_transform(R1, T1, object_slot=1)                           # the first emitter moves: its areas change in the last bits
    v, t = MESHES["three"][0][0]
    moved = oracle.Mesh.from_arrays(v, t).build_bvh().transform(R1, T1)
    after = [dict(dicts[0], vertices=moved.vertices)] + dicts[1:]
    tb = _model(after, les)
    _same_table(ctx, tb)
    hs, seg = _keys(0x9E3779B1, 1 << 12)
    tri, point = ctx.kat_emission_sample(hs, seg)
    t_, Q = tb.sample(hs, seg)
    assert (tri == t_).all()
    _bits_equal(point, Q)
    arr, order = ctx.mesh_rebuild(len(t), mode="lbvh", object_slot=1)   # ... and gets a new tree: the stored order is the one tri_order_out and the new tree give
    rebuilt = [dict(after[0], indices=np.asarray(after[0]["indices"])[order], bvh_arr10=arr)] + dicts[1:]
    tb = _model(rebuilt, les)
    _same_table(ctx, tb)
    tri, point = ctx.kat_emission_sample(hs, seg)
    t_, Q = tb.sample(hs, seg)
    assert (tri == t_).all()
    _bits_equal(point, Q)


def test_no_emission_is_no_table_and_invalid_arguments_leave_the_state_untouched(ctx, oracle):
    dicts = _upload(ctx, oracle, "three", emit=False)
    assert ctx.emission_sampling() == 0.5
    c, prefix, total = ctx.kat_emission_table()
    assert total == 0 and len(c) == 60 + 56 + 2 and not c.any() and not prefix.any()
    with pytest.raises(rt.RtError):
        ctx.kat_emission_sample([1, 2], 0)
    les = [(2.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 3.0, 0.5)]
    ctx.set_emission(1, les[0])
    ctx.set_emission(3, les[2])
    ctx.set_emission_sampling(0.25)
    tb = _model(dicts, les)
    _same_table(ctx, tb)
    lib, h = ctx._L, ctx._h
    bad_rgb = [(np.nan, 1, 1), (1, -1.0, 1), (1, 1, np.inf), (-0.0, 1, 1), (1, 2.0 ** 96, 1), (1, 1, -np.inf)]
    for rgb in bad_rgb:
        assert lib.rt_scene_set_emission(h, 1, (C.c_float * 3)(*rgb)) == -1, rgb
        assert b"emission" in lib.rt_last_error(h)
    good = (C.c_float * 3)(1, 1, 1)
    for slot in (0, -1, 4, 16, 1000):                                   # the floor sphere's slot, and slots outside the scene
        assert lib.rt_scene_set_emission(h, slot, good) == -1, slot
        out = (C.c_float * 3)(-7, -7, -7)
        assert lib.rt_scene_get_emission(h, slot, out) == -1 and tuple(out) == (-7, -7, -7)
    assert lib.rt_scene_set_emission(h, 1, None) == -1 and lib.rt_scene_get_emission(h, 1, None) == -1
    for bad in (np.nan, -0.25, 1.0000001, np.inf, -np.inf, 2.0):
        assert lib.rt_scene_set_emission_sampling(h, C.c_float(bad)) == -1, bad
        assert b"emission sampling" in lib.rt_last_error(h)
    assert lib.rt_scene_get_emission_sampling(h, None) == -1
    assert ctx.emission_sampling() == 0.25
    assert [ctx.emission(k) for k in (1, 2, 3)] == [tuple(map(float, np.asarray(l, f32))) for l in les]
    _same_table(ctx, tb)                                                # nothing that was refused touched the table
    ctx.set_emission(1, (2.0, 0.0, 0.0))                                # the same radiance again: nothing to do
    _same_table(ctx, tb)
    ctx.set_emission(2, (0.0, 0.0, 2.0 ** 95))                          # the largest radiances still quantise: every positive weight keeps a count of at least 1
    tb2 = _model(dicts, [les[0], (0.0, 0.0, 2.0 ** 95), les[2]])
    assert (tb2.c[tb2.W > 0] >= 1).all() and (tb2.c[:60] == 1).sum() > 0
    _same_table(ctx, tb2)
    ctx.set_emission(2, (0, 0, 0))
    ctx.set_emission(1, (0, 0, 0))                                      # one emitter left
    _same_table(ctx, _model(dicts, [(0, 0, 0), (0, 0, 0), les[2]]))
    ctx.set_emission(3, (0, 0, 0))                                      # none: the table is dropped
    assert ctx.kat_emission_table()[2] == 0
    with pytest.raises(rt.RtError):
        ctx.kat_emission_sample([1], 0)


def test_an_upload_clears_the_emission_and_resets_the_share_and_no_scene_is_refused(ctx, oracle):
    _upload(ctx, oracle, "panel")
    ctx.set_emission_sampling(1.0)
    assert ctx.emission(1) == (10.0, 9.0, 8.0) and ctx.emission_sampling() == 1.0
    assert ctx.kat_emission_table()[2] > 0
    _upload(ctx, oracle, "panel", emit=False)
    assert ctx.emission(1) == (0.0, 0.0, 0.0) and ctx.emission_sampling() == 0.5
    assert ctx.kat_emission_table()[2] == 0
    fresh = rt.Context(0)                                               # no upload: RT_ERR_NO_SCENE, and nothing is written
    try:
        lib, h = fresh._L, fresh._h
        s = C.c_float(-7.0)
        assert lib.rt_scene_get_emission_sampling(h, C.byref(s)) == -4 and s.value == -7.0
        assert lib.rt_scene_set_emission_sampling(h, C.c_float(0.5)) == -4
        v = (C.c_float * 3)(-7, -7, -7)
        assert lib.rt_scene_get_emission(h, 0, v) == -4 and tuple(v) == (-7, -7, -7)
        assert lib.rt_scene_set_emission(h, 0, v) == -4
        total, nt = C.c_uint64(7), C.c_int32(7)
        assert lib.rt_kat_emission_table(h, None, None, C.byref(total), C.byref(nt)) == -4 and total.value == 7 and nt.value == 7
        assert lib.rt_kat_emission_sample(h, 0, None, None, None, None) == -4
    finally:
        fresh.close()


def test_a_weight_that_is_not_finite_is_refused_until_the_radiance_is_lowered(ctx, oracle):
    """twice the area 2^35 times a radiance of 2^95: W overflows.  The radiance itself is valid, so the set succeeds; what asks for the table -- a known answer, a frame --
    answers RT_ERR_INVALID with "emission" in the text instead of drawing from a table that the overflow has made flat"""
    v = np.array([[0, 50, 0], [2.0 ** 18, 50, 1], [3, 51, 2.0 ** 17]], f32)
    m = oracle.Mesh.from_arrays(v, np.array([[0, 1, 2]], np.int32)).build_bvh()
    d = dict(vertices=m.vertices, indices=m.triangles, bvh_arr10=m.bvh_array(), albedo=(0.5, 0.5, 0.5), object_slot=1)
    ctx.scene_upload([FLOOR], d)
    ctx.set_emission(1, (0.0, 2.0 ** 95, 0.0))
    for call in (ctx.kat_emission_table, lambda: ctx.kat_emission_sample([1, 2], 0)):
        with pytest.raises(rt.RtError) as e:
            call()
        assert e.value.code == -1 and "emission" in str(e.value)
    out = np.full((8, 8, 4), -7.0, f32)
    p = rt.make_params(8, 8, 1, 1, **rt.scenes.CPU_LAUNCHER)
    assert ctx._L.rt_render(ctx._h, C.byref(p), 0, 8, out.ctypes.data_as(C.POINTER(C.c_float))) == -1 and (out == -7.0).all()
    assert ctx.emission(1) == (0.0, float(f32(2.0 ** 95)), 0.0)
    ctx.set_emission(1, (0.0, 2.0 ** 60, 0.0))
    _same_table(ctx, _model([d], [(0.0, 2.0 ** 60, 0.0)]))
    assert ctx.render(p).shape == (8, 8, 4)

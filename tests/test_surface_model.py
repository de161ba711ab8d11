"""tests/surface_model.py against the reference's own Scene::getColor (the CPU oracle), and the model's two elementwise maps.  No GPU.

The chain is the reference's: a camera ray given k segments of depth returns, bit for bit, what the model's ray after k specular segments returns with none --
both are the direct light at the first diffuse surface (the bounce behind it gets depth -1 and is black) -- and with one segment less it is black."""
import ctypes as C

import numpy as np
import pytest

import raytracinggpu_amd as rt
from . import denoise_model as dm
from . import material_scenes as ms
from . import surface_model as sm

F = np.float32
FP = C.POINTER(C.c_float)


def _get_color(oracle, scene, O, u, depth, eps=1e-3, tri_tmin=1e-4):
    O = np.ascontiguousarray(O, np.float32)
    u = np.ascontiguousarray(u, np.float32)
    out = np.zeros(3, np.float32)
    oracle.lib().or_scene_get_color(scene.h, O.ctypes.data_as(FP), u.ctypes.data_as(FP), int(depth), eps, tri_tmin, 123456, 77, 0, out.ctypes.data_as(FP), None)
    return out


def _scene(name, oracle, cat_golden):
    if name == "demo10":
        return (oracle.Scene.preset("demo10"),) + sm.sphere_tables(rt.scenes.spheres("demo10"))
    v, t = cat_golden["vertices"], cat_golden["tri_obj_order"]
    return (ms.oracle_scene(oracle, name, v, t),) + sm.described_tables(ms.describe(name, v))


# (scene, W, H, max_specular, least diffuse-ended chain pixels, largest chain length or None, exhausted pixels expected)
CASES = [("demo10", 96, 64, 8, 2000, 7, False), ("cpu_mirror", 64, 48, 4, 300, None, False), ("cpu_glass", 64, 48, 8, 300, None, True)]


@pytest.mark.parametrize("name,W,H,max_specular,least,longest,exhausted", CASES)
def test_the_model_is_the_references(oracle, cat_golden, name, W, H, max_specular, least, longest, exhausted):
    scene, materials, albedos = _scene(name, oracle, cat_golden)
    chains = {}
    planes = sm.oracle_aov_surface(scene, materials, albedos, W, H, max_specular, chains=chains)
    O, u = dm.camera_rays(W, H)
    n_chain = n_left_out = 0
    ks = []
    for (r, c), ch in chains.items():
        if ch.status != sm.DIFFUSE or ch.k < 1:
            continue
        n_chain += 1
        ks.append(ch.k)
        if ch.refr != F(1):                                          # arrives inside glass: the oracle starts every ray at index 1
            n_left_out += 1
            continue
        a = _get_color(oracle, scene, O, u[r, c], ch.k)
        b = _get_color(oracle, scene, ch.O, ch.u, 0)
        assert a.view(np.uint32).tolist() == b.view(np.uint32).tolist(), (name, r, c, ch.k, a, b)
        assert not _get_color(oracle, scene, O, u[r, c], ch.k - 1).any(), (name, r, c, ch.k)
    n_exhausted = sum(1 for ch in chains.values() if ch.status == sm.EXHAUSTED)
    print(f"{name} {W}x{H} max_specular {max_specular}: {n_chain} diffuse-ended chain pixels, longest {max(ks)}, {n_left_out} arrive inside glass, {n_exhausted} exhausted")
    assert n_chain >= least, n_chain
    assert n_left_out <= 0.02 * n_chain, (n_left_out, n_chain)
    if longest is not None:
        assert max(ks) == longest, max(ks)
    assert (n_exhausted > 0) == exhausted, n_exhausted
    # the planes say the same: plane 2 .w marks the diffuse ends, the code carries k
    code = planes[0, ..., 3]
    assert int(((planes[2, ..., 3] == 1) & (code >= 256)).sum()) == n_chain
    assert int(((planes[2, ..., 3] == 0) & (code >= 0)).sum()) == n_exhausted


def test_max_specular_0_is_the_first_hit(oracle):
    scene, materials, albedos = _scene("demo10", oracle, None)
    got = sm.oracle_aov_surface(scene, materials, albedos, 48, 32, 0)
    exp = dm.oracle_aov(scene, albedos, 48, 32)
    np.testing.assert_array_equal(got[:2].view(np.uint32), exp[:2].view(np.uint32))
    np.testing.assert_array_equal(got[2, ..., :3].view(np.uint32), exp[2, ..., :3].view(np.uint32))
    specular = np.isin(exp[0, ..., 3], [0, 1, 2, 3])
    assert specular.any() and not got[2, ..., 3][specular].any() and (got[2, ..., 3][~specular & (exp[0, ..., 3] >= 0)] == 1).all()


def test_path_codes_round_trip():
    seen = {}
    for k in range(16):
        for first in range(16):
            for oid in range(16):
                if k == 0 and first != oid:
                    continue                                         # without a chain the first hit is the recorded one
                code = sm.path_code(oid, first, k)
                assert 0 <= code <= 4095 and F(code) == code
                assert code not in seen, (code, seen.get(code), (oid, first, k))
                seen[code] = (oid, first, k)
                assert sm.decode_path(code) == (oid, first, k)
                assert rt.Context.decode_path(F(code)) == (oid, first, k)
                if k == 0:
                    assert code == oid
    assert len(seen) == 16 + 15 * 256
    assert rt.Context.decode_path(-1.0) == sm.decode_path(-1) == (-1, -1, 0)
    codes = np.array(sorted(seen), np.float32)
    i, f, k = rt.Context.decode_path(codes)
    assert [tuple(t) for t in zip(i.tolist(), f.tolist(), k.tolist())] == [seen[int(c)] for c in codes]


def _ulps(a, b):
    a = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


def test_demodulate_then_modulate_in_the_model():
    rng = np.random.default_rng(11)
    Hh, W = 31, 45
    color = rng.uniform(0.0, 4.0, (Hh, W, 4)).astype(np.float32)
    aov = np.zeros((3, Hh, W, 4), np.float32)
    aov[2, ..., :3] = np.exp(rng.uniform(np.log(1e-6), 0.0, (Hh, W, 3))).astype(np.float32)
    aov[2, ..., 3] = rng.integers(0, 2, (Hh, W))
    aov[2, 3, :, 0] = 0.0
    aov[2, 5, :, 1] = -0.25
    aov[2, 7, :, 2] = np.nan
    on = aov[2, ..., 3] == 1
    for floor in (0.0, 1e-3):
        d = sm.demodulate(color, aov, floor)
        back = sm.modulate(d, aov, floor)
        assert d.dtype == np.float32 and back.dtype == np.float32
        assert _ulps(back[..., :3], color[..., :3]).max() <= 2     # a correctly rounded quotient and a product: (1 + e1)(1 + e2), |e| <= 2^-24 each
        np.testing.assert_array_equal(back[..., 3], color[..., 3])
        np.testing.assert_array_equal(d[..., 3], color[..., 3])
        # the identity where plane 2 .w is 0 ...
        np.testing.assert_array_equal(d[~on].view(np.uint32), color[~on].view(np.uint32))
        np.testing.assert_array_equal(sm.modulate(color, aov, floor)[~on].view(np.uint32), color[~on].view(np.uint32))
        # ... and on a channel whose divisor is not > 0: a zero, a negative and a NaN albedo under floor 0; a floor lifts all three
        for row, ch in ((3, 0), (5, 1), (7, 2)):
            m = on[row]
            assert m.any()
            for f in (sm.demodulate, sm.modulate):
                same = f(color, aov, floor)[row, :, ch][m].view(np.uint32) == color[row, :, ch][m].view(np.uint32)
                assert same.all() if floor == 0.0 else not same.any(), (row, ch, floor)
        moved = on & (aov[2, ..., 0] > 0) & (aov[2, ..., 0] < 0.5)
        assert moved.any() and (d[..., 0][moved] > color[..., 0][moved]).all()
    # first-hit planes (plane 2 .w == 0 everywhere): both maps are the identity
    aov[2, ..., 3] = 0
    np.testing.assert_array_equal(sm.demodulate(color, aov).view(np.uint32), color.view(np.uint32))
    np.testing.assert_array_equal(sm.modulate(color, aov).view(np.uint32), color.view(np.uint32))

"""The generated scenes of tests/scene_fuzz.py on the CPU: the generator is reproducible, binary32-exact and finite; the oracle gives the reference's own frames on
them (tests/golden/ref_fuzz.npz, made by oracle/make_golden.py `fuzz` from the reference's Sphere, TriangleMesh, Scene and Scene::getColor); and the scenes reach the
branches they were written for, counted by the oracle's branch census (or_render_census) -- so that tests/test_gpu_scene_fuzz.py is not vacuous.

If a condition fails, the generator changes, never the bound."""
import numpy as np
import pytest

from . import scene_fuzz as sf
from .conftest import load_golden
from .denoise_model import oracle_aov

FIXTURE_SEEDS, FIXTURE_W, FIXTURE_H = range(8), 32, 24


def _flat(d):
    out = [d["spheres"], d["light"], d["cam"], d["pose"], np.array([d["eps"], d["tri_tmin"], d["sigma"]])]
    if d["mesh"] is not None:
        m = d["mesh"]
        out += [m["vertices"], m["albedo"], np.array([m["n_in"], m["n_out"]])]
    return out


@pytest.mark.parametrize("family", sf.FAMILIES)
def test_scene_is_reproducible_float32_exact_and_finite(family):
    small = 0
    for seed in sf.SEEDS:
        a, b = sf.scene(family, seed), sf.scene(family, seed)
        np.testing.assert_array_equal(sf.pack(a).view(np.uint32), sf.pack(b).view(np.uint32))
        assert a["tied"] == b["tied"] and (a["pose"] == b["pose"]).all()
        for x in _flat(a):
            assert x.dtype == np.float32 and np.isfinite(x).all(), (family, seed)
        assert a["sigma"] == 0 and 0 <= a["num_bounce"] <= 15 and len(a["spheres"]) + (a["mesh"] is not None) <= sf.MAX_OBJECTS
        assert (a["W"], a["H"]) in ((64, 48), (61, 43))
        small += (a["W"], a["H"]) == (61, 43)
        if a["mesh"] is not None:
            assert a["mesh"]["triangles"].dtype == np.int32 and 0 <= a["mesh"]["slot"] <= len(a["spheres"])
        if seed:
            assert (sf.pack(a).shape != sf.pack(sf.scene(family, seed - 1)).shape) or (sf.pack(a) != sf.pack(sf.scene(family, seed - 1))).any()
    assert 4 * small >= len(sf.SEEDS), f"{family}: {small} of {len(sf.SEEDS)} scenes are 61 x 43"


def _fixture_scene(family, seed):
    """as oracle/make_golden.py fuzz_scene: 32 x 24, one sample, the reference's own eps (a literal 1e-3 in Scene::getColor)"""
    return sf.resized(sf.scene(family, seed), FIXTURE_W, FIXTURE_H, spp=1, eps=1e-3)


@pytest.mark.parametrize("family", sf.FAMILIES)
def test_oracle_equals_the_reference_on_generated_scenes(oracle, family):
    g = load_golden("ref_fuzz.npz")
    for seed in FIXTURE_SEEDS:
        d = _fixture_scene(family, seed)
        np.testing.assert_array_equal(sf.pack(d).view(np.uint32), g[f"{family}_{seed}_desc"].view(np.uint32),
                                      err_msg=f"{family} {seed}: the generator no longer draws the scene the fixture holds (python oracle/make_golden.py fuzz)")
        got = sf.oracle_render(oracle, d, rng_mode=1, threads=1)[0][..., :3]
        ref = g[f"{family}_{seed}_frame"]
        differ = (got.view(np.uint32) != ref.view(np.uint32)) & ~(np.isnan(got) & np.isnan(ref))
        if differ.any():
            r, c, k = np.argwhere(differ)[0]
            pytest.fail(f"{family} seed {seed}: {int(differ.sum())} words differ, first at pixel ({r}, {c}) channel {k}: "
                        f"oracle {got.view(np.uint32)[r, c, k]:#010x} reference {ref.view(np.uint32)[r, c, k]:#010x}")


def test_census_does_not_touch_the_frame(oracle):
    d = sf.scene("glass", 3)
    s = sf.oracle_scene(oracle, d)
    a, work = sf.oracle_render(oracle, d, scene=s)
    b, cen = sf.oracle_render(oracle, d, scene=s, census=True, threads=1)
    c, cen4 = sf.oracle_render(oracle, d, scene=s, census=True, threads=4)
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    np.testing.assert_array_equal(a.view(np.uint32), c.view(np.uint32))
    assert cen == cen4 and "rays" in work and cen["diffuse"] > 0
    assert cen["lit"] + cen["shaded"] == cen["diffuse"]
    assert cen["last_segment"] <= d["W"] * d["H"] * d["spp"]


@pytest.fixture(scope="module")
def survey(oracle):
    """per family: the census summed over seeds 0 to 23, the number of dull scenes, and whether a frame holds a non-finite pixel or a negative channel"""
    out = {}
    for family in sf.FAMILIES:
        total, dull, odd = {}, 0, False
        for seed in sf.SEEDS:
            rgba, cen = sf.oracle_render(oracle, sf.scene(family, seed), census=True, threads=1)
            rgb = rgba[..., :3]
            dull += (rgb != 0).any(-1).mean() < 0.1
            odd |= bool((~np.isfinite(rgb)).any() or (rgb < 0).any())
            for k, v in cen.items():
                total[k] = total.get(k, 0) + v
        out[family] = (total, dull, odd)
    return out


@pytest.mark.parametrize("family", sf.FAMILIES)
def test_few_scenes_are_dull(survey, family):
    """dull = fewer than 10 % of the pixels have a non-zero colour: at most half of `light_edge` and `odd_spheres`, a quarter of every other family"""
    dull = survey[family][1]
    print(f"{family}: {dull} dull scenes of {len(sf.SEEDS)}")
    assert dull * (2 if family in ("light_edge", "odd_spheres") else 4) <= len(sf.SEEDS)


@pytest.mark.parametrize("family,least,events", [("open", 200, ("camera_miss", "shadow_miss")), ("ties", 200, ("equal_t",)),
                                                 ("glass", 200, ("total_reflection", "out2in", "in2out", "mirror")),
                                                 ("light_edge", 100, ("lit_mx_zero", "lit_l_bad", "shaded", "lit"))])
def test_census_shows_the_branches_a_family_is_for(survey, family, least, events):
    total = survey[family][0]
    print(family, {k: total[k] for k in events})
    for k in events:
        assert total[k] >= least, (family, k, total[k])


def test_glass_paths_reach_segment_16(oracle):
    """`last_segment` of the scenes with num_bounce = 15 alone: paths that traced their sixteenth segment (RT_MAX_SEGMENTS)"""
    n = 0
    for seed in sf.SEEDS:
        d = sf.scene("glass", seed)
        if d["num_bounce"] == 15:
            n += sf.oracle_render(oracle, d, census=True, threads=1)[1]["last_segment"]
    print("glass: paths that reached segment 16:", n)
    assert n >= 100


def test_tied_objects_decide_the_image(oracle):
    """in at least 4 scenes of `ties` the frame changes when the two coincident spheres trade places: the strict '<' of cpu:554 is what picks the material"""
    changed = 0
    for seed in sf.SEEDS:
        d = sf.scene("ties", seed)
        a, b = sf.oracle_render(oracle, d)[0], sf.oracle_render(oracle, sf.swapped(d))[0]
        changed += bool((a.view(np.uint32) != b.view(np.uint32)).any())
    print("ties: scenes whose frame depends on the order of the tied pair:", changed)
    assert changed >= 4


def test_camera_rays_hit_the_mesh_in_both_kinds_of_material(oracle):
    """`with_mesh`: at least 200 first hits on a diffuse mesh and 200 on a mirror or glass one, by the first-hit object id (denoise_model.oracle_aov)"""
    diffuse = specular = 0
    for seed in sf.SEEDS:
        d = sf.scene("with_mesh", seed)
        m = d["mesh"]
        n_obj = len(d["spheres"]) + 1
        ids = oracle_aov(sf.oracle_scene(oracle, d), np.zeros((n_obj, 3), np.float32), d["W"], d["H"], tri_tmin=float(d["tri_tmin"]), cam=d["cam"])[0, ..., 3]
        hits = int((ids == m["slot"]).sum())
        if m["mirror"] or m["n_in"] != m["n_out"]:
            specular += hits
        else:
            diffuse += hits
    print(f"with_mesh: first hits on a diffuse mesh {diffuse}, on a mirror or glass mesh {specular}")
    assert diffuse >= 200 and specular >= 200


def test_most_families_hold_a_non_finite_or_negative_frame(survey):
    """otherwise the 8-bit image check of the GPU test sees nothing the preset scenes do not show"""
    odd = [f for f in sf.FAMILIES if survey[f][2]]
    print("families with a non-finite pixel or a negative channel:", odd)
    assert len(odd) >= 5

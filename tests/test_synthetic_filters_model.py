"""The synthetic planes of tests/synthetic_planes.py on the CPU, before the device sees them (tests/test_gpu_synthetic_filters.py):

  * the vectorised models (denoise_model, temporal_model) against the scalar reference written from the header (scalar_filter_reference), bit for bit, on every
    small case -- `taps` of accumulate included;
  * the feature counts: every case the device is held to reaches the branches it is meant to reach, by the models' own stats= (the minimums are conditions on the
    inputs, stated in synthetic_planes.py);
  * the mutants: every plausible fault of a kernel that scalar_filter_reference can imitate changes the bits of at least one of those cases (on a crop where the
    full frame is too slow for scalar code)."""
import numpy as np
import pytest

import raytracinggpu_amd as rt
from raytracinggpu_amd import _capi
from . import denoise_model as dm
from . import scalar_filter_reference as ref
from . import synthetic_planes as sp
from . import temporal_model as tm

NAMES = ("k_normal", "k_position", "k_albedo", "k_color")
VAR_NAMES = ("k_normal", "k_position", "k_albedo", "k_sigma", "var_floor")
FILTER = sp.filter_gpu_cases()
TEMPORAL = sp.temporal_gpu_cases(rt.make_pose)
CROP = (56, 136, 34, 94)                                               # of the 160 x 120 arithmetic frames: 80 x 60 around the corner where the four mega blocks meet


def plain_k(kw):
    return [float(np.float32(dict(_capi.DENOISE_DEFAULTS, **kw)[n])) for n in NAMES]


def var_k(kw):
    return [float(np.float32(dict(_capi.DENOISE_VAR_DEFAULTS, **kw)[n])) for n in VAR_NAMES]


def f32(kw):
    return {k: (float(np.float32(v)) if k in ("alpha_min", "min_normal_dot", "max_plane_dist") else v) for k, v in kw.items()}


def same_bits(a, b, msg=""):
    """bit for bit; where a NaN is concerned: NaN in the same places (its sign and payload are not part of the contract)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b), err_msg=msg + ": NaN in other places")
    np.testing.assert_array_equal(np.where(np.isnan(a), 0, a.view(np.uint32)), np.where(np.isnan(b), 0, b.view(np.uint32)), err_msg=msg)


def differ(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return bool(((a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))).any())


# ---------------------------------------------------------------- the models against the scalar reference ----------------------------------------------------------------
def small_filter_cases():
    out = []
    for name, (build, passes, plain, var, _) in FILTER.items():
        if name in sp.FILTER_CASES:
            W, H = sp.FILTER_CASES[name][:2]
            if W * H <= 4300:
                out.append((name, build, max(passes), plain, var))
        elif name.startswith("arithmetic:"):
            out.append((name, lambda build=build: sp.crop(build(), *CROP), 2, plain, var))
        else:
            out.append((name, lambda: sp.nonfinite_filter_case(72, 48, 12), max(passes), plain, var))
    return out


@pytest.mark.parametrize("name,build,n,plain,var", small_filter_cases(), ids=[c[0] for c in small_filter_cases()])
def test_filter_models_equal_the_scalar_reference(name, build, n, plain, var):
    p = build()
    if plain is not None:
        same_bits(dm.denoise(p["color"], p["aov"], n, *plain_k(plain)), ref.denoise(p["color"], p["aov"], n, *plain_k(plain)), f"rt_denoise, {name}")
    if var is not None:
        same_bits(tm.denoise_var(p["history"], p["aov"], n, *var_k(var)), ref.denoise_var(p["history"], p["aov"], n, *var_k(var)), f"rt_denoise_var, {name}")


def small_temporal_cases():
    out = []
    for name, (build, kw, _) in TEMPORAL.items():
        if name.startswith("96x64:") or name == "depths":
            out.append((name, build, kw))
        elif name.startswith("arithmetic:"):
            out.append((name, lambda build=build: sp.crop(build(), *CROP), kw))
    return out


@pytest.mark.parametrize("name,build,kw", small_temporal_cases(), ids=[c[0] for c in small_temporal_cases()])
def test_accumulate_model_equals_the_scalar_reference(name, build, kw):
    c = build()
    kw = f32(kw(c))
    for prev in ((c["prev_aov"], c["prev_history"]), (None, None)):
        ta, tb = {}, {}
        a = tm.accumulate(c["color"], c["aov"], *prev, taps=ta, **kw)
        b = ref.accumulate(c["color"], c["aov"], *prev, taps=tb, **kw)
        same_bits(a, b, f"rt_temporal_accumulate, {name}")
        np.testing.assert_array_equal(ta["q"], tb["q"])
        if name.startswith("arithmetic:") or name == "depths":
            assert np.isfinite(a).all()                                # "built so that the plain arithmetic stays finite"


# ---------------------------------------------------------------- the feature counts of the device's cases ----------------------------------------------------------------
@pytest.mark.parametrize("name", list(FILTER))
def test_filter_cases_reach_their_branches(name):
    build, passes, plain, var, finite = FILTER[name]
    p = build()
    n = max(passes)
    runs = []
    if plain is not None:
        st = {}
        runs.append(("rt_denoise", dm.denoise(p["color"], p["aov"], n, *plain_k(plain), stats=st), st))
    if var is not None:
        st = {}
        runs.append(("rt_denoise_var", tm.denoise_var(p["history"], p["aov"], n, *var_k(var), stats=st), st))
    for entry, out, st in runs:
        print(name, entry, st)
        if finite:
            assert np.isfinite(out).all(), (name, entry)
        else:
            assert 0 < np.isnan(out).sum() < sp.NAN_CHANNEL_CAP * out.size, (name, entry, int(np.isnan(out).sum()))
        if name in sp.FILTER_CASES:
            _, _, _, far_x, far_y, seam = sp.FILTER_CASES[name]
            for s in (32, 64, 128):
                if s in far_x:
                    assert st[s]["far_x"] >= sp.FILTER_MINIMUM, (name, entry, s)
                if s in far_y:
                    assert st[s]["far_y"] >= sp.FILTER_MINIMUM, (name, entry, s)
                if s in far_x or s in far_y:
                    assert st[s]["dropped_by_id"] >= sp.FILTER_MINIMUM, (name, entry, s)
            if seam:
                assert sum(v["across_seam"] for v in st.values()) >= sp.SEAM_MINIMUM, (name, entry)
            if far_x and name != "517x389":                            # two tiles per sub-image at step 128: taps cross that seam too
                assert st[128]["across_seam"] >= sp.SEAM_MINIMUM
            if far_y and name != "517x389":
                assert st[128]["across_seam"] >= sp.SEAM_MINIMUM
        if name.startswith("arithmetic:"):
            assert max(v["literal"] for v in st.values()) >= sp.ARITHMETIC_MINIMUM, (name, entry)
            assert max(v["shared"] for v in st.values()) >= sp.ARITHMETIC_MINIMUM, (name, entry)
    if name == "arithmetic:only_centre":                              # every neighbour's weight is 0: each pixel is (9/64 C) / (9/64)
        hit = p["ids"] != -1
        c = p["color"][hit][:, :3]
        with np.errstate(all="ignore"):
            np.testing.assert_array_equal(runs[0][1][hit][:, :3], (dm.F(0.140625) * c) / dm.F(0.140625))
    if name == "arithmetic:variances":                                # D == 0 beside unequal luminances: dl2 / 0 = +Inf, a weight of 0, nothing else
        V = p["history"][1, ..., 3]
        assert (V == 0).sum() > 1000 and ((V > 0) & (V < 1e-38)).sum() > 1000 and (V > 1e29).sum() > 1000


def test_reprojection_cases_reach_their_branches():
    build, kw, _ = TEMPORAL["517x389:movers"]
    c = build()
    assert set(np.unique(c["ids"])) >= set(range(16))                  # all 16 ids: motion record 15 and mask bit 15 are in use
    st = {}
    out = tm.accumulate(c["color"], c["aov"], c["prev_aov"], c["prev_history"], stats=st, **f32(kw(c)))
    print(st)
    assert np.isfinite(out).all()
    for key, least in sp.REPROJECTION_MINIMUMS.items():
        assert st[key] >= least, (key, st[key])
    for n in (2.0, 3.0, 4.0, 31.0, 32.0, 3.5):                         # 3.5: from the non-integer n_q = 2.5
        assert st["n"][n] >= sp.N_MINIMUM, (n, st["n"])
    ph_n = c["prev_history"][1, ..., 2]
    taps = {}
    tm.accumulate(c["color"], c["aov"], c["prev_aov"], c["prev_history"], taps=taps, **f32(kw(c)))
    q = taps["q"]
    took = q[..., 0] >= 0
    from_n = ph_n[q[..., 1][took], q[..., 0][took]]
    assert (from_n == 32).sum() >= sp.N_MINIMUM and (from_n == 40).sum() >= sp.N_MINIMUM and (from_n == 31).sum() >= sp.N_MINIMUM   # the clamp from n_q = max and above
    on15 = c["ids"] == 15
    ys, xs = np.meshgrid(np.arange(c["ids"].shape[0]), np.arange(c["ids"].shape[1]), indexing="ij")
    assert (took & on15 & (q[..., 0] == xs + 2) & (q[..., 1] == ys + 1)).sum() >= 200   # the mover follows its record
    # 15 masked: none of its pixels reuses history
    st_m = {}
    m = tm.accumulate(c["color"], c["aov"], c["prev_aov"], c["prev_history"], stats=st_m, **f32(TEMPORAL["517x389:masked"][1](c)))
    assert on15.sum() >= 200 and (m[1, ..., 2][on15] == 1).all() and (out[1, ..., 2][on15] > 1).sum() >= 200
    # the other cameras, the shorter memories and the floor under the blend weight: at least 200 reprojected pixels each
    for name in ("posed", "fixed_elsewhere", "no_motion_table", "max_history=1", "max_history=2", "alpha_min=0.4", "alpha_min=0.4,max_history=2", "nonfinite_history"):
        build_n, kw_n, finite = TEMPORAL["517x389:" + name]
        cn = build_n()
        s = {}
        o = tm.accumulate(cn["color"], cn["aov"], cn["prev_aov"], cn["prev_history"], stats=s, **f32(kw_n(cn)))
        print(name, s)
        assert s["reprojected"] >= 200, name
        if name.startswith("alpha_min=0.4"):
            assert s["alpha_min_below"] >= 200 and (s["alpha_min_above"] >= 200 or "max_history" in name), (name, s)   # (with max_history 2: 1 / n = 0.5 > 0.4 always)
        if name.startswith("max_history="):
            assert s["n"][float(name[-1])] >= 200
        if finite:
            assert np.isfinite(o).all(), name
        else:
            assert 0 < np.isnan(o).sum() < sp.NAN_CHANNEL_CAP * o.size
    s = {}
    cd = TEMPORAL["depths"][0]()
    o = tm.accumulate(cd["color"], cd["aov"], cd["prev_aov"], cd["prev_history"], stats=s, **f32(TEMPORAL["depths"][1](cd)))
    assert np.isfinite(o).all() and s["literal"] >= sp.ARITHMETIC_MINIMUM and s["shared"] >= sp.ARITHMETIC_MINIMUM, s


# ---------------------------------------------------------------- the mutants ----------------------------------------------------------------
def _filter_mutant(case, mutant, n, var=False, box=None, **kw):
    build, _, plain, vark, _ = FILTER[case]
    p = build() if box is None else sp.crop(build(), *box)
    if var:
        k = var_k(dict(vark, **kw))
        return ref.denoise_var(p["history"], p["aov"], n, *k), ref.denoise_var(p["history"], p["aov"], n, *k, mutant=mutant)
    k = plain_k(dict(plain, **kw))
    return ref.denoise(p["color"], p["aov"], n, *k), ref.denoise(p["color"], p["aov"], n, *k, mutant=mutant)


def _temporal_mutant(case, mutant):
    build, kw, _ = TEMPORAL[case]
    c = build()
    args = (c["color"], c["aov"], c["prev_aov"], c["prev_history"])
    return ref.accumulate(*args, **f32(kw(c))), ref.accumulate(*args, mutant=mutant, **f32(kw(c)))


MUTANT_CASES = {
    "halo1": lambda m: _filter_mutant("4200x24", m, 6, box=(0, 140, 0, 16)),                    # step 32: the taps 64 pixels away are inside the crop
    "dx_outer": lambda m: _filter_mutant("64x16", m, 1),
    "half_gt": lambda m: _temporal_mutant("96x64:movers", m),
    "gx_lt_width": lambda m: _temporal_mutant("96x64:movers", m),
    "tap_order": lambda m: _temporal_mutant("96x64:movers", m),
    "no_clamp": lambda m: _temporal_mutant("96x64:movers", m),
    "no_alpha_min": lambda m: _temporal_mutant("96x64:alpha_min=0.4", m),
    "n_le_4": lambda m: _temporal_mutant("96x64:movers", m),
    "var_lag": lambda m: _filter_mutant("129x33", m, 3, var=True),
    "div_seq": lambda m: _filter_mutant("arithmetic:denormal", m, 1, var=True, box=CROP),
    "k_color_unscaled": lambda m: _filter_mutant("129x33", m, 2),
    "w_ge_0": lambda m: _filter_mutant("nonfinite", m, 1, box=(0, 100, 0, 40)),
}


def test_the_mutants_are_the_listed_ones():
    assert set(MUTANT_CASES) == set(ref.MUTANTS)


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_each_mutant_changes_a_device_case(mutant):
    plain, mutated = MUTANT_CASES[mutant](mutant)
    assert differ(plain, mutated), mutant

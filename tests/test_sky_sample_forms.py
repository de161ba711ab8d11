"""Which form of wf_advance a launch runs once the chain's facts include sky sampling (csrc/rt_still.h adv_form; the host library's rth_advance_form_sky_sample): every
combination of (counting, tex, anim, list, lens, lights, shutter) with sky = 1 and sample = 1 at all five steps against a table, and with sample = 0 against the entry that
does not know the fact.

The opening launch is what it was; every later launch carries the sky bit, the sample bit and -- whatever the lights are -- the soft lights' table: two forms.  What the
environment refuses, sampling refuses; sampling without an environment is never asked for."""
import itertools

import pytest

from raytracinggpu_amd import hostlib

STATS, FIRST, TEX, ANIM, LIST, FILL, RESUME, LIGHTS, SOFT, LENS, CLOSE, SHUTTER, SKY, SAMPLE = (1 << k for k in range(14))
BEGIN, ADV_RESUME, PLAIN, ADV_FILL, ADV_CLOSE = range(5)                # rtk::StillAdv
NO = None
TABLE = {(0, tex, 0, 0, lens, lights, 0): (FIRST | (LENS if lens else 0), NO, (TEX if tex else 0) | SOFT | SKY | SAMPLE, NO, NO)
         for tex in (0, 1) for lens in (0, 1) for lights in (0, 1, 2)}
BUILT = {SOFT | SKY | SAMPLE, TEX | SOFT | SKY | SAMPLE}
FACTS = list(itertools.product((0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1, 2), (0, 1)))
STEPS = [BEGIN, ADV_RESUME, PLAIN, ADV_FILL, ADV_CLOSE]


def test_table_covers_the_two_forms():
    assert len(FACTS) == 192 and len(TABLE) == 12 and SAMPLE == 1 << 13
    asked = {f for row in TABLE.values() for f in row if f is not NO}
    assert {f for f in asked if f & SAMPLE} == BUILT
    assert {f for f in asked if not f & SAMPLE} == {FIRST, FIRST | LENS}


@pytest.mark.parametrize("adv", STEPS, ids=["opening", "resume", "plain", "fill", "close"])
def test_form_of_every_combination_with_sampling_on(adv):
    wrong = []
    for facts in FACTS:
        want = TABLE.get(facts, (NO,) * 5)[adv]
        got = hostlib.advance_form(*facts[:6], adv, shutter=facts[6], sky=1, sample=1)
        if got != want:
            wrong.append((facts, want, got))
    assert not wrong, wrong


def test_without_sampling_the_answers_are_the_existing_function_and_sampling_needs_the_environment():
    for facts in FACTS:
        for adv in STEPS + [5, -1]:
            for sky in (0, 1):
                a = hostlib.advance_form(*facts[:6], adv, shutter=facts[6], sky=sky, sample=0)
                assert a == hostlib.advance_form(*facts[:6], adv, shutter=facts[6], sky=sky), (facts, adv, sky)
                assert a is NO or not a & SAMPLE
            assert hostlib.advance_form(*facts[:6], adv, shutter=facts[6], sky=0, sample=1) is NO


def test_the_tools_know_the_two_forms():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    try:
        import advance_forms
    finally:
        sys.path.pop(0)
    assert advance_forms.BITS["sample"] == SAMPLE
    assert set(advance_forms.SKY_SAMPLE_FORMS) == BUILT and len(advance_forms.FORMS) == 25 and len(advance_forms.ALL_FORMS) == 29
    assert BUILT.isdisjoint(advance_forms.ALL_FORMS)
    name = "void rtk::wf_advance<12548u, rtk::TexScene, rtk::WfSoftLights, rtk::WfSky, rtk::WfSkyDist>(rtk::Scene, rtk::Frame, rtk::WfState, rtk::TexScene, rtk::WfSoftLights, rtk::WfSky, rtk::WfSkyDist)"
    assert advance_forms.form_of(name) == TEX | SOFT | SKY | SAMPLE


def test_static_counts_name_the_two_kernels():
    import json
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    keys = json.load(open(os.path.join(root, "raytracinggpu_amd", "static_counts.json")))
    for k in ("wf_advance_soft_sky_sample", "wf_advance_tex_soft_sky_sample"):
        assert keys[k]["whole_kernel"]["valu"] > keys[k.replace("_sample", "")]["whole_kernel"]["valu"], k     # the draw is in it

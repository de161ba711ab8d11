"""Which form of wf_advance a launch runs once the chain's facts include a mirror with an effective roughness (csrc/rt_still.h adv_form; the host library's
rth_advance_form_gloss): every combination of the eleven older facts (counting, tex, anim, list, lens, lights, shutter, sky, sample, emit, fresnel) with gloss = 1 at
all five steps against a Python restatement, and with gloss = 0 against the entry that does not know the fact.

The opening launch is what it was, the lens included; every later launch carries the gloss bit, and the soft lights' table where the scene holds a light list or a
radius: four forms.  Counting, a list, an animated batch, the shutter, an environment, sky sampling, an emitter and an effective Fresnel flag have no form with a
roughness; neither have the still view's fill and resume, nor the closing kernel."""
import itertools

import pytest

from raytracinggpu_amd import hostlib

STATS, FIRST, TEX, ANIM, LIST, FILL, RESUME, LIGHTS, SOFT, LENS, CLOSE, SHUTTER, SKY, SAMPLE, EMIT, FRESNEL, GLOSS = (1 << k for k in range(17))
BEGIN, ADV_RESUME, PLAIN, ADV_FILL, ADV_CLOSE = range(5)                # rtk::StillAdv
NO = None
BUILT = {GLOSS, TEX | GLOSS, SOFT | GLOSS, TEX | SOFT | GLOSS}
FACTS = list(itertools.product((0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1, 2), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1)))
STEPS = [BEGIN, ADV_RESUME, PLAIN, ADV_FILL, ADV_CLOSE]


def _want(facts, adv):
    """the rule, restated"""
    counting, tex, anim, list_, lens, lights, shutter, sky, sample, emit, fresnel = facts
    if counting or anim or list_ or shutter or sky or sample or emit or fresnel:
        return NO
    if adv == BEGIN:
        return FIRST | (LENS if lens else 0)
    if adv == PLAIN:
        return (TEX if tex else 0) | (SOFT if lights else 0) | GLOSS
    return NO


def _form(facts, adv, gloss):
    return hostlib.advance_form(*facts[:6], adv, shutter=facts[6], sky=facts[7], sample=facts[8], emit=facts[9], fresnel=facts[10], gloss=gloss)


def test_the_restatement_asks_for_exactly_the_four_forms():
    assert len(FACTS) == 3072 and GLOSS == 1 << 16
    asked = {_want(f, adv) for f in FACTS for adv in STEPS} - {NO}
    assert {f for f in asked if f & GLOSS} == BUILT
    assert {f for f in asked if not f & GLOSS} == {FIRST, FIRST | LENS}


@pytest.mark.parametrize("adv", STEPS, ids=["opening", "resume", "plain", "fill", "close"])
def test_form_of_every_combination_with_a_roughness(adv):
    wrong = [(facts, _want(facts, adv), _form(facts, adv, 1)) for facts in FACTS if _form(facts, adv, 1) != _want(facts, adv)]
    assert not wrong, wrong


def test_exactly_the_four_forms_are_built():
    got = {_form(facts, adv, 1) for facts in FACTS for adv in STEPS + [5, -1]} - {NO}
    assert {f for f in got if f & GLOSS} == BUILT
    for facts in FACTS:
        assert _form(facts, ADV_RESUME, 1) is NO and _form(facts, ADV_FILL, 1) is NO and _form(facts, ADV_CLOSE, 1) is NO, facts


def test_without_a_roughness_the_answers_are_the_existing_function():
    for facts in FACTS:
        for adv in STEPS + [5, -1]:
            a = _form(facts, adv, 0)
            assert a == hostlib.advance_form(*facts[:6], adv, shutter=facts[6], sky=facts[7], sample=facts[8], emit=facts[9], fresnel=facts[10]), (facts, adv)
            assert a is NO or not a & GLOSS


def test_the_tools_know_the_four_forms():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    try:
        import advance_forms
    finally:
        sys.path.pop(0)
    assert advance_forms.BITS["gloss"] == GLOSS
    assert set(advance_forms.GLOSS_FORMS) == BUILT and len(advance_forms.GLOSS_FORMS) == 4
    assert len(advance_forms.FORMS) == 25 and len(advance_forms.ALL_FORMS) == 29
    for older in (advance_forms.FORMS, advance_forms.SKY_FORMS, advance_forms.ALL_FORMS, advance_forms.SKY_SAMPLE_FORMS, advance_forms.EMISSION_FORMS,
                  advance_forms.FRESNEL_FORMS):
        assert BUILT.isdisjoint(older)
    name = "void rtk::wf_advance<65796u, rtk::TexScene, rtk::WfSoftLights, rtk::WfGloss>(rtk::Scene, rtk::Frame, rtk::WfState, rtk::TexScene, rtk::WfSoftLights, rtk::WfGloss)"
    assert advance_forms.form_of(name) == TEX | SOFT | GLOSS
    assert advance_forms.form_of("void rtk::wf_advance<65536u, rtk::WfGloss>(rtk::Scene, rtk::Frame, rtk::WfState, rtk::WfGloss)") == GLOSS


def test_static_counts_name_the_four_kernels():
    import json
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    keys = json.load(open(os.path.join(root, "raytracinggpu_amd", "static_counts.json")))
    # the facet and the two draws are in each (the textured plain form has no entry of its own in the table: against the untextured gloss form)
    for k, base in (("wf_advance_gloss", "wf_advance"), ("wf_advance_tex_gloss", "wf_advance_gloss"), ("wf_advance_soft_gloss", "wf_advance_soft"),
                    ("wf_advance_tex_soft_gloss", "wf_advance_tex_soft")):
        assert keys[k]["whole_kernel"]["valu"] > keys[base]["whole_kernel"]["valu"], k

"""Which form of wf_advance a launch runs once the chain's facts include an effectively tinted object (csrc/rt_still.h adv_form; the host library's
rth_advance_form_tint): every combination of the twelve older facts (counting, tex, anim, list, lens, lights, shutter, sky, sample, emit, fresnel, gloss) with tint = 1
at all five steps against a Python restatement, and with tint = 0 against the entry that does not know the fact.

The opening launch is what it was, the lens included; every later launch carries the tint bit AND the gloss bit, whether a mirror of the scene is rough or not (the
gloss arm is compiled in and its mask may be empty), and the soft lights' table where the scene holds a light list or a radius: four forms.  Counting, a list, an
animated batch, the shutter, an environment, sky sampling, an emitter and an effective Fresnel flag have no form with a tint; neither have the still view's fill and
resume, nor the closing kernel."""
import itertools

import pytest

from raytracinggpu_amd import hostlib

STATS, FIRST, TEX, ANIM, LIST, FILL, RESUME, LIGHTS, SOFT, LENS, CLOSE, SHUTTER, SKY, SAMPLE, EMIT, FRESNEL, GLOSS, TINT = (1 << k for k in range(18))
BEGIN, ADV_RESUME, PLAIN, ADV_FILL, ADV_CLOSE = range(5)                # rtk::StillAdv
NO = None
BUILT = {GLOSS | TINT, TEX | GLOSS | TINT, SOFT | GLOSS | TINT, TEX | SOFT | GLOSS | TINT}
FACTS = list(itertools.product((0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1, 2), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1)))
STEPS = [BEGIN, ADV_RESUME, PLAIN, ADV_FILL, ADV_CLOSE]


def _want(facts, adv):
    """the rule, restated"""
    counting, tex, anim, list_, lens, lights, shutter, sky, sample, emit, fresnel, gloss = facts
    if counting or anim or list_ or shutter or sky or sample or emit or fresnel:
        return NO
    if adv == BEGIN:
        return FIRST | (LENS if lens else 0)
    if adv == PLAIN:
        return (TEX if tex else 0) | (SOFT if lights else 0) | GLOSS | TINT
    return NO


def _kw(facts):
    return dict(shutter=facts[6], sky=facts[7], sample=facts[8], emit=facts[9], fresnel=facts[10], gloss=facts[11])


def _form(facts, adv, tint):
    return hostlib.advance_form(*facts[:6], adv, tint=tint, **_kw(facts))


def test_the_restatement_asks_for_exactly_the_four_forms():
    assert len(FACTS) == 6144 and TINT == 1 << 17
    asked = {_want(f, adv) for f in FACTS for adv in STEPS} - {NO}
    assert {f for f in asked if f & TINT} == BUILT
    assert {f for f in asked if not f & TINT} == {FIRST, FIRST | LENS}


@pytest.mark.parametrize("adv", STEPS, ids=["opening", "resume", "plain", "fill", "close"])
def test_form_of_every_combination_with_a_tint(adv):
    wrong = [(facts, _want(facts, adv), _form(facts, adv, 1)) for facts in FACTS if _form(facts, adv, 1) != _want(facts, adv)]
    assert not wrong, wrong[:8]


def test_exactly_the_four_forms_are_built_each_with_the_gloss_arm():
    got = {_form(facts, adv, 1) for facts in FACTS for adv in STEPS + [5, -1]} - {NO}
    assert {f for f in got if f & TINT} == BUILT
    assert all(f & GLOSS for f in BUILT)
    for facts in FACTS:
        assert _form(facts, ADV_RESUME, 1) is NO and _form(facts, ADV_FILL, 1) is NO and _form(facts, ADV_CLOSE, 1) is NO, facts
    # a rough mirror beside the tint changes no form: the mask is an argument, not a kernel
    for facts in FACTS:
        if not facts[11]:
            assert _form(facts, PLAIN, 1) == _form(facts[:11] + (1,), PLAIN, 1), facts


def test_without_a_tint_the_answers_are_the_existing_function():
    for facts in FACTS:
        for adv in STEPS + [5, -1]:
            a = _form(facts, adv, 0)
            assert a == hostlib.advance_form(*facts[:6], adv, **_kw(facts)), (facts, adv)     # rth_advance_form_gloss
            assert a is NO or not a & TINT
    # ... and the gloss entry answers what it answered (tests/test_gloss_forms.py holds every combination; one of each kind here)
    assert hostlib.advance_form(0, 1, 0, 0, 0, 2, PLAIN, gloss=1) == TEX | SOFT | GLOSS
    assert hostlib.advance_form(0, 0, 0, 0, 0, 0, PLAIN, gloss=0) == 0


def test_the_tools_know_the_four_forms():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    try:
        import advance_forms
    finally:
        sys.path.pop(0)
    assert advance_forms.BITS["tint"] == TINT
    assert set(advance_forms.TINT_FORMS) == BUILT and len(advance_forms.TINT_FORMS) == 4
    assert len(advance_forms.FORMS) == 25 and len(advance_forms.ALL_FORMS) == 29
    for older in (advance_forms.FORMS, advance_forms.SKY_FORMS, advance_forms.ALL_FORMS, advance_forms.SKY_SAMPLE_FORMS, advance_forms.EMISSION_FORMS,
                  advance_forms.FRESNEL_FORMS, advance_forms.GLOSS_FORMS):
        assert BUILT.isdisjoint(older)
    name = ("void rtk::wf_advance<196868u, rtk::TexScene, rtk::WfSoftLights, rtk::WfGloss, rtk::WfTint>(rtk::Scene, rtk::Frame, rtk::WfState, rtk::TexScene, "
            "rtk::WfSoftLights, rtk::WfGloss, rtk::WfTint)")
    assert advance_forms.form_of(name) == TEX | SOFT | GLOSS | TINT
    assert advance_forms.form_of("void rtk::wf_advance<196608u, rtk::WfGloss, rtk::WfTint>(rtk::Scene, rtk::Frame, rtk::WfState, rtk::WfGloss, rtk::WfTint)") == GLOSS | TINT
    assert advance_forms.describe(GLOSS | TINT) == "wf_advance<gloss | tint>"


def test_static_counts_name_the_four_kernels():
    import json
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    keys = json.load(open(os.path.join(root, "raytracinggpu_amd", "static_counts.json")))
    # the mask test, the two stores and the dead-channel byte are in each: more vector instructions than the gloss counterpart, and far fewer than a facet's 385
    for k, base in (("wf_advance_gloss_tint", "wf_advance_gloss"), ("wf_advance_tex_gloss_tint", "wf_advance_tex_gloss"),
                    ("wf_advance_soft_gloss_tint", "wf_advance_soft_gloss"), ("wf_advance_tex_soft_gloss_tint", "wf_advance_tex_soft_gloss")):
        more = keys[k]["whole_kernel"]["valu"] - keys[base]["whole_kernel"]["valu"]
        assert 0 < more < 385, (k, more)
    assert sum(1 for k in keys if k.endswith("_tint")) == 4

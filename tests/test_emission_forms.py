"""Which form of wf_advance a launch runs once the chain's facts include an emitting mesh (csrc/rt_still.h adv_form; the host library's rth_advance_form_emit): every
combination of (counting, tex, anim, list, lens, lights, shutter, sky, sample) with emit = 1 at all five steps against a table, and with emit = 0 against the entry that
does not know the fact.

The opening launch is what it was; every later launch carries the emit bit and -- whatever the lights are -- the soft lights' table: two forms.  An environment, sky
sampling, the shutter, counting, a list and an animated batch have no form with an emitter."""
import itertools

import pytest

from raytracinggpu_amd import hostlib

STATS, FIRST, TEX, ANIM, LIST, FILL, RESUME, LIGHTS, SOFT, LENS, CLOSE, SHUTTER, SKY, SAMPLE, EMIT = (1 << k for k in range(15))
BEGIN, ADV_RESUME, PLAIN, ADV_FILL, ADV_CLOSE = range(5)                # rtk::StillAdv
NO = None
# (counting, tex, anim, list, lens, lights, shutter, sky, sample) -> the forms of the five steps
TABLE = {(0, tex, 0, 0, lens, lights, 0, 0, 0): (FIRST | (LENS if lens else 0), NO, (TEX if tex else 0) | SOFT | EMIT, NO, NO)
         for tex in (0, 1) for lens in (0, 1) for lights in (0, 1, 2)}
BUILT = {SOFT | EMIT, TEX | SOFT | EMIT}
FACTS = list(itertools.product((0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1, 2), (0, 1), (0, 1), (0, 1)))
STEPS = [BEGIN, ADV_RESUME, PLAIN, ADV_FILL, ADV_CLOSE]


def _form(facts, adv, emit):
    return hostlib.advance_form(*facts[:6], adv, shutter=facts[6], sky=facts[7], sample=facts[8], emit=emit)


def test_table_covers_the_two_forms():
    assert len(FACTS) == 768 and len(TABLE) == 12 and EMIT == 1 << 14
    asked = {f for row in TABLE.values() for f in row if f is not NO}
    assert {f for f in asked if f & EMIT} == BUILT
    assert {f for f in asked if not f & EMIT} == {FIRST, FIRST | LENS}


@pytest.mark.parametrize("adv", STEPS, ids=["opening", "resume", "plain", "fill", "close"])
def test_form_of_every_combination_with_an_emitter(adv):
    wrong = []
    for facts in FACTS:
        want = TABLE.get(facts, (NO,) * 5)[adv]
        got = _form(facts, adv, 1)
        if got != want:
            wrong.append((facts, want, got))
    assert not wrong, wrong


def test_the_refused_combinations_are_not_built():
    """an emitter with an environment, sky sampling, the shutter, counting, a list or an animated batch: no step of the chain has a form"""
    for facts in FACTS:
        counting, _, anim, list_, _, _, shutter, sky, sample = facts
        if counting or anim or list_ or shutter or sky or sample:
            assert all(_form(facts, adv, 1) is NO for adv in STEPS), facts


def test_without_an_emitter_the_answers_are_the_existing_function():
    for facts in FACTS:
        for adv in STEPS + [5, -1]:
            a = _form(facts, adv, 0)
            assert a == hostlib.advance_form(*facts[:6], adv, shutter=facts[6], sky=facts[7], sample=facts[8]), (facts, adv)
            assert a is NO or not a & EMIT


def test_the_tools_know_the_two_forms():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    try:
        import advance_forms
    finally:
        sys.path.pop(0)
    assert advance_forms.BITS["emit"] == EMIT
    assert set(advance_forms.EMISSION_FORMS) == BUILT and len(advance_forms.FORMS) == 25 and len(advance_forms.ALL_FORMS) == 29
    assert BUILT.isdisjoint(advance_forms.ALL_FORMS) and BUILT.isdisjoint(advance_forms.SKY_SAMPLE_FORMS)
    name = "void rtk::wf_advance<16644u, rtk::TexScene, rtk::WfSoftLights, rtk::WfEmit>(rtk::Scene, rtk::Frame, rtk::WfState, rtk::TexScene, rtk::WfSoftLights, rtk::WfEmit)"
    assert advance_forms.form_of(name) == TEX | SOFT | EMIT


def test_static_counts_name_the_two_kernels():
    import json
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    keys = json.load(open(os.path.join(root, "raytracinggpu_amd", "static_counts.json")))
    for k in ("wf_advance_soft_emit", "wf_advance_tex_soft_emit"):
        assert keys[k]["whole_kernel"]["valu"] > keys[k.replace("_emit", "")]["whole_kernel"]["valu"], k     # the draw is in it

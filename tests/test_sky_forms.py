"""Which form of wf_advance a launch runs once the chain's facts include the environment (csrc/rt_still.h adv_form; the host library's rth_advance_form_sky, the entry
that takes the fact that came after the shutter): every combination of (counting, tex, anim, list, lens, lights, shutter) with sky = 1 at all five steps against a table,
and with sky = 0 against the entries that do not know the fact.

A ray meets the environment where it is closed, so the opening launch is what it was and every later launch carries the bit.  Four forms are built: with and without
textures, with and without the soft lights' table -- a light list without a radius goes through the soft forms with radii 0.  Counting, a list, an animated batch and the
shutter refuse the environment (lights_refuse); a sky chain knows no still view (no fill, no resume) and is not a plain chain (no closing kernel)."""
import itertools

import pytest

from raytracinggpu_amd import hostlib

STATS, FIRST, TEX, ANIM, LIST, FILL, RESUME, LIGHTS, SOFT, LENS, CLOSE, SHUTTER, SKY = (1 << k for k in range(13))
BEGIN, ADV_RESUME, PLAIN, ADV_FILL, ADV_CLOSE = range(5)                # rtk::StillAdv
NO = None


def _row(tex, lens, lights):
    later = (TEX if tex else 0) | (SOFT if lights else 0) | SKY
    return (FIRST | (LENS if lens else 0), NO, later, NO, NO)


# (counting, tex, anim, list, lens, lights, shutter) with the environment on -> (opening, resume, plain, fill, close).  Every combination that is not a row is never asked for.
TABLE = {(0, tex, 0, 0, lens, lights, 0): _row(tex, lens, lights) for tex in (0, 1) for lens in (0, 1) for lights in (0, 1, 2)}
BUILT = {SKY, TEX | SKY, SOFT | SKY, TEX | SOFT | SKY}
FACTS = list(itertools.product((0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1, 2), (0, 1)))
STEPS = [BEGIN, ADV_RESUME, PLAIN, ADV_FILL, ADV_CLOSE]


def test_table_covers_the_four_forms():
    assert len(FACTS) == 192 and len(TABLE) == 12 and SKY == 1 << 12
    asked = {f for row in TABLE.values() for f in row if f is not NO}
    assert {f for f in asked if f & SKY} == BUILT
    assert {f for f in asked if not f & SKY} == {FIRST, FIRST | LENS}     # the opening launches are what they were


@pytest.mark.parametrize("adv", STEPS, ids=["opening", "resume", "plain", "fill", "close"])
def test_form_of_every_combination_with_the_environment_on(adv):
    wrong = []
    for facts in FACTS:
        want = TABLE.get(facts, (NO,) * 5)[adv]
        got = hostlib.advance_form(*facts[:6], adv, shutter=facts[6], sky=1)
        if got != want:
            wrong.append((facts, want, got))
    assert not wrong, wrong


def test_without_the_environment_the_answers_are_the_existing_functions():
    seen = set()
    for facts in FACTS:
        for adv in STEPS + [5, -1]:
            a, b = hostlib.advance_form(*facts[:6], adv, shutter=facts[6], sky=0), hostlib.advance_form(*facts[:6], adv, shutter=facts[6])
            assert a == b, (facts, adv, a, b)
            if not facts[6]:
                assert a == hostlib.advance_form(*facts[:6], adv), (facts, adv)
            seen.add(a)
    assert len(seen - {None}) == 25 and not any(f & SKY for f in seen - {None})


def test_outside_the_enumerations():
    assert hostlib.advance_form(0, 0, 0, 0, 0, 3, PLAIN, sky=1) is NO
    assert hostlib.advance_form(0, 0, 0, 0, 0, -1, PLAIN, sky=1) is NO
    assert hostlib.advance_form(0, 0, 0, 0, 0, 0, 5, sky=1) is NO
    assert hostlib.advance_form(0, 0, 0, 0, 0, 0, -1, sky=1) is NO


def test_the_tools_know_the_four_forms():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    try:
        import advance_forms
    finally:
        sys.path.pop(0)
    assert advance_forms.BITS["sky"] == SKY
    assert set(advance_forms.SKY_FORMS) == BUILT and len(advance_forms.ALL_FORMS) == 29 and BUILT.isdisjoint(advance_forms.FORMS)
    name = "void rtk::wf_advance<4356u, rtk::TexScene, rtk::WfSoftLights, rtk::WfSky>(rtk::Scene, rtk::Frame, rtk::WfState, rtk::TexScene, rtk::WfSoftLights, rtk::WfSky)"
    assert advance_forms.form_of(name) == TEX | SOFT | SKY
    assert advance_forms.describe(SOFT | SKY) == "wf_advance<soft | sky>"

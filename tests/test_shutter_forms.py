"""Which form of wf_advance a launch runs once the chain's facts include the shutter (csrc/rt_still.h adv_form; the host library's rth_advance_form_shutter, the entry that
takes the fact that came after tests/test_advance_forms.py's six): every combination of (counting, tex, anim, list, lens, lights) with shutter = 1 at all five steps against
a table, and with shutter = 0 against the entry that does not know the fact.

With the shutter on every launch of a chain forms the sample's pose, so every launch carries the bit.  Four forms are built: the opening launch with and without the lens,
the later launches with and without textures.  Counting, a list and an animated batch refuse the shutter, and so do several lights and a radius (lights_refuse); a shutter
chain knows no still view (no fill, no resume) and is not a plain chain (the closing kernel reads the Scene's light): those launches are never asked for."""
import itertools

import pytest

from raytracinggpu_amd import hostlib

STATS, FIRST, TEX, ANIM, LIST, FILL, RESUME, LIGHTS, SOFT, LENS, CLOSE, SHUTTER = (1 << k for k in range(12))
BEGIN, ADV_RESUME, PLAIN, ADV_FILL, ADV_CLOSE = range(5)                # rtk::StillAdv
NO = None

# (counting, tex, anim, list, lens, lights) with the shutter on -> (opening, resume, plain, fill, close).  Every combination that is not a row is never asked for.
TABLE = {
    (0, 0, 0, 0, 0, 0): (FIRST | SHUTTER, NO, SHUTTER, NO, NO),
    (0, 1, 0, 0, 0, 0): (FIRST | SHUTTER, NO, TEX | SHUTTER, NO, NO),
    (0, 0, 0, 0, 1, 0): (FIRST | LENS | SHUTTER, NO, SHUTTER, NO, NO),
    (0, 1, 0, 0, 1, 0): (FIRST | LENS | SHUTTER, NO, TEX | SHUTTER, NO, NO),
}
BUILT = {FIRST | SHUTTER, FIRST | LENS | SHUTTER, SHUTTER, TEX | SHUTTER}
FACTS = list(itertools.product((0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1, 2)))
STEPS = [BEGIN, ADV_RESUME, PLAIN, ADV_FILL, ADV_CLOSE]


def test_table_covers_the_four_forms():
    assert len(FACTS) == 96 and SHUTTER == 1 << 11
    asked = {f for row in TABLE.values() for f in row if f is not NO}
    assert asked == BUILT


@pytest.mark.parametrize("adv", STEPS, ids=["opening", "resume", "plain", "fill", "close"])
def test_form_of_every_combination_with_the_shutter_on(adv):
    wrong = []
    for facts in FACTS:
        want = TABLE.get(facts, (NO,) * 5)[adv]
        got = hostlib.advance_form(*facts, adv, shutter=1)
        if got != want:
            wrong.append((facts, want, got))
    assert not wrong, wrong


def test_with_the_shutter_off_the_answers_are_the_existing_functions():
    seen = set()
    for facts in FACTS:
        for adv in STEPS + [5, -1]:
            a, b = hostlib.advance_form(*facts, adv, shutter=0), hostlib.advance_form(*facts, adv)
            assert a == b, (facts, adv, a, b)
            seen.add(a)
    assert len(seen - {None}) == 21 and not any(f & SHUTTER for f in seen - {None})


def test_outside_the_enumerations():
    assert hostlib.advance_form(0, 0, 0, 0, 0, 3, PLAIN, shutter=1) is NO
    assert hostlib.advance_form(0, 0, 0, 0, 0, -1, PLAIN, shutter=1) is NO
    assert hostlib.advance_form(0, 0, 0, 0, 0, 0, 5, shutter=1) is NO
    assert hostlib.advance_form(0, 0, 0, 0, 0, 0, -1, shutter=1) is NO


def test_the_tools_know_the_four_forms():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    try:
        import advance_forms
    finally:
        sys.path.pop(0)
    assert advance_forms.BITS["shutter"] == SHUTTER
    assert BUILT <= set(advance_forms.FORMS) and len(advance_forms.FORMS) == 25
    assert advance_forms.form_of("void rtk::wf_advance<2052u, rtk::TexScene, rtk::WfShutter>(rtk::Scene, rtk::Frame, rtk::WfState, rtk::TexScene, rtk::WfShutter)") == TEX | SHUTTER

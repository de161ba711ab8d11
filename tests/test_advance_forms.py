"""Which form of wf_advance a launch runs (csrc/rt_still.h adv_form, the one decision enqueue_chain and launch_render_counts share) without a GPU, through the host
library's rth_advance_form: every combination of the chain's facts -- counting, textured, animated batch, list, lens, lights none / several / soft -- at the opening launch
and at the steps kAdvResume, kAdvPlain, kAdvFill and kAdvClose, against a table written out from the two if / else ladders this function replaced.

The ladders, as they stood (rt_host_render.hip.h before the form word):
  opening launch   resume -> wf_advance_resume; animated -> wf_advance_anim<true>; lens -> wf_advance_lens; else wf_advance<counting, true>;
                   a list chain: wf_advance_list<true>
  later launches   fill -> wf_advance_fill; close -> wf_advance_close<counting>;
                   textured: animated -> wf_advance_tex_anim; soft -> wf_advance_tex_soft; several -> wf_advance_tex_lights; else wf_advance_tex<counting>;
                   animated -> wf_advance_anim<false>; soft -> wf_advance_soft; several -> wf_advance_lights; else wf_advance<counting, false>;
                   a list chain: textured -> wf_advance_list_tex; else wf_advance_list<false>
and what never reaches them: rt_count_work, rt_render_counts* and rt_render_device_batch_scenes refuse several lights, a radius and the lens (lights_refuse), and no two of
the three are one call; the records of a still view (fill, resume) need a chain that is none of the three, has no lens, one point light and no texture; the closing kernel
is the plain chain's -- no texture, no batch, no list, no lens, one point light."""
import itertools

import pytest

from raytracinggpu_amd import hostlib

STATS, FIRST, TEX, ANIM, LIST, FILL, RESUME, LIGHTS, SOFT, LENS, CLOSE = (1 << k for k in range(11))
BEGIN, ADV_RESUME, PLAIN, ADV_FILL, ADV_CLOSE = range(5)                # rtk::StillAdv
NO = None                                                              # never asked for: not built

# (counting, tex, anim, list, lens, lights) -> (opening, resume, plain, fill, close).  Every combination that is not a row is never asked for at any step.
TABLE = {
    # a frame: rt_render*, one point light
    (0, 0, 0, 0, 0, 0): (FIRST, RESUME, 0, FILL, CLOSE),
    (0, 1, 0, 0, 0, 0): (FIRST, NO, TEX, NO, NO),
    # ... several lights / lights with a radius: the opening launch knows no light
    (0, 0, 0, 0, 0, 1): (FIRST, NO, LIGHTS, NO, NO),
    (0, 1, 0, 0, 0, 1): (FIRST, NO, TEX | LIGHTS, NO, NO),
    (0, 0, 0, 0, 0, 2): (FIRST, NO, SOFT, NO, NO),
    (0, 1, 0, 0, 0, 2): (FIRST, NO, TEX | SOFT, NO, NO),
    # ... through a lens: the opening launch is the lens's, the later ones the scene's own; no still view, no closing kernel
    (0, 0, 0, 0, 1, 0): (FIRST | LENS, NO, 0, NO, NO),
    (0, 1, 0, 0, 1, 0): (FIRST | LENS, NO, TEX, NO, NO),
    (0, 0, 0, 0, 1, 1): (FIRST | LENS, NO, LIGHTS, NO, NO),
    (0, 1, 0, 0, 1, 1): (FIRST | LENS, NO, TEX | LIGHTS, NO, NO),
    (0, 0, 0, 0, 1, 2): (FIRST | LENS, NO, SOFT, NO, NO),
    (0, 1, 0, 0, 1, 2): (FIRST | LENS, NO, TEX | SOFT, NO, NO),
    # rt_count_work
    (1, 0, 0, 0, 0, 0): (FIRST | STATS, NO, STATS, NO, CLOSE | STATS),
    (1, 1, 0, 0, 0, 0): (FIRST | STATS, NO, TEX | STATS, NO, NO),
    # rt_render_device_batch_scenes
    (0, 0, 1, 0, 0, 0): (FIRST | ANIM, NO, ANIM, NO, NO),
    (0, 1, 1, 0, 0, 0): (FIRST | ANIM, NO, TEX | ANIM, NO, NO),
    # rt_render_counts*
    (0, 0, 0, 1, 0, 0): (FIRST | LIST, NO, LIST, NO, NO),
    (0, 1, 0, 1, 0, 0): (FIRST | LIST, NO, TEX | LIST, NO, NO),
}
# the 21 instantiations of launch_advance's switch
BUILT = {0, STATS, FIRST, FIRST | STATS, TEX, TEX | STATS, FILL, RESUME, LIGHTS, TEX | LIGHTS, SOFT, TEX | SOFT, FIRST | LENS, ANIM, FIRST | ANIM, TEX | ANIM, CLOSE,
         CLOSE | STATS, LIST, FIRST | LIST, TEX | LIST}
FACTS = list(itertools.product((0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1, 2)))


def test_table_covers_the_built_forms():
    assert len(FACTS) == 96 and len(BUILT) == 21
    asked = {f for row in TABLE.values() for f in row if f is not NO}
    assert asked == BUILT                                              # every built form is asked for somewhere, and nothing else is


@pytest.mark.parametrize("adv", [BEGIN, ADV_RESUME, PLAIN, ADV_FILL, ADV_CLOSE], ids=["opening", "resume", "plain", "fill", "close"])
def test_form_of_every_combination(adv):
    wrong = []
    for facts in FACTS:
        want = TABLE.get(facts, (NO,) * 5)[adv]
        got = hostlib.advance_form(*facts, adv)
        if got != want:
            wrong.append((facts, want, got))
    assert not wrong, wrong


def test_outside_the_enumerations():
    assert hostlib.advance_form(0, 0, 0, 0, 0, 3, PLAIN) is NO          # no such lights
    assert hostlib.advance_form(0, 0, 0, 0, 0, -1, PLAIN) is NO
    assert hostlib.advance_form(0, 0, 0, 0, 0, 0, 5) is NO              # no such step
    assert hostlib.advance_form(0, 0, 0, 0, 0, 0, -1) is NO

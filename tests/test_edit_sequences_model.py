"""tests/edit_sequences.py held to itself and to the headers, without a GPU: the generator is deterministic and keeps its two conditions (at most 15 % of a sequence's frame
ops predicted refused; four still runs in every sequence of the counted families), canonical() has the properties the device test's path-independence check rests on,
every state-changing entry of include/raytrace_hip.h is a row of the op table or an excuse in writing, the counted families' event lists exercise every level of the still
view (hostlib.still_replay: the device comparison is not vacuous), and no frame the generator predicts as rendered asks for a wf_advance form that is not built."""
import os
import re

import numpy as np
import pytest

from raytracinggpu_amd import hostlib
from . import edit_sequences as es

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(f, s) for f in es.FAMILIES for s in es.SEEDS]
BEGIN, RESUME, PLAIN, FILL, CLOSE = 0, 1, 2, 3, 4        # rtk::StillAdv


def _frames(ops):
    return [(op, S.predict(op)) for op, S in zip(ops, es.states(ops)) if op[0] == "frame"]


@pytest.mark.parametrize("family,seed", CASES)
def test_a_sequence_is_a_function_of_family_and_seed(family, seed):
    ops = es.sequence(family, seed)
    assert ops == es.sequence(family, seed) and len(ops) == es.LENGTH
    assert ops != es.sequence(family, seed + 100)
    assert eval(repr(ops), {}) == ops                                   # plain data: what is printed can be pasted
    assert ops[0] == ("scene_upload", es.FAMILY[family].scene)

    def numbers(x):
        if isinstance(x, float):
            yield x
        elif isinstance(x, (tuple, list)):
            for y in x:
                yield from numbers(y)
        elif isinstance(x, dict):
            yield from numbers(list(x.values()))
    for op in ops:
        for v in numbers(op):
            assert float(np.float32(v)) == v, (op, v)                    # every number is a binary32 value


@pytest.mark.parametrize("family,seed", CASES)
def test_refused_frames_are_few_and_still_runs_many(family, seed):
    ops = es.sequence(family, seed)
    frames = _frames(ops)
    refused = [op for op, code in frames if code != 0]
    assert len(refused) <= es.REFUSED_SHARE * len(frames), (len(refused), len(frames))
    if family in es.COUNTED:
        assert not refused or family == "toggles"
        assert len(es.still_runs(ops)) >= 4, es.still_runs(ops)
        assert all(op[1] == "render" for op, _ in frames)               # still_events knows `render` alone


def test_some_sequences_enter_refused_combinations_and_leave_them():
    entered = {f: sum(code == es.UNSUPPORTED for s in es.SEEDS for _, code in _frames(es.sequence(f, s))) for f in es.FAMILIES}
    assert entered["toggles"] > 0 and entered["emit"] > 0 and entered["everything"] > 0, entered
    for s in es.SEEDS:                                                   # `everything`: another scene, a failed upload with a frame that finds no scene, a good upload
        ops = es.sequence("everything", s)
        ups = [op[1] for op in ops if op[0] == "scene_upload"]
        assert ups[0] == "panel_cat" and "open_cat" in ups and ups[-1] == "cat" and ups[-2] in es.FAILING, ups
        assert any(code == es.NO_SCENE for _, code in _frames(ops))
    kinds = {op[0] for f in es.FAMILIES for s in es.SEEDS for op in es.sequence(f, s)}
    assert set(es.TABLE) <= kinds, set(es.TABLE) - kinds                   # every row is drawn somewhere
    entries = {op[1] for f in es.FAMILIES for s in es.SEEDS for op in es.sequence(f, s) if op[0] == "frame"}
    assert entries == set(es.ENTRIES)
    bys = {op[1] for f in es.FAMILIES for s in es.SEEDS for op in es.sequence(f, s) if op[0] == "by"}
    assert bys == set(es.BYSTANDERS)
    refusals = {op[2] for f in es.FAMILIES for s in es.SEEDS for op in es.sequence(f, s) if op[0] == "refuse"}
    assert refusals - {"set_light"} == {k for k, row in es.TABLE.items() if row.refuse is not None}, refusals   # (set_light: the edit that finds no scene)


# ---- canonical()
UP = ("scene_upload", "cat")
L1, L2 = ("set_light", (1.0, 2.0, 3.0), 1.0), ("set_light", (4.0, 5.0, 6.0), 2.0)
FRAME, BY, REFUSED = ("frame", "render", 64, 48, 1, 2, 5, 0.0), ("by", "getters", 64, 48), ("refuse", -1, "set_light_at", 7, (0.0, 0.0, 0.0), 1.0)


def test_canonical_keeps_the_last_call_of_an_absolute_state():
    assert es.canonical([UP, L1, FRAME, L2, BY, REFUSED]) == [UP, L2]
    lens, lens2 = ("set_lens", 1.0, 40.0), ("set_lens", 0.0, 1.0)
    assert es.canonical([UP, lens, L1, lens2, L2]) == [UP, lens2, L2]
    a, b, c = ("set_sphere", 1, es.WALL6[1]), ("set_sphere", 2, es.WALL6[2]), ("set_sphere", 1, es.WALL6[0])
    assert es.canonical([UP, a, b, c]) == [UP, b, c]                     # by object slot
    e6, e7 = ("set_emission", 6, (1.0, 1.0, 1.0)), ("set_emission", 7, (2.0, 2.0, 2.0))
    assert es.canonical([UP, e6, e7, ("set_emission", 6, (0.0, 0.0, 0.0))]) == [UP, e7, ("set_emission", 6, (0.0, 0.0, 0.0))]
    assert es.canonical([UP, L1, L2], upto=2) == [UP, L1]


def test_canonical_keeps_relative_ops_in_order_and_what_they_composed_with():
    m1, m2 = ("move_light", 1.0), ("move_light", 2.0)
    assert es.canonical([UP, m1, FRAME, m2, m1]) == [UP, m1, m2, m1]
    assert es.canonical([UP, L1, m1, L2]) == [UP, L1, m1, L2]            # the light that was moved stays before the move
    assert es.canonical([UP, L1, L2, m1]) == [UP, L2, m1]
    three = ("set_lights", [((0.0, 1.0, 2.0), 1.0)] * 3)
    radii = ("set_light_radii", [1.0, 0.0, 2.0])
    assert es.canonical([UP, three, radii, L1]) == [UP, L1]              # a new light is a point: the radii went with the list
    assert es.canonical([UP, three, radii, ("move_light_at", 2, 1.0), L1]) == [UP, three, radii, ("move_light_at", 2, 1.0), L1]
    t, n1, n2 = ("mesh_transform", ("ry", 10), (0.0, 0.0, 0.0), None), ("mesh_set_normals", ("radial", 0.0), None), ("mesh_compute_normals", None)
    assert es.canonical([UP, n1, t, n2]) == [UP, n1, t, n2]              # the transform turned the normals it found
    assert es.canonical([UP, t, n1, n2]) == [UP, t, n2]
    mv = ("move_sphere", 2, (1.0, 0.0, 0.0))
    a = ("set_sphere", 1, es.WALL6[1])
    assert es.canonical([UP, a, mv, ("set_sphere", 1, es.WALL6[0])]) == [UP, mv, ("set_sphere", 1, es.WALL6[0])]   # another sphere's move pins nothing


def test_canonical_starts_at_the_last_upload():
    up2 = ("scene_upload", "open_cat")
    assert es.canonical([UP, L1, ("move_light", 1.0), up2, L2]) == [up2, L2]
    assert es.canonical([UP, L1, ("scene_upload", "seventeen")]) == [("scene_upload", "seventeen")]
    assert es.canonical([]) == []
    for f, s in CASES:
        ops = es.sequence(f, s)
        for k in es.checkpoints(ops):
            c = es.canonical(ops, k)
            assert c[0][0] == "scene_upload" and all(es.is_edit(op) for op in c) and sum(op[0] == "scene_upload" for op in c) == 1
            a, b = es.states(c)[-1], es.states(ops[:k])[-1]                # the model's state is the same (but for the names of the values the device computes)
            for field in ("scene", "have", "meshes", "radii", "lens", "shutter", "env", "env_share", "emission", "emit_share", "tex", "smooth"):
                assert getattr(a, field) == getattr(b, field), (f, s, k, field)
            assert len(a.lights) == len(b.lights) and sorted(a.spheres) == sorted(b.spheres)


# ---- the header
ENTRY = re.compile(r"^(?:const char \*|int )(rt_(?:scene_(?:set|move|get|upload)\w*|camera_(?:set|get)\w*|mesh_\w+|multi_\w+))\(", re.M)


def header_entries(text):
    return sorted(set(ENTRY.findall(text)))


def methods_of(entry, capi_text):
    """the Context methods whose body calls `entry`"""
    body = capi_text[capi_text.index("class Context:"):capi_text.index("class MultiContext:")]
    out = []
    for m in re.finditer(r"^    def (\w+)\(self.*?(?=^    def |\Z)", body, re.M | re.S):
        if re.search(r"\b_L\." + entry + r"\b", m.group(0)):
            out.append(m.group(1))
    return out


def uncovered(header_text, capi_text):
    """the entries that are neither a row of the op table (through their Context method) nor excused"""
    missing = []
    for e in header_entries(header_text):
        if e in es.EXCLUDED:
            assert len(es.EXCLUDED[e].split()) >= 4 and es.EXCLUDED[e].endswith(".")   # a sentence
            continue
        ms = methods_of(e, capi_text)
        if not ms or not all(m in es.TABLE for m in ms):
            missing.append(e)
    return missing


def _texts():
    with open(os.path.join(ROOT, "include", "raytrace_hip.h")) as f, open(os.path.join(ROOT, "raytracinggpu_amd", "_capi.py")) as g:
        return f.read(), g.read()


def test_every_state_changing_entry_of_the_header_is_in_the_table():
    header, capi = _texts()
    entries = header_entries(header)
    assert len(entries) > 50 and "rt_scene_set_emission" in entries and "rt_mesh_set_vertices_device" in entries and "rt_camera_set_lens" in entries
    assert uncovered(header, capi) == []
    assert set(es.EXCLUDED) <= set(entries), set(es.EXCLUDED) - set(entries)      # no excuse outlives its entry
    rows = {m for e in entries if e not in es.EXCLUDED for m in methods_of(e, capi)}
    assert rows == set(es.TABLE), rows ^ set(es.TABLE)                             # and no row names a method that calls none of them


def test_a_new_setter_without_a_row_fails_the_coverage():
    header, capi = _texts()
    fog = header.replace("int rt_scene_set_emission_sampling(", "int rt_scene_set_fog(rt_ctx *ctx, float density);\nint rt_scene_set_emission_sampling(", 1)
    assert uncovered(fog, capi) == ["rt_scene_set_fog"]
    bound = capi.replace("    def set_emission_sampling(self, share):", "    def set_fog(self, density):\n        self._check(self._L.rt_scene_set_fog(self._h, density))\n\n    def set_emission_sampling(self, share):", 1)
    assert uncovered(fog, bound) == ["rt_scene_set_fog"]                          # bound in Python but not in the table: still missing


# ---- the still view's events
@pytest.mark.parametrize("family,seed", [(f, s) for f in es.COUNTED if f != "toggles" for s in es.SEEDS])
def test_the_counted_families_exercise_every_level(family, seed):
    ops = es.sequence(family, seed)
    ev, done = es.still_events(ops)
    assert len(done) == len(es.with_probes(ops)) and done[-1] == len(ev)
    counts, rows = hostlib.still_replay(ev)
    hit, shadow, records = counts
    assert hit[0] > 0 and hit[1] > 0 and hit[3] > 0, counts              # used, filled, and a key miss at the hit level
    assert shadow[0] > 0 and shadow[1] > 0 and shadow[3] > 0, counts
    assert records[0] > 0 and records[1] > 0 and records[3] > 0, counts   # (forest: around the run for which the texture is taken off)
    assert (rows[:, 7] == RESUME).any()                                  # a chain that resumed
    assert es.expected_use(ops) == (True, True, True)
    primed, done = es.still_events(ops, primer=es.PRIMER)               # the device test's form: the primer's events first, counted in
    assert len(done) == len(es.with_probes(ops)) and done[-1] == len(primed) == len(ev) + len(es.still_events(es.PRIMER, probes=False)[0])


def test_the_uncounted_families_hold_still_runs_that_must_use_a_level():
    """the device test's 'a level that must be used was used' is asked of something: some sequence of `lights` and of `everything` holds an eligible run through rt_render"""
    for family in ("lights", "everything"):
        uses = [es.expected_use(es.sequence(family, s)) for s in es.SEEDS]
        assert any(u[0] for u in uses), (family, uses)
    assert any(es.expected_use(es.sequence("lights", s)) == (True, True, True) for s in es.SEEDS)


def test_the_toggles_family_empties_and_refills_the_levels():
    """a feature that keeps the chains away is on for part of every sequence: over the family's seeds every level is used, filled and emptied, and a feature is turned off
    between two frames of one key at least once a sequence"""
    total = np.zeros((3, 4), np.int64)
    for seed in es.SEEDS:
        ops = es.sequence("toggles", seed)
        counts, _ = hostlib.still_replay(es.still_events(ops)[0])
        assert counts[0, 0] > 0 and counts[0, 1] > 0 and counts[0, 3] > 0, (seed, counts)
        total += counts
        sts = es.states(ops)
        assert any(a.apart and not b.apart for a, b in zip(sts, sts[1:])), seed
    assert (total[:, [0, 1, 3]] > 0).all(), total


def test_the_replay_of_the_documented_orders():
    """hand-written orders whose counters rt_still.h's text gives: the restatement is held to the documents, not to the device"""
    frame = lambda s=1, W=64, H=48, sigma=0.0: ("frame", "render", W, H, 1, 2, s, sigma)
    def counts(ops):
        return hostlib.still_replay(es.still_events(ops, probes=False)[0])[0].tolist()
    still = [UP] + [frame(k) for k in range(4)]
    assert counts(still) == [[6, 2, 0, 0], [6, 2, 0, 0], [4, 2, 0, 0]]                                   # fill; use and store; resume, resume
    assert counts(still + [L1, frame(9)]) == [[8, 2, 0, 0], [6, 4, 0, 1], [4, 2, 0, 1]]                  # a light edit: a shadow miss, the hits are kept
    assert counts(still + [L1, L1, frame(9)]) == counts(still + [L1, frame(9)])
    assert counts(still + [("set_light", *es.LIGHT), frame(9)]) == [[8, 2, 0, 0], [8, 2, 0, 0], [6, 2, 0, 0]]   # the value it had: no miss
    assert counts(still + [("mesh_transform", ("ry", 10), (0.0, 0.0, 0.0), None), frame(9)]) == [[6, 4, 0, 1], [6, 4, 0, 1], [4, 2, 0, 1]]
    assert counts(still + [("mesh_set_texture", ("noise", 0, "nearest", "repeat"), None), frame(9)]) == [[8, 2, 0, 0], [6, 4, 0, 1], [4, 2, 2, 1]]
    assert counts(still + [frame(9, 61, 43), frame(10)]) == [[6, 6, 0, 2], [6, 6, 0, 2], [4, 2, 0, 1]]   # another size is another ray key, both ways
    assert counts(still + [frame(9, sigma=0.25), ("by", "count_work", 64, 48), ("by", "stats_frame", 64, 48), ("by", "render_aov", 64, 48), frame(10)]) == \
        [[8, 2, 5, 0], [8, 2, 5, 0], [6, 2, 5, 0]]                                                       # level 0 counts as ineligible and touches nothing
    lens = [("set_lens", 1.0, 40.0), frame(8), L1, ("set_lens", 0.0, 1.0)]
    assert counts(still + lens + [frame(9)]) == [[6, 4, 0, 1], [6, 4, 0, 1], [4, 2, 0, 1]]               # frames went by unseen: everything is stale
    emit = [("set_emission", 6, (1.0, 1.0, 1.0)), frame(8), ("set_emission", 6, (0.0, 0.0, 0.0))]
    assert counts(still + emit + [frame(9)]) == [[8, 2, 0, 0], [8, 2, 0, 0], [6, 2, 0, 0]]               # an emission set and removed leaves the levels valid
    three = ("set_lights", [es.LIGHT, ((1.0, 2.0, 3.0), 1.0)])
    assert counts(still + [three, frame(8), frame(9)]) == [[10, 2, 0, 0], [6, 2, 4, 0], [4, 2, 4, 0]]    # several lights: the hit level only


# ---- the refusal table against rtk::adv_form
@pytest.mark.parametrize("family,seed", CASES)
def test_a_frame_predicted_as_rendered_asks_for_built_forms_only(family, seed):
    ops = es.sequence(family, seed)
    n = 0
    for op, S in zip(ops, es.states(ops)):
        if op[0] != "frame" or S.predict(op) != 0:
            continue
        f = S.facts()
        form = lambda adv: hostlib.advance_form(False, f["tex"], False, False, f["lens"], f["lights"], adv, shutter=f["shutter"], sky=f["sky"], sample=f["sample"], emit=f["emit"])
        chain = [BEGIN, PLAIN]
        level = S.still_level(op[7])
        if level == 3:
            chain += [FILL, RESUME]                                      # the records level
        if not (f["tex"] or f["lens"] or f["lights"] or f["shutter"] or f["sky"] or f["emit"]):
            chain.append(CLOSE)                                          # a plain chain's last launch
        for adv in chain:
            assert form(adv) is not None, (op, f, adv)
        n += 1
    assert n > 0
    for S in (s for s in es.states(ops) if s.have and s.frame_code() == es.UNSUPPORTED):    # and what it predicts as refused has no form for its later launches
        f = S.facts()
        assert hostlib.advance_form(False, f["tex"], False, False, f["lens"], f["lights"], PLAIN, shutter=f["shutter"], sky=f["sky"], sample=f["sample"], emit=f["emit"]) is None, f

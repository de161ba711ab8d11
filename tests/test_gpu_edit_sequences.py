"""A context as a long-lived state machine: generated sequences of scene edits, refused calls, bystander calls and frames (tests/edit_sequences.py), held to two references
that do not share the state under test.  -m gpu.

Three contexts, always driven in the same order: `on` with default knobs, `off` with RT_FIRST_HIT_CACHE=0 (all three levels of the still view off) and the same ops, and
`fresh`, knob-off too, which at checkpoints only is uploaded again and given canonical(ops, step).
  every frame op     on and off agree word for word (NaN equals NaN in a colour), and so do the 8-bit images; a frame predicted refused raises the predicted code on both and
                     leaves its sentinel-filled output as it was;
  every checkpoint   one more frame on all three, equal; every getter answers equally on `on` and `fresh`, and so do the emitters' and the sky's tables where they exist --
                     no op before the step matters except through canonical();
  every refused edit the promised code, and every getter reads as before;
  counters           `off` never uses or fills a level; in the families still, mesh, forest and toggles (es.COUNTED) `on`'s twelve counters after every op are hostlib.still_replay's of
                     still_events(ops) -- a wrong miss is a finding like a wrong hit; such a sequence is preceded by es.PRIMER (an upload and three frames), after which
                     the levels' state is known whatever ran before, so the comparison is exact from the first op; elsewhere a level that the sequence's own still runs must use did get used;
  named orders       the orders that found something, or that cross two features, kept apart from the generator.
The three contexts are shared by every sequence and named order of the file, on purpose: an upload has to wipe what the sequence before it left (an emission that
outlives an upload is found through the previous sequence's), so what a fault fails depends on the order the cases run in, and one finding can entail later ones.
Findings are collected and the test fails once, naming family, seed, step, op and the first differing pixel, with the ops up to that step."""
import time

import numpy as np
import pytest

import raytracinggpu_amd as rt
from raytracinggpu_amd import hostlib
from . import edit_sequences as es
from . import still_view as sv

pytestmark = pytest.mark.gpu

SHOWN = 6                                   # findings spelled out in a failure message
LEVELS = (sv.HIT, sv.SHADOW, sv.SHADE)
RT_ERR_HIP = -3


@pytest.fixture(scope="module")
def trio(cat_golden):
    import torch
    stream = torch.cuda.Stream()
    cs = dict(on=sv.context(), off=sv.context(RT_FIRST_HIT_CACHE="0"), fresh=sv.context(RT_FIRST_HIT_CACHE="0"))
    yield {k: es.Driver(c, cat_golden, stream.cuda_stream) for k, c in cs.items()}
    for c in cs.values():
        c.close()


def _counts(c):
    return np.array([[getattr(c, lv.counts)()[k] for k in (lv.used, "filled", "ineligible", "key_misses")] for lv in LEVELS], np.int64)


def _run(d, op):
    try:
        return ("ok", d.apply(op))
    except rt._capi.RtError as e:
        if e.code == RT_ERR_HIP:                                       # a HIP error ends the run where it stands: nothing more is started on the device
            pytest.exit(f"HIP error at {op}: {e}", returncode=3)
        return ("error", e.code)


def _differ(a, b, path=""):
    """None, or where two answers differ first; float frames as words with NaN equal to NaN in a colour"""
    if isinstance(a, np.ndarray) and isinstance(b, np.ndarray):
        if a.shape != b.shape or a.dtype != b.dtype:
            return f"{path} {a.dtype}{a.shape} against {b.dtype}{b.shape}"
        if a.dtype == np.float32:
            d = np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)
            if a.ndim == 3 and a.shape[-1] == 4:
                d[..., :3] &= ~(np.isnan(a[..., :3]) & np.isnan(b[..., :3]))
        else:
            d = a != b
        if d.any():
            at = tuple(int(x) for x in np.argwhere(d)[0])
            return f"{path} {int(d.sum())} of {d.size} differ, first at {at}: {a[at]!r} against {b[at]!r}"
        return None
    if isinstance(a, dict) and isinstance(b, dict) and a.keys() == b.keys():
        return next((r for r in (_differ(a[k], b[k], f"{path}[{k}]") for k in a) if r), None)
    if isinstance(a, (tuple, list)) and isinstance(b, (tuple, list)) and len(a) == len(b):
        return next((r for r in (_differ(x, y, f"{path}[{k}]") for k, (x, y) in enumerate(zip(a, b))) if r), None)
    return None if a == b else f"{path} {a!r} against {b!r}"


def _sequence(trio, label, ops, found, counted):
    """one sequence through the three contexts; findings go to `found`"""
    on, off, fresh = trio["on"], trio["off"], trio["fresh"]
    S, at = es.State(), set(es.checkpoints(ops))
    ev, done = es.still_events(ops, primer=es.PRIMER) if counted else ([], [])
    if counted:                                                        # whatever the sequences before left: the levels now hold this still view's words, where the replay starts
        for pop in es.PRIMER:
            for d in (on, off):
                r = _run(d, pop)
                if r[0] != "ok":
                    found.append(f"{label}: the primer's {pop} raised RT error {r[1]}")
    primed = hostlib.still_replay(ev[:len(es.still_events(es.PRIMER, probes=False)[0])])[0] if counted else None     # (the counters at the sequence's first op)
    base, seen = _counts(on.c), {"n": 0}

    def note(step, op, what):
        found.append(f"{label} step {step} {op}: {what}\n    ops so far: {ops[:step + 1]}")

    def counters(step, op):
        if not counted:
            return
        seen["n"] += 1
        want = hostlib.still_replay(ev[:done[seen["n"] - 1]])[0] - primed
        d = (_counts(on.c) - base) - want
        if d.any():
            note(step, op, f"the still view's counters (used, filled, ineligible, key misses per level) moved by {(_counts(on.c) - base).tolist()}, the replay says {want.tolist()}")
            base[...] = _counts(on.c) - want                            # one finding per divergence

    def frames_equal(step, op, a, b, names, da, db):
        diff = _differ(a, b)
        if diff:
            note(step, op, f"{names}: {diff}")
            return
        for k, (x, y) in enumerate(zip(a, b)) if isinstance(a, list) else ():
            if isinstance(x, np.ndarray) and x.dtype == np.float32 and x.ndim == 3 and x.shape[-1] == 4:
                diff = _differ(da.rgb8(x), db.rgb8(y))
                if diff:
                    note(step, op, f"{names}, the 8-bit image of frame {k}: {diff}")

    def one(step, op, drivers):
        """the op on every driver: the predicted refusal on each, or answers that agree with the first driver's"""
        code = S.predict(op)
        before = on.getters(S) if op[0] == "refuse" else None
        rs = [(_run(d, op), name, d) for name, d in drivers]
        for r, name, d in rs:
            if code != 0:
                if r != ("error", code):
                    note(step, op, f"predicted RT error {code}; `{name}` answered {r[0]} {r[1] if r[0] == 'error' else ''}")
                elif op[0] == "frame" and not all(es.untouched(a) for a in d.out):
                    note(step, op, f"`{name}` refused the frame and wrote to its output")
            elif r[0] != "ok":
                note(step, op, f"`{name}` raised RT error {r[1]}")
        if code == 0 and all(r[0] == "ok" for r, _, _ in rs):
            for r, name, d in rs[1:]:
                frames_equal(step, op, rs[0][0][1], r[1], f"`{rs[0][1]}` against `{name}`", rs[0][2], d)
        if before is not None and on.getters(S) != before:
            now = on.getters(S)
            note(step, op, f"a refused call changed {[k for k in now if now[k] != before.get(k)]}")

    for step, op in enumerate(ops):
        one(step, op, [("on", on), ("off", off)])
        S.apply(op)
        counters(step, op)
        if step + 1 not in at:
            continue
        # the checkpoint: a fresh upload and the canonical ops, then one more frame and every getter
        for cop in es.canonical(ops, step + 1):
            r = _run(fresh, cop)
            if r != (("error", es.INVALID) if cop[0] == "scene_upload" and cop[1] in es.FAILING else ("ok", None)):
                note(step, op, f"the canonical op {cop} answered {r} on `fresh`")
        probe = es.probe(step + 1)
        one(step, probe, [("on", on), ("off", off), ("fresh", fresh)])
        counters(step, probe)
        a, b = on.getters(S), fresh.getters(S)
        skip = () if S.have else ("lens",)                             # (without a scene the lens is what an earlier scene left: no getter is promised to answer)
        wrong = [k for k in a if k not in skip and _differ(a[k], b[k])]
        if wrong:
            note(step, op, f"after the canonical ops {es.canonical(ops, step + 1)} the getters {wrong} differ: {[(a[k], b[k]) for k in wrong][:2]}")
        for table, there in (("kat_emission_table", S.have and S.emit_on), ("kat_environment_table", S.have and S.env is not None and S.env_share > 0)):
            if there:
                ta, tb = _run(on, ("by", table, 64, 48)), _run(fresh, ("by", table, 64, 48))
                if ta[0] != "ok" or tb[0] != "ok":
                    note(step, op, f"{table} after the canonical ops: `on` answered {ta[:2] if ta[0] != 'ok' else 'ok'}, `fresh` {tb[:2] if tb[0] != 'ok' else 'ok'}")
                elif _differ(ta[1], tb[1]):
                    note(step, op, f"{table} after the canonical ops: {_differ(ta[1], tb[1])}")
    moved = _counts(on.c) - base
    zero = _counts(off.c)[:, :2]
    if zero.any():
        found.append(f"{label}: the context with RT_FIRST_HIT_CACHE=0 used or filled a level: {zero.tolist()}")
    if not counted:
        for lv, must, n in zip(LEVELS, es.expected_use(ops), moved[:, 0]):
            if must and n == 0:
                found.append(f"{label}: the sequence holds a still run that must use {lv.counts}, and its first counter did not move")


def _report(found, t0, what):
    print(f"{what}: {time.perf_counter() - t0:.2f} s")
    assert not found, f"{len(found)} findings, the first {min(len(found), SHOWN)}:\n" + "\n".join(found[:SHOWN])


@pytest.mark.parametrize("family", es.FAMILIES)
def test_generated_sequences(trio, family):
    found, t0 = [], time.perf_counter()
    for seed in es.SEEDS:
        _sequence(trio, f"{family} seed {seed}", es.sequence(family, seed), found, family in es.COUNTED)
    _report(found, t0, f"family {family}, {len(es.SEEDS)} sequences of {es.LENGTH} ops")


def _f(k, entry="render", W=64, H=48, b=2, spp=1):
    return ("frame", entry, W, H, spp, b, 100 + k, 0.0)


def _run3(k, **kw):
    return [_f(k + i, **kw) for i in range(3)]


LIGHT2 = ("set_light", (8.0, 30.0, 20.0), es.F(3e10))
SUN0, SUN1 = ("set_environment", ("sun", 0)), ("set_environment", ("sun", 1))
EMIT7 = ("set_emission", 7, tuple(es.F(c) for c in es.LE))
# name -> ops: fixed orders run through the same machinery, so that they survive a change of the generator
NAMED = {
    "lens on, light edit, lens off": [("scene_upload", "cat")] + _run3(0) + [("set_lens", 1.0, 40.0), _f(3), LIGHT2, ("set_lens", 0.0, 1.0)] + _run3(4),
    "shutter on, light edit, shutter off": [("scene_upload", "cat")] + _run3(0) + [("set_shutter", (0.5, 0.0, 0.25), None), _f(3), LIGHT2, ("set_shutter", None, None)] + _run3(4),
    "environment on, light edit, environment off": [("scene_upload", "open_cat")] + _run3(0) + [SUN0, _f(3), LIGHT2, ("set_environment", None)] + _run3(4),
    "environment on, texture edit, environment off": [("scene_upload", "open_cat")] + _run3(0) + [SUN0, _f(3), ("mesh_set_texture", ("noise", 0, "nearest", "repeat"), 2),
                                                                                               ("set_environment", None)] + _run3(4),
    "emission on, light edit, emission removed": [("scene_upload", "panel_cat")] + _run3(0) + [EMIT7, _f(3), LIGHT2, ("set_emission", 7, (0.0, 0.0, 0.0))] + _run3(4),
    "emission on, transform, LBVH rebuild, share 0 and 0.5": [("scene_upload", "panel_cat"), EMIT7, _f(0), ("mesh_transform", ("ry", 20), (1.0, -2.0, 0.5), 7), _f(1),
                                                             ("mesh_rebuild", "lbvh", 7), ("set_emission_sampling", 0.0), _f(2), ("set_emission_sampling", 0.5), _f(3),
                                                             ("by", "kat_emission_table", 64, 48)],
    "a frame of another size inside a still run": [("scene_upload", "cat")] + _run3(0) + [_f(3, W=61, H=43)] + _run3(4),
    "a frame on a caller's stream inside a still run": [("scene_upload", "cat")] + _run3(0) + [_f(3, entry="render_stream")] + _run3(4),
    "a frame under rt_stats_enable inside a still run": [("scene_upload", "cat")] + _run3(0) + [("by", "stats_frame", 64, 48)] + _run3(4),
    "several lights, then set_light": [("scene_upload", "cat"), ("set_lights", [es.LIGHT, ((10.0, 30.0, 20.0), es.F(1e10))]), ("set_light_radii", [0.0, 2.0]), _f(0), _f(1), LIGHT2] + _run3(2),
    "environment share 0.5, 0, 0.5 with the map replaced": [("scene_upload", "open_cat"), SUN0, ("set_environment_sampling", 0.5), _f(0), ("set_environment_sampling", 0.0), SUN1, _f(1),
                                                           ("set_environment_sampling", 0.5), _f(2), ("by", "kat_environment_table", 64, 48)],
    # found by family `everything`: an upload refused for its 17 objects had dropped the environment and the emissions and left the old scene in use
    "failed upload of 17 objects, good upload": [("scene_upload", "cat")] + _run3(0) + [("scene_upload", "seventeen"), _f(3), ("by", "getters", 64, 48), ("scene_upload", "cat")] + _run3(4),
    "failed upload of a bad index, good upload": [("scene_upload", "cat")] + _run3(0) + [("scene_upload", "bad_index"), _f(3), ("scene_upload", "cat")] + _run3(4),
}


@pytest.mark.parametrize("name", list(NAMED))
def test_named_orders(trio, name):
    found, t0 = [], time.perf_counter()
    ops = NAMED[name]
    counted = all(op[1] in ("render", "render_stream") for op in ops if op[0] == "frame")
    _sequence(trio, name, ops, found, counted)
    _report(found, t0, name)

"""Generated lives of a context (a helper module, like scene_fuzz.py and still_view.py): sequences of scene edits, refused calls, bystander calls and frames, the model that
predicts what each of them does, and what tests/test_gpu_edit_sequences.py holds the device to (tests/test_edit_sequences_model.py holds this file to itself, without a GPU).

An op is a small tuple of plain data -- print a sequence and paste it into replay(ctx, [...], cat_golden):
    (method, *arguments)                              an edit: a state-changing Context method, one row of TABLE each; arrays are named by a recipe (a tuple), not spelled out
    ("refuse", code, method, *arguments)              the same call with arguments the header promises to refuse with `code` and the state untouched ("nan": a NaN)
    ("frame", entry, W, H, spp, num_bounce, seed, sigma)
    ("by", name, W, H)                                a bystander: an entry that must change nothing
Two references that share no state with the context under test: a context with RT_FIRST_HIT_CACHE=0 given the same ops, and a context that is uploaded afresh and given
canonical(ops, step) -- the path-independence check; and for the counters of the still view the host library's replay of still_events(ops), which restates the documented
rules of csrc/rt_still.h and DESIGN.md section 5.1 (it was not written by watching the device)."""
from collections import namedtuple

import numpy as np

import raytracinggpu_amd as rt

f32 = np.float32
FAMILIES = ("still", "mesh", "forest", "lights", "toggles", "sky", "emit", "everything")
# the families whose still-view counters are held to the replay, chain by chain: their frames go through `render` alone.  `toggles` is one of them because a lens, a
# shutter or a sky that is turned on and off again without the levels being emptied leaves every PIXEL right in most orders: only the counters tell
COUNTED = ("still", "mesh", "forest", "toggles")
SEEDS = range(6)
LENGTH = 48
SIZES = ((64, 48), (61, 43))                           # two sub-frames of three 8-row tiles; partial tiles
ENTRIES = ("render", "render_rows", "render_stream", "render_pose", "render_async", "render_rgb8", "pipelined")
PROBE = (64, 48, 1, 2)                                 # the checkpoint's frame: W, H, spp, num_bounce
INVALID, NO_SCENE, UNSUPPORTED = -1, -4, -5            # RT_ERR_*
REFUSED_SHARE = 0.15                                   # of a sequence's frame ops, at most
LE = (4e5, 3e5, 2e5)
PANEL = ((-25, 32, -18), (50, 2, 0), (0, 1, 40))       # tilted: a box without thickness is entered by no ray
FAILING = ("seventeen", "bad_index")                   # uploads that fail: 17 objects; a triangle that names a vertex outside the mesh


def F(x):
    return float(f32(x))


def num(x):
    return float("nan") if x == "nan" else x


LIGHT = (tuple(F(v) for v in rt.scenes.LIGHT[0]), F(rt.scenes.LIGHT[1]))
WALL6 = [(tuple(F(v) for v in c), F(r), tuple(F(v) for v in a), 0, 1.0, 1.0) for c, r, a in rt.scenes.WALLS]
# name -> (the spheres as the getter answers them, by object slot; the meshes' object slots)
SCENES = {
    "cat": (dict(enumerate(WALL6)), (6,)),
    "cpu_glass": (dict(enumerate(WALL6)), (6,)),
    "open_cat": (dict(enumerate(WALL6[:2])), (2,)),                        # the back wall and the floor: most rays that leave the cat meet the sky
    "two_cats": (dict(zip((0, 1, 2, 4, 5, 6), WALL6)), (3, 7)),
    "panel_cat": (dict(enumerate(WALL6)), (6, 7)),                         # the cat and a tilted panel over it
}


# ---------------------------------------------------------------------------------------------------------------- the model: what the generator tracks of a context
class State:
    """the feature state of a context after some ops, as far as the header lets one predict it without a device"""

    def __init__(self):
        self.upload(None)

    def upload(self, name):
        self.scene = name if name in SCENES else None
        self.have = self.scene is not None
        self.spheres, self.meshes = (dict(SCENES[name][0]), SCENES[name][1]) if self.have else ({}, ())
        self.lights, self.radii = [LIGHT], [0.0]
        self.lens, self.shutter, self.env, self.env_share = (0.0, 1.0), False, None, 0.0
        self.emission, self.emit_share = {}, 0.5
        self.tex, self.smooth, self.moved = set(), set(), 0

    def copy(self):
        s = State.__new__(State)
        s.__dict__.update({k: (v.copy() if isinstance(v, (dict, set, list)) else v) for k, v in self.__dict__.items()})
        return s

    # -- facts
    forest = property(lambda s: len(s.meshes) > 1)
    lens_on = property(lambda s: s.lens[0] > 0)
    soft = property(lambda s: any(r > 0 for r in s.radii))
    emit_on = property(lambda s: any(c > 0 for rgb in s.emission.values() for c in rgb))
    lights_fact = property(lambda s: 2 if s.soft else 1 if len(s.lights) > 1 else 0)       # rtk::AdvFacts::lights
    apart = property(lambda s: s.lens_on or s.shutter or s.env is not None or s.emit_on)     # a frame's chains stay away from the still view

    def frame_code(self):
        """what a frame's own chain of wf_advance launches answers (lights_refuse in rt_host_render.hip.h, wf_chain): 0 it renders"""
        if not self.have:
            return NO_SCENE
        if self.emit_on and (self.env is not None or self.shutter):
            return UNSUPPORTED
        if self.env is not None and self.shutter:
            return UNSUPPORTED
        if self.shutter and (len(self.lights) > 1 or self.soft):
            return UNSUPPORTED
        return 0

    def other_code(self):
        """the entries that are no such chain -- rt_count_work, rt_render_counts*, the other variants, animated batches: any of the features refuses them"""
        if not self.have:
            return NO_SCENE
        return UNSUPPORTED if (self.apart or len(self.lights) > 1 or self.soft) else 0

    def predict(self, op):
        """0: the op does what it says; otherwise the RT_ERR_* it raises"""
        if op[0] == "refuse":
            return op[1]
        if op[0] == "frame":
            return self.frame_code()
        if op[0] == "by":
            if op[1] in ("count_work", "render_counts"):
                return self.other_code()
            if op[1] == "stats_frame":
                return self.frame_code()
            return 0 if self.have or op[1] == "getters" else NO_SCENE
        if op[0] == "scene_upload":
            return INVALID if op[1] in FAILING else 0
        return 0 if self.have else NO_SCENE

    def still_level(self, sigma):
        """what a rendered frame's chains are eligible for (launch_wavefront): None -- they do not come to the still view at all"""
        if self.apart:
            return None
        if sigma != 0:
            return 0
        return 1 if self.lights_fact else 2 if self.tex else 3

    def scene_bits(self):
        """what stands for the bytes of rtk::Scene that the host edits in place: the first light and the spheres"""
        return (self.lights[0], tuple(sorted(self.spheres.items())))

    def facts(self):
        """rtk::AdvFacts of a frame's chain"""
        return dict(tex=bool(self.tex), lens=self.lens_on, lights=self.lights_fact, shutter=self.shutter, sky=self.env is not None,
                    sample=self.env is not None and self.env_share > 0, emit=self.emit_on)

    # -- the ops
    def apply(self, op):
        if op[0] in ("refuse", "frame", "by"):
            return self
        if op[0] == "scene_upload":
            self.upload(op[1])
            return self
        if self.have:
            getattr(self, "_" + op[0])(*op[1:])
        return self

    def _fresh(self):
        self.moved += 1
        return ("moved", self.moved)                                   # a value the device computes: new, whatever it is

    def _set_light(self, pos, I):
        self.lights, self.radii = [(tuple(pos), I)], [0.0]

    def _set_lights(self, lights):
        self.lights, self.radii = [(tuple(p), I) for p, I in lights], [0.0] * len(lights)

    def _set_light_at(self, k, pos, I):
        self.lights[k] = (tuple(pos), I)

    def _move_light(self, w):
        self.lights, self.radii = [self._fresh()], self.radii[:1]     # the list collapses to light 0, moved; it keeps its radius

    def _move_light_at(self, k, w):
        self.lights[k] = self._fresh()

    def _set_light_radii(self, radii):
        self.radii = list(radii)

    def _set_light_radius_at(self, k, r):
        self.radii[k] = r

    def _set_lens(self, r, f):
        self.lens = (r, f)

    def _set_shutter(self, light, objects):
        self.shutter = any(v != 0 for v in (light or ())) or any(c != 0 for v in (objects or {}).values() for c in v)

    def _set_environment(self, recipe):
        self.env = recipe

    def _set_environment_sampling(self, s):
        self.env_share = s

    def _set_emission(self, slot, rgb):
        self.emission[slot] = tuple(rgb)

    def _set_emission_sampling(self, s):
        self.emit_share = s

    def _set_sphere(self, slot, sphere):
        self.spheres[slot] = sphere

    def _move_sphere(self, slot, v):
        self.spheres[slot] = self._fresh()

    def _mesh_transform(self, rot, t, slot):
        pass

    def _mesh_set_vertices(self, recipe, slot, form):
        pass

    def _mesh_snapshot_vertices(self, slot, keep):
        pass

    def _mesh_snapshot_normals(self, slot, keep):
        pass

    def _mesh_rebuild(self, mode, slot):
        pass

    def _slots(self, slot):
        return set(self.meshes) if slot is None else {slot}

    def _mesh_compute_normals(self, slot):
        self.smooth |= self._slots(slot)

    def _mesh_set_normals(self, recipe, slot):
        self.smooth = self.smooth | self._slots(slot) if recipe is not None else self.smooth - self._slots(slot)

    def _mesh_set_texture(self, recipe, slot):
        self.tex = self.tex | self._slots(slot) if recipe is not None else self.tex - self._slots(slot)


# ---------------------------------------------------------------------------------------------------------------- the op table
def _pos(rng):
    return tuple(float(v) / 2 for v in (rng.integers(-60, 61), rng.integers(0, 81), rng.integers(0, 101)))      # in the room, on a grid of 1/2


def _intensity(rng):
    return F(rng.choice([1e10, 3e10, 6e10]))


def _light(rng):
    return (_pos(rng), _intensity(rng))


def _mesh_slot(rng, S, plain=0.5):
    """a mesh of the scene: by its slot, or (a scene of one mesh, sometimes) None -- the plain entry"""
    if not S.forest and rng.random() < plain:
        return None
    return int(rng.choice(S.meshes))


def _sphere_slot(rng, S):
    return int(rng.choice(sorted(S.spheres)))


def _no_such_mesh(rng, S):
    """a slot the per-mesh entries refuse: a sphere's, or one outside the scene"""
    return _sphere_slot(rng, S) if rng.random() < 0.7 else len(S.spheres) + len(S.meshes) + int(rng.integers(0, 3))


def _vertices(rng):
    return ("scale", float(rng.choice([0.875, 1.0, 1.125])), float(rng.integers(-4, 5)) / 2)


def _rot(rng):
    return ("ry", int(rng.choice([-30, -10, 10, 20, 45])))


def _shift(rng):
    return tuple(float(v) / 2 for v in rng.integers(-4, 5, 3))


def _texture(rng):
    return ("noise", int(rng.integers(0, 4)), str(rng.choice(["nearest", "bilinear"])), str(rng.choice(["repeat", "clamp"])))


def _environment(rng):
    return ("sun", int(rng.integers(0, 4))) if rng.random() < 0.7 else ("flat", float(rng.choice([0.0, 0.5, 2.0])))


def _draw_set_lights(rng, S):
    n = int(rng.integers(2, 5))
    return ("set_lights", [_light(rng) for _ in range(n)])


def _draw_set_light_at(rng, S):
    return ("set_light_at", int(rng.integers(len(S.lights))), *_light(rng))


def _draw_radii(rng, S):
    r = [float(rng.choice([0.0, 0.5, 2.0])) for _ in S.lights]
    return ("set_light_radii", r)


def _draw_lens(rng, S):
    return ("set_lens", 0.0, 1.0) if S.lens_on and rng.random() < 0.7 else ("set_lens", float(rng.choice([0.5, 1.0])), float(rng.choice([40.0, 55.0])))


def _draw_shutter(rng, S):
    if S.shutter and rng.random() < 0.7:
        return ("set_shutter", None, None)
    move = lambda: tuple(float(v) / 4 for v in rng.integers(-8, 9, 3))
    light = move() if rng.random() < 0.6 else None
    objects = {_sphere_slot(rng, S): move()} if light is None or rng.random() < 0.5 else None
    return ("set_shutter", light, objects)


def _draw_environment(rng, S):
    return ("set_environment", None) if S.env is not None and rng.random() < 0.4 else ("set_environment", _environment(rng))


def _draw_emission(rng, S):
    slot = int(rng.choice(S.meshes))
    k = rng.random()
    rgb = (0.0, 0.0, 0.0) if k < 0.3 and S.emission.get(slot) else tuple(F(c * rng.choice([0.5, 1.0, 2.0])) for c in LE)
    return ("set_emission", slot, rgb)


def _draw_sphere(rng, S):
    slot = _sphere_slot(rng, S)
    c, r = SCENES[S.scene][0][slot][:2]
    centre = tuple(F(v + d) for v, d in zip(c, rng.integers(-2, 3, 3) / 2))
    albedo = tuple(float(v) for v in rng.choice([0.0, 0.25, 0.5, 1.0], 3))
    kind = rng.random()
    return ("set_sphere", slot, (centre, r, albedo, int(kind > 0.8), 1.5 if kind < 0.15 else 1.0, 1.0))


def _draw_normals(rng, S):
    slot = _mesh_slot(rng, S)
    return ("mesh_set_normals", None if rng.random() < 0.3 else ("radial", float(rng.choice([0.0, 8.0]))), slot)


def _draw_texture(rng, S):
    slot = _mesh_slot(rng, S)
    return ("mesh_set_texture", None if S.tex and rng.random() < 0.35 else _texture(rng), slot)


def _draw_snapshot(name):
    return lambda rng, S: (name, _mesh_slot(rng, S) if rng.random() < 0.7 else None, int(rng.random() < 0.7))


def _refuse_plain_or_slot(name, *rest):
    """a forest refuses the plain entry (RT_ERR_UNSUPPORTED); every scene refuses a sphere's slot"""
    def draw(rng, S):
        if S.forest and rng.random() < 0.5:
            return ("refuse", UNSUPPORTED, name, *[r(rng) if callable(r) else r for r in rest], None)
        return ("refuse", INVALID, name, *[r(rng) if callable(r) else r for r in rest], _no_such_mesh(rng, S))
    return draw


def _refuse_set_vertices(rng, S):
    """a vertex count that is not the mesh's; a forest refuses the plain entry; a sphere's slot"""
    k = rng.random()
    if k < 0.4:
        return ("refuse", INVALID, "mesh_set_vertices", ("short",), _mesh_slot(rng, S), "host")
    if S.forest and k < 0.7:
        return ("refuse", UNSUPPORTED, "mesh_set_vertices", _vertices(rng), None, "host")
    return ("refuse", INVALID, "mesh_set_vertices", _vertices(rng), _no_such_mesh(rng, S), str(rng.choice(["host", "device3"])))


def _k_outside(rng, S):
    return int(rng.choice([-1, len(S.lights), len(S.lights) + 3]))


def _slot_of(i):
    return lambda op: op[i]


# kind: "abs" -- the last call of its key wins; "rel" -- calls compose and are replayed in order.  still: what csrc/rt_still.h and DESIGN.md section 5.1 say the edit does to
# the three levels -- "mesh" everything is emptied, "shading" shadow and records are emptied, "scene" the key's Scene bytes change if the value does, "feature" the op turns the
# lens, the shutter, the sky or an emission on or off, "none".  domain: the state the op belongs to (a relative op pins every earlier op of its domain); key / resets: the state
# an absolute op sets whole, and what it sets besides; slot: where the op's object slot stands (None: it has none); draw / refuse: valid and refused arguments from the state
Row = namedtuple("Row", "kind still domain key resets slot draw refuse")
TABLE = {
    "scene_upload": Row("abs", "mesh", "scene", "scene", (), None, None, None),                     # (drawn by the families themselves)
    "set_light": Row("abs", "scene", "lights", "lights", ("radii",), None, lambda rng, S: ("set_light", *_light(rng)), None),   # (accepts every light)
    "set_lights": Row("abs", "scene", "lights", "lights", ("radii",), None, _draw_set_lights,
                      lambda rng, S: ("refuse", INVALID, "set_lights", [_light(rng), (_pos(rng), -1.0)])),
    "set_light_at": Row("rel", "scene", "lights", None, (), None, _draw_set_light_at, lambda rng, S: ("refuse", INVALID, "set_light_at", _k_outside(rng, S), *_light(rng))),
    "move_light": Row("rel", "scene", "lights", None, (), None, lambda rng, S: ("move_light", float(rng.choice([0.5, 1.0, 2.0]))), None),
    "move_light_at": Row("rel", "scene", "lights", None, (), None, lambda rng, S: ("move_light_at", int(rng.integers(len(S.lights))), float(rng.choice([0.5, 1.0, 2.0]))),
                         lambda rng, S: ("refuse", INVALID, "move_light_at", _k_outside(rng, S), 1.0)),
    "set_light_radii": Row("abs", "shading", "lights", "radii", (), None, _draw_radii,
                           lambda rng, S: ("refuse", INVALID, "set_light_radii", ["nan" if rng.random() < 0.5 else -1.0] + [0.0] * (len(S.lights) - 1))),
    "set_light_radius_at": Row("rel", "shading", "lights", None, (), None, lambda rng, S: ("set_light_radius_at", int(rng.integers(len(S.lights))), float(rng.choice([0.0, 0.5, 2.0]))),
                               lambda rng, S: ("refuse", INVALID, "set_light_radius_at", _k_outside(rng, S), 1.0)),
    "set_lens": Row("abs", "feature", "lens", "lens", (), None, _draw_lens, lambda rng, S: ("refuse", INVALID, "set_lens", *[("nan", 40.0), (-1.0, 40.0), (1.0, 0.0)][int(rng.integers(3))])),
    "set_shutter": Row("abs", "feature", "shutter", "shutter", (), None, _draw_shutter,
                       lambda rng, S: ("refuse", INVALID, "set_shutter", None, {int(rng.choice(S.meshes)) if rng.random() < 0.6 else 15: (0.5, 0.0, 0.0)})),
    "set_environment": Row("abs", "feature", "env", "env", (), None, _draw_environment, lambda rng, S: ("refuse", INVALID, "set_environment", ("bad", int(rng.integers(0, 3))))),
    "set_environment_sampling": Row("abs", "feature", "env_share", "env_share", (), None, lambda rng, S: ("set_environment_sampling", float(rng.choice([0.0, 0.25, 0.5, 1.0]))),
                                    lambda rng, S: ("refuse", INVALID, "set_environment_sampling", [1.5, -0.5, "nan"][int(rng.integers(3))])),
    "set_emission": Row("abs", "feature", "emission", "emission", (), _slot_of(1), _draw_emission,
                        lambda rng, S: ("refuse", INVALID, "set_emission", _sphere_slot(rng, S), LE) if rng.random() < 0.6 else
                        ("refuse", INVALID, "set_emission", int(rng.choice(S.meshes)), (1.0, -1.0, 1.0))),
    "set_emission_sampling": Row("abs", "none", "emit_share", "emit_share", (), None, lambda rng, S: ("set_emission_sampling", float(rng.choice([0.0, 0.5, 1.0]))),
                                 lambda rng, S: ("refuse", INVALID, "set_emission_sampling", [1.5, -0.5, "nan"][int(rng.integers(3))])),
    "set_sphere": Row("abs", "scene", "sphere", "sphere", (), _slot_of(1), _draw_sphere, lambda rng, S: ("refuse", INVALID, "set_sphere", int(rng.choice(S.meshes)), WALL6[0])),
    "move_sphere": Row("rel", "scene", "sphere", None, (), _slot_of(1), lambda rng, S: ("move_sphere", _sphere_slot(rng, S), _shift(rng)),
                       lambda rng, S: ("refuse", INVALID, "move_sphere", int(rng.choice(S.meshes)), (1.0, 0.0, 0.0))),
    "mesh_transform": Row("rel", "mesh", "mesh", None, (), _slot_of(3), lambda rng, S: ("mesh_transform", _rot(rng), _shift(rng), _mesh_slot(rng, S) if rng.random() < 0.8 else None),
                          lambda rng, S: ("refuse", INVALID, "mesh_transform", _rot(rng), _shift(rng), _no_such_mesh(rng, S))),
    "mesh_set_vertices": Row("rel", "mesh", "mesh", None, (), _slot_of(2), lambda rng, S: ("mesh_set_vertices", _vertices(rng), _mesh_slot(rng, S), str(rng.choice(["host", "device3", "device4"]))),
                             _refuse_set_vertices),
    "mesh_snapshot_vertices": Row("rel", "none", "mesh", None, (), _slot_of(1), _draw_snapshot("mesh_snapshot_vertices"),
                                  lambda rng, S: ("refuse", INVALID, "mesh_snapshot_vertices", *((_sphere_slot(rng, S), 1) if rng.random() < 0.5 else (None, 2)))),
    "mesh_snapshot_normals": Row("rel", "none", "mesh", None, (), _slot_of(1), _draw_snapshot("mesh_snapshot_normals"),
                                 lambda rng, S: ("refuse", INVALID, "mesh_snapshot_normals", *((_sphere_slot(rng, S), 1) if rng.random() < 0.5 else (None, 2)))),
    "mesh_compute_normals": Row("abs", "shading", "mesh", "normals", (), _slot_of(1), lambda rng, S: ("mesh_compute_normals", _mesh_slot(rng, S)), _refuse_plain_or_slot("mesh_compute_normals")),
    "mesh_set_normals": Row("abs", "shading", "mesh", "normals", (), _slot_of(2), _draw_normals, _refuse_plain_or_slot("mesh_set_normals", ("radial", 0.0))),
    "mesh_rebuild": Row("rel", "mesh", "mesh", None, (), _slot_of(2), lambda rng, S: ("mesh_rebuild", str(rng.choice(["reference", "lbvh"])), _mesh_slot(rng, S)),
                        lambda rng, S: ("refuse", INVALID, "mesh_rebuild", "lbvh", _no_such_mesh(rng, S))),
    "mesh_set_texture": Row("abs", "shading", "tex", "tex", (), _slot_of(2), _draw_texture, lambda rng, S: ("refuse", INVALID, "mesh_set_texture", ("noise", 0, "nearest", "repeat"), _no_such_mesh(rng, S))),
}
# the header's state-changing entries that have no row, and why (tests/test_edit_sequences_model.py reads the header and asks for one or the other)
EXCLUDED = {
    "rt_mesh_rebuild": "rt_mesh_rebuild_mode(RT_BVH_REFERENCE) under its first name; the row mesh_rebuild drives the mode entry with both modes.",
    "rt_mesh_build_stats": "A getter: the figures of the last LBVH build, which no frame reads.",
    "rt_mesh_get_vertex_normals": "A getter of what rt_mesh_compute_normals wrote; the row mesh_compute_normals is compared through the frames and the canonical replay.",
    "rt_mesh_snapshot_mask": "A getter; every checkpoint compares it.",
    "rt_mesh_normal_snapshot_mask": "A getter; every checkpoint compares it.",
    "rt_scene_get_light": "A getter; every checkpoint compares it.", "rt_scene_get_lights": "A getter; every checkpoint compares it.",
    "rt_scene_get_light_radii": "A getter; every checkpoint compares it.", "rt_scene_get_sphere": "A getter; every checkpoint compares it, slot by slot.",
    "rt_camera_get_lens": "A getter; every checkpoint compares it.", "rt_scene_get_shutter": "A getter; every checkpoint compares it.",
    "rt_scene_get_environment": "A getter; every checkpoint compares it.", "rt_scene_get_environment_sampling": "A getter; every checkpoint compares it.",
    "rt_scene_get_emission": "A getter; every checkpoint compares it, mesh by mesh.", "rt_scene_get_emission_sampling": "A getter; every checkpoint compares it.",
    "rt_multi_create": "The rt_multi_* group is another object: several contexts behind one handle, with an upload and no edit entries; tests/test_multi_rank.py drives it.",
    "rt_multi_destroy": "The rt_multi_* group: see rt_multi_create.", "rt_multi_last_error": "The rt_multi_* group: see rt_multi_create.",
    "rt_multi_scene_upload": "The rt_multi_* group: see rt_multi_create.", "rt_multi_scene_upload_meshes": "The rt_multi_* group: see rt_multi_create.",
    "rt_multi_get_stats": "The rt_multi_* group: see rt_multi_create.",
}
GETTERS = ("light", "lights", "light_radii", "lens", "shutter", "environment", "environment_sampling", "emission_sampling", "emission", "sphere", "mesh_snapshot_mask",
           "mesh_normal_snapshot_mask", "layout_hash")
BYSTANDERS = ("render_aov", "trace_rays", "kat_mesh", "kat_emission_table", "kat_environment_table", "count_work", "render_counts", "stats_frame", "getters")


def is_edit(op):
    return op[0] in TABLE


def _key(op):
    """(the state an absolute op sets, its object slot or None) and what else it sets"""
    row = TABLE[op[0]]
    slot = row.slot(op) if row.slot else None
    return [(row.key, slot)] + [(k, None) for k in row.resets]


def _domain(op):
    row = TABLE[op[0]]
    return (row.domain, row.slot(op) if row.slot and row.domain == "sphere" else None)


def canonical(ops, upto=None):
    """What a fresh context needs to stand where ops[:upto] left theirs: the last upload, then every relative op since it in order and, of every absolute state, the last
    call -- no frames, no bystanders, no refused calls.  An absolute call stays where it stood, and it stays although a later call of its key follows if a relative op of its
    domain lies between them: that op composed with it (set_lights before move_light_at, mesh_set_normals before mesh_transform)."""
    ops = list(ops if upto is None else ops[:upto])
    last = max((i for i, o in enumerate(ops) if o[0] == "scene_upload"), default=None)
    if last is None:
        return []
    kept = [o for o in ops[last:] if is_edit(o)]
    out = [kept[0]]
    for i, o in enumerate(kept[1:], 1):
        if TABLE[o[0]].kind == "abs":
            (mine, slot), dead = _key(o)[0], False
            for p in kept[i + 1:]:
                if TABLE[p[0]].kind == "rel" and _domain(p) == _domain(o):
                    break
                if TABLE[p[0]].kind == "abs" and any(k == mine and (s is None or s == slot) for k, s in _key(p)):
                    dead = True
                    break
            if dead:
                continue
        out.append(o)
    return out


# ---------------------------------------------------------------------------------------------------------------- the families and the generator
# name -> (start scene, the ops that follow the upload, the edit rows' weights, the frame entries, chance of a still run after an edit, chance to enter a refused combination)
Family = namedtuple("Family", "scene prologue weights entries run enter")
_MESH_ROWS = dict(mesh_transform=3, mesh_set_vertices=3, mesh_rebuild=2, mesh_compute_normals=1.5, mesh_set_normals=1.5, mesh_snapshot_vertices=1, mesh_snapshot_normals=1, set_light=1)
FAMILY = {
    "still": Family("cat", (), dict(set_light=3, move_light=2, set_sphere=3, move_sphere=2), ("render",), 0.6, 0.0),
    "mesh": Family("cat", (), _MESH_ROWS, ("render",), 0.45, 0.0),
    "forest": Family("two_cats", (("mesh_set_texture", ("noise", 1, "bilinear", "repeat"), 3), ("mesh_compute_normals", 7)), dict(_MESH_ROWS, mesh_set_texture=1.5), ("render",), 0.45, 0.0),
    "lights": Family("cat", (), dict(set_lights=3, set_light=2, set_light_radii=2, set_light_at=2, move_light_at=2, set_light_radius_at=2, move_light=1), ENTRIES, 0.4, 0.0),
    "toggles": Family("open_cat", (), dict(set_lens=3, set_shutter=3, set_environment=3, set_light=2, mesh_set_texture=2, mesh_transform=1.5, set_lights=1, set_sphere=1, set_light_radii=0.5),
                      ("render",), 0.4, 0.5),
    "sky": Family("open_cat", (("mesh_set_texture", ("noise", 2, "bilinear", "clamp"), None), ("set_environment", ("sun", 0)), ("set_lights", [LIGHT, ((10.0, 30.0, 20.0), F(1e10))])),
                  dict(set_environment=3, set_environment_sampling=3, set_lights=1.5, set_light_at=1, mesh_set_texture=1, set_light=1, set_shutter=0.5), ENTRIES, 0.4, 0.5),
    "emit": Family("panel_cat", (("set_emission", 7, tuple(F(c) for c in LE)),),
                   dict(set_emission=4, set_emission_sampling=3, mesh_transform=2, mesh_set_vertices=1.5, mesh_rebuild=1.5, set_light=1, set_lights=1, set_environment=0.5, set_shutter=0.5),
                   ENTRIES, 0.4, 0.5),
    "everything": Family("panel_cat", (), {k: 1 for k in TABLE if k != "scene_upload"}, ENTRIES, 0.4, 0.8),
}


def _draw_frame(rng, fam, size=None, entry=None):
    W, H = size or SIZES[int(rng.integers(2))]
    entry = entry or str(rng.choice(fam.entries))
    sigma = F(0.2) if size is None and rng.random() < 0.1 else 0.0           # one frame kind with a jittered camera: never eligible
    return ("frame", entry, W, H, int(rng.integers(1, 3)), int(rng.integers(0, 4)), int(rng.integers(1, 1 << 20)), sigma)


def _draw_bystander(rng, S):
    names = [n for n in BYSTANDERS if not (n == "kat_emission_table" and not S.emit_on) and not (n == "kat_environment_table" and not (S.env is not None and S.env_share > 0))]
    W, H = SIZES[int(rng.integers(2))]
    tables = [n for n in names if n.endswith("_table")]
    if tables and rng.random() < 0.4:                                       # the known answers of a feature that is on: while it is
        names = tables
    return ("by", str(rng.choice(names)), W, H)


def _cure(S):
    """the edits that lead out of a combination no frame renders"""
    if S.shutter:
        return ("set_shutter", None, None)
    return ("set_environment", None)


def still_runs(ops):
    """the stretches of three or more consecutive frame ops of one entry and size with a still camera, as lists of steps"""
    runs, cur = [], []
    for k, op in enumerate(ops):
        still = op[0] == "frame" and op[7] == 0
        if still and cur and ops[cur[-1]][1:4] == op[1:4]:
            cur.append(k)
            continue
        if len(cur) >= 3:
            runs.append(cur)
        cur = [k] if still else []
    if len(cur) >= 3:
        runs.append(cur)
    return runs


def sequence(family, seed):
    """LENGTH ops drawn from np.random.default_rng([family index, seed]); every number in them is a binary32 value"""
    fam = FAMILY[family]
    rng = np.random.default_rng([FAMILIES.index(family), int(seed)])
    S, ops, refused = State(), [], 0
    names, weights = list(fam.weights), np.array(list(fam.weights.values()), float)

    def push(op):
        ops.append(op)
        S.apply(op)

    def run(n=3):
        size, entry = SIZES[int(rng.integers(2))], str(rng.choice(fam.entries))
        for _ in range(n):
            push(_draw_frame(rng, fam, size, entry))

    push(("scene_upload", fam.scene))
    for op in fam.prologue:
        push(op)
    # family `everything`: another scene in mid-sequence; an upload that fails, one frame and one edit that find no scene, and a good upload
    events = {16: [("scene_upload", "open_cat")], 30: None} if family == "everything" else {}
    if family == "forest":
        # one of the two cats is textured from the start, and a textured scene keeps no records: once a sequence the texture is taken off around a still run at the
        # checkpoints' size -- a fill, a store and two resumes --, a light edit empties what was stored, and the texture comes back
        events = {18: [("mesh_set_texture", None, None)] + [_draw_frame(rng, fam, SIZES[0], "render") for _ in range(4)] +
                      [("set_light", *_light(rng)), _draw_frame(rng, fam, SIZES[0], "render"), ("mesh_set_texture", _texture(rng), 3)]}
    while len(ops) < LENGTH:
        due = [k for k in events if k <= len(ops)]
        if due:
            k = due[0]
            for op in events.pop(k) or [("scene_upload", FAILING[int(seed) % 2]), _draw_frame(rng, fam), ("refuse", NO_SCENE, "set_light", *_light(rng)), ("scene_upload", "cat")]:
                refused += op[0] == "frame" and S.predict(op) != 0
                push(op)
            continue
        owed = 4 - len(still_runs(ops))                                    # the floor of four still runs: the last ops are theirs if the draw has not made them
        force = family in COUNTED and owed > 0 and len(ops) >= LENGTH - 4 * owed - 1
        r = rng.random()
        if force or r < 0.34:
            op = None
            if family == "toggles" and S.apart and rng.random() < 0.6:     # what is turned on is soon turned off again: the frames on either side are the test
                op = ("set_lens", 0.0, 1.0) if S.lens_on else ("set_shutter", None, None) if S.shutter else ("set_environment", None)
            for _ in range(8 if op is None else 0):
                name = names[int(rng.choice(len(names), p=weights / weights.sum()))]
                cand = TABLE[name].draw(rng, S)
                if S.forest and cand[0] in ("mesh_set_normals", "mesh_set_texture") and cand[2] is None and cand[1] is not None:
                    continue                                               # (the plain entries set ONE mesh's normals or texture; they take one back on every mesh)
                entering = S.copy().apply(cand).frame_code() != 0
                if entering and (force or not (rng.random() < fam.enter and refused < 2)):
                    continue
                op = cand
                break
            if op is None:
                continue
            push(op)
            if S.frame_code() != 0:                                        # entered on purpose: one frame that is refused, then the way out
                push(_draw_frame(rng, fam))
                refused += 1
                while S.frame_code() != 0:
                    push(_cure(S))
            elif force or rng.random() < fam.run:
                run(3 if family != "still" else int(rng.integers(3, 6)))
        elif r < 0.42:
            make = TABLE[names[int(rng.integers(len(names)))]].refuse
            if make is not None:
                push(make(rng, S))
        elif r < 0.54:
            push(_draw_bystander(rng, S))
        else:
            push(_draw_frame(rng, fam))
    return ops[:LENGTH]


def checkpoints(ops):
    """the steps k at which the context after ops[:k] is compared with a fresh one: every eighth, the step after every op that is predicted refused, and the end"""
    S, out = State(), set()
    for k, op in enumerate(ops):
        if S.predict(op) != 0:
            out.add(k + 1)
        S.apply(op)
        if (k + 1) % 8 == 0:
            out.add(k + 1)
    out.add(len(ops))
    return sorted(out)


def probe(k):
    return ("frame", "render", *PROBE, 1000 + k, 0.0)


def with_probes(ops):
    """the ops as the device test issues them to the context under test: the checkpoints' frames between them"""
    at, out = set(checkpoints(ops)), []
    for k, op in enumerate(ops):
        out.append(op)
        if k + 1 in at:
            out.append(probe(k + 1))
    return out


def states(ops):
    """the state before every op, and the one after the last"""
    S, out = State(), []
    for op in ops:
        out.append(S.copy())
        S.apply(op)
    return out + [S]


# ---------------------------------------------------------------------------------------------------------------- the still view's counters
# What the device test renders on a counted sequence's contexts first: whatever the sequences before it left, the three levels then hold the words of this still view under
# its keys -- a state the replay can start from, so that the first misses of the sequence are exact too
PRIMER = (("scene_upload", "cat"),) + tuple(("frame", "render", 64, 48, 1, 2, 900 + k, 0.0) for k in range(3))


def still_events(ops, probes=True, primer=()):
    """The events of hostlib.still_replay for what a default context does with `ops` (the checkpoints' frames included), and after how many events each op is done.  For the
    COUNTED families: frames through `render` alone (and, for the named orders, render_device on a caller's stream), two sub-frames.  Written from csrc/rt_still.h's rules and DESIGN.md section 5.1:
      an upload is a shading change and a mesh change; a "mesh" op is a mesh change, a "shading" op a shading change (a radius: if it changes); a "scene" op changes the Scene
      bytes of the shading key if the value differs; a "feature" op that turns the lens, the shutter or the sky on or off empties everything like a mesh change;
      a rendered frame is one chunk of two chains -- at level 3, 2 with a textured mesh, 1 with several lights or a radius, 0 with a jittered camera, and none at all while a
      feature keeps the chains away; rt_count_work is one chain of level 0, a frame under rt_stats_enable two; refused calls and the other bystanders are nothing.
    primer: ops issued before `ops` (PRIMER); their events come first and `done` counts them in."""
    S, ev, done, ids = State(), [], [], {}
    ident = lambda *k: ids.setdefault(k, len(ids) + 1)
    MESH, SHADING, FLAGS = (2,), (3,), 7

    def chunk(level, W, H, segs, parts=2, entry="render"):
        ev.append((0, level, ident("ray", W, H, parts, entry), ident("scene", S.scene_bits()), 1))     # (a caller's stream is part of the ray key)
        ev.extend((1, j, segs, FLAGS) for j in range(parts))

    for op in list(primer) + (with_probes(ops) if probes else list(ops)):
        code = S.predict(op)
        if op[0] == "scene_upload":
            ev.extend([SHADING, MESH])                                      # (also when it fails: the old scene's words are stale either way)
        elif code != 0:
            pass
        elif op[0] == "frame":
            level = S.still_level(op[7])
            if level is not None:
                chunk(level, op[2], op[3], op[5] + 1, entry=op[1])
        elif op[0] == "by":
            if op[1] == "count_work":
                chunk(0, op[2], op[3], 2, parts=1)
            elif op[1] == "stats_frame" and not S.apart:
                chunk(0, op[2], op[3], 2)
        else:
            cls, before = TABLE[op[0]].still, S.copy()
            after = S.copy().apply(op)
            if cls == "mesh":
                ev.append(MESH)
            elif cls == "shading" and op[0] not in ("set_light_radii", "set_light_radius_at"):
                ev.append(SHADING)
            elif cls == "feature" and (before.lens_on != after.lens_on or before.shutter != after.shutter or op[0] == "set_environment" and (before.env, after.env) != (None, None) or
                                       op[0] == "set_environment_sampling" and before.env_share != after.env_share):
                ev.append(MESH)
            elif _padded(before.radii) != _padded(after.radii):
                ev.append(SHADING)                                          # a new light is a point, a list that collapses drops its other radii: a radius that changes
        S.apply(op)
        done.append(len(ev))
    return ev, done[len(primer):]


def _padded(radii):
    return tuple(radii) + (0.0,) * (16 - len(radii))


def expected_use(ops):
    """(hit, shadow, records): whether the sequence holds a still run through `render` that must use the level -- two frames in a row for the first two, three for the
    records -- with no feature in the way and no checkpoint's frame of another size between them"""
    use, vops = [False, False, False], with_probes(ops)
    sts = states(vops)
    run, key = 0, None
    for op, S in zip(vops, sts):
        ok = op[0] == "frame" and op[1] == "render" and op[7] == 0 and S.predict(op) == 0 and S.still_level(0.0) is not None
        k = (op[2:4], S.still_level(0.0), S.scene_bits()) if ok else None
        run = run + 1 if ok and k == key else 1 if ok else 0
        key = k
        if ok and run >= 2:
            use[0] = True
            use[1] = use[1] or k[1] >= 2
        if ok and run >= 3 and k[1] >= 3:
            use[2] = True
    return tuple(use)


# ---------------------------------------------------------------------------------------------------------------- driving a context
_ASSETS = {}


def scene_assets(name, g):
    """-> (spheres, mesh argument of scene_upload, {slot: (base vertices, triangles' vertex indices as uploaded)}), built once"""
    if name in _ASSETS:
        return _ASSETS[name]
    from raytracinggpu_amd import hostlib
    from . import material_scenes as ms
    from . import still_view as sv
    tri = lambda d: np.asarray(d["indices"], np.int32).reshape(len(d["indices"]), -1)[:, :3].copy()
    if name in ("cat", "cpu_glass", "open_cat", "bad_index"):
        spheres = list(rt.scenes.WALLS[:2]) if name == "open_cat" else rt.scenes.spheres("cpu")
        m = sv.cat(g, slot=len(spheres))
        if name == "cpu_glass":
            m.update(in_refraction_index=1.5, out_refraction_index=1.0)
        if name == "bad_index":
            ix = np.array(m["indices"], np.int32)
            ix[len(ix) // 2, 1] = len(m["vertices"])
            m["indices"] = ix
        meshes = [m]
    elif name == "two_cats":
        spheres, meshes = ms.capi_scene("two_cats", g["vertices"], g["tri_obj_order"])
    elif name == "panel_cat":
        spheres = rt.scenes.spheres("cpu")
        meshes = [sv.cat(g), hostlib.build_mesh(*rt.scenes.panel(*PANEL), albedo=(0.5, 0.5, 0.5), object_slot=7)]
    elif name == "seventeen":
        spheres, meshes = [((float(4 * k - 32), 0.0, 0.0), 1.5, (0.5, 0.5, 0.5)) for k in range(17)], []
    else:
        raise ValueError(name)
    parts = {int(m["object_slot"]): (np.asarray(m["vertices"], f32).reshape(-1, 3), tri(m)) for m in meshes}
    _ASSETS[name] = (spheres, (meshes[0] if len(meshes) == 1 else meshes) if meshes else None, parts)
    return _ASSETS[name]


def rotation(recipe):
    a = np.deg2rad(recipe[1])
    c, s = f32(np.cos(a)), f32(np.sin(a))
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], f32)


def vertices(recipe, base):
    if recipe[0] == "short":
        return base[:-1]
    return (base * f32(recipe[1]) + np.array([0, recipe[2], 0], f32)).astype(f32)


def normals(recipe, base):
    c = base - base.mean(0) + np.array([0, recipe[1], 0], f32)
    return (c / np.maximum(np.linalg.norm(c, axis=1, keepdims=True), 1e-6)).astype(f32)


def planar_uv(v):
    lo, hi = v.min(0), v.max(0)
    span = np.where(hi[:2] > lo[:2], hi[:2] - lo[:2], 1).astype(f32)
    return (((v[:, :2] - lo[:2]) / span) * f32(2.6) - f32(0.8)).astype(f32)     # outside [0, 1] on purpose


def texture(recipe):
    r = np.random.default_rng(100 + recipe[1])
    return r.integers(0, 256, size=(23, 37, 3), dtype=np.uint8), r.random(256).astype(f32)


def environment(recipe):
    from raytracinggpu_amd import environment as envm
    if recipe[0] == "flat":
        return np.full((8, 8, 3), recipe[1], f32)
    if recipe[0] == "bad":
        a = np.full((8, 8, 3), 0.5, f32)
        a[3, 4, recipe[1]] = -1.0
        return a
    sky = envm.gradient_sky((0.2, 0.4, 1.0), (0.8, 0.8, 0.7), (0.1, 0.1, 0.1), 16)
    d = [(0.3, 0.8, 0.5), (-0.5, 0.6, 0.2), (0.0, 1.0, 0.1), (0.6, 0.3, 0.7)][recipe[1]]
    return envm.add_sun(sky, np.asarray(d) / np.linalg.norm(d), 0.25, (3e3, 2.5e3, 2e3))


SENTINEL = np.uint32(0x7fc12345)


def sentinel(shape, dtype=f32):
    a = np.empty(shape, dtype)
    a.view(np.uint8 if dtype == np.uint8 else np.uint32)[...] = 0xa5 if dtype == np.uint8 else SENTINEL
    return a


def untouched(a):
    return bool((a.view(np.uint8) == 0xa5).all()) if a.dtype == np.uint8 else bool((a.view(np.uint32) == SENTINEL).all())


class Driver:
    """A context and what a caller has to remember of its scene to go on editing it: the meshes' base vertices and their triangles in the order the last rebuild reported"""

    def __init__(self, ctx, g, stream=None):
        self.c, self.g, self.stream, self.parts, self.name = ctx, g, stream, {}, None
        self.out = None                                                # the buffers the last frame op was given, sentinel-filled: a refused frame leaves them as they were

    # -- edits
    def apply(self, op):
        """an edit, a refused edit (raises), a frame -> list of arrays, or a bystander -> whatever it answers"""
        if op[0] == "refuse":
            return self.apply(op[2:])
        if op[0] == "frame":
            return self.frame(*op[1:])
        if op[0] == "by":
            return self.by(*op[1:])
        return getattr(self, "_" + op[0])(*op[1:])

    def _scene_upload(self, name):
        spheres, mesh, parts = scene_assets(name, self.g)
        self.parts, self.name = {}, None                                # (a failed upload leaves no scene)
        self.c.scene_upload(spheres, mesh)
        self.parts, self.name = {k: [v, t.copy()] for k, (v, t) in parts.items()}, name

    def _part(self, slot):
        if slot in self.parts:
            return self.parts[slot]
        if slot is None and self.parts:
            return self.parts[min(self.parts)]
        return next(iter(scene_assets("cat", self.g)[2].values()))       # a refused call's arrays: any

    def _set_light(self, pos, I):
        self.c.set_light(pos, num(I))

    def _set_lights(self, lights):
        self.c.set_lights([(p, num(I)) for p, I in lights])

    def _set_light_at(self, k, pos, I):
        self.c.set_light_at(k, pos, num(I))

    def _move_light(self, w):
        self.c.move_light(w)

    def _move_light_at(self, k, w):
        self.c.move_light_at(k, w)

    def _set_light_radii(self, radii):
        self.c.set_light_radii([num(r) for r in radii])

    def _set_light_radius_at(self, k, r):
        self.c.set_light_radius_at(k, num(r))

    def _set_lens(self, r, f):
        self.c.set_lens(num(r), num(f))

    def _set_shutter(self, light, objects):
        self.c.set_shutter(light, objects)

    def _set_environment(self, recipe):
        self.c.set_environment(None if recipe is None else environment(recipe))

    def _set_environment_sampling(self, s):
        self.c.set_environment_sampling(num(s))

    def _set_emission(self, slot, rgb):
        self.c.set_emission(slot, rgb)

    def _set_emission_sampling(self, s):
        self.c.set_emission_sampling(num(s))

    def _set_sphere(self, slot, sphere):
        self.c.set_sphere(slot, sphere)

    def _move_sphere(self, slot, v):
        self.c.move_sphere(slot, v, dt=0.25)

    def _mesh_transform(self, rot, t, slot):
        self.c.mesh_transform(rotation(rot), np.asarray(t, f32), object_slot=slot)

    def _mesh_set_vertices(self, recipe, slot, form):
        v = vertices(recipe, self._part(slot)[0])
        if form == "host":
            self.c.mesh_set_vertices(v, object_slot=slot)
            return
        import torch
        stride = int(form[-1])
        rec = np.zeros((len(v), stride), f32)
        rec[:, :3] = v
        dev = torch.from_numpy(rec).cuda()
        self.c.mesh_set_vertices(object_slot=slot, device_ptr=dev.data_ptr(), stride=stride, n_vertices=len(v))
        self.c.synchronize()                                             # (the positions are read on the context's stream: the tensor lives until then)

    def _mesh_snapshot_vertices(self, slot, keep):
        self.c.mesh_snapshot_vertices(slot, keep)

    def _mesh_snapshot_normals(self, slot, keep):
        self.c.mesh_snapshot_normals(slot, keep)

    def _mesh_compute_normals(self, slot):
        self.c.mesh_compute_normals(slot)

    def _mesh_set_normals(self, recipe, slot):
        v, t = self._part(slot)
        if recipe is None:
            self.c.mesh_set_normals(None, None, object_slot=slot)
        else:
            self.c.mesh_set_normals(normals(recipe, v), t, object_slot=slot)

    def _mesh_rebuild(self, mode, slot):
        part = self._part(slot)
        _, order = self.c.mesh_rebuild(len(part[1]), mode, object_slot=slot)
        if slot in self.parts or slot is None:
            part[1] = part[1][order]                                     # per-triangle arrays go in the order the last rebuild reported

    def _mesh_set_texture(self, recipe, slot):
        v, t = self._part(slot)
        if recipe is None:
            self.c.mesh_set_texture(None, None, None, object_slot=slot)
        else:
            texels, decode = texture(recipe)
            self.c.mesh_set_texture(planar_uv(v), t, texels, filter=recipe[2], wrap=recipe[3], decode=decode, object_slot=slot)

    # -- frames
    @staticmethod
    def params(W, H, spp, b, seed, sigma=0.0):
        d = dict(rt.scenes.CPU_LAUNCHER)
        d.update(sigma=sigma, seed=seed)
        return rt.make_params(W, H, spp, b, **d)

    def frame(self, entry, W, H, spp, b, seed, sigma):
        """-> the frame's arrays: [rows, W, 4] float32, or uint8 for the 8-bit entries"""
        import ctypes as C
        import torch
        c, p = self.c, self.params(W, H, spp, b, seed, sigma)
        if entry == "render":
            self.out = [sentinel((H, W, 4))]
            c.render(p, out=self.out[0])
        elif entry == "render_rgb8":
            self.out = [sentinel((H, W, 3), np.uint8)]
            c._check(c._L.rt_render_rgb8(c._h, C.byref(p), 0, H, self.out[0].ctypes.data_as(C.POINTER(C.c_uint8))))
        elif entry == "render_pose":
            self.out = [sentinel((H, W, 4))]
            pose = rt.make_pose(position=(0.5, 1.0, 54.0), yaw=0.05, pitch=0.25)
            c._check(c._L.rt_render_pose(c._h, C.byref(p), C.byref(pose), self.out[0].ctypes.data_as(C.POINTER(C.c_float))))
        elif entry == "render_async":
            self.out = [sentinel((H, W, 4))]
            c.render_async(p, self.out[0], slot=0)
            c.wait(0)
        elif entry in ("render_rows", "render_stream", "pipelined"):
            rows, _ = rt.interleaved_rows(H, 8, seed % 2, 2) if entry == "render_rows" else (rt._capi.Rows(0, H, H, 1), None)
            n = 2 if entry == "pipelined" else 1
            bufs = [torch.from_numpy(sentinel((rows.n_rows, W, 4))).cuda() for _ in range(n)]
            self.out = []
            if entry == "pipelined":
                c.set_pipelining(True)
            try:
                for k, bf in enumerate(bufs):
                    p.seed = seed + k
                    c.render_device(p, rows, bf.data_ptr(), stream=self.stream if entry == "render_stream" else None)
            finally:
                if entry == "pipelined":
                    c.set_pipelining(False)
                if entry == "render_stream" and self.stream:
                    torch.cuda.synchronize()
                c.synchronize()
                self.out = [bf.cpu().numpy() for bf in bufs]
        else:
            raise ValueError(entry)
        return list(self.out)

    def rgb8(self, rgba):
        """the 8-bit image of a float frame, by the device's own tone map"""
        import torch
        src = torch.from_numpy(np.ascontiguousarray(rgba, f32)).cuda()
        dst = torch.empty(rgba.shape[0] * rgba.shape[1] * 3 + 16, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()                                         # (the copy above is torch's; the tone map runs on the context's own stream)
        self.c.tonemap_device(src.data_ptr(), rgba.shape[0] * rgba.shape[1], dst.data_ptr())
        self.c.synchronize()
        return dst.cpu().numpy()[:rgba.shape[0] * rgba.shape[1] * 3]

    # -- bystanders
    def by(self, name, W, H):
        c, p = self.c, self.params(W, H, 1, 1, 7)
        rays = np.array([[0, 0, 55, 0, -0.1, -1], [0, 0, 55, 0.2, 0.0, -1], [5, 30, 40, 0, -1, 0.01]], f32)
        if name == "render_aov":
            return c.render_aov(p)
        if name == "trace_rays":
            return c.trace_rays(rays)
        if name == "kat_mesh":
            return c.kat_mesh(rays)[0]
        if name == "kat_emission_table":
            return c.kat_emission_table()
        if name == "kat_environment_table":
            return c.kat_environment_table()
        if name == "count_work":
            return c.count_work(p)
        if name == "render_counts":
            counts = (1 + (np.add.outer(np.arange(H), np.arange(W)) % 3 == 0)).astype(np.uint8)
            return c.render_counts(p, counts)
        if name == "stats_frame":
            c.stats_enable(True)
            try:
                return self.frame("render", W, H, 1, 1, 7, 0.0)[0]
            finally:
                c.stats_enable(False)
        if name == "getters":
            return self.getters()
        raise ValueError(name)

    def getters(self, S=None):
        """every getter's answer as plain data -- or the error code it raises; S: the model's state, for the slots to ask"""
        c, out = self.c, {}
        spheres, meshes = (sorted(S.spheres), S.meshes) if S is not None and S.have else (sorted(SCENES[self.name][0]), SCENES[self.name][1]) if self.name else ((0,), (6,))

        def ask(name, fn):
            try:
                out[name] = fn()
            except rt._capi.RtError as e:
                out[name] = ("error", e.code)

        plain = lambda v: v.tobytes() if isinstance(v, np.ndarray) else tuple(plain(x) for x in v) if isinstance(v, (tuple, list)) else v
        for name in GETTERS:
            if name == "emission":
                for s in meshes:
                    ask(f"emission[{s}]", lambda s=s: c.emission(s))
            elif name == "sphere":
                for s in spheres:
                    ask(f"sphere[{s}]", lambda s=s: c.sphere(s))
            elif name == "environment":
                ask(name, lambda: (lambda e: None if e is None else (e.shape, e.tobytes()))(c.environment()))
            else:
                ask(name, lambda name=name: plain(getattr(c, name)()))
        return out


def replay(ctx, ops, g, stream=None):
    """drive `ctx` through `ops` (what print(sequence(...)) shows can be pasted here); refused ops are expected to raise -> the results of the frame and bystander ops"""
    d, out = Driver(ctx, g, stream), []
    for op in ops:
        try:
            r = d.apply(op)
        except rt._capi.RtError as e:
            r = ("error", e.code)
        if op[0] in ("frame", "by"):
            out.append(r)
    return out

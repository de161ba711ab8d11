"""Tinted mirrors and glass at the boundary, without a GPU: the library exports the two entries, the header declares them and the package binds them alike; a NULL
context is refused and a refused call writes nothing; the Python methods marshal; the C++ Renderer members compile; the host library's form entry is exported; the
header pins the rule the model is written from.  What needs a context needs a device: tests/test_gpu_tint.py."""
import ctypes as C
import os
import subprocess

import raytracinggpu_amd as rt
from raytracinggpu_amd import _capi, hostlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rt_material_set_tint", "rt_material_get_tint")


def test_tint_symbols_are_exported_declared_and_bound():
    lib = _capi.load()
    hdr = open(os.path.join(ROOT, "include", "raytrace_hip.h")).read()
    for n in NEW:
        assert hasattr(lib, n), n
        assert n in _capi.EXPORTS, n
        assert f"int {n}(" in hdr, n
        assert getattr(lib, n).argtypes is not None, n
    assert "int rt_material_set_tint(rt_ctx *ctx, int object_slot, int on);" in hdr
    assert "int rt_material_get_tint(const rt_ctx *ctx, int object_slot, int *on);" in hdr
    assert lib.rt_material_set_tint.argtypes[1:] == [C.c_int, C.c_int]
    assert lib.rt_material_get_tint.argtypes[1:] == [C.c_int, C.POINTER(C.c_int)]
    assert "#define RT_ABI_VERSION 6" in hdr and lib.rt_abi_version() == 6          # additive: the ABI number stays
    assert not hasattr(lib, "rt_kat_tint") and "rt_kat_tint" not in hdr              # no new device step: no known-answer entry
    for m in ("set_tint", "tint"):
        assert callable(getattr(rt.Context, m)), m
    assert "rth_advance_form_tint" in hostlib.EXPORTS and hasattr(hostlib.load(), "rth_advance_form_tint")
    assert "rth_advance_form_gloss" in hostlib.EXPORTS and hasattr(hostlib.load(), "rth_advance_form_gloss")   # the older entry stays
    assert len(hostlib.load().rth_advance_form_tint.argtypes) == 14


def test_the_header_states_the_rule():
    """the model is written from the header: the flag, what makes it effective, the colour, the hit's two stores, glass per interface, the dead channels, the close"""
    hdr = open(os.path.join(ROOT, "include", "raytrace_hip.h")).read()
    sec = hdr[hdr.index("--- TINT"):hdr.index("int rt_material_set_tint(")]
    for phrase in ("THE FLAG", "EFFECTIVE", "THE COLOUR", "THE HIT", "GLASS", "DEAD CHANNELS", "THE CLOSE OF A SHADOW RAY", "SID[d] = the object's id", "LS[d] = +0", "0xff",
                   "fl(alb ans)", "PER INTERFACE", "NOT Beer's law", "wf_dead_channels(dead, alb, +0)", "PF_HASX", "rt_deadlast.h", "A texture is not sampled",
                   "RT_ERR_NO_SCENE", "\"tint\" in the error text", "kFormTint"):
        assert phrase in sec, phrase


def test_the_new_entries_keep_clear_of_the_edit_table_prefixes():
    """tests/test_edit_sequences_model.py asks every rt_scene_set* / move* / get* / upload*, rt_camera_*, rt_mesh_* and rt_multi_* entry to be a row of its table"""
    for n in NEW:
        assert n.startswith("rt_material_"), n
        assert not n.startswith(("rt_scene_", "rt_camera_", "rt_mesh_", "rt_multi_")), n


def test_null_context_is_refused():
    lib = _capi.load()
    l = _capi.Light()
    v = C.c_int(-7)
    for call in (lambda: lib.rt_material_set_tint(None, 0, 1), lambda: lib.rt_material_get_tint(None, 0, C.byref(v))):
        lib.rt_light_orbit(C.byref(l), C.c_float(0), C.c_float(0), C.byref(l))       # (a success in between: the message below is this call's own)
        assert call() == -1
        assert b"NULL" in lib.rt_last_error(None)
    assert v.value == -7


class _Recorder:
    """stands in for the loaded library: records every call with its arguments"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            if name == "rt_material_get_tint":
                args[2]._obj.value = 1 if args[1] == 3 else 0
            return 0
        return fn


def test_python_routes_and_marshals_the_tint_calls():
    c = rt.Context.__new__(rt.Context)
    c._L, c._h = _Recorder(), C.c_void_p()
    c.set_tint(3)
    c.set_tint(4, False)
    c.set_tint(5, 17)
    assert c.tint(3) is True and c.tint(4) is False
    names = [n for n, _ in c._L.calls]
    assert names == ["rt_material_set_tint"] * 3 + ["rt_material_get_tint"] * 2
    assert [a[1:] for _, a in c._L.calls[:3]] == [(3, 1), (4, 0), (5, 1)]
    assert c._L.calls[3][1][1] == 3 and c._L.calls[4][1][1] == 4
    c._h = None


def test_renderer_tint_members_compile(tmp_path):
    src = tmp_path / "tint.cpp"
    src.write_text("""
#include "raytracer.hpp"
using namespace raytracer;
bool use(Renderer &r) {
    r.set_tint(3);
    r.set_tint(4, false);
    return r.tint(3);
}
""")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)

"""Rough mirrors at the boundary, without a GPU: the library exports the three entries, the header declares them and the package binds them alike; a NULL context
is refused and a refused call writes nothing; the Python methods marshal; the C++ Renderer members compile; the host library's form entry is exported.  What needs a
context needs a device: tests/test_gpu_gloss.py."""
import ctypes as C
import os
import subprocess

import numpy as np

import raytracinggpu_amd as rt
from raytracinggpu_amd import _capi, hostlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rt_material_set_roughness", "rt_material_get_roughness", "rt_kat_gloss")
UP = C.POINTER(C.c_uint32)


def test_gloss_symbols_are_exported_declared_and_bound():
    lib = _capi.load()
    hdr = open(os.path.join(ROOT, "include", "raytrace_hip.h")).read()
    for n in NEW:
        assert hasattr(lib, n), n
        assert n in _capi.EXPORTS, n
        assert f"int {n}(" in hdr, n
        assert getattr(lib, n).argtypes is not None, n
    assert "int rt_material_set_roughness(rt_ctx *ctx, int object_slot, float alpha);" in hdr
    assert "int rt_material_get_roughness(const rt_ctx *ctx, int object_slot, float *alpha);" in hdr
    assert "int rt_kat_gloss(rt_ctx *ctx, int count, const uint32_t *items, uint32_t *out);" in hdr
    assert lib.rt_material_set_roughness.argtypes[1:] == [C.c_int, C.c_float]
    assert lib.rt_material_get_roughness.argtypes[1:] == [C.c_int, C.POINTER(C.c_float)]
    assert lib.rt_kat_gloss.argtypes[1:] == [C.c_int, UP, UP]
    assert "#define RT_ABI_VERSION 6" in hdr and lib.rt_abi_version() == 6          # additive: the ABI number stays
    assert "ROUGH MIRRORS" in hdr and "roughness" in hdr
    for m in ("set_roughness", "roughness", "kat_gloss"):
        assert callable(getattr(rt.Context, m)), m
    assert "rth_advance_form_gloss" in hostlib.EXPORTS and hasattr(hostlib.load(), "rth_advance_form_gloss")
    assert "rth_advance_form_fresnel" in hostlib.EXPORTS and hasattr(hostlib.load(), "rth_advance_form_fresnel")   # the older entry stays


def test_the_header_states_the_rule():
    """the model is written from the header: the keys, the range argument and the lobe are there"""
    hdr = open(os.path.join(ROOT, "include", "raytrace_hip.h")).read()
    sec = hdr[hdr.index("ROUGH MIRRORS"):hdr.index("int rt_material_set_roughness(")]
    for phrase in ("2^25 + d", "2^27 + 4 d + dim", "[2^-12, 1]", "THE RANGE", "shadowing-masking", "not reciprocal", "FOLDED BACK", "16 32-bit words", "12 words"):
        assert phrase in sec, phrase


def test_the_new_entries_keep_clear_of_the_edit_table_prefixes():
    """tests/test_edit_sequences_model.py asks every rt_scene_set* / move* / get* / upload*, rt_camera_*, rt_mesh_* and rt_multi_* entry to be a row of its table"""
    for n in NEW:
        assert not n.startswith(("rt_scene_", "rt_camera_", "rt_mesh_", "rt_multi_")), n


def test_null_context_is_refused():
    lib = _capi.load()
    l = _capi.Light()
    a = C.c_float(-7)
    items, out = (C.c_uint32 * 16)(*([7] * 16)), (C.c_uint32 * 12)(*([7] * 12))
    for call in (lambda: lib.rt_material_set_roughness(None, 0, 0.5), lambda: lib.rt_material_get_roughness(None, 0, C.byref(a)), lambda: lib.rt_kat_gloss(None, 1, items, out)):
        lib.rt_light_orbit(C.byref(l), C.c_float(0), C.c_float(0), C.byref(l))       # (a success in between: the message below is this call's own)
        assert call() == -1
        assert b"NULL" in lib.rt_last_error(None)
    assert a.value == -7 and list(out) == [7] * 12 and list(items) == [7] * 16


class _Recorder:
    """stands in for the loaded library: records every call with its arguments"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            if name == "rt_material_get_roughness":
                args[2]._obj.value = 0.25
            if name == "rt_kat_gloss":
                self.items = np.ctypeslib.as_array(args[2], shape=(args[1] * 16,)).copy().reshape(-1, 16)
                o = np.ctypeslib.as_array(args[3], shape=(args[1] * 12,)).reshape(-1, 12)
                o[:, 0:3] = self.items[:, 5:8]                                       # h := N
                o[:, 3] = self.items[:, 12] % 2
                o[:, 4:7] = self.items[:, 2:5]                                       # O := P
                o[:, 7:10] = self.items[:, 8:11]                                     # u := u
            return 0
        return fn


def test_python_routes_and_marshals_the_gloss_calls():
    c = rt.Context.__new__(rt.Context)
    c._L, c._h = _Recorder(), C.c_void_p()
    c.set_roughness(3, 0.5)
    c.set_roughness(4, 0)
    assert c.roughness(3) == 0.25
    P = np.arange(6, dtype=np.float32).reshape(2, 3)
    N = np.array([[0, 0, 1], [0, 1, 0]], np.float32)
    h, code, O, u = c.kat_gloss(0.25, 1e-3, P, N, -N, np.array([5, 6], np.int64), [4, 5])
    names = [n for n, _ in c._L.calls]
    assert names == ["rt_material_set_roughness", "rt_material_set_roughness", "rt_material_get_roughness", "rt_kat_gloss"]
    assert c._L.calls[0][1][1:] == (3, 0.5) and c._L.calls[1][1][1:] == (4, 0.0) and c._L.calls[2][1][1] == 3
    assert c._L.calls[3][1][1] == 2
    it = c._L.items
    f = it.view(np.float32)
    assert f[:, 0].tolist() == [0.25, 0.25] and (f[:, 1] == np.float32(1e-3)).all()
    assert (f[:, 2:5] == P).all() and (f[:, 5:8] == N).all() and (f[:, 8:11] == -N).all()
    assert it[:, 11].tolist() == [5, 6] and it[:, 12].tolist() == [4, 5] and (it[:, 13:] == 0).all()
    assert h.dtype == np.float32 and (h == N).all() and code.dtype == np.int32 and code.tolist() == [0, 1]
    assert (O == P).all() and (u == -N).all()
    _, code, *_ = c.kat_gloss(0.25, 1e-3, P, N, -N, [1, 2], 7)                        # one segment for all
    assert code.tolist() == [1, 1]
    c._h = None


def test_renderer_gloss_members_compile(tmp_path):
    src = tmp_path / "gloss.cpp"
    src.write_text("""
#include "raytracer.hpp"
using namespace raytracer;
float use(Renderer &r) {
    r.set_roughness(3, 0.25f);
    r.set_roughness(4, 0.f);
    return r.roughness(3);
}
""")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)

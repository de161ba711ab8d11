"""Fresnel dielectrics at the boundary, without a GPU: the library exports the three entries, the header declares them and the package binds them alike; a NULL context
is refused and a refused call writes nothing; the Python methods marshal; the C++ Renderer members compile; the host library's form entry is exported.  What needs a
context needs a device: tests/test_gpu_fresnel.py."""
import ctypes as C
import os
import subprocess

import numpy as np

import raytracinggpu_amd as rt
from raytracinggpu_amd import _capi, hostlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rt_material_set_fresnel", "rt_material_get_fresnel", "rt_kat_fresnel")
UP = C.POINTER(C.c_uint32)


def test_fresnel_symbols_are_exported_declared_and_bound():
    lib = _capi.load()
    hdr = open(os.path.join(ROOT, "include", "raytrace_hip.h")).read()
    for n in NEW:
        assert hasattr(lib, n), n
        assert n in _capi.EXPORTS, n
        assert f"int {n}(" in hdr, n
        assert getattr(lib, n).argtypes is not None, n
    assert "int rt_material_set_fresnel(rt_ctx *ctx, int object_slot, int on);" in hdr
    assert "int rt_material_get_fresnel(const rt_ctx *ctx, int object_slot, int *on);" in hdr
    assert "int rt_kat_fresnel(rt_ctx *ctx, int count, const uint32_t *items, uint32_t *out);" in hdr
    assert lib.rt_material_set_fresnel.argtypes[1:] == [C.c_int, C.c_int]
    assert lib.rt_material_get_fresnel.argtypes[1:] == [C.c_int, C.POINTER(C.c_int)]
    assert lib.rt_kat_fresnel.argtypes[1:] == [C.c_int, UP, UP]
    assert "#define RT_ABI_VERSION 6" in hdr and lib.rt_abi_version() == 6          # additive: the ABI number stays
    assert "FRESNEL DIELECTRICS" in hdr
    for m in ("set_fresnel", "fresnel", "kat_fresnel"):
        assert callable(getattr(rt.Context, m)), m
    assert "rth_advance_form_fresnel" in hostlib.EXPORTS and hasattr(hostlib.load(), "rth_advance_form_fresnel")


def test_the_new_entries_keep_clear_of_the_edit_table_prefixes():
    """tests/test_edit_sequences_model.py asks every rt_scene_set* / move* / get* / upload*, rt_camera_*, rt_mesh_* and rt_multi_* entry to be a row of its table"""
    for n in NEW:
        assert not n.startswith(("rt_scene_", "rt_camera_", "rt_mesh_", "rt_multi_")), n


def test_null_context_is_refused():
    lib = _capi.load()
    l = _capi.Light()
    on = C.c_int(-7)
    items, out = (C.c_uint32 * 16)(*([7] * 16)), (C.c_uint32 * 9)(*([7] * 9))
    for call in (lambda: lib.rt_material_set_fresnel(None, 0, 1), lambda: lib.rt_material_get_fresnel(None, 0, C.byref(on)), lambda: lib.rt_kat_fresnel(None, 1, items, out)):
        lib.rt_light_orbit(C.byref(l), C.c_float(0), C.c_float(0), C.byref(l))       # (a success in between: the message below is this call's own)
        assert call() == -1
        assert b"NULL" in lib.rt_last_error(None)
    assert on.value == -7 and list(out) == [7] * 9 and list(items) == [7] * 16


class _Recorder:
    """stands in for the loaded library: records every call with its arguments"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            if name == "rt_material_get_fresnel":
                args[2]._obj.value = 1
            if name == "rt_kat_fresnel":
                self.items = np.ctypeslib.as_array(args[2], shape=(args[1] * 16,)).copy().reshape(-1, 16)
                o = np.ctypeslib.as_array(args[3], shape=(args[1] * 9,)).reshape(-1, 9)
                o[:, 0] = np.float32(0.25).view(np.uint32)
                o[:, 1] = self.items[:, 14] % 3
                o[:, 2:8] = self.items[:, 4:10]
                o[:, 8] = self.items[:, 0]
            return 0
        return fn


def test_python_routes_and_marshals_the_fresnel_calls():
    c = rt.Context.__new__(rt.Context)
    c._L, c._h = _Recorder(), C.c_void_p()
    c.set_fresnel(3)
    c.set_fresnel(4, False)
    assert c.fresnel(3) is True
    P = np.arange(6, dtype=np.float32).reshape(2, 3)
    N = np.array([[0, 0, 1], [0, 1, 0]], np.float32)
    R, code, O, u, after = c.kat_fresnel(1.5, 1.0, 1.0, 1e-3, P, N, -N, np.array([5, 6], np.int64), [4, 5])
    names = [n for n, _ in c._L.calls]
    assert names == ["rt_material_set_fresnel", "rt_material_set_fresnel", "rt_material_get_fresnel", "rt_kat_fresnel"]
    assert c._L.calls[0][1][1:] == (3, 1) and c._L.calls[1][1][1:] == (4, 0) and c._L.calls[2][1][1] == 3
    assert c._L.calls[3][1][1] == 2
    it = c._L.items
    f = it.view(np.float32)
    assert f[:, 0].tolist() == [1.5, 1.5] and f[:, 1].tolist() == [1.0, 1.0] and f[:, 2].tolist() == [1.0, 1.0] and (f[:, 3] == np.float32(1e-3)).all()
    assert (f[:, 4:7] == P).all() and (f[:, 7:10] == N).all() and (f[:, 10:13] == -N).all()
    assert it[:, 13].tolist() == [5, 6] and it[:, 14].tolist() == [4, 5] and it[:, 15].tolist() == [0, 0]
    assert R.dtype == np.float32 and R.tolist() == [0.25, 0.25] and code.dtype == np.int32 and code.tolist() == [1, 2]
    assert (O == P).all() and (u == N).all() and after.tolist() == [1.5, 1.5]
    _, code, *_ = c.kat_fresnel(1.5, 1.0, 1.0, 1e-3, P, N, -N, [1, 2], 7)            # one segment for all
    assert code.tolist() == [1, 1]
    c._h = None


def test_renderer_fresnel_members_compile(tmp_path):
    src = tmp_path / "fresnel.cpp"
    src.write_text("""
#include "raytracer.hpp"
using namespace raytracer;
bool use(Renderer &r) {
    r.set_fresnel(3, true);
    r.set_fresnel(4, false);
    return r.fresnel(3);
}
""")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)

"""The still view's three count entries at the boundary, without a GPU: the library exports rt_first_{hit,shadow,shade}_cache_counts, the header declares each and names
its knob, the ABI number stays, every entry refuses a NULL context and a NULL output pointer before it looks at either, and the Python methods name the four counters."""
import ctypes as C
import os

import pytest

import raytracinggpu_amd as rt
from raytracinggpu_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = [("first_hit_cache_counts", "RT_FIRST_HIT_CACHE", "skipped"), ("first_shadow_cache_counts", "RT_FIRST_SHADOW_CACHE", "skipped"),
          ("first_shade_cache_counts", "RT_FIRST_SHADE_CACHE", "resumed")]
pytestmark = pytest.mark.parametrize("method, knob, used", LEVELS, ids=[m for m, _, _ in LEVELS])


def test_the_entry_is_exported_and_declared(method, knob, used):
    lib = _capi.load()
    hdr = open(os.path.join(ROOT, "include", "raytrace_hip.h")).read()
    assert hasattr(lib, "rt_" + method)
    assert "rt_" + method in _capi.EXPORTS
    assert f"int rt_{method}(" in hdr
    assert knob in hdr
    assert "#define RT_ABI_VERSION 6" in hdr and lib.rt_abi_version() == 6          # additive: the ABI number stays


def test_null_arguments_are_refused(method, knob, used):
    lib = _capi.load()
    out = (C.c_uint64 * 4)(7, 7, 7, 7)
    l = _capi.Light()
    not_a_context = C.create_string_buffer(64)                                      # never read: the entry checks both pointers first
    for ctx, o in ((None, out), (None, None), (C.cast(not_a_context, C.c_void_p), None)):
        lib.rt_light_orbit(C.byref(l), C.c_float(0), C.c_float(0), C.byref(l))       # (a success in between: the message below is this call's own)
        assert getattr(lib, "rt_" + method)(ctx, o) == -1
        assert b"bad arguments" in lib.rt_last_error(None)
    assert list(out) == [7, 7, 7, 7]


def test_python_names_the_counters(method, knob, used):
    def entry(h, out):
        out[0], out[1], out[2], out[3] = 5, 2, 3, 1
        return 0

    c = rt.Context.__new__(rt.Context)
    c._L, c._h = type("_Lib", (), {"rt_" + method: staticmethod(entry)})(), C.c_void_p()
    assert getattr(c, method)() == {used: 5, "filled": 2, "ineligible": 3, "key_misses": 1}
    doc = getattr(rt.Context, method).__doc__
    assert doc and "rt_" + method in doc

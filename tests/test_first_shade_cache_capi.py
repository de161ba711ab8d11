"""The first-shade cache at the boundary, without a GPU: the library exports rt_first_shade_cache_counts, the header declares it, the ABI number stays, the entry refuses
a NULL context and a NULL output pointer before it looks at either, and the Python method names the four counters."""
import ctypes as C
import os

import raytracinggpu_amd as rt
from raytracinggpu_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_is_exported_and_declared():
    lib = _capi.load()
    hdr = open(os.path.join(ROOT, "include", "raytrace_hip.h")).read()
    assert hasattr(lib, "rt_first_shade_cache_counts")
    assert "rt_first_shade_cache_counts" in _capi.EXPORTS
    assert "int rt_first_shade_cache_counts(" in hdr
    assert "RT_FIRST_SHADE_CACHE" in hdr
    assert "#define RT_ABI_VERSION 6" in hdr and lib.rt_abi_version() == 6          # additive: the ABI number stays


def test_null_arguments_are_refused():
    lib = _capi.load()
    out = (C.c_uint64 * 4)(7, 7, 7, 7)
    l = _capi.Light()
    not_a_context = C.create_string_buffer(64)                                      # never read: the entry checks both pointers first
    for ctx, o in ((None, out), (None, None), (C.cast(not_a_context, C.c_void_p), None)):
        lib.rt_light_orbit(C.byref(l), C.c_float(0), C.c_float(0), C.byref(l))       # (a success in between: the message below is this call's own)
        assert lib.rt_first_shade_cache_counts(ctx, o) == -1
        assert b"bad arguments" in lib.rt_last_error(None)
    assert list(out) == [7, 7, 7, 7]


def test_python_names_the_counters():
    class _Lib:
        def rt_first_shade_cache_counts(self, h, out):
            out[0], out[1], out[2], out[3] = 5, 2, 3, 1
            return 0

    c = rt.Context.__new__(rt.Context)
    c._L, c._h = _Lib(), C.c_void_p()
    assert c.first_shade_cache_counts() == dict(resumed=5, filled=2, ineligible=3, key_misses=1)
    assert c.first_shade_cache_counts.__doc__ and "rt_first_shade_cache_counts" in c.first_shade_cache_counts.__doc__

"""Who owns what of a context (rt_host_ctx.hip.h): rt_ctx and rt_multi give their buffers, events and streams back by member destruction, ~rt_ctx only waits for the
context's streams first; the temporaries of the known-answer entries free themselves on every exit.  Seen from outside: closing a context with copies in flight
completes them, a refused creation leaves nothing that disturbs the next context, and a refused call between two equal calls changes nothing.  Every comparison is
bit for bit with what a plain context gave first.  (That nothing leaks is the destructors' to show, by reading: the device-wide free-memory counter moves with other
processes' work.)"""
import ctypes as C

import numpy as np
import pytest

import raytracinggpu_amd as rt

pytestmark = pytest.mark.gpu

W, H = 96, 64                                                     # eight 8-row tiles: both sub-frame chains and their streams exist
RT_ERR_INVALID, RT_ERR_UNSUPPORTED = -1, -5


def _context(cat_golden):
    c = rt.Context(0)
    c.scene_upload(rt.scenes.spheres("cpu"), dict(vertices=cat_golden["vertices"], indices=cat_golden["tri_bvh_order"], bvh_arr10=cat_golden["bvh_arr10"],
                                                  albedo=rt.scenes.CAT_ALBEDO, object_slot=6))
    return c


@pytest.fixture(scope="module")
def params():
    return rt.make_params(W, H, 1, 2, **rt.scenes.CPU_LAUNCHER), rt.make_params(W, H, 1, 2, seed=7, **dict(rt.scenes.CPU_LAUNCHER, sigma=0.2))


@pytest.fixture(scope="module")
def reference(cat_golden, params):
    """(float frame of params[0], float frame of params[1], 8-bit image of params[1]) of a plain context; read-only"""
    c = _context(cat_golden)
    ref = c.render(params[0]), c.render(params[1]), c.render_rgb8(params[1])
    c.close()
    for a in ref:
        a.setflags(write=False)
    assert not np.array_equal(ref[0], ref[1])
    return ref


def _same_bits(got, want, what):
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=what)


def _renders_reference(cat_golden, params, reference, what):
    c = _context(cat_golden)
    _same_bits(c.render(params[0]), reference[0], what)
    c.selfcheck()
    c.close()


def test_close_with_copies_in_flight(cat_golden, params, reference):
    """A pipelining context renders four frames on a caller's stream (its sub-frame chains run on the context's part streams), issues one float and one 8-bit
    asynchronous frame and is closed without a wait: rt_ctx_destroy waits for the copy streams, so the pinned outputs hold the frames when close() returns."""
    import torch
    st = torch.cuda.Stream()
    rows, _ = rt.interleaved_rows(H, 8, 0, 1)
    for cycle in range(5):
        c = _context(cat_golden)
        c.set_pipelining(True)
        dev = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0") for _ in range(2)]
        torch.cuda.synchronize()
        for k in range(4):
            c.render_device(params[k & 1], rows, dev[k & 1].data_ptr(), st.cuda_stream)
        st.synchronize()
        pin_f, pin_8 = rt.PinnedArray((H, W, 4)), rt.PinnedArray((H, W, 3), np.uint8)
        out_f, out_8 = pin_f.array, pin_8.array
        out_f[:] = 0
        out_8[:] = 0
        c.render_async(params[0], out_f, slot=0)
        c.render_async(params[1], out_8, slot=1, rgb8=True)
        c.selfcheck()
        c.close()
        _same_bits(out_f, reference[0], f"cycle {cycle}: float frame of slot 0")
        np.testing.assert_array_equal(out_8, reference[2], err_msg=f"cycle {cycle}: 8-bit frame of slot 1")
        for k in range(2):
            _same_bits(dev[k].cpu().numpy(), reference[k], f"cycle {cycle}: device frame {k}")
        _renders_reference(cat_golden, params, reference, f"cycle {cycle}: a context created after the close")


def test_failed_creation_leaves_nothing_behind(cat_golden, params, reference):
    L = rt._capi.load()
    h = C.c_void_p(1)
    assert L.rt_ctx_create(C.byref(h), rt.device_count()) == RT_ERR_INVALID
    assert not h.value
    _renders_reference(cat_golden, params, reference, "after a refused rt_ctx_create")
    with pytest.raises(rt.RtError):                                # its first context exists when the second one is refused
        rt.MultiContext([0, 99])
    _renders_reference(cat_golden, params, reference, "after a refused rt_multi_create")


def test_temporaries_around_refused_calls(cat_golden):
    """rt_trace_rays, rt_kat_surface and rt_kat_box hold their device arrays in temporaries: three equal calls each, at one ray and at 257 (two workgroups),
    a refused call of the entry in between, and the answers stay the same."""
    rng = np.random.default_rng(5)
    c = _context(cat_golden)
    for n in (1, 257):
        u = np.concatenate([rng.uniform(-0.35, 0.35, (n, 2)), -np.ones((n, 1))], axis=1)
        rays = np.concatenate([np.tile([0.0, 0.0, 55.0], (n, 1)), u / np.linalg.norm(u, axis=1, keepdims=True)], axis=1).astype(np.float32)
        lo = rng.uniform(-10, 0, (n, 3))
        boxes = np.concatenate([lo, lo + rng.uniform(0, 10, (n, 3)), rng.uniform(-20, 20, (n, 3)), rng.normal(size=(n, 3))], axis=1).astype(np.float32)
        first = c.trace_rays(rays), c.kat_surface(rays), c.kat_box(boxes, 2)
        if n == 257:
            assert first[0][:, 0].any() and not first[0][:, 0].all() and first[2][0].any() and not first[2][0].all(), "hits and misses"
        for k in range(2):
            with pytest.raises(rt.RtError) as e:
                c.trace_rays(rays, variant="lockstep")
            assert e.value.code == RT_ERR_UNSUPPORTED
            with pytest.raises(rt.RtError) as e:
                c.kat_box(boxes, 9)
            assert e.value.code == RT_ERR_INVALID
            again = c.trace_rays(rays), c.kat_surface(rays), c.kat_box(boxes, 2)
            _same_bits(again[0], first[0], f"rt_trace_rays, n = {n}, call {k + 2}")
            _same_bits(again[1], first[1], f"rt_kat_surface, n = {n}, call {k + 2}")
            _same_bits(again[2][0], first[2][0], f"rt_kat_box, n = {n}, call {k + 2}")
            assert again[2][1] == first[2][1]
    c.selfcheck()
    c.close()

"""The two float -> byte kernels on synthetic values, against the exact model (tests/gamma_model.py: the byte of the correctly rounded power).  -m gpu.

  tonemap_kernel      through rt_tonemap_device on torch buffers: T_k - 4 ... T_k + 3 in floats around every threshold of the binary64 path, 2048 and 177147 (the two
                      inputs whose exact 2.2-th root is a code: the byte is the code below) with two neighbours on either side, the special values, 4096 log-uniform
                      values; every frame size at which the kernel takes another path (whole quads, a tail of 1, 2, 3 pixels, one and several workgroups) at each of
                      the four alignments of the image, between guard bytes; and the entries that deliver bytes to the host (rt_render_rgb8, rt_render_async)
  accumulate_kernel   through rt_kat_progressive: every row of the reference's own recording (tests/golden/ref_realtime.npz, prog_*), and the binary32 path's own
                      edges -- its exponent is 1 / 2.2f, so they are not the binary64 path's, nor the fixture's fl(k^2.2)

Every case is a few thousand values.  The expected bytes of the synthetic sets are computed once per module."""
import ctypes as C

import numpy as np
import pytest

import raytracinggpu_amd as rt

from . import gamma_model as gm
from .conftest import load_golden

pytestmark = pytest.mark.gpu

GUARD = 16
SIZES = [1, 2, 3, 4, 5, 7, 255, 256, 257, 1023, 1025]


@pytest.fixture(scope="module")
def ctx():
    c_ = rt.Context(0)
    yield c_
    c_.close()


@pytest.fixture(scope="module")
def ref():
    return load_golden("ref_realtime.npz")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def pixels_of(values, seed):
    """values shuffled (the special values share waves with ordinary ones) and spread over .x, .y, .z of float4 pixels; .w holds junk that must not be read"""
    rng = np.random.default_rng(seed)
    v = np.concatenate([values, np.full((-len(values)) % 3, 0.25, np.float32)]).astype(np.float32)
    v = v[rng.permutation(len(v))]
    px = np.empty((len(v) // 3, 4), np.float32)
    px[:, :3] = v.reshape(-1, 3)
    px[:, 3] = rng.choice(np.array([np.nan, np.inf, -np.inf, -1.0, 3e38, 1e-45, 7.0], np.float32), len(px))
    return px


@pytest.fixture(scope="module")
def set_d():
    """(pixels [n, 4], expected bytes [n, 3]) of the binary64 path"""
    values = np.concatenate([gm.edge_values(gm.thresholds_d()).ravel(), gm.exact_root_values(), gm.SPECIALS, gm.log_uniform()])
    px = pixels_of(values, 714)
    exp = gm.bytes_of(gm.byte_d, px[:, :3])
    exp.setflags(write=False)
    return px, exp


@pytest.fixture(scope="module")
def set_f():
    """(pixels [n, 4], expected bytes [n, 3]) of the binary32 path"""
    values = np.concatenate([gm.edge_values(gm.thresholds_f()).ravel(), gm.SPECIALS, gm.log_uniform()])
    px = pixels_of(values, 1136)
    exp = gm.bytes_of(gm.byte_f, px[:, :3])
    exp.setflags(write=False)
    return px, exp


def report(px, got, exp, what):
    bad = np.argwhere(got != exp)
    rows = [(repr(px[i, k]), hex(int(bits(px)[i, k])), int(got[i, k]), int(exp[i, k])) for i, k in bad[:8]]
    assert len(bad) == 0, f"{what}: {len(bad)} of {exp.size} bytes differ (value, bits, device, model): {rows}"


def tonemap(ctx, px, npix, offset=0):
    """rt_tonemap_device of the first npix pixels into an image `offset` bytes past a 4-byte boundary -> (bytes [npix, 3], the guard before, the guard after)"""
    import torch
    src = torch.from_numpy(np.ascontiguousarray(px[:max(npix, 1)])).to("cuda:0")
    dst = torch.full((GUARD + 4 + 3 * npix + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
    assert dst.data_ptr() % 4 == 0
    torch.cuda.synchronize()                                           # the copies above are torch's; the tone map runs on the context's own stream
    ctx.tonemap_device(src.data_ptr(), npix, dst.data_ptr() + GUARD + offset)
    ctx.synchronize()
    out = dst.cpu().numpy()
    at = GUARD + offset
    return out[at:at + 3 * npix].reshape(npix, 3), out[:at], out[at + 3 * npix:]


def test_the_inputs_reach_every_code_boundary(set_d, set_f):
    """what the tests say about their own inputs: all 256 codes occur, and for every k both k - 1 and k occur among T_k's eight neighbours"""
    assert gm.edges_are_covered(set_d[0][:, :3], set_d[1], gm.thresholds_d())
    assert gm.edges_are_covered(set_f[0][:, :3], set_f[1], gm.thresholds_f())
    d = dict(zip(bits(set_d[0][:, :3]).ravel().tolist(), set_d[1].ravel().tolist()))
    assert d[gm.bits_of_f32(2048.0)] == 31 and d[gm.bits_of_f32(2048.0) + 1] == 32 and d[gm.bits_of_f32(177147.0)] == 242 and d[gm.bits_of_f32(177147.0) + 1] == 243


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_tonemap_equals_the_exactly_rounded_power(ctx, set_d, offset):
    px, exp = set_d
    got, before, after = tonemap(ctx, px, len(px), offset)
    report(px, got, exp, f"rt_tonemap_device, image {offset} bytes past a 4-byte boundary")
    assert (before == 0xA5).all() and (after == 0xA5).all()


@pytest.mark.parametrize("npix", SIZES)
def test_tonemap_sizes_and_alignments(ctx, set_d, npix):
    """whole quads, tails of 1, 2 and 3 pixels, one workgroup (up to 1024 pixels) and two: exactly 3 * npix bytes are written, wherever the image starts"""
    px, exp = set_d
    for offset in range(4):
        got, before, after = tonemap(ctx, px, npix, offset)
        report(px[:npix], got, exp[:npix], f"npix {npix}, offset {offset}")
        assert (before == 0xA5).all() and (after == 0xA5).all(), f"npix {npix}, offset {offset}: bytes outside the image were written"


def test_tonemap_of_no_pixels_writes_nothing(ctx, set_d):
    for offset in range(4):
        got, before, after = tonemap(ctx, set_d[0], 0, offset)
        assert got.size == 0 and (before == 0xA5).all() and (after == 0xA5).all()


def dim_scene(ctx):
    """the spheres scene with walls of mixed colours under a dim light, as test_gpu_realtime_pinned.py::test_progressive_output builds it: the bytes spread over the range"""
    albedos = [(0.8, 0.5, 0.3), (0.3, 0.6, 0.9), (0.9, 0.2, 0.4), (0.5, 0.9, 0.6), (0.7, 0.7, 0.2), (0.6, 0.35, 0.85)]
    spheres = [(c, r, a) for (c, r, _), a in zip(rt.scenes.spheres("cpu"), albedos)] + [((0.0, 4.0, 56.0), 3.0, (0.9, 0.8, 0.7))]
    ctx.scene_upload(spheres, light=((-10.0, 20.0, 40.0), 2e9))


def test_the_byte_delivering_entries(ctx):
    """rt_render_rgb8 and rt_render_async(rgb8) on both slots: the bytes are the model's of the float frame the same parameters render.  61 x 37: 2257 pixels, a tail of one"""
    dim_scene(ctx)
    W, H = 61, 37
    p = rt.make_params(W, H, 2, 2, **dict(rt.scenes.CPU_LAUNCHER, sigma=0.2))
    frame = ctx.render(p)
    exp = gm.bytes_of(gm.byte_d, frame[..., :3])
    print(f"{len(np.unique(exp))} byte values, {exp.min()} to {exp.max()}")
    assert len(np.unique(exp)) > 32 and exp.max() < 255
    flat = frame.reshape(-1, 4)
    report(flat, ctx.render_rgb8(p).reshape(-1, 3), exp.reshape(-1, 3), "rt_render_rgb8")
    pin8, pinf = rt.PinnedArray((H, W, 3), dtype=np.uint8), rt.PinnedArray((H, W, 4))
    try:
        for slot in (0, 1):
            pin8.array[:] = 0xA5
            ctx.render_async(p, pin8.array, slot=slot, rgb8=True)
            ctx.wait(slot)
            report(flat, pin8.array.reshape(-1, 3), exp.reshape(-1, 3), f"rt_render_async(rgb8), slot {slot}")
        ctx.render_async(p, pinf.array, slot=0)                       # and the float frame of the asynchronous entry is the frame the bytes were held to
        ctx.wait(0)
        assert np.array_equal(bits(pinf.array), bits(frame))
    finally:
        pin8.close(); pinf.close()


def kat_progressive(ctx, accum, frame, framenumber):
    """rt_kat_progressive with each output between two guards -> (accum_out [n, 4], display [n, 4], rgb8 [n, 3])"""
    n = len(accum)
    a, f = np.ascontiguousarray(accum, np.float32), np.ascontiguousarray(frame, np.float32)
    outs = [np.full(GUARD + 4 * n + GUARD, np.float32(-77.0), np.float32), np.full(GUARD + 4 * n + GUARD, np.float32(-77.0), np.float32),
            np.full(GUARD + 3 * n + GUARD, 0xA5, np.uint8)]
    fp, bp = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    ctx._check(ctx._L.rt_kat_progressive(ctx._h, a.ctypes.data_as(fp), f.ctypes.data_as(fp), n, int(framenumber), outs[0][GUARD:].ctypes.data_as(fp),
                                         outs[1][GUARD:].ctypes.data_as(fp), outs[2][GUARD:].ctypes.data_as(bp)))
    for o, fill in zip(outs, (np.float32(-77.0), np.float32(-77.0), 0xA5)):
        assert (o[:GUARD] == fill).all() and (o[len(o) - GUARD:] == fill).all(), "an output was written outside its n elements"
    return outs[0][GUARD:GUARD + 4 * n].reshape(n, 4), outs[1][GUARD:GUARD + 4 * n].reshape(n, 4), outs[2][GUARD:GUARD + 3 * n].reshape(n, 3)


def test_progressive_kernel_equals_the_recorded_reference(ctx, ref):
    """every prog_<n>_* row: the reference's kernel added its probe's miss (0) to accumbuffer = fl(c * n), divided by n = 1, 2, 3, 7, 1000 and wrote the bytes"""
    rng = np.random.default_rng(1147)
    before = ctx.progressive_frames()
    for n in ref["prog_frames"]:
        acc_in, exp_acc, exp_disp, exp_bytes = (ref[f"prog_{n}_{k}"] for k in ("accum_in", "accum_out", "display", "bytes"))
        accum, frame = np.zeros((len(acc_in), 4), np.float32), np.zeros((len(acc_in), 4), np.float32)
        accum[:, :3] = acc_in
        accum[:, 3], frame[:, 3] = rng.integers(0, 1000, len(acc_in)), rng.integers(1, 12, len(acc_in))      # .w: rays so far + this frame's rays
        got_acc, got_disp, got8 = kat_progressive(ctx, accum, frame, int(n))
        bad = np.argwhere(bits(got_acc[:, :3]) != bits(exp_acc))
        assert len(bad) == 0, f"frame {n}: accumbuffer differs at {bad[:4].tolist()}"
        bad = np.argwhere(bits(got_disp[:, :3]) != bits(exp_disp))
        assert len(bad) == 0, f"frame {n}: display differs at {bad[:4].tolist()}: {got_disp[bad[0][0], bad[0][1]]!r}, reference {exp_disp[bad[0][0], bad[0][1]]!r}"
        assert np.array_equal(got_acc[:, 3], accum[:, 3] + frame[:, 3]) and np.array_equal(got_disp[:, 3], got_acc[:, 3])
        px = np.concatenate([exp_disp, np.zeros((len(exp_disp), 1), np.float32)], 1)
        report(px, got8, exp_bytes[:, :3], f"frame {n}")
    assert ctx.progressive_frames() == before                         # the context's own progressive state is not the entry's


def test_progressive_kernel_equals_the_exactly_rounded_power(ctx, set_f):
    """framenumber 1 on accumbuffer 0: the display value is the input itself (0 + -0 is +0: byte 0 either way), the bytes are the model's"""
    px, exp = set_f
    acc, disp, got8 = kat_progressive(ctx, np.zeros_like(px), px, 1)
    keep = bits(px[:, :3]) != 0x80000000
    assert np.array_equal(bits(disp[:, :3])[keep], bits(px[:, :3])[keep]) and np.array_equal(bits(acc[:, :3]), bits(disp[:, :3]))
    report(px, got8, exp, "rt_kat_progressive")


@pytest.mark.parametrize("n", [1, 255, 257])
def test_progressive_kernel_sizes(ctx, set_f, n):
    """one lane, one workgroup short of a lane, one lane into the second workgroup: n * 3 bytes and n float4 twice, and nothing beyond them"""
    px, exp = set_f
    acc, disp, got8 = kat_progressive(ctx, np.zeros((n, 4), np.float32), px[:n], 1)
    report(px[:n], got8, exp[:n], f"n {n}")
    assert np.array_equal(bits(acc[:, :3]), bits(disp[:, :3]))


def test_kat_progressive_refusals(ctx):
    assert ctx._L.rt_kat_progressive(ctx._h, None, None, 0, 1, None, None, None) == 0
    z = np.zeros((1, 4), np.float32)
    fp = C.POINTER(C.c_float)
    assert ctx._L.rt_kat_progressive(ctx._h, None, z.ctypes.data_as(fp), 1, 1, None, None, None) == -1
    assert ctx._L.rt_kat_progressive(ctx._h, z.ctypes.data_as(fp), z.ctypes.data_as(fp), 1, 0, None, None, None) == -1
    assert ctx._L.rt_kat_progressive(ctx._h, z.ctypes.data_as(fp), z.ctypes.data_as(fp), -1, 1, None, None, None) == -1
    acc, disp, rgb8 = ctx.kat_progressive(z, np.array([[1.0, 2048.0, 0.0, 3.0]], np.float32), 1)
    assert acc.tolist() == [[1.0, 2048.0, 0.0, 3.0]] and disp.tolist() == acc.tolist() and rgb8.tolist() == [[gm.byte_f(1.0), gm.byte_f(2048.0), 0]]

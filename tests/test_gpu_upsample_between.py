"""The pipelining note of rt_upsample_device (Pipe::between, rt_host_ctx.hip.h), in the manner of tests/test_gpu_post_between.py: with rt_ctx_set_pipelining a frame
starts behind the PREVIOUS render call, so the call's four ranges -- the low-resolution values, both sets of planes (three planes each), the output -- must keep a frame
into the same buffer from taking the relaxed start.  The -DRT_DEBUG library refuses such a frame instead of racing: one child process under RT_LIB = the debug library,
one context, the cat scene, one stream, API refusals only.  Frame: 64 x 48, upsampled from 32 x 24.  -m gpu."""
import os
import subprocess
import sys

import pytest

import raytracinggpu_amd as rt

pytestmark = pytest.mark.gpu

CHILD = """
import sys
sys.path.insert(0, {root!r})
import numpy as np, torch
import raytracinggpu_amd as rt
g = np.load(rt.scenes.CAT_FIXTURE, allow_pickle=False)
ctx = rt.Context(0)
ctx.scene_upload(rt.scenes.spheres("cpu"), dict(vertices=g["vertices"], indices=g["tri_bvh_order"], bvh_arr10=g["bvh_arr10"], albedo=rt.scenes.CAT_ALBEDO, object_slot=6))
W, H, f = 64, 48, 2
st = torch.cuda.Stream()
s = st.cuda_stream
rows, _ = rt.interleaved_rows(H, 8, 0, 1)
p = rt.make_params(W, H, 1, 3, **rt.scenes.CPU_LAUNCHER)
buf = lambda n, h=H, w=W: torch.zeros((n, h, w, 4), dtype=torch.float32, device="cuda:0")
big = buf(3)                         # frame A is plane 2 of `big`: full-resolution planes laid over `big` cover it with the plane the kernel does not read
A = big[2].data_ptr()
B, out, out2, planes = buf(1), buf(1), buf(2), buf(3)
low, low_planes = buf(2, H // f, W // f), buf(3, H // f, W // f)
ctx.set_pipelining(True)

def case(name, between):
    ctx.render_device(p, rows, A, s)
    ctx.render_device(p, rows, B.data_ptr(), s)
    between()
    try:
        ctx.render_device(p, rows, A, s)
        print(name, "ACCEPTED", flush=True)
    except rt.RtError as e:
        print(name, "REFUSED", e.code, e, flush=True)

up = lambda low_=low.data_ptr(), lp=low_planes.data_ptr(), fp=planes.data_ptr(), o=out.data_ptr(), n=1: ctx.upsample_device(low_, lp, fp, W, H, f, o, n_planes=n, stream=s)
case("frame written into A:", lambda: up(o=A))
case("history written over A:", lambda: up(o=A - W * H * 16, n=2))     # (its second plane is A)
case("values read from A:", lambda: up(low_=A))
case("low planes read from A:", lambda: up(lp=A))
case("planes laid over A:", lambda: up(fp=big.data_ptr()))
case("elsewhere:", lambda: up())
case("elsewhere, two planes:", lambda: up(o=out2.data_ptr(), n=2))
torch.cuda.synchronize()
print("END", flush=True)
"""


def test_a_pipelined_frame_does_not_overtake_an_upsample_on_its_buffer(tmp_path):
    dbg = os.path.join(os.path.dirname(rt.__file__), "libraytrace_hip_debug.so")
    assert os.path.exists(dbg), "build() compiles the -DRT_DEBUG library"
    script = tmp_path / "upsample_between.py"
    script.write_text(CHILD.format(root=os.path.dirname(os.path.dirname(rt.__file__))))
    r = subprocess.run([sys.executable, str(script)], env=dict(os.environ, RT_LIB=dbg), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(r.stdout)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and lines[-1] == "END", r.stdout[-2000:]
    verdict = {ln.split(":")[0]: ln for ln in lines if ":" in ln}
    for name in ("frame written into A", "history written over A", "values read from A", "low planes read from A", "planes laid over A"):
        assert "REFUSED -1" in verdict[name] and "pipelining rule broken" in verdict[name], verdict[name]
    for name in ("elsewhere", "elsewhere, two planes"):
        assert "ACCEPTED" in verdict[name], verdict[name]

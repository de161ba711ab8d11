"""The pipelining note of the seven post-process device entries (Pipe::between, rt_host_ctx.hip.h): with rt_ctx_set_pipelining a frame starts behind the
PREVIOUS render call, so what the library itself put on the stream since then -- a filter that reads the frame, planes written over it -- must keep a frame into
the same buffer from taking the relaxed start.  The -DRT_DEBUG library refuses such a call instead of racing, which makes the check deterministic: one child
process under RT_LIB = the debug library, one context, the cat scene, one stream, API refusals only.  The second half of
test_pipelining_hazard_the_library_can_see (test_gpu_parity.py) is the same check for rt_tonemap_device.
Frame: 64 x 48 with interleaved_rows(H, 8, 0, 1) -- the debug library refuses the tone-mapping sequence at that size too (its first case here), so the
existing test's 640 x 360 is not needed.  The test asks nothing new of the library: it passes on the commit before the entries shared one helper.  -m gpu."""
import os
import subprocess
import sys

import pytest

import raytracinggpu_amd as rt

pytestmark = pytest.mark.gpu

W, H = 64, 48
ENTRIES = ("render_aov_device", "render_aov_surface_device", "denoise_device", "denoise_var_device", "temporal_accumulate_device", "demodulate_device",
           "modulate_device")

CHILD = """
import sys
sys.path.insert(0, {root!r})
import numpy as np, torch
import raytracinggpu_amd as rt
g = np.load(rt.scenes.CAT_FIXTURE, allow_pickle=False)
ctx = rt.Context(0)
ctx.scene_upload(rt.scenes.spheres("cpu"), dict(vertices=g["vertices"], indices=g["tri_bvh_order"], bvh_arr10=g["bvh_arr10"], albedo=rt.scenes.CAT_ALBEDO, object_slot=6))
W, H = {W}, {H}
st = torch.cuda.Stream()
s = st.cuda_stream
rows, _ = rt.interleaved_rows(H, 8, 0, 1)
p = rt.make_params(W, H, 1, 3, **rt.scenes.CPU_LAUNCHER)
buf = lambda *shape: torch.zeros(shape + (H, W, 4), dtype=torch.float32, device="cuda:0")
big, other = buf(3), buf(3)          # frame A is plane 0 of `big`: planes or a history laid over `big` cover it; `other` is disjoint from it
tensors = [buf(), buf(), buf(), buf(3), buf(2), torch.zeros((H * W * 3 + 16,), dtype=torch.uint8, device="cuda:0")]
A = big[0].data_ptr()
B, C, out, planes, hist, img = (t.data_ptr() for t in tensors)
ctx.set_pipelining(True)

def case(name, between):
    ctx.render_device(p, rows, A, s)
    ctx.render_device(p, rows, B, s)
    between()
    try:
        ctx.render_device(p, rows, A, s)
        print(name, "ACCEPTED", flush=True)
    except rt.RtError as e:
        print(name, "REFUSED", e.code, e, flush=True)

# entry -> the call with `frame` as its frame input (the filters) or under its plane output (the two plane entries)
entries = dict(
    tonemap_device=lambda frame, planes3: ctx.tonemap_device(frame, H * W, img, s),
    render_aov_device=lambda frame, planes3: ctx.render_aov_device(p, planes3, stream=s),
    render_aov_surface_device=lambda frame, planes3: ctx.render_aov_surface_device(p, 1, planes3, stream=s),
    denoise_device=lambda frame, planes3: ctx.denoise_device(frame, planes, W, H, out, stream=s),
    denoise_var_device=lambda frame, planes3: ctx.denoise_var_device(planes3, planes, W, H, out, stream=s),     # (history: the first two planes)
    temporal_accumulate_device=lambda frame, planes3: ctx.temporal_accumulate_device(frame, planes, None, None, W, H, hist, stream=s),
    demodulate_device=lambda frame, planes3: ctx.demodulate_device(frame, planes, H * W, out, stream=s),
    modulate_device=lambda frame, planes3: ctx.modulate_device(frame, planes, H * W, out, stream=s),
)
for name, call in entries.items():
    case(name + " on A:", lambda: call(A, big.data_ptr()))
    case(name + " elsewhere:", lambda: call(C, other.data_ptr()))
for n in (32, 33):                   # two ranges a call: 64 are kept, the 65th and 66th are not
    case(f"{{n}} calls elsewhere:", lambda: [ctx.demodulate_device(C, planes, H * W, out, stream=s) for _ in range(n)])
torch.cuda.synchronize()
print("END", flush=True)
"""


def test_a_frame_does_not_overtake_post_process_work_on_its_buffer(tmp_path):
    dbg = os.path.join(os.path.dirname(rt.__file__), "libraytrace_hip_debug.so")
    assert os.path.exists(dbg), "build() compiles the -DRT_DEBUG library"
    script = tmp_path / "post_between.py"
    script.write_text(CHILD.format(root=os.path.dirname(os.path.dirname(rt.__file__)), W=W, H=H))
    r = subprocess.run([sys.executable, str(script)], env=dict(os.environ, RT_LIB=dbg), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(r.stdout)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and lines[-1] == "END", r.stdout[-2000:]

    def verdict(case):
        found = [ln for ln in lines if ln.startswith(case + ":")]
        assert len(found) == 1, (case, r.stdout[-2000:])
        return found[0]

    wrong = []
    for name in ("tonemap_device",) + ENTRIES:
        hit, clear = verdict(name + " on A"), verdict(name + " elsewhere")
        if not ("REFUSED -1" in hit and "pipelining rule broken" in hit):
            wrong.append(hit)
        if "ACCEPTED" not in clear:
            wrong.append(clear)
    if "ACCEPTED" not in verdict("32 calls elsewhere"):
        wrong.append(verdict("32 calls elsewhere"))
    over = verdict("33 calls elsewhere")                             # 66 ranges: more than are kept, so the frame must not take the relaxed start
    if not ("REFUSED -1" in over and "pipelining rule broken" in over):
        wrong.append(over)
    assert not wrong, "\n".join(wrong)

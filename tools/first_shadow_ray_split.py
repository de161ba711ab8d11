"""GPU box: which rays the chain's traversal launches carry, per segment, with every elision rule on (RT_TRAVQ_QW_COUNT=1: the 4-wide kernel's own counting run, any-hit
and the dead-channel rule in force).  A segment's rays do not depend on the number of bounces (the bounce keys are (pixel, sample, depth)), so the counting runs of
num_bounce 0 .. B differ by exactly one segment each: launch k of the chain traces segment k's continuation rays and segment k - 1's shadow rays.

usage: RT_TRAVQ_QW_COUNT=1 python tools/first_shadow_ray_split.py [--width 1920 --height 1080 --bounces 3]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import raytracinggpu_amd as rt
from raytracinggpu_amd import hostlib

ap = argparse.ArgumentParser()
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--bounces", type=int, default=3)
args = ap.parse_args()
if os.environ.get("RT_TRAVQ_QW_COUNT") != "1":
    raise SystemExit("set RT_TRAVQ_QW_COUNT=1: the float-pair counting run traces every shadow ray to the end")
v, t = rt.scenes.load_cat_arrays()
c = rt.Context(0)
c.scene_upload(rt.scenes.spheres("cpu"), hostlib.build_mesh(v, t, albedo=rt.scenes.CAT_ALBEDO, object_slot=rt.scenes.mesh_slot("cpu")))
ys, xs = [0], [0]
for b in range(args.bounces + 1):
    d = c.count_work(rt.make_params(args.width, args.height, 1, b, **rt.scenes.CPU_LAUNCHER), detail=True)["dead_channels"]
    ys.append(d["trav_continuation"])
    xs.append(d["trav_shadow"])
seg_y = [ys[k + 1] - ys[k] for k in range(args.bounces + 1)]
seg_x = [xs[k + 1] - xs[k] for k in range(args.bounces + 1)]
print("cat %dx%d, 1 sample, %d bounces: rays handed to the mesh traversal per segment" % (args.width, args.height, args.bounces))
print("segment:            " + "".join("%12d" % k for k in range(args.bounces + 1)))
print("continuation rays:  " + "".join("%12d" % n for n in seg_y))
print("shadow rays:        " + "".join("%12d" % n for n in seg_x))
for k in range(args.bounces + 2):
    y = seg_y[k] if k <= args.bounces else 0
    x = seg_x[k - 1] if k >= 1 else 0
    print("traversal launch %d: %9d continuation + %9d shadow = %9d rays (%.0f %% shadow)" % (k, y, x, x + y, 100.0 * x / max(x + y, 1)))
c.close()

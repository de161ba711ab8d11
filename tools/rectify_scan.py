#!/usr/bin/env python3
"""The quality scan behind DESIGN.md section 5.12, on the CPU: the oracle renders the sequences, the numpy models (tests/) run the chain.

Section 5.8's protocol -- 128 x 128, b = 3, one-sample frames with a new seed each, RMSE in the tonemap's [0, 1] scale against a 256-sample frame of the frame's own
scene -- over (a) a moving light on the cat scene and on demo10 (16 frames, the light still for frames 0 - 7 and stepped by rt_light_orbit from frame 8), (b) section
5.10's moving sphere, (c) section 5.8's two static sequences.  Rows: the chain as it is, alpha_min raised globally (two values), and rectification over fast_history x
radius x k_clamp.  Prints the table; --json FILE keeps every figure."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--sequences", default="light:cpu,light:demo10,moving,static:cpu,static:demo10")
    args = ap.parse_args()
    from oracle import oracle_py
    from tests import test_rectify_model as t
    from tests.conftest import load_golden
    oracle_py.lib()
    g = load_golden("cat_mesh.npz")
    cat = oracle_py.Mesh.from_arrays(g["vertices"], g["tri_obj_order"]).build_bvh()
    rows = dict(t.BASE_ROWS)
    rows.update({f"rectify h{h} r{r} k{k:g}": dict(fast_history=h, radius=r, k_clamp=k) for h in t.SCAN_FAST for r in t.SCAN_RADIUS for k in t.SCAN_K})
    res = {}
    for name in args.sequences.split(","):
        seq = t.sequence(oracle_py, cat, name)
        res[name] = {}
        for row, kw in rows.items():
            res[name][row] = t.errors(oracle_py, seq, **kw)
            e = res[name][row]
            late = e[8:] if name.startswith("light") else e[-1:]
            print(f"{name:14s} {row:22s} mean late {sum(late) / len(late):.5f}  per frame " + " ".join(f"{v:.5f}" for v in e), flush=True)
        if args.json:
            with open(args.json, "w") as f:
                json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

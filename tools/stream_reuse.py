#!/usr/bin/env python3
"""Which streams of the default pipeline can live in the 256 MiB Infinity Cache: a reuse table from the layouts alone (no GPU).

From width, height, segments (bounces + 1), sub-frames and the chain plan of csrc/rt_still.h (through the host library's rth_still_replay: the plan of a still view's
third frame, the steady state, or of its first with --frame 0) this prints, for every stream of the wavefront pipeline (csrc/rt_wavefront.hip.h WfState, WfShade; the
buffers of csrc/rt_host_render.hip.h size_wavefront):

    bytes per frame (all sub-frames), the launch that writes it, the launch that reads it last, and what every kernel of ALL chains moves between the two --
    `traffic`: bytes loaded or stored by the launches strictly between writer and reader; `footprint`: the distinct bytes those launches and the two ends touch
    (a queue record rewritten in place counts once).  A line can still be in the cache when its reader comes only if the footprint fits (the residency rule of the
    Infinity Cache: the line plus every byte loaded or stored between two uses of it within about 256 MiB).

The figures are UPPER BOUNDS by layout: every path alive in every launch, every ray through the mesh's root box, every shadow ray emitted.  A real frame's paths die
along the chain (a miss is folded in the launch that meets it), so its traffic is lower; the sizes of the buffers, and with them the footprints, are exact.
The sub-frames' chains run side by side, so every launch counts once per sub-frame.

usage: python tools/stream_reuse.py [--width 1920 --height 1080 --bounces 3 --parts 2 --frame 2] [--json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CACHE = 256 << 20                                                    # the Infinity Cache
# bytes per path (or per pixel slot) of every region, as the kernels lay them out
QR_REC = 32                                                          # one queue record (two float4); a path owns a continuation (Y) and a shadow (X) slot
M_WORD = 8                                                           # one traversal result
LS_WORD, SID_BYTE, DCH_BYTE = 4, 1, 1                                # per shaded segment: the direct term, the surface id; per path: the dead channels
S0_REC = 32                                                          # first-shade record per pixel slot (WfShade::rec)
LEVEL_WORD = 8                                                       # first-hit / first-shadow word per pixel slot (M0, X0)
PIXEL = 16                                                           # the frame: one float4 per pixel
ADV_BEGIN, ADV_RESUME, ADV_PLAIN, ADV_FILL, ADV_CLOSE = range(5)     # rt_still.h StillAdv
WIN_NONE, WIN_Y, WIN_X = range(3)                                    # rt_still.h StillWin
ADV_NAME = {ADV_BEGIN: "wf_advance<first>", ADV_RESUME: "wf_advance<resume>", ADV_PLAIN: "wf_advance", ADV_FILL: "wf_advance<fill>", ADV_CLOSE: "wf_advance<close>"}


def pixel_slots(width, height, parts):
    """pixel slots of the frame: every sub-frame is a band of rows cut into 8 x 8 tiles, 64 slots each"""
    rows = -(-height // parts)
    return parts * (-(-width // 8)) * (-(-rows // 8)) * 64


def chain_plan(segs, frame):
    """(position, traversal, window, m0, x0, wf_advance) of every launch of part 0's chain in frame `frame` of a still view of the plain default pipeline"""
    from raytracinggpu_amd import hostlib
    ev = []
    for _ in range(frame + 1):
        ev += [(0, 3, 1, 1, 1), (1, 0, segs, 1 | 2 | 4 | 8), (1, 1, segs, 1 | 2 | 4 | 8)]
    _, rows = hostlib.still_replay(ev)
    first = 3 * frame + 1
    return [(int(r[1]), bool(r[2]), int(r[3]), int(r[5]), int(r[6]), int(r[7]), int(r[8])) for r in rows if int(r[0]) == first]


def launches(segs, plan):
    """every launch of one chain as (name, {region: (bytes read, bytes written) per path})"""
    out = []
    for pos, trav, win, m0, x0, adv, kill_x in plan:
        if trav:
            t = {}
            res = "M0" if (pos == 0 and m0) else "M.y"
            if win != WIN_X:
                t["QR.y"] = (QR_REC, 0); t[res] = (0, M_WORD)
            if win != WIN_Y and pos >= 1:
                t["QR.x"] = (QR_REC, 0); t["M.x"] = (0, M_WORD)
            out.append((f"wf_travq@{pos}", t))
        a = {}
        if adv == ADV_BEGIN:
            a["QR.y"] = (0, QR_REC); a["DCH"] = (0, DCH_BYTE)
            out.append((f"{ADV_NAME[adv]}", a))
            continue
        if adv == ADV_RESUME:
            a["S0"] = (S0_REC, 0); a["QR.y"] = (0, QR_REC); a["DCH"] = (0, DCH_BYTE)
            if kill_x:
                a["QR.x"] = (0, QR_REC // 2)
            a["LS[0]"] = (0, LS_WORD); a["SID[0]"] = (0, SID_BYTE)
            a["frame"] = (0, PIXEL)                                  # a path that misses at once is folded here
            out.append((f"{ADV_NAME[adv]}", a))
            continue
        shade = pos < segs                                           # the launch at position `pos` shades segment `pos`; the last one only closes and folds
        a["QR.y"] = (QR_REC if shade else QR_REC // 2, QR_REC if shade else 0)
        if shade:
            a["M0" if m0 else "M.y"] = (M_WORD, 0)
            a["QR.x"] = (0, QR_REC); a["DCH"] = (DCH_BYTE, DCH_BYTE)
            a[f"LS[{pos}]"] = (0, LS_WORD); a[f"SID[{pos}]"] = (0, SID_BYTE)
        if pos >= 1:                                                 # the shadow ray of segment pos - 1 comes back
            a["X0" if x0 == 2 else "M.x"] = (M_WORD, 0)
            r, w = a.get("QR.x", (0, 0)); a["QR.x"] = (r + QR_REC, w)
            a[f"LS[{pos - 1}]"] = (0, LS_WORD)                       # zeroed where the ray is blocked
        if x0 == 1 and pos >= 1:
            a["X0"] = (0, LEVEL_WORD)
        if adv == ADV_FILL:
            a["S0"] = (0, S0_REC)
            a["X0"] = (LEVEL_WORD, 0)
        for k in range(min(pos + (1 if shade else 0), segs)):        # the fold of a path that ends here
            r, w = a.get(f"LS[{k}]", (0, 0)); a[f"LS[{k}]"] = (r + LS_WORD, w)
            r, w = a.get(f"SID[{k}]", (0, 0)); a[f"SID[{k}]"] = (r + SID_BYTE, w)
        a["frame"] = (0, PIXEL)
        out.append((f"{ADV_NAME[adv]}@{pos}", a))
    return out


def table(width=1920, height=1080, bounces=3, parts=2, frame=2, plan=None):
    segs = bounces + 1
    plan = plan if plan is not None else chain_plan(segs, frame)
    n = pixel_slots(width, height, parts)                            # one sample: paths == pixel slots
    ls = launches(segs, plan)
    size = {"QR.y": QR_REC * n, "QR.x": QR_REC * n, "M.y": M_WORD * n, "M.x": M_WORD * n, "M0": LEVEL_WORD * n, "X0": LEVEL_WORD * n, "DCH": DCH_BYTE * n,
            "S0": S0_REC * n, "frame": PIXEL * width * height}
    for k in range(segs):
        size[f"LS[{k}]"] = LS_WORD * n; size[f"SID[{k}]"] = SID_BYTE * n

    def moved(touch):                                                # bytes one launch moves, all sub-frames
        return sum((r + w) * (n if reg != "frame" else width * height) for reg, (r, w) in touch.items())

    per_launch = [(name, moved(t)) for name, t in ls]
    frame_traffic = sum(b for _, b in per_launch)
    touched_frame = set().union(*[set(t) for _, t in ls])
    frame_footprint = sum(size[r] for r in touched_frame)
    rows = []
    for reg in sorted(touched_frame, key=lambda r: (r.split("[")[0], r)):
        writers = [i for i, (_, t) in enumerate(ls) if t.get(reg, (0, 0))[1]]
        readers = [i for i, (_, t) in enumerate(ls) if t.get(reg, (0, 0))[0]]
        if writers and readers and max(readers) > min(writers):       # written and read inside one chain: the first write to the last read
            wi, ri = min(writers), max(readers)
            if reg in ("QR.y", "QR.x", "M.y", "M.x", "DCH"):          # rewritten every launch: the nearest read after a write
                wi = max(w for w in writers if w < ri)
                ri = min(r for r in readers if r > wi)
            between = ls[wi + 1:ri]
            traffic = sum(per_launch[i][1] for i in range(wi + 1, ri))
            regs = set(ls[wi][1]) | set(ls[ri][1])
            for _, t in between:
                regs |= set(t)
            foot = sum(size[r] for r in regs)
            rows.append(dict(stream=reg, bytes=size[reg], writer=ls[wi][0], reader=ls[ri][0], traffic=traffic, footprint=foot, reach=foot <= CACHE))
        else:                                                         # once per frame (or once per still view): the next use is a frame away
            who_w = ls[writers[0]][0] if writers else "(an earlier frame)"
            who_r = ls[readers[0]][0] + ", next frame" if readers else "(nobody on the GPU)"
            rows.append(dict(stream=reg, bytes=size[reg], writer=who_w, reader=who_r, traffic=frame_traffic, footprint=frame_footprint, reach=frame_footprint <= CACHE))
    return dict(width=width, height=height, segs=segs, parts=parts, paths=n, launches=per_launch, frame_traffic=frame_traffic, frame_footprint=frame_footprint, rows=rows)


def group_totals(t):
    """bytes per frame of the streams the issue's four policy groups cover, and of the path state that is to stay cached"""
    b = {r["stream"]: r["bytes"] for r in t["rows"]}
    segs = t["segs"]
    return dict(QR=b.get("QR.y", 0) + b.get("QR.x", 0), M=b.get("M.y", 0) + b.get("M.x", 0), LS=sum(b.get(f"LS[{k}]", 0) for k in range(segs)),
                SID=sum(b.get(f"SID[{k}]", 0) for k in range(segs)), DCH=b.get("DCH", 0), S0=b.get("S0", 0), frame=b.get("frame", 0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--bounces", type=int, default=3)
    ap.add_argument("--parts", type=int, default=2)
    ap.add_argument("--frame", type=int, default=2, help="frame of a still view whose chains are planned: 0 fills the hit and shadow levels, 1 stores the records, 2 resumes")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    t = table(a.width, a.height, a.bounces, a.parts, a.frame)
    if a.json:
        print(json.dumps(t))
        return
    mb = lambda x: f"{x / 1e6:8.1f}"
    print(f"{a.width}x{a.height}, {t['segs']} segments, {a.parts} sub-frames, frame {a.frame} of a still view: {t['paths']} paths; MB = 1e6 bytes; cache {CACHE / 1e6:.1f} MB")
    print("launches of one frame (all sub-frames), upper bound of the bytes each moves:")
    for name, b in t["launches"]:
        print(f"    {name:22s} {mb(b)} MB")
    print(f"    {'the frame':22s} {mb(t['frame_traffic'])} MB moved, {mb(t['frame_footprint'])} MB distinct")
    print(f"{'stream':8s} {'MB/frame':>9s}  {'written by':22s} {'read last by':34s} {'traffic MB':>10s} {'footprint MB':>12s}  in reach")
    for r in t["rows"]:
        print(f"{r['stream']:8s} {mb(r['bytes'])}   {r['writer']:22s} {r['reader']:34s} {mb(r['traffic'])}   {mb(r['footprint'])}     {'yes' if r['reach'] else 'NO'}")
    g = group_totals(t)
    print("totals: " + ", ".join(f"{k} {v / 1e6:.1f}" for k, v in g.items()) + f" -- sum {sum(g.values()) / 1e6:.1f} MB")


if __name__ == "__main__":
    main()

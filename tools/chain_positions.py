"""Per-position averages of a launch chain's kernels from a rocprofv3 kernel trace (CPU only).

`rocprofv3 --kernel-trace --stats` averages wf_travq and wf_advance over the five launches of the headline's chain, which differ by a factor of three; this splits the trace
by queue, restarts the position at every opening launch (form `first`) and averages each position on its own -- what the first and the last launch of the chain cost.  A
resumed chain (first-shade cache) opens with the form `resume`, which stands for the opening launch and the launch at position 0: its launches are filed from position 1 on.
Which form a wf_advance launch is: tools/advance_forms.py (the names of before the one kernel template too).

The last line files the wf_travq launches at position 1 by their chain's number on its queue mod 4 -- the two bits of WfState::nonce: a stale shadow record that a launch
takes for its own every fourth chain would show as one class slower than the other three.

usage: python tools/chain_positions.py DIR   (DIR: what rocprofv3 -d wrote; reads the first *kernel_trace.csv below it)"""
import collections
import csv
import glob
import sys

from advance_forms import form, form_of

fs = glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)
if not fs:
    raise SystemExit("no kernel trace under " + sys.argv[1])
per = collections.defaultdict(list)
for r in csv.DictReader(open(fs[0])):
    per[r.get("Queue_Id", "0")].append(r)
acc = {"wf_travq": collections.defaultdict(list), "wf_advance": collections.defaultdict(list), "wf_advance<FIRST>": collections.defaultdict(list),
       "wf_advance_resume": collections.defaultdict(list)}
turn = collections.defaultdict(list)
for rs in per.values():
    rs.sort(key=lambda r: int(r["Start_Timestamp"]))
    kt = ka = chain = -1
    for r in rs:
        name, dur = r["Kernel_Name"], int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        f = form_of(name)
        if f == form("first"):
            kt = ka = 0
            chain += 1
            acc["wf_advance<FIRST>"][0].append(dur)
        elif f == form("resume"):
            kt = ka = 1
            chain += 1
            acc["wf_advance_resume"][0].append(dur)
        elif kt >= 0 and "wf_travq" in name:
            if ka == 1:
                turn[chain & 3].append(dur)
            acc["wf_travq"][ka].append(dur)                      # the launch before wf_advance number ka: a chain that skipped its first traversal launch (first-hit cache) has none at 0
            kt += 1
        elif ka >= 0 and f is not None:
            acc["wf_advance"][ka].append(dur)
            ka += 1
for kind, a in acc.items():
    if a:
        print("%s by position in the chain, average / fastest / slowest us (launches): %s" % (
            kind, ", ".join("%d: %.1f / %.1f / %.1f (%d)" % (k, sum(v) / len(v) / 1e3, min(v) / 1e3, max(v) / 1e3, len(v)) for k, v in sorted(a.items()))))
print("wf_travq at position 1 by chain number mod 4, average / fastest / slowest us (launches): %s" % (
    ", ".join("%d: %.1f / %.1f / %.1f (%d)" % (k, sum(v) / len(v) / 1e3, min(v) / 1e3, max(v) / 1e3, len(v)) for k, v in sorted(turn.items()))))

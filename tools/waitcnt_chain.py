#!/usr/bin/env python3
"""How many times does a kernel's main path stop for memory before its first store?  (CPU only.)

Reads a gfx950 device assembly (`hipcc <the build's flags> -S --cuda-device-only`, as for tools/asm_compare.py) and walks one kernel's text in the order it is
written, from its first vector load to the first vector store behind the label `--until` (default: the first store of all).  A `s_waitcnt vmcnt(n)` counts as a DRAIN when
more than n loads were issued since the last wait that left fewer: a wait with nothing in flight costs nothing and is listed apart, as are the partial waits of one burst
of loads (several vmcnt(k) in a row with no load between them count once).  Text order is not execution order: a block that few lanes enter (the read-back of a shadow
record) is walked like any other, so the lines are printed and the reader strikes those out.

usage: python tools/waitcnt_chain.py FILE.s KERNEL_REGEX [--until LABEL_REGEX]     e.g.  ... branch.s 'wf_advanceILj0EJEEE' --until rt_mark_adv_diffuse_begin"""
import re
import sys

path, pat = sys.argv[1], sys.argv[2]
until = sys.argv[sys.argv.index("--until") + 1] if "--until" in sys.argv else None
lines, on = [], False
for ln in open(path):
    if not on and re.match(r"^_Z\w*(%s)\w*:" % pat, ln):
        on = True
        continue
    if on:
        if ln.startswith(".Lfunc_end"):
            break
        lines.append(ln.split(";")[0].rstrip())
inflight, started, armed, drains, idle, burst = 0, False, until is None, [], 0, False
for n, t in enumerate(lines, 1):
    s = t.strip()
    if until and re.search(until, s):
        armed = True
    if re.match(r"(global|flat|buffer)_load", s):
        inflight += 1
        started, burst = True, False
    elif re.match(r"(global|flat|buffer)_store", s):
        if started and armed:
            break
    else:
        m = re.match(r"s_waitcnt.*vmcnt\((\d+)\)", s)
        if m and started:
            k = int(m.group(1))
            if inflight > k:
                if not burst:
                    drains.append((n, s, inflight))
                inflight, burst = k, True
            else:
                idle += 1
print("%s: %d drains between the first load and the first store%s; %d waits with nothing more in flight than they allow" % (
    pat, len(drains), " behind " + until if until else "", idle))
for n, s, k in drains:
    print("    line %5d  %-24s %d in flight" % (n, s, k))

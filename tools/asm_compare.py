#!/usr/bin/env python3
"""Did a change move an existing kernel?  Compares two gfx950 device assemblies of rt_capi.hip function by function.

usage: hipcc <the build's flags without -fPIC -shared> -S --cuda-device-only -o parent.s raytracinggpu_amd/csrc/rt_capi.hip   (once in each tree)
       python tools/asm_compare.py parent.s this.s [old_name=new_name ... | @file of such lines]

A function is the text from its label to its .Lfunc_end, comments dropped; what the compiler numbers per translation unit (.LBB<n>_, .Ltmp<n>, the
__hip_cuid symbol) is normalised, and a function's own name is replaced by a placeholder, so that a kernel that only changed its name (old=new on the command
line, or a unique match by the name in front of the template arguments) still compares instruction for instruction.  Section directives are not instructions
and are dropped.  The function comparison stops at .Lfunc_end, so what the code object says ABOUT a kernel is compared too: the fields META of its entry in the
amdhsa metadata (registers, scratch, argument segment, workgroup size, LDS).  Prints one line per function that differs, is missing or is new, one per kernel
whose metadata differs, and a summary; exit status 1 if an existing function differs or is missing, or a kernel's metadata differs."""
import re
import sys


def functions(path):
    out, cur, closed = {}, None, set()
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m and cur is None:
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            closed.add(cur)
            cur = None
            continue
        t = line.split(";")[0].rstrip()
        t = re.sub(r"\.LBB\d+_", ".LBB_", t)
        t = re.sub(r"\.Ltmp\d+", ".Ltmp", t)
        t = re.sub(r"__hip_cuid_\w+", "__hip_cuid", t)
        t = re.sub(r"^(\s*rt_mark_\w+?)_\d+:", r"\1:", t)            # the kernels' code-object markers (ADV_MARK, WQ_MARK): labels numbered through the translation unit too
        if t.strip() and not t.lstrip().startswith((".section", ".text")):
            out[cur].append(t.replace(cur, "<self>"))
    return {k: v for k, v in out.items() if k in closed}             # (a label that never reaches .Lfunc_end is an object, not a function)


META = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".kernarg_segment_size", ".max_flat_workgroup_size", ".group_segment_fixed_size")


def metadata(path):
    """{kernel: {field: value}} from the amdhsa.kernels list: a kernel's fields stand between two "  - .agpr_count:" / "  - .args:" list heads, its .name among them"""
    out, cur = {}, {}
    for line in open(path):
        if re.match(r"^  - \.", line) and cur:
            out[cur.get(".name")] = cur
            cur = {}
        m = re.match(r"^(?:  - |    )(\.\w+):\s+(\S+)\s*$", line)
        if m and (m.group(1) in META or m.group(1) == ".name"):
            cur[m.group(1)] = m.group(2)
        if line.startswith("amdhsa.target") and cur:
            out[cur.get(".name")] = cur
            cur = {}
    return {k: {f: v[f] for f in META if f in v} for k, v in out.items() if k}


def base(name):
    m = re.match(r"_ZN(\d+)rtk(\d+)", name)
    return name[:m.end() + int(m.group(2))] if m else name


def main():
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    pairs = [y for x in sys.argv[3:] for y in (open(x[1:]).read().split() if x.startswith("@") else [x])]
    renamed = dict(x.split("=") for x in pairs)
    ma, mb = metadata(sys.argv[1]), metadata(sys.argv[2])
    bad = same = meta_same = meta_bad = 0
    for k, body in a.items():
        to = renamed.get(k, k)
        if to not in b:
            cands = [n for n in b if n not in a and base(n) == base(k) and b[n] == body]
            to = cands[0] if len(cands) == 1 else None
        if to is None:
            print("MISSING in the new assembly:", k)
            bad += 1
        elif b[to] != body:
            print(f"DIFFERS: {k} ({len(body)} lines against {len(b[to])})")
            bad += 1
        else:
            same += 1
            if to != k:
                print(f"identical under a new name ({len(body)} lines): {k} -> {to}")
        if to is not None and k in ma:
            if ma[k] != mb.get(to):
                print(f"METADATA DIFFERS: {k}: {ma[k]} against {mb.get(to)}")
                meta_bad += 1
            else:
                meta_same += 1
                if to != k:
                    print(f"    its metadata too: " + ", ".join(f"{f[1:]} {v}" for f, v in ma[k].items()))
    matched = set(a) | {n for n in b if any(base(n) == base(k) and b[n] == a[k] for k in a if k not in b)}
    for k in b:
        if k not in matched and k not in renamed.values():
            print(f"NEW: {k} ({len(b[k])} lines)")
    n_new = sum(1 for k in b if k not in matched and k not in renamed.values())
    print(f"{len(a)} functions in the old assembly: {same} identical, {bad} differing or missing; {len(b)} functions in the new one, {n_new} new")
    print(f"{len(ma)} kernels in the old metadata: {meta_same} with equal {' '.join(f[1:] for f in META)}, {meta_bad} differing")
    return 1 if bad or meta_bad else 0


if __name__ == "__main__":
    sys.exit(main())

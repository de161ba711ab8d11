#!/usr/bin/env python3
"""Writes the threshold tables of raytracinggpu_amd/csrc/rt_gamma.h from the exact model (tests/gamma_model.py: `decimal` at 80 digits, never the machine's libm).

    python tools/gen_gamma_table.py            rewrite the lines between the markers of each table the header holds
    python tools/gen_gamma_table.py --check    exit 1 if the header's lines are not what the model gives

A table is the 255 binary32 bit patterns T_1 ... T_255, T_k the least binary32 whose byte is >= k; the header marks one with
`// gamma-table-begin <path>` ... `// gamma-table-end`, <path> = f (powf(c, 1 / 2.2f)) or d (pow((double)c, 1./2.2))."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "raytracinggpu_amd", "csrc", "rt_gamma.h")
sys.path.insert(0, ROOT)
from tests import gamma_model as gm  # noqa: E402

BLOCK = re.compile(r"(// gamma-table-begin (\w)\n)(.*?)(// gamma-table-end)", re.S)


def table_text(path):
    t = gm.thresholds_f() if path == "f" else gm.thresholds_d()
    rows = [", ".join(f"0x{b:08x}u" for b in t[i:i + 8]) for i in range(0, 255, 8)]
    return "\n".join("    " + r + ("," if i + 1 < len(rows) else "") for i, r in enumerate(rows))


def header_tables(text):
    """-> {path: [255 ints]} as the header holds them"""
    return {m.group(2): [int(x, 16) for x in re.findall(r"0x([0-9a-f]{8})u", m.group(3))] for m in BLOCK.finditer(text)}


def main():
    with open(HEADER) as f:
        old = f.read()
    new = BLOCK.sub(lambda m: m.group(1) + table_text(m.group(2)) + "\n" + m.group(4), old)
    if not BLOCK.search(old):
        sys.exit(f"{HEADER}: no table markers")
    if "--check" in sys.argv[1:]:
        sys.exit(0 if new == old else 1)
    if new != old:
        with open(HEADER, "w") as f:
            f.write(new)
    print(f"{HEADER}: tables {sorted(header_tables(new))}")


if __name__ == "__main__":
    main()

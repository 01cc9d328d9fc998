#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds of libmpinets_hip.so:  tools/isa_diff.py OLD.so NEW.so [--md OUT.md]

For a refactor that must not change what the compiler emits.  Both libraries' code objects are extracted the way
tests/test_code_objects.py does (its ``code_objects`` is imported, not restated), disassembled with ``llvm-objdump -d``
and compared kernel by kernel after normalisation: instruction addresses and encodings are dropped, and so is the
literal of the ``s_add_u32`` / ``s_addc_u32`` pair behind an ``s_getpc_b64`` (a pc-relative distance to another symbol
of the code object, which moves when any function in front of it changes size).

One line per kernel: ``identical``, or -- for a stream that differs -- its metadata (registers, spills, scratch, LDS,
kernarg size) and its counts of matrix, memory, LDS, wait and barrier instructions, old -> new.  Exit status 1 if the
sets of kernel symbols differ, or a differing kernel's metadata or counts differ.
"""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from test_code_objects import _tool, code_objects, demangle_head, kernel_metadata  # noqa: E402

META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
        ".private_segment_fixed_size", ".group_segment_fixed_size", ".kernarg_segment_size")
COUNTED = (("v_mfma", r"v_mfma"), ("vmem loads", r"(buffer|global)_load"), ("ds", r"ds_"), ("s_waitcnt", r"s_waitcnt"),
           ("s_barrier", r"s_barrier"))


def functions(so_path):
    """-> {symbol: [normalised instruction lines]} over every gfx950 code object of ``so_path``."""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in code_objects(so_path, tmp):
            text = subprocess.run([_tool("llvm-objdump"), "-d", co], check=True, capture_output=True, text=True).stdout
            cur, pcrel = None, 0
            for line in text.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if m:
                    cur, pcrel = out.setdefault(m.group(1), []), 0
                    continue
                if cur is None or not line.startswith("\t"):
                    continue
                ins = re.sub(r"\s+", " ", line.split("//")[0].strip())
                if ins.startswith("s_getpc_b64"):
                    pcrel = 2
                elif pcrel and ins.startswith(("s_add_u32", "s_addc_u32")):
                    ins, pcrel = ins.rsplit(",", 1)[0] + ", <pcrel>", pcrel - 1
                if ins:
                    cur.append(ins)
    for lines in out.values():  # (alignment padding behind a function's last instruction)
        while lines and lines[-1].startswith(("s_nop", "s_code_end")):
            lines.pop()
    return out


def counts(lines):
    return {name: sum(1 for ln in lines if re.match(rx, ln)) for name, rx in COUNTED}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--md", help="also write the summary to this file")
    ap.add_argument("--show", metavar="SUBSTR", help="print the unified diff of the kernels whose name contains SUBSTR")
    args = ap.parse_args()
    md_old, md_new = kernel_metadata(args.old), kernel_metadata(args.new)
    fn_old, fn_new = functions(args.old), functions(args.new)
    rows, bad = [], False
    only_old, only_new = sorted(set(md_old) - set(md_new)), sorted(set(md_new) - set(md_old))
    for sym in only_old:
        rows.append(f"- `{sym}`: ONLY IN OLD")
    for sym in only_new:
        rows.append(f"- `{sym}`: ONLY IN NEW")
    bad |= bool(only_old or only_new)
    n_same = 0
    for sym in sorted(set(md_old) & set(md_new), key=lambda s: (demangle_head(s), s)):
        a, b = fn_old.get(sym, []), fn_new.get(sym, [])
        if a and a == b:
            n_same += 1
            rows.append(f"- `{demangle_head(sym)}` (`{sym}`): identical")
            continue
        changed = sum(1 for ln in difflib.unified_diff(a, b, lineterm="", n=0) if ln[:1] in "+-" and ln[:3] not in ("+++", "---"))
        meta = ", ".join(f"{k[1:]} {md_old[sym].get(k)} -> {md_new[sym].get(k)}" for k in META)
        ca, cb = counts(a), counts(b)
        cnt = ", ".join(f"{k} {ca[k]} -> {cb[k]}" for k in ca)
        equal = all(md_old[sym].get(k) == md_new[sym].get(k) for k in META) and ca == cb
        bad |= not equal
        rows.append(f"- `{demangle_head(sym)}` (`{sym}`): DIFFERS, {changed} changed lines of {len(a)} -> {len(b)}; "
                    f"metadata and counts {'equal' if equal else 'NOT EQUAL'}: {meta}; {cnt}")
        if args.show and args.show in sym:
            print("\n".join(difflib.unified_diff(a, b, "old", "new", lineterm="", n=2)))
    head = f"{len(md_old)} kernels in the old library, {len(md_new)} in the new one; {n_same} identical instruction streams."
    text = "\n".join([head, ""] + rows) + "\n"
    sys.stdout.write(text)
    if args.md:
        with open(args.md, "w") as f:
            f.write("# Kernel-by-kernel comparison of two builds (tools/isa_diff.py)\n\n" + text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Did the unweighted k_contrib<QW, QH> keep its instruction stream when it became k_contrib<QW, QH, false>?  (No GPU needed.)

  hipcc <the Makefile's COMMON flags> --cuda-device-only -S csrc/contrib.hip -o {old,new}.s       (old: the parent commit's tree)
  python scripts/attrib_asm_diff.py old.s new.s > profiles/attrib/contrib_asm_diff.txt

The kernels' names differ (the new template argument) and so does the kernarg segment (ContribParams grew at its END), so
blend_asm_diff.py's named comparison cannot pass.  This pairs old k_contrib<a, b> with new k_contrib<a, b, false>, normalises
both with blend_asm_diff.kernels (own name -> placeholder, label indices and comments stripped) and prints, per pair, the unified
diff of (1) the function body without its .amdhsa_* lines -- the instruction stream -- and (2) the .amdhsa_* descriptor lines, then
the metadata row of each.  Exit status 0 iff every instruction stream is identical; descriptor / metadata differences are listed."""
import difflib
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import blend_asm_diff as B  # noqa: E402


def split(text):
    """(instruction stream, descriptor lines)"""
    lines = text.split("\n")
    desc = [ln for ln in lines if re.match(r"\s*\.(amdhsa_|end_amdhsa_kernel)", ln)]
    return [ln for ln in lines if ln not in desc], desc


def main(old_path, new_path):
    old, new = B.kernels(old_path), B.kernels(new_path)
    old_meta, new_meta = B.metadata(old_path), B.metadata(new_path)
    names = B.demangle(sorted(set(old) | set(new)))
    by_name_old = {names[n]: n for n in old}
    streams_same = True
    pairs = 0
    for n in sorted(new, key=lambda n: names[n]):
        m = re.search(r"k_contrib<(\d+), (\d+), false>", names[n])
        if not m:
            continue
        want = names[n].replace(f"<{m.group(1)}, {m.group(2)}, false>", f"<{m.group(1)}, {m.group(2)}>")
        o = by_name_old.get(want)
        print(f"==== {names[n]}  <-  {want}")
        if o is None:
            print("  missing in old")
            streams_same = False
            continue
        pairs += 1
        (body_o, desc_o), (body_n, desc_n) = split(old[o]), split(new[n])
        d = list(difflib.unified_diff(body_o, body_n, "old", "new", lineterm="", n=2))
        print(f"  instruction stream: {len(body_o)} lines old, {len(body_n)} lines new: {'IDENTICAL' if not d else 'DIFFERENT'}")
        for ln in d:
            print("    " + ln)
        streams_same &= not d
        d = list(difflib.unified_diff(desc_o, desc_n, "old", "new", lineterm="", n=0))
        print(f"  descriptor: {'identical' if not d else 'differs'}")
        for ln in d:
            print("    " + ln)
        for side, meta in (("old", old_meta[o]), ("new", new_meta[n])):
            print(f"  {side}: kernarg {meta[0]} vgpr {meta[1]} sgpr {meta[2]} lds {meta[3]} scratch {meta[4]} args {len(meta[5])}")
        print()
    print(f"{'k_contrib<.., true>':24s} {'kernarg':>7s} {'vgpr':>4s} {'sgpr':>4s} {'lds':>6s} {'scratch':>7s} {'lines':>6s}")
    for n in sorted(new, key=lambda n: names[n]):
        m = re.search(r"k_contrib<(\d+), (\d+), true>", names[n])
        if m:
            t = new_meta[n]
            print(f"k_contrib<{m.group(1)}, {m.group(2)}, true>{'':5s} {t[0]:7d} {t[1]:4d} {t[2]:4d} {t[3]:6d} {t[4]:7d} {len(split(new[n])[0]):6d}")
    print()
    others_same = all(old.get(n) == t for n, t in new.items() if "k_contrib<" not in names[n])
    print(f"other kernels of the translation unit (k_contrib_merge, k_pc_gather): {'identical with their names' if others_same else 'DIFFERENT'}")
    ok = streams_same and pairs == 3 and others_same
    print("verdict:", "SAME instruction streams (3 unweighted k_contrib pairs)" if ok else "DIFFERENT (the lines above)")
    return 0 if ok else 1


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))

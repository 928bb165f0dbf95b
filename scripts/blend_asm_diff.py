#!/usr/bin/env python3
"""Is the device code of a translation unit (raster.hip, contrib.hip, ...) the same, kernel for kernel, in two trees?  (The check of
a kernel refactor: no GPU needed.)

  hipcc <the Makefile's COMMON flags> [-DWS_EXPERIMENTAL] --cuda-device-only -S csrc/raster.hip -o {old,new}.s
  python scripts/blend_asm_diff.py [--may-differ REGEX] old.s new.s > profiles/.../blend_asm_diff_<build>.txt

Per .amdhsa_kernel: the function body and its .amdhsa_* descriptor block, the kernel's own mangled name replaced by a
placeholder, the function index stripped from .LBB<n>_ / .Lfunc_end<n> labels, comment lines and trailing comments dropped.
Verdict SAME iff (1) the multisets of normalised kernels are equal, (2) the kernels that are not k_blend / k_blend_strict are equal
WITH their names, (3) the paired k_blend / k_blend_strict kernels agree in the metadata note: kernarg segment size, argument
offsets and sizes, VGPRs, SGPRs, LDS, scratch.  Prints the per-kernel resource table of the new file; exit status 1 unless SAME.
Kernels whose demangled name matches --may-differ are left out of the verdict and listed with their resources before and after."""
import collections
import hashlib
import re
import subprocess
import sys

META_KEYS = (".kernarg_segment_size", ".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def kernels(path):
    """{mangled name: normalised text}"""
    lines = open(path).read().split("\n")
    names = [ln.split()[1] for ln in lines if ln.strip().startswith(".amdhsa_kernel ")]
    start = {}
    for i, ln in enumerate(lines):
        m = re.match(r"^(\S+):\s", ln + " ")
        if m and m.group(1) in names and m.group(1) not in start:
            start[m.group(1)] = i
    out = {}
    for name in names:
        body = []
        for ln in lines[start[name]:]:
            ln = re.sub(r"\s*;.*$", "", ln).rstrip()  # (no string literal in the device code holds a ';')
            if ln.strip():
                body.append(re.sub(r"\.(LBB|Lfunc_end|Lfunc_begin)\d+", r".\1", ln.replace(name, "@K").replace(name[2:], "@k")))
            if ln.startswith(".Lfunc_end"):
                break
        out[name] = "\n".join(body)
    return out


def metadata(path):
    """{mangled name: (kernarg size, vgprs, sgprs, lds, scratch, ((offset, size) of every argument))}"""
    text = open(path).read()
    note = text[text.index("amdhsa.kernels:"):text.index(".end_amdgpu_metadata")]
    out = {}
    for entry in re.split(r"\n  - ", note)[1:]:
        if ".name:" not in entry:  # (amdhsa.version's list, behind the kernels)
            continue
        args = tuple((int(o), int(s)) for o, s in re.findall(r"\.offset:\s+(\d+)\n\s+\.size:\s+(\d+)", entry))
        vals = tuple(int(re.search(re.escape(k) + r":\s+(\d+)", entry).group(1)) for k in META_KEYS)
        out[re.search(r"\.name:\s+(\S+)", entry).group(1)] = vals + (args,)
    return out


def demangle(names):
    res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, res))


def is_blend(demangled):
    return re.search(r"\bk_blend(_strict)?<", demangled) is not None


def main(old_path, new_path, may_differ=None):
    old, new = kernels(old_path), kernels(new_path)
    old_meta, new_meta = metadata(old_path), metadata(new_path)
    names = demangle(sorted(set(old) | set(new)))
    problems = []
    if may_differ:  # before / after rows of the kernels the verdict leaves out; both sides must still have them
        print(f"left out of the verdict (--may-differ {may_differ!r}):")
        print(f"{'':6s} {'kernarg':>7s} {'vgpr':>4s} {'sgpr':>4s} {'lds':>6s} {'scratch':>7s} {'lines':>6s}  kernel")
        for n in sorted((n for n in set(old) | set(new) if re.search(may_differ, names[n])), key=lambda n: names[n]):
            for side, ks, meta in (("old", old, old_meta), ("new", new, new_meta)):
                if n in ks:
                    m = meta[n]
                    print(f"{side:6s} {m[0]:7d} {m[1]:4d} {m[2]:4d} {m[3]:6d} {m[4]:7d} {len(ks[n].splitlines()):6d}  {names[n]}"
                          f"{'  (body unchanged)' if side == 'new' and old.get(n) == ks[n] else ''}")
                else:
                    problems.append(f"missing in {side}: {names[n]}")
            old.pop(n, None)
            new.pop(n, None)
        print()
    digest = lambda t: hashlib.sha256(t.encode()).hexdigest()[:16]
    by_text_old = collections.defaultdict(list)
    for n, t in old.items():
        by_text_old[t].append(n)
    if collections.Counter(old.values()) != collections.Counter(new.values()):
        only_old = collections.Counter(old.values()) - collections.Counter(new.values())
        only_new = collections.Counter(new.values()) - collections.Counter(old.values())
        problems.append(f"multisets differ: {sum(only_old.values())} kernel(s) only in old, {sum(only_new.values())} only in new")
        for n, t in new.items():
            if t in only_new:
                problems.append(f"  only in new: {names[n]}")
        for n, t in old.items():
            if t in only_old:
                problems.append(f"  only in old: {names[n]}")
    for side, ks in (("old", old), ("new", new)):
        blend = [t for n, t in ks.items() if is_blend(names[n])]
        if len(set(blend)) != len(blend):
            problems.append(f"{side}: k_blend bodies are not pairwise distinct (the pairing is not one-to-one)")
    for n, t in new.items():
        if not is_blend(names[n]) and old.get(n) != t:
            problems.append(f"not equal with its name: {names[n]}")
    for n in old:
        if not is_blend(names[n]) and n not in new:
            problems.append(f"missing in new: {names[n]}")
    print(f"old: {old_path}: {len(old)} kernels, {sum(is_blend(names[n]) for n in old)} k_blend / k_blend_strict")
    print(f"new: {new_path}: {len(new)} kernels, {sum(is_blend(names[n]) for n in new)} k_blend / k_blend_strict")
    print()
    print(f"{'text sha256':16s} {'kernarg':>7s} {'vgpr':>4s} {'sgpr':>4s} {'lds':>6s} {'scratch':>7s} {'args':>4s}  kernel (new)  <-  kernel (old)")
    for n in sorted(new, key=lambda n: names[n]):
        m = new_meta[n]
        was = by_text_old.get(new[n], [])
        partner = n if n in was else (was[0] if was else None)
        if partner is not None and old_meta[partner] != m:
            problems.append(f"metadata differs: {names[n]}: {old_meta[partner]} -> {m}")
        arrow = "" if partner == n else f"  <-  {names[partner] if partner else '?'}"
        print(f"{digest(new[n])} {m[0]:7d} {m[1]:4d} {m[2]:4d} {m[3]:6d} {m[4]:7d} {len(m[5]):4d}  {names[n]}{arrow}")
    print()
    for p in problems:
        print("DIFFERENT:", p)
    print("verdict:", "DIFFERENT" if problems else "SAME (multiset of normalised kernels, named non-blend kernels, metadata of every pair)")
    return 1 if problems else 0


if __name__ == "__main__":
    args = sys.argv[1:]
    pattern = args[1] if len(args) == 4 and args[0] == "--may-differ" else None
    if len(args) != (4 if pattern else 2):
        sys.exit(__doc__)
    sys.exit(main(args[-2], args[-1], pattern))

"""Compare the kernels of two device-assembly files (refactor guard).

    hipcc <the Makefile's flags for the file> --cuda-device-only -S gibbs_sweep.hip -o old.s   # at the old commit
    hipcc <the same flags>                    --cuda-device-only -S gibbs_sweep.hip -o new.s   # at the new one
    python tools/kernel_diff.py old.s new.s

Kernels are matched by mangled name, so code that moved between translation units compares as well:
concatenate the .s files of the units on each side (cat gibbs_bdraw.s gibbs_bdraw_tiled.s gibbs_lnlike.s
gibbs_sweep.s > new.s for the b-draw family, each compiled with its own flags of the Makefile).

Each file is cut into kernels by mangled name: the text from the kernel's label to its .Lfunc_end
(the code, then the .amdhsa_kernel descriptor block, compared separately).  The function index in
local labels (.LBB<n>_, .Lfunc_end<n>, .Ltmp<n>) is normalised and the kernel's own name replaced, so a
body can also be compared with another kernel's.  Prints the kernels only in one file (for those that
left: a surviving or parent kernel with the same code and descriptor, if any), the kernels whose code or descriptor
changed, and the resource figures of the changed ones.  Exit status 1 if a common kernel changed.
CPU only; two compiles of the same source give no difference.
"""
import re
import sys

RES_KEYS = ("vgpr_count", "vgpr_spill_count", "sgpr_count", "sgpr_spill_count", "agpr_count",
            "group_segment_fixed_size", "private_segment_fixed_size")


def kernels(path):
    """{name: (code lines, descriptor lines)} and {name: {resource key: value}}"""
    lines = open(path).read().splitlines()
    names = {m.group(1) for ln in lines for m in [re.match(r"\s+\.amdhsa_kernel\s+(\S+)", ln)] if m}
    out, i = {}, 0
    while i < len(lines):
        m = re.match(r"(\S+):", lines[i])
        if not (m and m.group(1) in names):
            i += 1
            continue
        name, code, desc, in_desc = m.group(1), [], [], False
        i += 1
        while i < len(lines) and not re.match(r"\.Lfunc_end\d+:", lines[i]):
            ln = re.sub(r"\.(LBB|Lfunc_end|Ltmp)\d+", r".\1N", lines[i])
            ln = re.sub(r"\bBB\d+_", "BBN_", ln).replace(name, "SELF")  # (block names in loop comments)
            ln = re.sub(r"\s+", " ", ln)  # (the comments' column shifts with the index's width)
            in_desc = in_desc or ".amdhsa_kernel" in ln
            (desc if in_desc else code).append(ln)
            in_desc = in_desc and ".end_amdhsa_kernel" not in ln
            i += 1
        out[name] = (code, desc)
    res, cur = {}, None
    for ln in lines:
        m = re.match(r"\s+\.name:\s+(\S+)", ln)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        m = re.match(r"\s+\.(\w+):\s+(\d+)\s*$", ln)
        if m and cur is not None and m.group(1) in RES_KEYS:
            cur[m.group(1)] = int(m.group(2))
    return out, res


def main(old_path, new_path):
    old, old_res = kernels(old_path)
    new, new_res = kernels(new_path)
    print(f"kernels: {len(old)} -> {len(new)}")
    by_code = {}
    for n in sorted(old):
        by_code.setdefault("\n".join(old[n][0] + old[n][1]), []).append(n)
    for n in sorted(set(old) - set(new)):
        twins = [t for t in by_code["\n".join(old[n][0] + old[n][1])] if t != n]
        kept = [t for t in twins if t in new]
        print(f"  gone: {n}" + (f"  (same code and descriptor as {(kept or twins)[0]})" if twins else ""))
    for n in sorted(set(new) - set(old)):
        print(f"  new:  {n}")
    changed = 0
    for n in sorted(set(old) & set(new)):
        what = [w for w, k in (("code", 0), ("descriptor", 1)) if old[n][k] != new[n][k]]
        if what:
            changed += 1
            print(f"  CHANGED ({', '.join(what)}): {n}")
            for k in RES_KEYS:
                print(f"      {k}: {old_res.get(n, {}).get(k)} -> {new_res.get(n, {}).get(k)}")
    print(f"common kernels: {len(set(old) & set(new))}, changed: {changed}")
    return 1 if changed else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))

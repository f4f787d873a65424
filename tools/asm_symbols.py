#!/usr/bin/env python3
"""Compare device assembly per kernel symbol, for refactors that move kernels between files.

    python tools/asm_symbols.py PARENT_DIR BRANCH_DIR

Both directories hold ``<file>.hip.s`` as written by ``hipcc --cuda-device-only -S -fuse-cuid=none`` with the
flags of ``csrc/build.py``, run from inside ``csrc/`` (the method of ``profiles/shared_device_helpers.md``).
A file present on both sides is compared byte by byte.  Every other file is cut into its kernels: the text from a
kernel's label to the end of its resource summary (instructions, the ``.amdhsa_`` resource directives, LDS and
scratch sizes) plus the kernel's entry in the ``amdgpu_metadata`` note.  Local labels carry the function's position in its
file (``.LBB12_3``, ``.Lfunc_end12``, ``BB12_3`` in loop comments); that position is blanked and the padding in
front of a comment collapsed, nothing else.  Each kernel symbol of the files
that exist only in the parent must appear exactly once in the files that exist only in the branch, with equal text.
Exit status 1 on any difference.
"""
import os
import re
import sys

LOCAL = re.compile(r"(\.L)?(BB|func_end|func_begin|tmp|JTI)\d+")
PAD = re.compile(r"[ \t]+;")  # a label's comment is padded to a column, so the label's width moves it


def kernels(path):
    """{symbol: normalised text} of one assembly file."""
    lines = open(path).read().split("\n")
    names = [m.group(1) for ln in lines if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln))]
    out = {}
    for name in names:
        start = next(i for i, ln in enumerate(lines) if ln.startswith(name + ":"))
        end = next(i for i in range(start, len(lines)) if "-- End function" in lines[i])
        # ... and the resource summary behind it: ``.set <symbol>.num_vgpr`` and the ``; Kernel info`` comments
        while end + 1 < len(lines) and re.match(r"\s*(\.set\s|;|\.section\s+\.AMDGPU\.csdata)", lines[end + 1]):
            end += 1
        body = [PAD.sub(" ;", LOCAL.sub(lambda m: m.group(2), ln)) for ln in lines[start:end + 1]]
        meta = []
        for i, ln in enumerate(lines):
            if ln.strip() == f".name:           {name}" or ln.strip() == f".name: {name}":
                lo = max(j for j in range(i + 1) if lines[j].startswith("  - "))
                hi = next(j for j in range(i + 1, len(lines)) if lines[j].startswith("  - ") or not lines[j].startswith("   "))
                meta = lines[lo:hi]
        assert name not in out, f"{path}: {name} twice"
        out[name] = "\n".join(body + meta)
    return out


def main(parent, branch):
    pf, bf = sorted(os.listdir(parent)), sorted(os.listdir(branch))
    bad = 0
    for f in sorted(set(pf) & set(bf)):
        same = open(os.path.join(parent, f), "rb").read() == open(os.path.join(branch, f), "rb").read()
        bad += not same
        print(f"{f}: {'byte-identical' if same else 'DIFFERS'}")
    old, new, where = {}, {}, {}
    for f in sorted(set(pf) - set(bf)):
        old.update(kernels(os.path.join(parent, f)))
        print(f"{f} (parent only): {len(old)} kernels")
    for f in sorted(set(bf) - set(pf)):
        ks = kernels(os.path.join(branch, f))
        for k, v in ks.items():
            if k in new:
                print(f"DUPLICATE {k}: {where[k]} and {f}")
                bad += 1
            new[k], where[k] = v, f
        same = sum(1 for k in ks if old.get(k) == ks[k])
        lines = sum(v.count("\n") + 1 for v in ks.values())
        print(f"{f} (branch only): {len(ks)} kernels, {same} identical to the parent's, {lines} lines compared")
    for k in sorted(set(old) | set(new)):
        if k not in new:
            print(f"MISSING in branch: {k}")
        elif k not in old:
            print(f"NEW in branch: {k} ({where[k]})")
        elif old[k] != new[k]:
            print(f"DIFFERS: {k} ({where[k]}): {old[k].count(chr(10)) + 1} -> {new[k].count(chr(10)) + 1} lines")
        else:
            continue
        bad += 1
    print(f"{len(old)} parent kernels, {len(new)} branch kernels, {bad} problems")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))

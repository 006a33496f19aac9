#!/usr/bin/env python3
"""Instruction-identity check that follows a kernel from one file into another.

    tools/kernel_asm_diff.py PARENT_DIR CHANGE_DIR

Both directories hold the device assembly (`hipcc --cuda-device-only -S`) of every translation unit of one checkout.  Every
*.s is cut into functions by symbol: the function text, its .amdhsa_kernel block, its `.set <symbol>.num_vgpr` etc. lines, the
"Kernel info" comments and its entry of the code-object metadata.  What depends on the position in the file is normalised
(.LBB<n>_, .Lfunc_end<n>, .Ltmp<n>, the __hip_cuid_ lines), then symbol -> text is compared over the union of both sides.
Builds are told apart by the file name (x.s and x-DITTS_HALF_F16.s are different builds).  Exit status 0 = identical.
"""
import collections
import glob
import os
import re
import sys

BEGIN = re.compile(r"^\t\.globl\t(\S+)\s*; -- Begin function ")
TAIL = re.compile(r"^\s*;|^\t\.(size|set)\s|^\t\.section\t\.AMDGPU\.csdata")  # what follows .Lfunc_end and still belongs to the function
NORM = [(re.compile(r"BB\d+_"), "BB_"), (re.compile(r"\.Lfunc_end\d+"), ".Lfunc_end"), (re.compile(r"\.Ltmp\d+"), ".Ltmp"),
        (re.compile(r"\s+;"), " ;")]  # (a label's comment is padded to a column: the padding depends on the label's digits)
FIGURES = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def build_of(path):
    m = re.search(r"(-D\w+)\.s$", path)
    return m.group(1) if m else "bf16"


def functions(path):
    """{symbol: normalised text} of one assembly file."""
    lines = [ln for ln in open(path).read().split("\n") if "__hip_cuid_" not in ln]
    for pat, rep in NORM:
        lines = [pat.sub(rep, ln) for ln in lines]
    out, i, meta = {}, 0, {}
    if "amdhsa.kernels:" in lines:  # metadata entries: '  - ' starts one, '.name:' says whose
        j = lines.index("amdhsa.kernels:") + 1
        entry = []
        while j < len(lines) and lines[j].startswith("  "):
            if lines[j].startswith("  - ") and entry:
                meta[next(e.split()[-1] for e in entry if e.startswith("    .name:"))] = entry
                entry = []
            entry.append(lines[j])
            j += 1
        if entry:
            meta[next(e.split()[-1] for e in entry if e.startswith("    .name:"))] = entry
    while i < len(lines):
        m = BEGIN.match(lines[i])
        if not m:
            i += 1
            continue
        j, ended = i + 1, False
        while j < len(lines) and not BEGIN.match(lines[j]) and not (ended and not TAIL.match(lines[j])):
            ended = ended or lines[j].startswith(".Lfunc_end")
            j += 1
        body = [ln for ln in lines[i:j] if not ln.startswith("\t.section\t.text")]  # (the next function's section line names it)
        out[m.group(1)] = "\n".join(body + meta.get(m.group(1), []))
        i = j
    return out


def figures(text):
    f = {k: next((ln.split()[-1] for ln in text.split("\n") if ln.strip().startswith(k + ":")), "-") for k in FIGURES}
    n = sum(1 for ln in text.split("\n") if re.match(r"^\t[a-z]", ln))
    return "instr %d vgpr %s sgpr %s lds %s scratch %s" % ((n,) + tuple(f[k] for k in FIGURES))


def side(d):
    """{(build, symbol): [(file, text), ...]}"""
    fn = collections.defaultdict(list)
    for path in sorted(glob.glob(os.path.join(d, "*.s"))):
        for sym, text in functions(path).items():
            fn[(build_of(path), sym)].append((os.path.basename(path), text))
    return fn


def main(parent_dir, change_dir):
    a, b = side(parent_dir), side(change_dir)
    bad = 0
    for name, fn in (("parent", a), ("change", b)):
        for (bld, sym), defs in sorted(fn.items()):
            if len(defs) > 1 and ".amdhsa_kernel" in defs[0][1]:
                bad += 1
                print("TWICE in %s [%s] %s: %s" % (name, bld, sym, ", ".join(f for f, _ in defs)))
    for key in sorted(set(a) | set(b)):
        if key not in a or key not in b:
            bad += 1
            print("ONLY in %s [%s] %s (%s)" % ("parent" if key in a else "change", key[0], key[1], (a.get(key) or b.get(key))[0][0]))
        elif a[key][0][1] != b[key][0][1]:
            bad += 1
            print("DIFFERS [%s] %s\n  parent %s: %s\n  change %s: %s" % (key + (a[key][0][0], figures(a[key][0][1]), b[key][0][0], figures(b[key][0][1]))))
    for bld in sorted({k[0] for k in set(a) | set(b)}):
        kern = lambda fn: sum(1 for k, v in fn.items() if k[0] == bld and ".amdhsa_kernel" in v[0][1])
        moved = sum(1 for k in a if k[0] == bld and k in b and ".amdhsa_kernel" in a[k][0][1] and a[k][0][0] != b[k][0][0])
        print("[%s] kernels: parent %d, change %d; %d in another file than in the parent" % (bld, kern(a), kern(b), moved))
    print("IDENTICAL" if not bad else "%d findings" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))

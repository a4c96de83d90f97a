#!/usr/bin/env python
"""Compare the gfx950 device code of two checkouts kernel by kernel (no GPU needed).

  python tools/isa_diff.py OLD_TREE NEW_TREE [--opcodes] [--allow-removed REGEX] [--allow-added REGEX] [--show N]

Compiles every cc_amd/csrc/*.hip of both trees to assembly with the flags of cc_amd/build.py (tools/isa_scan.py compile_asm) and
matches the kernels by symbol name across files, so a kernel may move to another translation unit.  Two kernels are equal when
their instruction streams are equal -- comments stripped, local labels renumbered (a function's index in its file is part of
.LBB<n>_<m>) -- and all their .amdhsa_* descriptor values (registers, LDS, scratch, ...) are.  Exit status 0: every kernel present
on both sides is equal and the sets of kernels differ only by what the two REGEXes (matched against the demangled name) allow.

--opcodes: for a change that moves code between functions without changing it, after which the scheduler may order independent
instructions differently and name registers differently.  Two kernels are then equal when their .amdhsa_* values and the MULTISET
of their instruction mnemonics (labels and directives left out) are equal; every kernel is printed with both verdicts, so that the
strictly equal ones can be told from the merely opcode-equal ones."""
import argparse
import glob
import os
import re
import subprocess
import sys
import tempfile
from collections import Counter
from concurrent.futures import ThreadPoolExecutor

from isa_scan import FILT, compile_asm


def demangle_all(names):
    try:
        out = subprocess.run([FILT], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    except OSError:
        out = []
    return {n: (out[i] if i < len(out) and out[i] else n) for i, n in enumerate(names)}


def normalise(lines):
    out = []
    for ln in lines:
        ln = ln.split(";", 1)[0].strip()
        if not ln:
            continue
        out.append(re.sub(r"\.L([A-Za-z_]+?)\d+_(\d+)", r".L\1_\2", ln))
    return out


def opcodes(body):
    """normalised lines -> Counter of mnemonics"""
    return Counter(ln.split()[0] for ln in body if not ln.endswith(":") and not ln.startswith("."))


def kernels_of(asm_path):
    """-> {symbol: (instruction lines, {amdhsa directive: value})}"""
    lines = open(asm_path).read().split("\n")
    desc, cur = {}, None
    for ln in lines:
        t = ln.strip()
        if t.startswith(".amdhsa_kernel "):
            cur = t.split()[1]
            desc[cur] = {}
        elif t.startswith(".end_amdhsa_kernel"):
            cur = None
        elif cur is not None and t.startswith(".amdhsa_"):
            k, _, v = t.partition(" ")
            desc[cur][k] = v.strip()
    body, cur = {}, None
    for ln in lines:
        m = re.match(r"^([A-Za-z_$][\w$.]*):", ln)
        if m and m.group(1) in desc and cur is None:
            cur = m.group(1)
            body[cur] = []
        elif cur is not None:
            if ln.startswith(".Lfunc_end"):
                cur = None
            else:
                body[cur].append(ln)
    return {k: (normalise(body.get(k, [])), desc[k]) for k in desc}


def tree_kernels(tree, tmp, tag):
    files = sorted(glob.glob(os.path.join(tree, "cc_amd", "csrc", "*.hip")))
    if not files:
        sys.exit("%s: no cc_amd/csrc/*.hip" % tree)

    def one(f):
        out = os.path.join(tmp, "%s_%s.s" % (tag, os.path.basename(f)))
        r = compile_asm(f, out, tree)
        if r.returncode != 0:
            sys.exit("%s: hipcc failed\n%s" % (f, r.stderr[-2000:]))
        return os.path.basename(f), kernels_of(out)

    with ThreadPoolExecutor(max_workers=8) as ex:
        per_file = list(ex.map(one, files))
    ks = {}
    for fname, d in per_file:
        for name, v in d.items():
            ks.setdefault(name, []).append((fname, v))      # (file-local kernels of two files may share a name)
    return ks


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old_tree")
    ap.add_argument("new_tree")
    ap.add_argument("--allow-removed", default=None, help="kernels (demangled name, regex) that may be missing from NEW_TREE")
    ap.add_argument("--allow-added", default=None, help="kernels (demangled name, regex) that may be new in NEW_TREE")
    ap.add_argument("--opcodes", action="store_true", help="equal = same descriptors and same multiset of mnemonics; print both verdicts")
    ap.add_argument("--show", type=int, default=20, help="differing lines printed per kernel")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        old = tree_kernels(a.old_tree, tmp, "old")
        new = tree_kernels(a.new_tree, tmp, "new")
    names = demangle_all(sorted(set(old) | set(new)))
    bad = 0
    moved = 0
    for k in sorted(set(old) | set(new)):
        o, n = old.get(k, []), new.get(k, [])
        if len(o) != len(n):
            gone = len(o) > len(n)
            pat = a.allow_removed if gone else a.allow_added
            ok = pat is not None and re.search(pat, names[k]) is not None
            print("%s %-9s %s  (%s)" % ("ok  " if ok else "DIFF", "removed" if gone else "added", names[k],
                                         ", ".join(f for f, _ in (o if gone else n))))
            bad += 0 if ok else 1
            continue
        # same-named kernels of several files: compare in the order of their code
        o = sorted(o, key=lambda fv: fv[1][0])
        n = sorted(n, key=lambda fv: fv[1][0])
        for (fo, (bo, do)), (fn, (bn, dn)) in zip(o, n):
            moved += fo != fn
            strict = bo == bn and do == dn
            if a.opcodes:
                loose = do == dn and opcodes(bo) == opcodes(bn)
                print("%s strict %-5s opcodes %-5s %s  (%s)" % ("ok  " if loose else "DIFF", "equal" if strict else "DIFF",
                                                               "equal" if loose else "DIFF", names[k], fn))
                if loose:
                    continue
                d = opcodes(bn)
                d.subtract(opcodes(bo))
                print("       opcodes new - old: %s" % {m: c for m, c in sorted(d.items()) if c})
            elif strict:
                continue
            bad += 1
            print("DIFF kernel    %s  (%s -> %s)" % (names[k], fo, fn))
            for key in sorted(set(do) | set(dn)):
                if do.get(key) != dn.get(key):
                    print("       %s: %s -> %s" % (key, do.get(key), dn.get(key)))
            if bo != bn:
                print("       instructions: %d -> %d lines" % (len(bo), len(bn)))
                shown = 0
                for i in range(max(len(bo), len(bn))):
                    x, y = (bo[i] if i < len(bo) else None), (bn[i] if i < len(bn) else None)
                    if x != y and shown < a.show:
                        print("       @%d  - %s\n            + %s" % (i, x, y))
                        shown += 1
    print("%d kernels in OLD, %d in NEW, %d in another file, %d difference(s)" %
          (sum(map(len, old.values())), sum(map(len, new.values())), moved, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

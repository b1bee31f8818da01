#!/usr/bin/env python3
"""Prove that two versions of dino-x_amd/csrc hold the same device code.

    python tools/device_asm_diff.py --rev HEAD~1          # that commit against the working tree
    python tools/device_asm_diff.py OLD_CSRC NEW_CSRC     # two csrc directories (each next to its ../../include)

Every .hip of both trees is compiled to device assembly with the Makefile's own flags (CXXFLAGS and the per-file
FLAGS_<name>) plus `--cuda-device-only -S`; no GPU is needed.  Each output is split at its function symbols and
compared symbol by symbol: everything from `.type <sym>,@function` to `.size <sym>`, which is the instruction
text and, for a kernel, its .amdhsa_kernel descriptor.  Two things are normalised because they are not code: the
`__hip_cuid_<hash>` and `.ident` lines (they differ between two compilations of the same file) and the function
ordinal in local labels (`.LBB<n>_<m>`, `.Lfunc_end<n>`, `Header=BB<n>_<m>` in comments), which follows the order
in which host code instantiates the templates.  Exit status 0 iff the symbol sets are equal and every symbol is
identical.  (--keep DIR stores the .s files; --reuse compares what an earlier --keep left there.)"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("dino-x_amd", "csrc")


def make_flags(csrc: str) -> tuple[list[str], dict[str, list[str]]]:
    """CXXFLAGS and the FLAGS_<file> overrides, read from the tree's own Makefile."""
    text = open(os.path.join(csrc, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    cxx = re.search(r"^CXXFLAGS\s*=\s*(.*)$", text, re.M).group(1).replace("$(ARCH)", arch).split()
    per = {m.group(1): m.group(2).split() for m in re.finditer(r"^FLAGS_(\w+)\s*=\s*(.*)$", text, re.M)}
    return cxx, per


def emit(csrc: str, out: str, jobs: int) -> dict[str, str]:
    cxx, per = make_flags(csrc)
    os.makedirs(out, exist_ok=True)
    srcs = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))

    def one(f: str) -> tuple[str, str]:
        stem = f[:-4]
        dst = os.path.join(out, stem + ".s")
        cmd = [os.environ.get("HIPCC", "hipcc"), *cxx, *per.get(stem, []), "--cuda-device-only", "-S", f, "-o", os.path.abspath(dst)]
        subprocess.run(cmd, cwd=csrc, check=True)
        return stem, open(dst).read()

    with cf.ThreadPoolExecutor(jobs) as ex:
        return dict(ex.map(one, srcs))


_DROP = re.compile(r"__hip_cuid_|^\s*\.ident\b")
_LOCAL = re.compile(r"(?<!\w)(\.LBB|\.Lfunc_begin|\.Lfunc_end|\.LJTI|\.Ltmp|BB)\d+(?=_|\b)")


def split(asm: str) -> dict[str, str]:
    """function symbol -> its normalised text (a kernel's text holds its .amdhsa_kernel descriptor)."""
    out: dict[str, str] = {}
    lines = [ln for ln in asm.splitlines() if not _DROP.search(ln)]
    i = 0
    while i < len(lines):
        ln = lines[i].strip()
        m = re.match(r"\.type\s+([^,\s]+),@function", ln)
        if m:
            sym = m.group(1)
            end = re.compile(r"\.size\s+" + re.escape(sym) + r"\s*,")
            j = i
            while j < len(lines) and not end.match(lines[j].strip()):
                j += 1
            assert j < len(lines), f"unterminated {sym}"
            assert sym not in out, sym
            out[sym] = "\n".join(_LOCAL.sub(lambda x: x.group(1), s) for s in lines[i:j + 1])
            i = j + 1
        else:
            i += 1
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("dirs", nargs="*", help="OLD_CSRC NEW_CSRC")
    ap.add_argument("--rev", help="compare this git revision's csrc against the working tree's")
    ap.add_argument("-j", "--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--keep", help="write the .s files under this directory (old/, new/) instead of a temporary one")
    ap.add_argument("--reuse", action="store_true", help="do not compile: compare the .s files already under --keep")
    a = ap.parse_args()

    def load(d: str) -> dict[str, str]:
        return {f[:-2]: open(os.path.join(d, f)).read() for f in sorted(os.listdir(d)) if f.endswith(".s")}

    with tempfile.TemporaryDirectory() as tmp:
        if a.reuse and a.keep:
            asm_old, asm_new = load(os.path.join(a.keep, "old")), load(os.path.join(a.keep, "new"))
        elif a.rev:
            tar = subprocess.run(["git", "-C", ROOT, "archive", a.rev, CSRC, "include"], check=True, stdout=subprocess.PIPE).stdout
            subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
            old, new = os.path.join(tmp, CSRC), os.path.join(ROOT, CSRC)
        elif len(a.dirs) == 2:
            old, new = a.dirs
        else:
            ap.error("give --rev REV or two csrc directories")
        if not a.reuse:
            work = a.keep or os.path.join(tmp, "asm")
            asm_old, asm_new = emit(old, os.path.join(work, "old"), a.jobs), emit(new, os.path.join(work, "new"), a.jobs)
    bad = n_fn = n_kd = 0
    for stem in sorted(set(asm_old) | set(asm_new)):
        so, sn = split(asm_old.get(stem, "")), split(asm_new.get(stem, ""))
        gone, added = sorted(set(so) - set(sn)), sorted(set(sn) - set(so))
        diff = sorted(s for s in set(so) & set(sn) if so[s] != sn[s])
        kd = sum(".amdhsa_kernel" in t for t in sn.values())
        n_fn += len(sn)
        n_kd += kd
        state = "identical" if not (gone or added or diff) else "DIFFERS"
        print(f"{stem:24s} {kd:4d} kernels {len(sn) - kd:4d} other device functions  {state}")
        for tag, syms in (("only in old", gone), ("only in new", added), ("text differs", diff)):
            for s in syms:
                print(f"    {tag}: {s}")
        bad += len(gone) + len(added) + len(diff)
    print(f"total: {len(asm_new)} files, {n_kd} kernels, {n_fn - n_kd} other device functions, {bad} differing symbols")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

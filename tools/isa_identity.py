#!/usr/bin/env python
"""isa_identity.py -- is the device code of this tree the device code of another commit?  The gate of a refactor of the kernels.

    python tools/isa_identity.py PARENT_REV [--out FILE] [--keep DIR]

Compiles every kernel source of PARENT_REV (git archive into a temporary directory) and of the working tree with the Makefile's flags and
-save-temps, and compares per kernel symbol
  * the instruction stream as isa_census.parse_kernel reads it: mnemonics and operands; comments and directives are not in it, and the
    function number inside .LBB<n>_<m> labels is dropped;
  * the kernel descriptor's resource fields (FIELDS).
One line per kernel: `same`, or the fields and instruction counts that differ, with the scratch instructions inside loops (what
tests/test_isa_census.py asserts to be none for the two hot kernels).  A kernel whose mangled name exists on one side only (its signature
changed) is paired by its unmangled name and template arguments.  Exit status 1 if a kernel is missing on either side.
"""
import argparse
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_census as IC  # noqa: E402
from isa_profile import FLAGS  # noqa: E402

PKG_CSRC = os.path.relpath(IC.CSRC, IC.ROOT)
FIELDS = ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size", "accum_offset")


def build(csrc, work):
    """-> the device assembly files of every *.hip of csrc"""
    shutil.rmtree(work, ignore_errors=True)
    os.makedirs(work)
    out = []
    for src in sorted(glob.glob(os.path.join(csrc, "*.hip"))):
        stem = os.path.basename(src)[:-4]
        subprocess.check_call(["/opt/rocm/bin/hipcc"] + FLAGS + ["-save-temps", "-c", src, "-o", os.path.join(work, stem + ".o")], cwd=work,
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        out.append(os.path.join(work, stem + "-hip-amdgcn-amd-amdhsa-gfx950.s"))
    return out


def kernels_of(asm_files):
    """{mangled name: {"insns": [(mnemonic, operands)], "fields": {..}, "loop_scratch": n}}"""
    res = {}
    for asm in asm_files:
        text = open(asm).read()
        for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", text, re.M | re.S):
            name, desc = m.group(1), m.group(2)
            found, blocks = IC.parse_kernel(asm, name)
            assert found == name, (found, name)
            cen, _ = IC.census(blocks)
            res[name] = {"insns": [(mn, re.sub(r"\.LBB\d+_", ".LBB_", ops)) for b in blocks for mn, ops, _, _ in b["insns"]],
                         "fields": {f: int(re.search(r"\.amdhsa_%s\s+(\d+)" % f, desc).group(1)) for f in FIELDS},
                         "loop_scratch": sum(b["classes"].get("scratch", 0) for b in cen if b["depth"] > 0)}
    return res


def base_name(mangled):
    """_ZN4csky23frame_setup_taps_kernelILi0EEEv... -> frame_setup_taps_kernel<0>: enough to pair a kernel across a change of its parameters.
    Template arguments may be integers, class names of the namespace and bools; a trailing `true` is dropped, so that a kernel that gained a
    bool parameter pairs its <..., true> instantiation with the parent's kernel (<..., false> has no counterpart there); trailing `0`s likewise, for a
    kernel that gained an integer parameter whose 0 is the form the parent had."""
    m = re.match(r"_ZN4csky(\d+)", mangled)
    n = int(m.group(1))
    name, rest = mangled[m.end():m.end() + n], mangled[m.end() + n:]
    args = []
    if rest.startswith("I"):
        rest = rest[1:]
        while not rest.startswith("E"):
            t = re.match(r"Li(\d+)E", rest) or re.match(r"Lb([01])E", rest)
            if t:
                args.append(t.group(1) if rest[1] == "i" else ("false", "true")[int(t.group(1))])
                rest = rest[t.end():]
                continue
            t = re.match(r"NS_(\d+)", rest)
            if not t:
                return name
            k = int(t.group(1))
            args.append(rest[t.end():t.end() + k])
            rest = rest[t.end() + k + 1:]                      # the name and the E that closes the nested name
    while args and args[-1] in ("true", "0"):
        args.pop()
    return name + ("<%s>" % ",".join(args) if args else "")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("--out", default=None)
    ap.add_argument("--keep", default=None, help="keep the two builds in this directory")
    a = ap.parse_args()
    work = a.keep or tempfile.mkdtemp(prefix="isa_identity_")
    shutil.rmtree(os.path.join(work, "parent_src"), ignore_errors=True)
    os.makedirs(os.path.join(work, "parent_src"))
    rev = subprocess.check_output(["git", "rev-parse", a.parent], cwd=IC.ROOT, text=True).strip()
    tar = subprocess.Popen(["git", "archive", rev, PKG_CSRC, "include"], cwd=IC.ROOT, stdout=subprocess.PIPE)
    subprocess.check_call(["tar", "-x", "-C", os.path.join(work, "parent_src")], stdin=tar.stdout)
    old = kernels_of(build(os.path.join(work, "parent_src", PKG_CSRC), os.path.join(work, "parent")))
    new = kernels_of(build(IC.CSRC, os.path.join(work, "change")))
    compiler = subprocess.check_output(["/opt/rocm/bin/hipcc", "--version"], text=True).splitlines()
    lines = ["parent   %s" % rev, "compiler %s" % "; ".join(compiler[:2]), "flags    %s" % " ".join(FLAGS), ""]
    renamed = {base_name(k): k for k in old if k not in new}
    missing = 0
    for name in sorted(new):
        o = old.get(name)
        tag = ""
        if o is None and base_name(name) in renamed:
            o = old[renamed.pop(base_name(name))]
            tag = "  (paired by unmangled name: the signature changed)"
        if o is None:
            lines.append("%-110s NOT IN THE PARENT" % name); missing += 1
            continue
        n = new[name]
        diff = ["%s %d -> %d" % (f, o["fields"][f], n["fields"][f]) for f in FIELDS if o["fields"][f] != n["fields"][f]]
        if o["insns"] != n["insns"]:
            common = sum(1 for x, y in zip(o["insns"], n["insns"]) if x == y)
            diff.append("instructions %d -> %d (%d equal in place), scratch in loops %d -> %d" % (len(o["insns"]), len(n["insns"]), common, o["loop_scratch"], n["loop_scratch"]))
        lines.append("%-110s %s%s" % (name, "; ".join(diff) or "same", tag))
    for b, k in sorted(renamed.items()):
        lines.append("%-110s NOT IN THE CHANGE" % k); missing += 1
    same = sum(1 for ln in lines if ln.rstrip().endswith("same") or " same  (" in ln)
    lines += ["", "%d kernels, %d same, %d missing on one side" % (len(new), same, missing)]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        open(a.out, "w").write(text)
    if not a.keep:
        shutil.rmtree(work, ignore_errors=True)
    return 1 if missing else 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Device code of two builds, kernel by kernel: the gfx950 code object of every translation unit is unbundled (as tools/kregs.py does),
disassembled and compared.  A refactor that moves no arithmetic should pass all four checks for every kernel:
  symbols   the set of kernel symbols of the two builds is the same
  multiset  the sorted instruction lines are the same
  order     the ordered listing is the same once scalar instructions are dropped (mnemonics beginning s_; s_waitcnt* and s_barrier stay)
  regs      vgpr / agpr / sgpr / spill / scratch / static LDS of the code object's metadata are the same
usage: isa_diff.py PARENT_BUILD CHILD_BUILD [UNIT.o ...]      (directories of *.o, e.g. csrc/build; exit status 1 when anything differs)"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


def run(*cmd):
    return subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout.decode()


def code_object(obj, tmp):
    fat, co = os.path.join(tmp, "fat"), os.path.join(tmp, "co")
    run(f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", obj, os.path.join(tmp, "x"))
    run(f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}", f"--output={co}",
        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950")
    return co


def kernels(obj):
    """{kernel symbol: (instruction lines, register figures)} of one object file; {} for a unit without device code"""
    with tempfile.TemporaryDirectory() as tmp:
        try:
            co = code_object(obj, tmp)
        except subprocess.CalledProcessError:
            return {}
        notes = run(f"{LLVM}/llvm-readelf", "--notes", co)
        asm = run(f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co)
    regs = {}
    for blk in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
        get = lambda k: (re.search(rf"\.{k}:\s+(\S+)", blk) or [None, "?"])[1]
        regs[get("name").strip("'\"")] = (get("vgpr_count"), (re.match(r"\s*(\d+)", blk) or [None, "?"])[1], get("sgpr_count"),
                                          get("vgpr_spill_count"), get("private_segment_fixed_size"), get("group_segment_fixed_size"))
    body, cur = {}, None
    for line in asm.split("\n"):
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = m.group(1)
            body.setdefault(cur, [])
        elif cur is not None and line.startswith("\t"):
            body[cur].append(re.sub(r"\s*//.*$", "", line).strip())
    return {k: (body.get(k, []), r) for k, r in regs.items()}


def vector_part(lines):
    keep = []
    for ln in lines:
        op = ln.split()[0] if ln else ""
        if op.startswith("s_") and not (op.startswith("s_waitcnt") or op == "s_barrier"):
            continue
        keep.append(ln)
    return keep


def main():
    parent, child = sys.argv[1:3]
    only = set(sys.argv[3:])                  # (while working on one file: isa_diff.py A B level_bwd3.o)
    units = sorted(f for f in os.listdir(parent) if f.endswith(".o") and (not only or f in only))
    theirs = sorted(f for f in os.listdir(child) if f.endswith(".o") and (not only or f in only))
    bad = 0
    if units != theirs:
        print(f"translation units differ: {sorted(set(units) ^ set(theirs))}")
        bad += 1
    total = 0
    for u in units:
        if u not in theirs:
            continue
        a, b = kernels(os.path.join(parent, u)), kernels(os.path.join(child, u))
        if set(a) != set(b):
            print(f"{u}: symbols   differ: {sorted(set(a) ^ set(b))}")
            bad += 1
        miss = {"multiset": 0, "order": 0, "regs": 0}
        for k in sorted(set(a) & set(b)):
            total += 1
            fails = []
            if sorted(a[k][0]) != sorted(b[k][0]):
                fails.append("multiset")
            if vector_part(a[k][0]) != vector_part(b[k][0]):
                fails.append("order")
            if a[k][1] != b[k][1]:
                fails.append(f"regs {a[k][1]} -> {b[k][1]}")
            for f in fails:
                miss[f.split()[0]] += 1
            if fails:
                name = run("c++filt", k).strip()
                print(f"{u}: {', '.join(fails)}: {re.sub(r'[(].*$', '', name)[:150]}  [{len(a[k][0])} -> {len(b[k][0])} lines]")
                bad += 1
        print(f"{u:28s} {len(set(a) & set(b)):4d} kernels   multiset {miss['multiset']}  order {miss['order']}  regs {miss['regs']} differ")
    print(f"{total} kernels compared, none skipped; {bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

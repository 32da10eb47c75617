#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of csrc/, kernel by kernel.

usage: compare_code_objects.py OLD_CSRC_DIR NEW_CSRC_DIR

For every *.o of each directory the gfx950 code object is extracted (llvm-objcopy, clang-offload-bundler) and every kernel
symbol is reduced to (instruction text + encoding words with the address column and the trailing padding dropped, .vgpr_count, .sgpr_count,
.group_segment_fixed_size, .private_segment_fixed_size).  Prints the kernel count per object, the kernels only one side has and
those that differ.  Exit status 0 when every kernel both sides have is identical.  A throw-away tool for refactors that must not
change device code; not a test.
"""
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
META = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def run(*a):
    return subprocess.run(a, check=True, capture_output=True, text=True).stdout


def kernels_of(obj, tmp):
    base = os.path.join(tmp, os.path.basename(obj))
    fat, co = base + ".fatbin", base + ".co"
    run(f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat)
    if not os.path.exists(fat) or os.path.getsize(fat) == 0:
        return {}
    run(f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={fat}", f"--output={co}")
    # metadata: one YAML map per kernel under amdhsa.kernels
    # (a kernel's entry opens with "  - .key:", its own keys sit at four spaces, the argument lists deeper)
    meta, cur = {}, None
    for line in run(f"{LLVM}/llvm-readelf", "--notes", co).split("\n"):
        m = re.match(r"^(  - |    )(\.[a-z_]+):\s*(.*)$", line)
        if not m:
            continue
        k, v = m.group(2), m.group(3).strip().strip("'\"")
        if m.group(1) == "  - ":
            cur = {}
        if cur is None:
            continue
        if k in META:
            cur[k] = v
        if k == ".symbol":
            meta[v[:-3] if v.endswith(".kd") else v] = cur
    # disassembly: symbol -> instruction lines without their address
    code, sym = {}, None
    for line in run(f"{LLVM}/llvm-objdump", "-d", co).split("\n"):
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            sym = m.group(1)
            code[sym] = []
            continue
        if sym is None or not line.strip():
            continue
        code[sym].append(re.sub(r"//\s*[0-9A-Fa-f]+:", "//", line).strip())
    out = {}
    for s, md in meta.items():
        body = code.get(s, [])
        # the padding behind a function's last instruction (up to the next symbol or the section's end) is not part of it
        while body and re.match(r"^(s_nop 0\s|s_code_end\s|\.\.\.$)", body[-1]):
            body.pop()
        out[s] = ("\n".join(body), tuple(md.get(k) for k in META))
    return out


def load(d, tmp):
    per_obj, allk = {}, {}
    for obj in sorted(glob.glob(os.path.join(d, "*.o"))):
        sub = os.path.join(tmp, str(len(per_obj)))
        os.makedirs(sub)
        ks = kernels_of(obj, sub)
        per_obj[os.path.basename(obj)] = ks
        for s, v in ks.items():
            assert s not in allk, f"{s} defined twice"
            allk[s] = (os.path.basename(obj), v)
    return per_obj, allk


def demangle(names):
    filt = shutil.which("llvm-cxxfilt", path=LLVM) or shutil.which("c++filt")
    if not names or not filt:
        return {n: n for n in names}
    out = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, out))


def main():
    old_dir, new_dir = sys.argv[1], sys.argv[2]
    with tempfile.TemporaryDirectory() as t:
        os.makedirs(t + "/a"), os.makedirs(t + "/b")
        po, ko = load(old_dir, t + "/a")
        pn, kn = load(new_dir, t + "/b")
    for tag, per in (("old", po), ("new", pn)):
        print(f"{tag}: " + ", ".join(f"{o} {len(k)}" for o, k in per.items()) + f"  (total {sum(len(k) for k in per.values())})")
    only_old, only_new = sorted(set(ko) - set(kn)), sorted(set(kn) - set(ko))
    dm = demangle(only_old + only_new + sorted(set(ko) & set(kn)))
    for s in only_old:
        print(f"only old ({ko[s][0]}): {dm[s]}")
    for s in only_new:
        print(f"only new ({kn[s][0]}): {dm[s]}")
    same = diff = empty = 0
    for s in sorted(set(ko) & set(kn)):
        (oo, (ct, mt)), (no, (cn, mn)) = ko[s], kn[s]
        if not ct or None in mt:
            empty += 1
            print(f"UNPARSED {dm[s]}")
        if ct == cn and mt == mn:
            same += 1
        else:
            diff += 1
            print(f"DIFFERENT {dm[s]}  {oo} -> {no}: " + ", ".join(f"{k} {a} -> {b}" for k, a, b in zip(META, mt, mn))
                  + ("" if ct != cn else "  (same instructions)"))
    print(f"identical kernels: {same}   different: {diff}   only old: {len(only_old)}   only new: {len(only_new)}")
    return 1 if diff or empty else 0


if __name__ == "__main__":
    sys.exit(main())

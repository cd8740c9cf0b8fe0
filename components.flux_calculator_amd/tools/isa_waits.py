#!/usr/bin/env python3
"""Vector-memory waits and sub-dword vector loads of the gfx950 kernels of fcx_kernels.hip.

  python tools/isa_waits.py [filter]                 the built lib/libfcx.so, disassembled
  python tools/isa_waits.py --lib PATH [filter]      another build of the library
  python tools/isa_waits.py --compile [-D...] [filter]   csrc/fcx_kernels.hip compiled to assembly
                                                     with the Makefile's flags (plus any -D given)
  python tools/isa_waits.py --asm FILE.s [filter]    an assembly file from such a compile
  python tools/isa_waits.py --same LIB_A LIB_B       two builds compared instruction for instruction:
                                                     the kernels only in one, the kernels that differ
                                                     with their first differing line; exit status 1
                                                     unless the two hold the same code

Per kernel: the instructions, the sub-dword vector loads (a byte or short member of the
parameter block read through the vector-memory pipeline: a round trip and a wait, where an
aligned word is a scalar load), the `s_waitcnt` instructions that wait for vmcnt(0), and the
flux passes.  A flux pass is a run of at least MIN_STORES 16-B vector stores with no vector
load between them: a single-type (TM = 1) kernel requests every input of the type before its
first flux store, and what follows the pass (the averages, the atmosphere cells of the
compacted map) begins with a load.  One pass per inlined variant body (the group kernel has
three); the kernels of separate u and v grids have one per grid.  For each pass: its 16-B
stores and the vector-memory waits (any s_waitcnt with a vmcnt field) between its first and
its last store -- each of those also waits for the stores of the flux blocks before it.
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
LLVM = "/opt/rocm/lib/llvm/bin"
HIPCC = "/opt/rocm/bin/hipcc"
MAKE_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wno-unused-function",
              "-I" + os.path.join(PKG, "csrc"), "-I" + os.path.join(PKG, "..", "include")]
MIN_STORES = 5

SUBDWORD = re.compile(r"^(global|flat|buffer|scratch)_load_[us](byte|short)")
VLOAD = re.compile(r"^(global|flat|buffer)_load_")
STORE16 = re.compile(r"^(global|flat)_store_dwordx4\b")
VMWAIT = re.compile(r"^s_waitcnt\b.*\bvmcnt\(\d+\)")
VMWAIT0 = re.compile(r"^s_waitcnt\b.*\bvmcnt\(0\)")


def tool(name):
    p = os.path.join(LLVM, name)
    return p if os.path.exists(p) else shutil.which(name)


def have_disassembler():
    return tool("llvm-objdump") is not None


def demangle(names):
    filt = tool("llvm-cxxfilt") or shutil.which("c++filt")
    if not filt or not names:
        return {n: n for n in names}
    out = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return dict(zip(names, out))


def disassemble(lib):
    """{mangled kernel or function name: [instruction text]} of the gfx950 code objects of a library"""
    with tempfile.TemporaryDirectory() as tmp:
        copy = os.path.join(tmp, os.path.basename(lib))
        shutil.copy(lib, copy)  # (the bundles are extracted beside the file)
        subprocess.run([tool("llvm-objdump"), "--offloading", copy], capture_output=True, text=True, check=True)
        funcs = {}
        for f in sorted(os.listdir(tmp)):
            if "amdgcn" not in f:
                continue
            text = subprocess.run([tool("llvm-objdump"), "-d", "--no-show-raw-insn", os.path.join(tmp, f)],
                                  capture_output=True, text=True, check=True).stdout
            cur = None
            for line in text.splitlines():
                m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
                if m:
                    cur = funcs.setdefault(m.group(1), [])
                    continue
                if cur is not None and line.startswith((" ", "\t")):
                    ins = line.split("//")[0].strip()
                    if ins:
                        cur.append(ins)
        return funcs


def parse_asm(path):
    """the same from a compiler assembly file (-S)"""
    funcs, cur = {}, None
    for line in open(path):
        m = re.match(r"^([A-Za-z_][\w$.]*):", line)
        if m and not m.group(1).startswith(".L"):
            cur = funcs.setdefault(m.group(1), [])
            continue
        if re.match(r"^\.Lfunc_end\d+:", line):
            cur = None
            continue
        if cur is not None and line.startswith("\t") and not line.lstrip().startswith((".", ";")):
            ins = line.split(";")[0].strip()
            if ins:
                cur.append(ins)
    return {k: v for k, v in funcs.items() if v}


def compile_asm(defines):
    out = os.path.join(tempfile.mkdtemp(), "fcx_kernels.s")
    subprocess.run([HIPCC] + MAKE_FLAGS + defines + ["--cuda-device-only", "-S", os.path.join(PKG, "csrc", "fcx_kernels.hip"),
                                                     "-o", out], check=True)
    return out


def analyse(ins):
    passes, run = [], []

    def close():
        if len(run) >= MIN_STORES:
            passes.append({"stores": len(run), "vm_waits": sum(1 for x in ins[run[0]:run[-1]] if VMWAIT.match(x))})
        del run[:]

    for i, x in enumerate(ins):
        if VLOAD.match(x):
            close()
        elif STORE16.match(x):
            run.append(i)
    close()
    return {"instructions": len(ins), "subdword_loads": sum(1 for x in ins if SUBDWORD.match(x)),
            "vmcnt0_waits": sum(1 for x in ins if VMWAIT0.match(x)), "flux_passes": passes}


def report(funcs, flt=""):
    names = demangle(sorted(funcs))
    rows = {}
    for mangled, ins in funcs.items():
        name = names[mangled]
        if name.startswith("void "):
            name = name[5:]
        name = name.split("(")[0]
        if flt in name:
            rows[name] = analyse(ins)
    return rows


def same(funcs_a, funcs_b):
    """two {kernel: [instructions]} compared: (names only in A, names only in B, {name of a kernel
    whose lists differ: (index, instruction of A, instruction of B) of the first differing line,
    None standing for the end of the shorter list})"""
    only_a = sorted(set(funcs_a) - set(funcs_b))
    only_b = sorted(set(funcs_b) - set(funcs_a))
    differ = {}
    for name in sorted(set(funcs_a) & set(funcs_b)):
        a, b = funcs_a[name], funcs_b[name]
        if a == b:
            continue
        i = next((k for k, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        differ[name] = (i, a[i] if i < len(a) else None, b[i] if i < len(b) else None)
    return only_a, only_b, differ


def main_same(lib_a, lib_b):
    fa, fb = disassemble(lib_a), disassemble(lib_b)
    only_a, only_b, differ = same(fa, fb)
    names = demangle(sorted(set(fa) | set(fb)))
    print(f"A: {lib_a}: {len(fa)} functions, {sum(map(len, fa.values()))} instructions")
    print(f"B: {lib_b}: {len(fb)} functions, {sum(map(len, fb.values()))} instructions")
    for title, only in (("only in A", only_a), ("only in B", only_b)):
        print(f"{title}: {len(only)}")
        for n in only:
            print(f"    {names[n]}")
    print(f"differ: {len(differ)}")
    for n, (i, x, y) in differ.items():
        print(f"    {names[n]}\n        instruction {i}: A: {x}\n        {'':>{len(str(i)) + 13}}B: {y}")
    ok = not (only_a or only_b or differ)
    print("same: " + ("yes" if ok else "NO"))
    return 0 if ok else 1


def main(argv):
    if argv and argv[0] == "--same":
        if len(argv) != 3:
            sys.exit("usage: isa_waits.py --same LIB_A LIB_B")
        sys.exit(main_same(argv[1], argv[2]))
    args, defines, src = list(argv), [], ("lib", os.path.join(PKG, "lib", "libfcx.so"))
    flt = ""
    while args:
        a = args.pop(0)
        if a == "--lib":
            src = ("lib", args.pop(0))
        elif a == "--asm":
            src = ("asm", args.pop(0))
        elif a == "--compile":
            src = ("compile", None)
        elif a.startswith("-D"):
            defines.append(a)
        else:
            flt = a
    if src[0] == "lib":
        funcs = disassemble(src[1])
    else:
        funcs = parse_asm(src[1] if src[0] == "asm" else compile_asm(defines))
    rows = report(funcs, flt)
    tot = {"subdword_loads": 0, "vmcnt0_waits": 0}
    for name in sorted(rows):
        r = rows[name]
        for k in tot:
            tot[k] += r[k]
        passes = " ".join(f"[{p['stores']} stores, {p['vm_waits']} vm waits]" for p in r["flux_passes"])
        print(f"{r['subdword_loads']:>4} subdword  {r['vmcnt0_waits']:>4} vmcnt(0)  {r['instructions']:>6} ins  {name}"
              + (f"\n{'':>8}flux passes: {passes}" if passes else ""))
    print(f"total: {len(rows)} functions, {tot['subdword_loads']} sub-dword vector loads, {tot['vmcnt0_waits']} s_waitcnt vmcnt(0)")


if __name__ == "__main__":
    main(sys.argv[1:])

#!/usr/bin/env python3
"""Kernel-by-kernel comparison of two gfx950 device objects, usually two builds of one source of csrc/ (ss_kernels.hip, ss_guided.hip,
...): instruction streams, the .rodata section (kernel descriptors, constant tables) and the per-kernel metadata the streams do
not show.

    hipcc --offload-arch=gfx950 <Makefile CXXFLAGS> --cuda-device-only -c csrc/<source>.hip -o before.co   (parent commit)
    hipcc ... -o after.co                                                                                 (this tree)
    python3 profiles/tools/isa_diff.py before.co after.co

Runs on a machine without a GPU.  The batch matchers gained a table form through a trailing
template parameter pack (`typename... TAB`, empty in the existing forms): an instantiation with the empty pack is compared
with the kernel of the same name and template arguments before; kernels only the new build has are listed.  Branch targets are compared as
offsets inside their function, so code that moved inside the object still compares equal.  .rodata is compared byte
for byte (a kernel descriptor holds the distance to its kernel's code, so it also changes when kernels come, go or change places); of the
metadata notes, the register counts, LDS, scratch and kernel-argument sizes and the workgroup limit of every kernel.
Exit status 1 when anything differs."""
import os
import re
import subprocess
import sys
import tempfile

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


META = (".vgpr_count", ".sgpr_count", ".agpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
        ".kernarg_segment_size", ".max_flat_workgroup_size")


def read_object(bundle):
    """(instruction streams by symbol, .rodata bytes as hex, the META fields by kernel symbol)"""
    with tempfile.TemporaryDirectory() as d:
        elf = os.path.join(d, "k.elf")
        subprocess.check_call([f"{ROCM}/llvm/bin/clang-offload-bundler", "--unbundle", "--type=o", f"--input={bundle}",
                               f"--targets={TARGET}", f"--output={elf}"])
        text = subprocess.check_output([f"{ROCM}/llvm/bin/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", elf], text=True)
        dump = subprocess.check_output([f"{ROCM}/llvm/bin/llvm-objdump", "-s", "-j", ".rodata", elf], text=True)
        notes = subprocess.check_output([f"{ROCM}/llvm/bin/llvm-readelf", "--notes", elf], text=True)
    # " ADDR hex hex hex hex  ascii": the bytes without the addresses (where the linker put the section)
    rodata = "".join("".join(m.group(1).split()) for m in re.finditer(r"^ [0-9a-f]+ ((?:[0-9a-f]+ ){1,4}) ", dump, re.M))
    meta, entry = {}, None
    for line in notes.splitlines():
        m = re.match(r"^  (-| ) (\.\w+):\s*(.*)$", line)  # a key of a kernel's own map: the arguments' keys sit deeper
        if not m:
            continue
        if m.group(1) == "-":
            entry = {}
        if entry is None:
            continue
        if m.group(2) == ".name":
            meta[m.group(3)] = entry
        elif m.group(2) in META:
            entry[m.group(2)] = m.group(3)
    return functions(text), rodata, meta


def functions(text):
    funcs, name = {}, None
    for line in text.splitlines():
        m = re.match(r"^<(\S+)>:$", line)
        if m:
            name = m.group(1)
            funcs[name] = []
            continue
        if name is None or not line.strip():
            continue
        # "op args  // ADDR: ENC <sym+0xoff>" -> "op args <sym+0xoff>"; branch immediates are relative already
        ins = line.split("//")[0].strip()
        tgt = re.search(r"<[^>]*(\+0x[0-9a-f]+)>", line)
        body = funcs[name]
        if body and body[-1].startswith("s_getpc_b64") and ins.startswith("s_add_u32"):
            ins = re.sub(r"0x[0-9a-f]+$", "<pc-relative>", ins)  # address of a constant table: where the linker put it
        body.append(ins + (f" <{tgt.group(1)}>" if tgt else ""))
    return funcs


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    return dict(zip(names, out))


def old_name(dem):
    """the name the kernel had before the table form: the table is a trailing parameter pack, empty in the forms without it
    (k_match<>(...) was the plain function k_match(...), whose demangled name has no return type)"""
    return re.sub(r"^void (.*)<>\(", r"\1(", dem)


def main():
    (before, ro_b, meta_b), (after, ro_a, meta_a) = read_object(sys.argv[1]), read_object(sys.argv[2])
    db, da = demangle(list(before)), demangle(list(after))
    by_old = {db[n]: n for n in before}
    same = differ = checked = meta_differ = 0
    matched = set()
    for n in after:
        o = da[n] if da[n] in by_old else old_name(da[n])  # both builds have the table form: the name is unchanged
        if o not in by_old:
            print(f"new   {da[n][:140]}")
            continue
        matched.add(o)
        if before[by_old[o]] == after[n]:
            same += 1
        else:
            differ += 1
            print(f"DIFF  {o[:140]}  ({len(before[by_old[o]])} -> {len(after[n])} instructions)")
        if n in meta_a or by_old[o] in meta_b:  # a kernel (device functions have no metadata)
            mb, ma = meta_b.get(by_old[o], {}), meta_a.get(n, {})
            checked += 1
            if len(ma) != len(META) or ma != mb:
                meta_differ += 1
                print(f"META  {o[:140]}  " + ", ".join(f"{k} {mb.get(k)} -> {ma.get(k)}" for k in META if mb.get(k) != ma.get(k)))
    for o in by_old:
        if o not in matched:
            print(f"gone  {o[:140]}")
            differ += 1
    print(f"{same} kernels identical, {differ} differ or are gone")
    print(f".rodata: {len(ro_a) // 2} bytes, " + ("identical" if ro_a and ro_a == ro_b else f"DIFFERENT (before: {len(ro_b) // 2} bytes)"))
    print(f"metadata ({', '.join(k[1:] for k in META)}): {checked - meta_differ} of {checked} kernels identical")
    return 1 if differ or meta_differ or not checked or not ro_a or ro_a != ro_b else 0


if __name__ == "__main__":
    sys.exit(main())

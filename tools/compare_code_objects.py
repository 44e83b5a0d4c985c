#!/usr/bin/env python3
"""Are the kernels of two builds of the library the same code?  For every object of two build directories (inst*.o,
api.o, jacobi.o: whatever holds a .hip_fatbin) the gfx950 code object is extracted (llvm-objcopy, clang-offload-bundler
--unbundle) and held against its counterpart: the same set of kernel symbols -- no instantiation gained, lost or
moved --, every kernel's machine code byte for byte, and every kernel's register counts, scratch, spill counts, LDS and
largest workgroup (the notes of the code object, llvm-readelf --notes).  The order of the kernels inside an object may
differ.  Not compared: device functions that were not inlined into a kernel, .rodata and the kernel descriptors (.kd)
beyond what the notes restate.  Prints one verdict per object and the totals of objects and kernel entries; exits 1 on
any difference.  Needs no GPU.

    python tools/compare_code_objects.py <build dir A> <build dir B> [--arch gfx950] [--llvm /opt/rocm/llvm/bin]
"""
import argparse
import glob
import os
import re
import struct
import subprocess
import sys
import tempfile

FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".sgpr_spill_count",
          ".vgpr_spill_count", ".group_segment_fixed_size", ".max_flat_workgroup_size")


def code_object(llvm, arch, obj, tmp):
    """the bytes of the object's code object for `arch`, or None where the object has no device code"""
    fatbin, out = os.path.join(tmp, "fatbin"), os.path.join(tmp, "co")
    for f in (fatbin, out):
        if os.path.exists(f):
            os.remove(f)
    subprocess.run([os.path.join(llvm, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fatbin, obj, os.devnull],
                   capture_output=True)
    if not os.path.exists(fatbin) or os.path.getsize(fatbin) == 0:
        return None
    subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fatbin,
                    "--targets=hipv4-amdgcn-amd-amdhsa--" + arch, "--output=" + out], check=True, capture_output=True)
    return out


def functions(path):
    """{symbol: its bytes} of every function of an ELF64 little-endian file"""
    data = open(path, "rb").read()
    assert data[:6] == b"\x7fELF\x02\x01", path
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", data, 0x3A)
    sections = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize) for i in range(shnum)]
    out = {}
    for _, kind, _, _, offset, size, link, _, _, entsize in sections:
        if kind != 2:       # SHT_SYMTAB
            continue
        strings = sections[link][4]
        for at in range(offset, offset + size, entsize):
            name, info, _, shndx, value, length = struct.unpack_from("<IBBHQQ", data, at)
            if info & 0xF != 2 or shndx == 0 or shndx >= shnum:     # STT_FUNC, defined
                continue
            _, _, _, addr, sec_offset, _, _, _, _, _ = sections[shndx]
            begin = sec_offset + value - addr
            out[data[strings + name:data.index(b"\0", strings + name)].decode()] = data[begin:begin + length]
    return out


def kernels(llvm, path):
    """{kernel name: {field: value}} of the code object's metadata note"""
    notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", path], check=True, capture_output=True,
                           text=True).stdout
    out, entry = {}, None
    for line in notes.splitlines():
        if line.startswith("  - "):
            entry = {}
            line = "    " + line[4:]
        m = re.match(r"    (\.\w+): +(\S+)$", line)
        if m and entry is not None:
            entry[m.group(1)] = m.group(2)
            if m.group(1) == ".name":
                out[m.group(2)] = entry
        elif not line.startswith("    "):
            entry = None
    return out


def compare(llvm, arch, a, b, tmp_a, tmp_b):
    """(verdict, kernel entries) of one pair of objects"""
    co_a, co_b = code_object(llvm, arch, a, tmp_a), code_object(llvm, arch, b, tmp_b)
    if co_a is None and co_b is None:
        return "no device code", 0
    if co_a is None or co_b is None:
        return "DIFFERENT: device code on one side only", 0
    k_a, k_b = kernels(llvm, co_a), kernels(llvm, co_b)
    if set(k_a) != set(k_b):
        return f"DIFFERENT: {len(set(k_a) - set(k_b))} kernels only in A, {len(set(k_b) - set(k_a))} only in B", len(k_a)
    f_a, f_b = functions(co_a), functions(co_b)
    text = [k for k in k_a if k not in f_a or f_a[k] != f_b.get(k)]
    if text:
        return f"DIFFERENT: the code of {len(text)} kernels, the first {text[0]}", len(k_a)
    notes = [k for k in k_a if any(k_a[k].get(f) != k_b[k].get(f) for f in FIELDS) or
             any(f not in k_a[k] for f in FIELDS)]
    if notes:
        return f"DIFFERENT: the resources of {len(notes)} kernels, the first {notes[0]}", len(k_a)
    return f"identical: {len(k_a)} kernels", len(k_a)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("build_a")
    ap.add_argument("build_b")
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("--llvm", default="/opt/rocm/llvm/bin")
    args = ap.parse_args()
    names = [sorted(os.path.basename(p) for p in glob.glob(os.path.join(d, "*.o"))) for d in (args.build_a, args.build_b)]
    objects = entries = different = 0
    with tempfile.TemporaryDirectory() as tmp_a, tempfile.TemporaryDirectory() as tmp_b:
        for name in sorted(set(names[0]) | set(names[1])):
            if name not in names[0] or name not in names[1]:
                verdict, n = "DIFFERENT: the object is in one build only", 0
            else:
                verdict, n = compare(args.llvm, args.arch, os.path.join(args.build_a, name),
                                     os.path.join(args.build_b, name), tmp_a, tmp_b)
            print(f"{name}: {verdict}")
            if verdict != "no device code":
                objects += 1
                entries += n
            different += verdict.startswith("DIFFERENT")
    print(f"{objects} objects with kernels, {entries} kernel entries, {different} objects differ")
    return 1 if different else 0


if __name__ == "__main__":
    sys.exit(main())

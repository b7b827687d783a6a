#!/usr/bin/env python3
"""Are the kernels of two gfx950 code objects the same?  For a refactor that moves text and must not move code.

    hipcc <flags of _build.py for the file> --cuda-device-only --no-gpu-bundle-output -c csrc/otw.hip -o new.o   (and old.o)
    python tools/compare_device_code.py old.o new.o

For every kernel (a FUNC symbol with a `<name>.kd` descriptor) it compares the instruction bytes and the per-kernel
metadata of the code object's note (register counts, LDS, scratch, kernarg size, arguments).  Addresses and the order of
the kernels in the object may differ: a kernel's branches are relative to itself.  Prints one line per kernel that
differs and a verdict; exit status 0 = identical.  Where the code differs at equal length, the line also says whether
the two disassemblies hold the same multiset of instruction lines, i.e. whether the kernels differ in order only.
"""
import collections
import re
import struct
import subprocess
import sys

import yaml

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"  # where tools/check_lds_waits.py finds its llvm-objdump
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


def instruction_lines(path):
    """{kernel name: Counter of its disassembled instruction lines, addresses and comments stripped}."""
    text = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", path], check=True, capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:", line)
        if m:
            cur = out.setdefault(m.group(1), collections.Counter())
        elif cur is not None and line.strip():
            cur[re.sub(r"\s*//.*", "", line).strip()] += 1
    return out


def kernels(path):
    """{name: (instruction bytes, metadata dict)} of an ELF64 little-endian code object."""
    blob = open(path, "rb").read()
    shoff, = struct.unpack_from("<Q", blob, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", blob, 0x3A)
    sections = [struct.unpack_from("<IIQQQQIIQQ", blob, shoff + i * shentsize) for i in range(shnum)]
    symtab = next(s for s in sections if s[1] == 2)  # SHT_SYMTAB
    strtab = sections[symtab[6]]
    syms = {}
    for off in range(symtab[4], symtab[4] + symtab[5], 24):
        name_off, info, _other, shndx, value, size = struct.unpack_from("<IBBHQQ", blob, off)
        end = blob.index(b"\0", strtab[4] + name_off)
        syms[blob[strtab[4] + name_off:end].decode()] = (info & 15, shndx, value, size)
    notes = subprocess.run([READELF, "--notes", path], check=True, capture_output=True, text=True).stdout
    meta = yaml.safe_load(notes[notes.index("---"):notes.rindex("...")])
    out = {}
    for k in meta["amdhsa.kernels"]:
        name = k[".name"]
        kind, shndx, value, size = syms[name]
        assert kind == 2 and k[".symbol"] in syms, name  # STT_FUNC with a descriptor
        sec = sections[shndx]
        start = sec[4] + value - sec[3]
        out[name] = (blob[start:start + size], {key: v for key, v in k.items() if key != ".symbol"})
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad, lines = 0, None
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print("only in %s: %s" % (sys.argv[2] if name in b else sys.argv[1], name))
            bad += 1
            continue
        (code_a, meta_a), (code_b, meta_b) = a[name], b[name]
        what = []
        if code_a != code_b:
            what.append("code (%d / %d bytes)" % (len(code_a), len(code_b)))
            if len(code_a) == len(code_b):
                lines = lines or (instruction_lines(sys.argv[1]), instruction_lines(sys.argv[2]))
                what.append("same instruction lines, order differs" if lines[0][name] == lines[1][name]
                            else "instruction lines differ")
        what += ["%s %r / %r" % (key, meta_a.get(key), meta_b.get(key)) for key in sorted(set(meta_a) | set(meta_b))
                 if key != ".args" and meta_a.get(key) != meta_b.get(key)]
        if meta_a.get(".args") != meta_b.get(".args"):
            what.append("arguments")
        if what:
            print("%s: %s" % (name, "; ".join(what)))
            bad += 1
    print("%d kernels / %d kernels, %s" % (len(a), len(b), "%d differ" % bad if bad else "all identical"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

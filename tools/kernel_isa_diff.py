#!/usr/bin/env python3
"""Per-kernel comparison of the gfx950 code of TWO built objects or libraries: the code objects are pulled out of .hip_fatbin the
way tools/kernel_metadata.py does, disassembled (llvm-objdump -d --no-show-raw-insn, the address comments stripped) and compared
kernel by kernel - one line per kernel, `identical` or both instruction counts, and the kernels only one side has.  Needs no GPU.

  tools/kernel_isa_diff.py old/build/kernels.o build/kernels.o
"""
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM", "/opt/rocm"), "lib", "llvm", "bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def kernels_of(path):
    """{mangled kernel name: [instruction lines]} over every gfx950 code object bundled in `path`"""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fat.bin")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, path, os.path.join(d, "copy")])
        blob = open(fat, "rb").read()
        for k, at in enumerate(m.start() for m in re.finditer(MAGIC, blob)):
            (count,) = struct.unpack_from("<Q", blob, at + len(MAGIC))
            pos = at + len(MAGIC) + 8
            for _ in range(count):
                off, size, tlen = struct.unpack_from("<QQQ", blob, pos)
                triple = blob[pos + 24:pos + 24 + tlen].decode()
                pos += 24 + tlen
                if "gfx950" not in triple:
                    continue
                co = os.path.join(d, f"co{k}")
                open(co, "wb").write(blob[at + off:at + off + size])
                notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
                names = set(re.findall(r"\.name:\s+(\S+)", notes))
                text = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], text=True)
                cur = None
                for line in text.splitlines():
                    head = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
                    if head:
                        cur = out.setdefault(head.group(1), []) if head.group(1) in names else None
                    elif cur is not None and line.startswith(("\t", " ")) and line.strip():
                        cur.append(re.sub(r"\s*//.*$", "", line).strip())
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = kernels_of(sys.argv[1]), kernels_of(sys.argv[2])
    for name in sorted(set(a) | set(b)):
        if name not in b:
            print(f"{name}: only in {sys.argv[1]}")
        elif name not in a:
            print(f"{name}: only in {sys.argv[2]}")
        elif a[name] == b[name]:
            print(f"{name}: identical")
        else:
            print(f"{name}: {len(a[name])} -> {len(b[name])} instructions")


if __name__ == "__main__":
    main()

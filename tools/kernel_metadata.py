#!/usr/bin/env python3
"""Per-kernel resources of a BUILT library, read from the code-object metadata the way tests/test_abi_and_host.py reads it (the
gfx950 code objects bundled in .hip_fatbin, llvm-readelf --notes): VGPRs, SGPRs, LDS, scratch and the two spill counts, one
line per kernel, sorted by name - two builds compare with diff.

  tools/kernel_metadata.py [library=libeddsa_amd/libeddsa_amd.so]
"""
import os
import re
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = os.path.join(os.environ.get("ROCM", "/opt/rocm"), "lib", "llvm", "bin")
lib = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "libeddsa_amd", "libeddsa_amd.so")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"

notes = ""
with tempfile.TemporaryDirectory() as d:
    fat = os.path.join(d, "fat.bin")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, os.path.join(d, "copy.so")])
    blob = open(fat, "rb").read()
    for k, at in enumerate(m.start() for m in re.finditer(MAGIC, blob)):
        (count,) = struct.unpack_from("<Q", blob, at + len(MAGIC))
        pos = at + len(MAGIC) + 8
        for _ in range(count):
            off, size, tlen = struct.unpack_from("<QQQ", blob, pos)
            triple = blob[pos + 24:pos + 24 + tlen].decode()
            pos += 24 + tlen
            if "gfx950" in triple:
                co = os.path.join(d, f"co{k}")
                open(co, "wb").write(blob[at + off:at + off + size])
                notes += subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)

rows = []
for block in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
    field = lambda key: re.search(r"\." + key + r":\s+(\S+)", block).group(1)   # noqa: E731
    name = field("name")
    try:
        name = re.sub(r"^void ed::|\(.*$", "", subprocess.check_output(["c++filt", name], text=True).strip())
    except (OSError, subprocess.CalledProcessError):
        pass                                        # (no demangler here: the mangled names sort and compare as well)
    rows.append((name, field("vgpr_count"), field("sgpr_count"), field("group_segment_fixed_size"), field("private_segment_fixed_size"),
                 field("vgpr_spill_count"), field("sgpr_spill_count")))
print("%-52s %5s %5s %7s %8s %11s %11s" % ("kernel", "VGPR", "SGPR", "LDS", "scratch", "vgpr_spill", "sgpr_spill"))
for r in sorted(rows):
    print("%-52s %5s %5s %7s %8s %11s %11s" % r)

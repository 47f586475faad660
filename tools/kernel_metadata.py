"""One line per device kernel of a built libspatialclip_hip.so: name, VGPR / AGPR / SGPR counts, scratch bytes, LDS bytes and
code size, sorted by name -- the figures a host-side refactor must leave untouched.  Diff the output for two builds:

    python tools/kernel_metadata.py A.so > a.txt; python tools/kernel_metadata.py B.so > b.txt; diff a.txt b.txt

Needs only the ROCm LLVM tools (no GPU): every gfx code object is cut out of the library's .hip_fatbin section."""
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(lib, tmp):
    fat = os.path.join(tmp, "fatbin")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, os.path.join(tmp, "x")],
                   check=True)
    data = open(fat, "rb").read()
    out, pos = [], data.find(MAGIC)
    while pos >= 0:
        n, = struct.unpack_from("<Q", data, pos + len(MAGIC))
        p = pos + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", data, p)
            triple = data[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if "amdgcn" in triple and size:
                path = os.path.join(tmp, "co%d.o" % len(out))
                open(path, "wb").write(data[pos + off:pos + off + size])
                out.append(path)
        pos = data.find(MAGIC, pos + 1)
    return out


def kernels(co):
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
    syms = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-sW", co], capture_output=True, text=True, check=True).stdout
    size = {}
    for line in syms.splitlines():
        f = line.split()
        if len(f) >= 8 and f[3] == "FUNC":
            size[f[7]] = int(f[2], 0)
    rows = []
    for block in re.split(r"\n\s+- \.agpr_count:", "\n" + notes)[1:]:
        block = ".agpr_count:" + block
        get = lambda k: re.search(r"\.%s:\s+(\S+)" % k, block).group(1)      # noqa: E731
        name = get("name")
        rows.append("%s vgpr=%s agpr=%s sgpr=%s scratch=%s lds=%s code=%d" % (
            name, get("vgpr_count"), get("agpr_count"), get("sgpr_count"), get("private_segment_fixed_size"),
            get("group_segment_fixed_size"), size[name]))
    return rows


def main(lib):
    with tempfile.TemporaryDirectory() as tmp:
        rows = [r for co in code_objects(lib, tmp) for r in kernels(co)]
    print("\n".join(sorted(rows)))


if __name__ == "__main__":
    main(sys.argv[1])

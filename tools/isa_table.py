#!/usr/bin/env python3
"""Per-kernel resource and instruction-class table of gfx950 assembly files (hipcc --save-temps leaves one *.s per source):
VGPRs, SGPRs, scratch bytes, waves per SIMD, LDS bytes, instruction count, and the counts of v_mfma*, ds_read*, ds_write*,
global_load*, global_store*.  A changed count of one of these between two commits means a kernel's loop body changed.
An instruction is a line of a kernel's body that is left when comments, labels and directives are dropped.  Kernels are
the symbols whose mangled name holds `kernel`; names are demangled with binutils' c++filt, which must be on the PATH.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=fast --save-temps -c spatial-clip_amd/csrc/X.hip -o X.o
    python tools/isa_table.py X-hip-amdgcn-amd-amdhsa-gfx950.s [more.s ...]

With `--against <the same files compiled at the parent commit>` after the files, the table is followed by one line per kernel:
whether its instruction stream, as kernels() extracts it, equals the parent's, and if not the index of the first instruction
that differs.  A refactor that leaves every stream identical has changed neither behaviour nor speed.

    python tools/isa_table.py X-hip-amdgcn-amd-amdhsa-gfx950.s --against parent/X-hip-amdgcn-amd-amdhsa-gfx950.s
"""
import re
import subprocess
import sys

CLASSES = ("v_mfma", "ds_read", "ds_write", "global_load", "global_store")
FIELDS = ("TotalNumSgprs", "NumVgprs", "ScratchSize", "Occupancy", "LDSByteSize")


def kernels(path):
    """{mangled name: (instructions, {field: value})} of one .s file; labels, directives and comments are dropped."""
    out, name, body, res = {}, None, [], {}
    for line in open(path):
        m = re.match(r"^(_Z\w*kernel\w*):", line)
        if m:
            name, body, res = m.group(1), [], {}
            continue
        if name is None:
            continue
        m = re.match(r"^; (\w+): (\d+)", line)
        if m and m.group(1) in FIELDS:
            res[m.group(1)] = int(m.group(2))
            if len(res) == len(FIELDS):
                out[name], name = (body, res), None
            continue
        s = line.split(";")[0].strip()
        if s and not s.startswith(".") and not s.endswith(":"):
            body.append(re.sub(r"\.LBB\d+_\d+", "L", s))
    return out


def against(ks, parent, names):
    """One line per kernel of either side: identical to the parent's stream, or where the first difference lies."""
    same = 0
    for k in list(ks) + [k for k in parent if k not in ks]:
        nm = names.get(k, k)
        if k not in parent or k not in ks:
            print(f"{'only in this tree' if k in ks else 'only in the parent'}  {nm}")
            continue
        a, b = ks[k][0], parent[k][0]
        if a == b:
            same += 1
            print(f"identical ({len(a)} instructions)  {nm}")
        else:
            i = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            print(f"DIFFERS at instruction {i} (this tree {len(a)}, parent {len(b)} instructions)  {nm}")
    print(f"{same} of {len(set(ks) | set(parent))} kernels identical to the parent")
    return same == len(set(ks) | set(parent))


def main():
    args = sys.argv[1:]
    cut = args.index("--against") if "--against" in args else len(args)
    ks, parent = {}, {}
    for f in args[:cut]:
        ks.update(kernels(f))
    for f in args[cut + 1:]:
        parent.update(kernels(f))
    names = subprocess.run(["c++filt", "-p"], input="\n".join(ks), capture_output=True, text=True, check=True).stdout.split("\n")
    assert len(names) >= len(ks), "c++filt returned fewer names than kernels"
    print(f"{'VGPR':>4} {'SGPR':>4} {'scr':>3} {'wav':>3} {'LDS':>6} {'instr':>5} " + " ".join(f"{c:>12}" for c in CLASSES) + "  kernel")
    for (body, res), nm in zip(ks.values(), names):
        n = [sum(i.startswith(c) for i in body) for c in CLASSES]
        print(f"{res['NumVgprs']:4d} {res['TotalNumSgprs']:4d} {res['ScratchSize']:3d} {res['Occupancy']:3d} {res['LDSByteSize']:6d} {len(body):5d} "
              + " ".join(f"{x:12d}" for x in n) + "  " + nm.replace("(anonymous namespace)::", ""))
    if cut < len(args):
        short = {k: nm.replace("(anonymous namespace)::", "") for k, nm in zip(ks, names)}
        sys.exit(0 if against(ks, parent, short) else 1)


if __name__ == "__main__":
    main()

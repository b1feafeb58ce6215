#!/usr/bin/env python3
"""Registers, scratch, LDS, code size, scalar loads and full scalar-memory waits of every kernel of csrc/po_count.hip, compiled for gfx950 with the Makefile's flags
(no GPU needed) - the table a restructuring of stage 1 is judged by: same kernels, no scratch, no instantiation a step lower
in waves per SIMD = min(8, 512 // roundup(vgprs, 8)); scalar loads (s_load_*) and `s_waitcnt lgkmcnt(0)` from the disassembly
show whether the kernel's parameters are still read once into scalar registers or again in the unrolled loops.
    stage1_resources.py                      the table of the working tree
    stage1_resources.py --before OTHER       two columns, OTHER and the working tree.  OTHER.hip is compiled here against the
                                             working tree's headers with the working tree's flags; OTHER.co is a gfx950 code
                                             object compiled elsewhere (an earlier commit's file with that commit's own flags:
                                             hipcc <its Makefile's flags> -x hip --cuda-device-only --no-gpu-bundle-output -c)"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "phyloligo_amd", "csrc")
LLVM = "/opt/rocm/lib/llvm/bin"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from check_spills import FLAGS as COMMON, PER_FILE  # noqa: E402  (the Makefile's flags, kept in one place on this side)
FLAGS = COMMON + ["-I" + CSRC] + PER_FILE["po_count.hip"]
FIELDS = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")


def kernels(src):
    """{kernel: (vgprs, sgprs, scratch bytes, static LDS bytes, code bytes, scalar loads, lgkmcnt(0) waits)} of one source file (or of its gfx950 code object *.co)"""
    with tempfile.TemporaryDirectory() as tmp:
        co = src if src.endswith(".co") else os.path.join(tmp, "unit.co")
        if co != src:
            subprocess.run([HIPCC] + FLAGS + ["-x", "hip", "--cuda-device-only", "--no-gpu-bundle-output", "-c", src, "-o", co], check=True, cwd=CSRC)
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
        syms = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--symbols", "--wide", co], capture_output=True, text=True, check=True).stdout
        dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], capture_output=True, text=True, check=True).stdout
    loads = {}
    for part in re.split(r"\n[0-9a-f]+ <", dis)[1:]:
        loads[part[:part.index(">")]] = (len(re.findall(r"\ts_load_", part)), len(re.findall(r"s_waitcnt lgkmcnt\(0\)", part)))
    size = {}
    for line in syms.splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC":
            size[f[7]] = int(f[2], 0)
    out = {}
    for block in re.split(r"\n\s+- \.agpr_count:|\n\s+- \.args:", notes)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        vals = [re.search(r"\.%s:\s+(\d+)" % f, block) for f in FIELDS]
        if name and all(vals):
            out[name.group(1)] = tuple(int(v.group(1)) for v in vals) + (size.get(name.group(1), -1),) + loads.get(name.group(1), (-1, -1))
    return out


def short_name(mangled):
    """count_kernel<true, 0, 2, -1> from _ZN12_GLOBAL__N_112count_kernelILb1ELi0ELi2ELin1EEEv...; other kernels by their plain name"""
    m = re.match(r"_ZN12_GLOBAL__N_1\d+([a-z_0-9]+?)(?:ILb(\d)ELi(n?\d+)ELi(n?\d+)ELi(n?\d+)EEEv|E)", mangled)
    if not m:
        return mangled
    if m.group(2) is None:
        return m.group(1)
    return "%s<%s, %s>" % (m.group(1), "true" if m.group(2) == "1" else "false", ", ".join(g.replace("n", "-") for g in m.groups()[2:]))


def waves(vgprs):
    return min(8, 512 // max(8, (vgprs + 7) // 8 * 8))


def main():
    after = kernels(os.path.join(CSRC, "po_count.hip"))
    before = kernels(os.path.abspath(sys.argv[2])) if len(sys.argv) == 3 and sys.argv[1] == "--before" else None
    short = {m: short_name(m) for m in after}
    print("%d kernels" % len(after) + ("" if before is None else " (before: %d; same names: %s)" % (len(before), sorted(before) == sorted(after))))
    print("columns: vgprs sgprs scratch-bytes static-LDS-bytes code-bytes scalar-loads lgkmcnt(0)-waits waves/SIMD" + ("" if before is None else ", before -> after"))
    bad = 0
    for name in sorted(after, key=lambda m: short[m]):
        a = after[name]
        if before is None:
            print("%-44s %3d %3d %3d %5d %6d %4d %4d  %d" % ((short[name],) + a + (waves(a[0]),)))
            bad += a[2] != 0
            continue
        b = before.get(name, (0, 0, 0, 0, 0, 0, 0))
        lower = waves(a[0]) < waves(b[0])
        bad += a[2] != 0 or lower
        print("%-44s %3d -> %3d  %3d -> %3d  %d -> %d  %5d -> %5d  %6d -> %6d (%+5.1f %%)  %4d -> %4d  %4d -> %4d  %d -> %d%s"
              % (short[name], b[0], a[0], b[1], a[1], b[2], a[2], b[3], a[3], b[4], a[4], 100.0 * (a[4] - b[4]) / max(b[4], 1), b[5], a[5], b[6], a[6],
                 waves(b[0]), waves(a[0]), "  <-- a step lower" if lower else ""))
    print("kernels with scratch or a lower step: %d" % bad)
    return 1 if bad or (before is not None and sorted(before) != sorted(after)) else 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Instruction classes per basic block of a gfx950 assembly file (development aid; needs no GPU).

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -mllvm -amdgpu-kernarg-preload-count=8 -S --cuda-device-only \
          -I open3d_slam_amd/csrc -I include one_kernel.hip -o one_kernel.s
    scripts/isa_block_counts.py one_kernel.s

one_kernel.hip includes common.hpp and icp_kernels.hpp and explicitly instantiates one kernel inside namespace o3ds, e.g.
    template __global__ void icp_fused_kernel<P4f, false, 512, 4, false>(const IcpStateDev*, const double*, int, IcpFusedArgs);

Counts VALU / SALU / VMEM / LDS / other instructions per basic block, in the order of the file, and in total.  The counts are STATIC:
which blocks make up a region of the source (a stage of the search, say) is read from the assembly beside them.  It counts and does
nothing else.
"""
import collections
import re
import sys

CLASSES = ("valu", "salu", "vmem", "lds", "other")


def classify(op: str) -> str:
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("s_"):
        return "other" if op.startswith(("s_waitcnt", "s_nop", "s_barrier", "s_endpgm", "s_sleep", "s_setprio")) else "salu"
    return "other"


def main() -> None:
    if len(sys.argv) != 2:
        sys.exit("usage: isa_block_counts.py FILE.s")
    block = "entry"
    per_block = collections.OrderedDict()
    for raw in open(sys.argv[1]):
        line = raw.strip()
        if not line or line.startswith(";"):
            continue
        m = re.match(r"([.\w$]+):", line)
        if m:
            if not m.group(1).startswith((".Ltmp", ".Lfunc", ".Ldebug", ".Lline", ".Lcu", ".Linfo", ".Lsec")):  # (debug labels split no block)
                block = m.group(1)
            continue
        if line.startswith("."):
            continue
        per_block.setdefault(block, collections.Counter())[classify(line.split()[0])] += 1

    fmt = "%-34s" + " %7s" * len(CLASSES)
    print(fmt % (("block",) + CLASSES))
    total = collections.Counter()
    for b, cnt in per_block.items():
        print(fmt % ((b,) + tuple(cnt[c] for c in CLASSES)))
        total.update(cnt)
    print(fmt % (("total",) + tuple(total[c] for c in CLASSES)))


if __name__ == "__main__":
    main()

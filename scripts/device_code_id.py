#!/usr/bin/env python3
"""Prints the sha256 and the size of the gfx950 code object inside each given library.

    python scripts/device_code_id.py open3d_slam_amd/lib/libo3ds_backend.so open3d_slam_amd/lib/libo3ds_backend_ab.so

Two builds whose lines are equal hold the same machine code at the same offsets: no kernel's speed or result can differ
between them, and only host code is left to judge.  That is the rule a host-side refactor of csrc/ states: build the parent
and the change with the same command (build.py's flags, from the tree root, backend.hip by its relative path) and compare,
shipped library with shipped, A/B with A/B.
"""
from __future__ import annotations

import hashlib
import os
import shutil
import subprocess
import sys
import tempfile

TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def _tool(name: str) -> str:
    for c in (shutil.which(name), os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", name)):
        if c and os.path.exists(c):
            return c
    raise RuntimeError(f"{name} not found")


def device_code(lib: str) -> bytes:
    """The code object for TARGET: the library's .hip_fatbin section, unbundled."""
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dev.co")
        subprocess.run([_tool("llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, fat], check=True)
        subprocess.run([_tool("clang-offload-bundler"), "--type=o", f"--targets={TARGET}", "--unbundle", f"--input={fat}", f"--output={co}"],
                       check=True)
        with open(co, "rb") as f:
            return f.read()


def main(argv) -> int:
    if not argv:
        print(__doc__)
        return 2
    for lib in argv:
        code = device_code(lib)
        print(f"{hashlib.sha256(code).hexdigest()}  {len(code):9d}  {lib}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))

#!/usr/bin/env python3
"""Build check (CPU): the GEMM kernels of an object file or library with their register, LDS and scratch sizes.

Reads the gfx950 code objects (tools/check_asm_loads.py's extraction) and prints, from the code-object metadata, one
sorted line per kernel whose name contains "gemm": mangled name, VGPRs, SGPRs, static LDS bytes, scratch bytes.  Two
builds instantiate and compile the same GEMM kernels exactly when their lists are equal:

  python tools/gemm_kernel_list.py [panopticdiffusionmodels_amd/csrc/build/gemm.o] > list.txt
"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from check_asm_loads import LLVM, REPO, code_objects  # noqa: E402

FIELDS = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def kernels(path):
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in code_objects(path, tmp):
            notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True,
                                   check=True).stdout
            # amdhsa.kernels: a YAML list, one "- .args:" item per kernel, keys sorted
            for item in re.split(r"\n\s+- \.agpr_count:|\n\s+- \.args:", notes)[1:]:
                kv = dict(re.findall(r"^\s+(\.[a-z_]+):\s+(\S+)\s*$", item, re.M))
                if "gemm" in kv.get(".name", ""):
                    out[kv[".name"]] = tuple(int(kv[f]) for f in FIELDS)
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "panopticdiffusionmodels_amd", "csrc", "build",
                                                               "gemm.o")
    ks = kernels(path)
    print(f"# {len(ks)} GEMM kernels: name vgpr sgpr lds scratch")
    for name in sorted(ks):
        print(name, *ks[name])
    return 0 if ks else 1


if __name__ == "__main__":
    sys.exit(main())

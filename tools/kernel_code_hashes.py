#!/usr/bin/env python3
"""`symbol  bytes  sha256` of the machine code of EVERY function of every gfx950 code object inside a built
libsvbrdf_hip.so, sorted: two builds with identical listings run identical device code.  No GPU needed.
    python tools/kernel_code_hashes.py [library.so]                     default: the shipped library
"""
import hashlib
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("_codehash", os.path.join(ROOT, "svbrdf_estimation_amd", "_codehash.py"))
_codehash = importlib.util.module_from_spec(spec)
spec.loader.exec_module(_codehash)           # (without importing the package: no torch needed)

if __name__ == "__main__":
    so = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "svbrdf_estimation_amd", "lib", "libsvbrdf_hip.so")
    with open(so, "rb") as f:
        data = f.read()
    lines = ["%s  %d  %s" % (name, len(code), hashlib.sha256(code).hexdigest())
             for elf in _codehash.device_code_objects(data) for name, code in _codehash.function_symbols(elf).items()]
    print("\n".join(sorted(lines)))

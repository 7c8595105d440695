#!/usr/bin/env python3
"""Compare the gfx950 code objects of two builds of csrc/*.hip, unit by unit.

    scripts/device_code_cmp.py <build dir A> <build dir B> [> profiles/..._device_code.txt]

For every <unit>.hip.o in both directories: the device code object is taken out of the host
object's .hip_fatbin bundle, and .text, .rodata (which holds the kernel descriptors) and the
notes (the per-kernel resource metadata) are compared byte for byte. hipcc puts a per-build unit
id (a hash of the source path and the command line) into the names of kernels with internal
linkage; it appears in the notes and the symbol table only, and is replaced by zeros of the same
length before the comparison (reported as "normalised" where that was needed). Exit status 1 if
any unit differs.
"""
import glob
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
SECTIONS = (".text", ".rodata", ".note")
UNIT_ID = re.compile(rb"(?<=[._])[0-9a-f]{16}(?![0-9a-f])")  # ..._GLOBAL__N__<id>... / __hip_cuid_<id>


def run(*cmd):
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)


def sections(obj, tmp):
    """{section: bytes} of the gfx950 code object inside host object `obj` ({} if it has none)."""
    fat, co = os.path.join(tmp, "fat"), os.path.join(tmp, "co")
    try:
        run(os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj)
    except subprocess.CalledProcessError:
        return {}
    run(os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET,
        "--input=" + fat, "--output=" + co)
    out = {}
    for sec in SECTIONS:
        path = os.path.join(tmp, "sec")
        open(path, "wb").close()
        try:
            run(os.path.join(LLVM, "llvm-objcopy"), "--dump-section", sec + "=" + path, co)
        except subprocess.CalledProcessError:
            continue  # a unit without kernels has no such section
        out[sec] = open(path, "rb").read()
    return out


def main():
    a_dir, b_dir = sys.argv[1:3]
    units = sorted(os.path.basename(p) for p in glob.glob(os.path.join(a_dir, "*.hip.o")))
    differ = 0
    with tempfile.TemporaryDirectory() as tmp:
        for u in units:
            a = sections(os.path.join(a_dir, u), tmp)
            b = sections(os.path.join(b_dir, u), tmp)
            parts, verdict = [], "identical"
            for sec in SECTIONS:
                x, y = a.get(sec, b""), b.get(sec, b"")
                how = "same"
                if x != y:
                    if UNIT_ID.sub(b"0" * 16, x) == UNIT_ID.sub(b"0" * 16, y):
                        how = "same (unit id normalised)"
                    else:
                        how, verdict = "DIFFERENT", "DIFFERENT"
                parts.append("%s %d B sha256 %s %s" % (sec, len(x), hashlib.sha256(x).hexdigest()[:12], how))
            differ += verdict != "identical"
            print("%-24s %s\n    %s" % (u[:-2], verdict, "\n    ".join(parts)))
    print("%d of %d units differ" % (differ, len(units)))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Do two builds of libnastar_hip.so hold the same machine code for the device functions they share?  (CPU; needs the ROCm LLVM tools.)

A change that adds kernel instantiations behind ``if constexpr`` branches of the shared ``csrc/*_body.inc`` files claims that every existing
kernel keeps its instruction stream.  This checks the claim: both libraries' gfx950 code objects are unbundled from their ``.hip_fatbin``
sections, and the bytes of every FUNC symbol of ``.text`` are hashed and compared by (mangled) name.  Prints the counts -- identical,
different, missing, new -- and the names that differ; exit code 1 when a shared function differs or one went missing.

Usage:  python tools/compare_device_code.py <old libnastar_hip.so> <new libnastar_hip.so> [--llvm /opt/rocm/llvm/bin] [--arch gfx950]
(build the old one from a checkout of the parent commit: make -C neural-astar_amd/csrc OUT=/tmp/old.so BUILD=/tmp/old_build)
"""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile


def device_functions(so, llvm, arch, tmp, tag):
    run = lambda tool, *a, **k: subprocess.check_output([os.path.join(llvm, tool), *a], **k)  # noqa: E731
    fat = os.path.join(tmp, tag + ".fatbin")
    run("llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", so, fat)
    data = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(b"__CLANG_OFFLOAD_BUNDLE__"), data)]  # one bundle per translation unit
    out = {}
    for n, st in enumerate(starts):
        part, co = f"{fat}.{n}", os.path.join(tmp, f"{tag}.{n}.co")
        open(part, "wb").write(data[st:starts[n + 1] if n + 1 < len(starts) else len(data)])
        run("clang-offload-bundler", "--unbundle", "--type=o", f"--input={part}", f"--targets=hipv4-amdgcn-amd-amdhsa--{arch}", f"--output={co}")
        sect = re.search(r"\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", run("llvm-readelf", "-SW", co, text=True))
        addr0, off0 = int(sect.group(1), 16), int(sect.group(2), 16)
        blob = open(co, "rb").read()
        for line in run("llvm-readelf", "-sW", co, text=True).splitlines():
            f = line.split()
            if len(f) >= 8 and f[3] == "FUNC" and f[6] != "UND":
                a, size = int(f[1], 16), int(f[2])
                out[f[7]] = hashlib.sha256(blob[off0 + a - addr0:off0 + a - addr0 + size]).hexdigest()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--llvm", default="/opt/rocm/llvm/bin")
    ap.add_argument("--arch", default="gfx950")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        a = device_functions(args.old, args.llvm, args.arch, tmp, "old")
        b = device_functions(args.new, args.llvm, args.arch, tmp, "new")
    differ = sorted(k for k in a if k in b and a[k] != b[k])
    missing = sorted(k for k in a if k not in b)
    print(f"old {len(a)} functions, new {len(b)}: identical {sum(a[k] == b.get(k) for k in a)}, different {len(differ)}, missing {len(missing)}, "
          f"added {sum(k not in a for k in b)}")
    for k in differ:
        print("DIFFERENT", k)
    for k in missing:
        print("MISSING", k)
    return 1 if differ or missing else 0


if __name__ == "__main__":
    sys.exit(main())

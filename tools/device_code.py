#!/usr/bin/env python3
"""Diff aid for host-only refactors: compiles the device side of every file in gm3d_amd.build.SOURCES
(no GPU needed) and prints JSON {file: {kernel symbol: {"code": sha1, "meta": sha1}}}.

"code" hashes the instruction words of the symbol as llvm-objdump -d prints them (position independent: the
addresses are left out); "meta" hashes the kernel's record in the AMDGPU metadata note (registers, LDS, scratch,
kernarg layout) from llvm-readelf --notes.  Run it at two commits and diff the outputs:

    python tools/device_code.py > after.json
"""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gm3d_amd import build  # noqa: E402

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
WORDS = re.compile(r"//\s*[0-9A-F]+:((?:\s[0-9A-F]{8})+)")


def sha(lines):
    return hashlib.sha1("\n".join(lines).encode()).hexdigest()


def code_by_symbol(obj):
    """symbol -> the instruction words between its `<symbol>:` label and the next one"""
    out, cur = {}, None
    for line in subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", obj], text=True).splitlines():
        m = re.match(r"(?:[0-9a-fA-F]+ )?<(\S+)>:$", line)      # `<symbol>:`, after its address where objdump prints one
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and (w := WORDS.search(line)):
            cur.append(w.group(1).strip())
    return out


def meta_by_kernel(obj):
    """kernel name -> the lines of its amdhsa.kernels record"""
    records, inside = [], False
    for line in subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", obj], text=True).splitlines():
        if line.startswith("amdhsa."):
            inside = line.startswith("amdhsa.kernels:")
        elif inside and line.startswith("  - "):
            records.append([line])
        elif inside and records and line.startswith("  "):
            records[-1].append(line)
    return {next(ln.split(":", 1)[1].strip() for ln in rec if ln.lstrip().startswith(".name:")): rec for rec in records}


def main():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    result = {}
    with tempfile.TemporaryDirectory() as tmp:
        for src, extra in build.SOURCES.items():
            obj = os.path.join(tmp, src + ".co")
            subprocess.check_call([hipcc] + build.COMMON + extra + ["--cuda-device-only", "--no-gpu-bundle-output", "-c",
                                                                     os.path.join(build.CSRC, src), "-o", obj])
            code, meta = code_by_symbol(obj), meta_by_kernel(obj)
            empty = [k for k in meta if not code.get(k)]
            if empty:
                sys.exit("%s: no instruction words found for %s" % (src, ", ".join(empty)))
            result[src] = {k: {"code": sha(code[k]), "meta": sha(rec)} for k, rec in sorted(meta.items())}
    json.dump(result, sys.stdout, indent=1, sort_keys=True)
    print()
    print("%d kernels in %d files" % (sum(len(v) for v in result.values()), len(result)), file=sys.stderr)


if __name__ == "__main__":
    main()

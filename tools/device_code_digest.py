#!/usr/bin/env python3
"""Digest of a library's device code, for "did this host-side change touch a kernel?":

    python tools/device_code_digest.py raytracing.jl_amd/csrc/librt_segmentize.so [out.s]

Takes every gfx950 code object out of the library's fat binary, disassembles it (llvm-objdump of the ROCm toolchain) and prints the
number of functions, a hash of the sorted kernel symbol list and a hash of the per-function disassembly, functions sorted by name.
What depends only on where the linker put a function is left out: the instructions' addresses (their encodings stay), the padding
between functions and behind the last one of a code object, the symbol annotation of branch targets, the compile unit's id in symbol names; a pc-relative literal (s_getpc_b64
followed by s_add_u32 with a literal) is replaced by the symbol it lands on.  Two builds whose kernels are the same instructions
print the same two hashes, whatever order the host code instantiated them in.  `out.s`: the normalised disassembly, for diff."""
import hashlib
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/lib/llvm/bin")
CUID = re.compile(r"__hip_cuid_[0-9a-f]+")


def code_objects(lib, tmp):
    fat = os.path.join(tmp, "fatbin")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, fat])
    d = open(fat, "rb").read()
    magic, pos, out = b"__CLANG_OFFLOAD_BUNDLE__", 0, []
    while (i := d.find(magic, pos)) >= 0:
        (n,) = struct.unpack_from("<Q", d, i + 24)
        p = i + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", d, p)
            triple = d[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            if "gfx950" in triple and size:
                out.append(os.path.join(tmp, "co%d" % len(out)))
                open(out[-1], "wb").write(d[i + off:i + off + size])
        pos = i + 24
    return out


def run(tool, *args):
    return subprocess.run([os.path.join(LLVM, tool), *args], capture_output=True, text=True, check=True).stdout


def main():
    lib = sys.argv[1]
    funcs, kernels = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        for co in code_objects(lib, tmp):
            syms = {}
            for l in run("llvm-readelf", "-s", "--wide", co).splitlines():
                p = l.split()
                if len(p) >= 8 and p[3] in ("FUNC", "OBJECT", "NOTYPE") and p[6] != "UND":
                    syms.setdefault(int(p[1], 16), CUID.sub("__hip_cuid_X", p[7]))
                    if p[3] == "FUNC" and p[4] == "GLOBAL":
                        kernels.append(p[7])
            name, getpc = None, None
            for line in run("llvm-objdump", "-d", co).splitlines():
                m = re.match(r"^[0-9a-f]{16} <(.+)>:$", line)
                if m:
                    name = CUID.sub("__hip_cuid_X", m.group(1))
                    # a device function of a shared header that two units keep out of line (rt_device.hpp's find_element_fallback in
                    # rt_march.hip and rt_locate.hip) has one copy per code object: the later ones are told apart by a counter
                    base, n = name, 1
                    while name in funcs:
                        n += 1
                        name = "%s [copy %d]" % (base, n)
                    funcs[name] = []
                    continue
                if name is None or not line.strip() or line.strip() == "...":
                    continue
                a = re.search(r"// ([0-9A-F]+): ", line)
                addr = int(a.group(1), 16) if a else None
                if "s_getpc_b64" in line:
                    getpc = addr + 4
                m = re.match(r"^(\s*s_add_u32 s\d+, s\d+, )0x([0-9a-f]+)(\s+// )[0-9A-F]+: ([0-9A-F]+) [0-9A-F]+$", line)
                if m and getpc is not None and addr == getpc:
                    lit = int(m.group(2), 16)
                    lit -= (1 << 32) if lit >= (1 << 31) else 0
                    line = "%s<%s>%s%s" % (m.group(1), syms.get(getpc + lit, "?"), m.group(3), m.group(4))
                else:
                    line = re.sub(r" <[^>]+>$", "", line)
                funcs[name].append(re.sub(r"// [0-9A-F]+: ", "// ", line).rstrip())
    for body in funcs.values():  # the s_nop fill behind a function's last instruction: up to the next function, or the code object's tail
        while body and re.match(r"^\s*s_nop 0\s+// BF800000$", body[-1]):
            body.pop()
    text = "".join("<%s>:\n%s\n" % (k, "\n".join(funcs[k])) for k in sorted(funcs))
    if len(sys.argv) > 2:
        open(sys.argv[2], "w").write(text)
    print("%d functions, %d kernels; kernel symbols sha256 %s; disassembly sha256 %s" % (
        len(funcs), len(kernels), hashlib.sha256("\n".join(sorted(kernels)).encode()).hexdigest()[:16], hashlib.sha256(text.encode()).hexdigest()[:16]))


if __name__ == "__main__":
    main()

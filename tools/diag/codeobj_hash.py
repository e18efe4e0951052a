"""sha256 of every gfx950 code object bundled in a libsdrgpu.so (one clang offload bundle per
translation unit), each named by the kernel families it holds: run on two builds of the library
to show which translation units' device code a change left byte-identical.  Diagnostic only.

    python tools/diag/codeobj_hash.py [path/to/libsdrgpu.so]"""
import hashlib
import os
import re
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def main():
    lib = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "unnamed-rust-sdr_amd", "libsdrgpu.so")
    with tempfile.TemporaryDirectory() as tmp:
        sec = os.path.join(tmp, "fatbin")
        subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={sec}", lib,
                        os.path.join(tmp, "copy.so")], check=True)
        data = open(sec, "rb").read()
    rows, pos = [], 0
    while (i := data.find(MAGIC, pos)) >= 0:
        n = struct.unpack_from("<Q", data, i + 24)[0]
        p = i + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", data, p)
            triple = data[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            if "gfx950" in triple and size:
                co = data[i + off:i + off + size]
                fams = sorted({m.decode() for m in re.findall(rb"_ZN6sdrgpu\w*?\d+([a-z][a-z0-9_]*_kernel)I?", co)})
                rows.append((" ".join(fams) or "(no kernels)", hashlib.sha256(co).hexdigest()[:16], size))
        pos = i + len(MAGIC)
    for fams, h, size in sorted(rows):
        print(f"{h} {size:8d} B  {fams}")


if __name__ == "__main__":
    main()

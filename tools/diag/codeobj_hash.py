"""sha256 of every gfx950 code object bundled in a libsdrgpu.so (one clang offload bundle per
translation unit), each named by the kernel families it holds: run on two builds of the library
to show which translation units' device code a change left byte-identical.  Diagnostic only.

    python tools/diag/codeobj_hash.py [path/to/libsdrgpu.so]

With --kernels, one line per kernel instead: sha256 of the kernel's machine code and of its
64-byte descriptor, so that a change which adds or drops kernels of a translation unit (and so
changes that unit's code object) can still show every remaining kernel byte-identical.

    python tools/diag/codeobj_hash.py --kernels [path/to/libsdrgpu.so]"""
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


def kernel_rows(co):
    """(mangled name, hash of code + descriptor, code bytes) of every kernel of one ELF code object."""
    assert co[:4] == b"\x7fELF" and co[4] == 2 and co[5] == 1, "not a little-endian ELF64"
    shoff, = struct.unpack_from("<Q", co, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", co, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", co, shoff + i * shentsize) for i in range(shnum)]
    symtab = next(s for s in secs if s[1] == 2)  # SHT_SYMTAB
    strtab = secs[symtab[6]]
    syms = {}
    for o in range(symtab[4], symtab[4] + symtab[5], 24):
        name_off, _, _, shndx, value, size = struct.unpack_from("<IBBHQQ", co, o)
        end = co.index(b"\0", strtab[4] + name_off)
        if 0 < shndx < shnum and size:
            sec = secs[shndx]
            syms[co[strtab[4] + name_off:end].decode()] = co[sec[4] + value - sec[3]:sec[4] + value - sec[3] + size]
    names = [n[:-3] for n in syms if n.endswith(".kd") and n[:-3] in syms]
    # the descriptor's bytes 16..23 are the distance from the descriptor to the kernel's entry: that
    # is where the kernel lies in the unit, not what it is
    return [(n, hashlib.sha256(syms[n] + syms[n + ".kd"][:16] + syms[n + ".kd"][24:]).hexdigest()[:16], len(syms[n]))
            for n in names]


def main():
    args = [a for a in sys.argv[1:] if a != "--kernels"]
    per_kernel = len(args) != len(sys.argv) - 1
    lib = args[0] if args else os.path.join(ROOT, "unnamed-rust-sdr_amd", "libsdrgpu.so")
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
                if per_kernel:
                    rows += [(name, h, n_code) for name, h, n_code in kernel_rows(co)]
                    continue
                fams = sorted({m.decode() for m in re.findall(rb"_ZN6sdrgpu\w*?\d+([a-z][a-z0-9_]*_kernel)I?", co)})
                rows.append((" ".join(fams) or "(no kernels)", hashlib.sha256(co).hexdigest()[:16], size))
        pos = i + len(MAGIC)
    for fams, h, size in sorted(rows):
        print(f"{h} {size:8d} B  {fams}")


if __name__ == "__main__":
    main()

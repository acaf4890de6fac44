#!/usr/bin/env python3
"""Kernel by kernel, do two builds of libvargeno_hip.so run the same machine code?

    python3 profiles/device_code_diff.py A/libvargeno_hip.so B/libvargeno_hip.so

device_code_sha.sh hashes the gfx950 code object's whole .text: that also changes when the same kernels are merely emitted in
another order (the order in which a translation unit first asks for its template instantiations).  This compares, per kernel symbol,
the bytes of its code and its kernel descriptor -- registers, LDS, scratch and the other launch settings; the descriptor's
kernel_code_entry_byte_offset (bytes 16-23: where the code lies relative to the descriptor) is left out.  Exit status 0: the same
kernels with the same code and settings, in whatever order."""
import hashlib
import os
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


def kernels(lib):
    with tempfile.TemporaryDirectory() as t:
        fb, co = os.path.join(t, "fb.bin"), os.path.join(t, "co.o")
        subprocess.check_call([LLVM + "/llvm-objcopy", "--dump-section", ".hip_fatbin=" + fb, lib, os.path.join(t, "discard.so")])
        subprocess.check_call([LLVM + "/clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fb, "--output=" + co, "--unbundle"])
        image = open(co, "rb").read()
        sections = {}                                   # index -> (address, file offset)
        for line in subprocess.check_output(["readelf", "-SW", co], text=True).splitlines():
            if line.lstrip().startswith("[") and "]" in line:
                f = line.split("]", 1)[1].split()
                if len(f) >= 4 and f[0].startswith("."):
                    sections[line.split("[", 1)[1].split("]", 1)[0].strip()] = (int(f[2], 16), int(f[3], 16))
        out, order = {}, []
        for line in subprocess.check_output(["readelf", "-sW", "--dyn-syms", co], text=True).splitlines():
            f = line.split()
            if len(f) < 8 or f[3] not in ("FUNC", "OBJECT") or f[6] not in sections or (f[3] == "OBJECT" and not f[7].endswith(".kd")):
                continue
            addr, off = sections[f[6]]
            start, size = off + int(f[1], 16) - addr, int(f[2], 0)
            body = bytearray(image[start:start + size])
            if f[3] == "OBJECT":
                body[16:24] = bytes(8)
            else:
                order.append((int(f[1], 16), f[7]))
            out[f[7]] = (size, hashlib.sha256(body).hexdigest())
        return out, [name for _, name in sorted(set(order))]


def main():
    (a, order_a), (b, order_b) = kernels(sys.argv[1]), kernels(sys.argv[2])
    differ = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
    print("%d kernels in A, %d in B; code bytes in all: %d and %d" % (len(order_a), len(order_b), sum(a[k][0] for k in order_a), sum(b[k][0] for k in order_b)))
    print("emission order: %s" % ("the same" if order_a == order_b else "differs (%d of %d positions)" % (sum(x != y for x, y in zip(order_a, order_b)), len(order_a))))
    for k in differ:
        print("DIFFERS  %s  A %s  B %s" % (k, a.get(k, ("absent",))[0], b.get(k, ("absent",))[0]))
    print("verdict: %s" % ("every kernel's code and descriptor byte-identical" if not differ else "%d symbols differ" % len(differ)))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())

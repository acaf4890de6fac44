#!/usr/bin/env python3
"""Plain gzip inflate, library level: vg_gunzip_device over a VG_GZ_CHUNK sweep against the host's sequential decoders.

    python3 profiles/gzip_inflate.py [text MB, default 128] > profiles/gzip_inflate.txt

A FASTQ-like text (seeded: 150-base reads, skewed qualities) is compressed by zlib at level 6 into one gzip member.  Legs, three
alternated rounds each: Python's zlib (what `zcat` does: one host thread), vg_gunzip_host (the reference decoder of vg_gunzip.h),
vg_gunzip_device at each chunk size.  The device legs' wall time includes the copy of the whole file in and of the text out; the
library's own line under VG_VERBOSE (stderr) has the stages alone.  Every leg's text is compared with zlib's."""
import os
import sys
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vargeno_amd import api, synth  # noqa: E402

CHUNKS = (8192, 16384, 32768, 65536, 131072, 262144)


def fastq_text(mb, seed=7):
    rng = np.random.default_rng(seed)
    n = mb * (1 << 20) // 330
    seq = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), (n, 150), p=[0.3, 0.2, 0.2, 0.3])
    qual = rng.choice(np.frombuffer(b"FF:,#", dtype=np.uint8), (n, 150), p=[0.7, 0.15, 0.1, 0.04, 0.01])
    out = []
    for i in range(n):
        out.append(b"@SIM:1:FCX:1:%d:%d:%d 1:N:0:ATCACG\n" % (1101 + i // 100000, 1000 + i % 9973, 2000 + (i * 7) % 9967))
        out.append(seq[i].tobytes() + b"\n+\n" + qual[i].tobytes() + b"\n")
    return b"".join(out)


def main():
    mb = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    text = fastq_text(mb)
    t0 = time.time()
    data = synth.gzip_bytes(text, level=6)
    print("text %.1f MB, gzip -6 %.1f MB (%.2f : 1), compressed in %.1f s" % (len(text) / 1e6, len(data) / 1e6, len(text) / len(data), time.time() - t0))
    legs = [("zlib (python)", None)] + [("vg_gunzip_host", "host")] + [("vg_gunzip_device chunk %d" % c, c) for c in CHUNKS]
    times = {name: [] for name, _ in legs}
    stats = {}
    api.gunzip(data[:0] + synth.gzip_bytes(text[:100000]), device=0)          # (the device and the library warmed up)
    for rnd in range(3):
        for name, how in legs:
            t0 = time.time()
            if how is None:
                got = zlib.decompress(data, 31)
            elif how == "host":
                got = api.gunzip(data, device=None, text_cap=len(text)).text
            else:
                sys.stderr.write("round %d, %s\n" % (rnd, name)); sys.stderr.flush()
                r = api.gunzip(data, device=0, chunk=how, text_cap=len(text))
                assert r.error is None and r.stats["slots_refused"] == 0, (name, r.error, r.stats)
                got, stats[name] = r.text, r.stats
            dt = time.time() - t0
            assert got == text, name
            times[name].append(dt)
    base = min(times["zlib (python)"])
    for name, _ in legs:
        t = times[name]
        print("%-34s %s s   best %.2f GB/s of text   x%.2f of zlib   %s" % (name, " ".join("%.3f" % v for v in t), len(text) / 1e9 / min(t), base / min(t),
                                                                            {k: v for k, v in stats.get(name, {}).items() if k in ("chunks", "guessed", "confirmed", "repaired", "tested")} or ""))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""BGZF output: what it costs and what it saves (writes profiles/vcf_bgzf.txt).

    python3 profiles/vcf_bgzf.py --ratio                      no GPU: compression ratio against zlib, on the golden VCF texts
    python3 profiles/vcf_bgzf.py --zip [--gb 2]               `vargeno bgzfzip` on a VCF-like text: host route and device route
    python3 profiles/vcf_bgzf.py --geno [--reads 20000000]    `vargeno geno` at chr22 scale: VARGENO_VCF_BGZF unset, host, device
    python3 profiles/vcf_bgzf.py --kernel                     the deflate kernels by their own clock (VG_VERBOSE) on 196 MB of the --zip text
  --codes fixed|dynamic|both   the coding mode(s) of --ratio (a `dynamic` column), --zip and --kernel (default fixed: what the script
                               did before the dynamic mode; profiles/vcf_bgzf_dynamic.txt was taken with `both`)

Every step that uses the GPU is a process of its own under `timeout -k 10`; the steps run one after the other and the recipe stops
at the first one that fails.  Each mode appends its section to the output file (--out), so the three can be taken in separate
sittings.
  --ratio  the host route writes the device's bytes (tests/test_gpu_deflate.py), so the file sizes need no GPU: per text, the
           size of the library's file against zlib level 1 and level 6 (and level 1 with fixed codes, the same kind of coder)
           over the same 65 280-byte blocks with the same 26 bytes of header and trailer.
  --zip    --gb gigabytes of joint-VCF-like text (a golden joint header and `\\t0/0:40` columns, drawn with a seed); text GB/s
           of `bgzfzip` from a file in memory (/dev/shm) to one, three rounds per route, the host route on the CPUs this
           process may use.  The files must be identical.
  --kernel api.bgzf_deflate(text, device=0, codes=...) three times per mode in one process with VG_VERBOSE set, on the first
           196 439 600 bytes of the --zip text (3 010 blocks): the library's own line per call.  With the dynamic mode also the
           code-length builder's kernel alone: api.deflate_code_lengths(device=0) over 3 000 and over 30 000 histograms of the
           text's own kind, whose difference (the copies and the launch cancel) bounds what the three builds per block cost.
  --geno   the set-up of profiles/bgzf_ingest.py; wall time of `geno` three times per setting, alternated.  Unset is the parent
           commit's path: the plain sink is the fwrite it was."""
import argparse
import glob
import gzip
import json
import os
import statistics
import subprocess
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BIN = os.path.join(ROOT, "vargeno_amd", "csrc", "vargeno")
BLOCK = 65280


def zlib_size(text, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    total = 28
    for at in range(0, len(text), BLOCK):
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
        total += len(c.compress(text[at:at + BLOCK]) + c.flush()) + 26
    return total


def ratio(lines, codes=("fixed",)):
    from vargeno_amd import api

    dyn = "dynamic" in codes
    lines.append("## compression ratio (file bytes / text bytes; blocks of 65 280 bytes), host route = device route byte for byte")
    cols = ["ours"] + (["dynamic"] if dyn else []) + ["z1fixed", "zlib1", "zlib6"]
    fmt = "%-28s %10d" + " %8.3f" * len(cols)
    lines.append(("%-28s %10s" + " %8s" * len(cols)) % (("text", "bytes") + tuple(cols)))
    tot = np.zeros(1 + len(cols))
    for f in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "*.vcf.gz"))):
        text = gzip.open(f, "rb").read()
        sizes = [len(api.bgzf_deflate(text))] + ([len(api.bgzf_deflate(text, codes="dynamic"))] if dyn else []) + [zlib_size(text, 1, zlib.Z_FIXED), zlib_size(text, 1), zlib_size(text, 6)]
        tot += [len(text)] + sizes
        lines.append(fmt % ((os.path.basename(f), len(text)) + tuple(s / len(text) for s in sizes)))
    lines.append(fmt % (("all",  int(tot[0])) + tuple(s / tot[0] for s in tot[1:])))


def joint_like_text(path, gb, samples=200, seed=3):
    """A joint VCF's shape: a header, then records of eight fields, GT:GQ and a column per sample.  64 MB of records are drawn and
    written again and again (a repeat 64 MB away is beyond every window: the ratio is that of the 64 MB)."""
    rng = np.random.default_rng(seed)
    gts = [b"0/0", b"0/1", b"1/1", b"./."]
    rows, pos, size = [], 0, 0
    while size < 64e6:
        g = rng.choice(4, size=(2000, samples), p=[0.8, 0.12, 0.06, 0.02]).tolist()
        q = rng.integers(3, 99, size=(2000, samples)).tolist()
        for gr, qr in zip(g, q):
            pos += int(rng.integers(1, 3000))
            cols = b"\t".join(gts[gi] + (b":." if gi == 3 else b":%d" % qi) for gi, qi in zip(gr, qr))
            rows.append(b"chr22\t%d\trs%d\t%s\t%s\t.\t.\t.\tGT:GQ\t" % (pos, pos * 7 % 99999989, b"ACGT"[pos % 4:pos % 4 + 1], b"CGTA"[pos % 4:pos % 4 + 1]) + cols + b"\n")
            size += len(rows[-1])
    unit = b"".join(rows)
    with open(path, "wb") as f:
        f.write(b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + b"\t".join(b"S%03d" % i for i in range(samples)) + b"\n")
        for _ in range(max(1, int(gb * 1e9 / len(unit)))):
            f.write(unit)
    return os.path.getsize(path)


def timed(cmd, env, limit):
    """One GPU step: a process of its own under `timeout -k 10`.  Returns (seconds, stderr); raises when it fails."""
    t0 = time.time()
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, env=env, capture_output=True, text=True)
    if p.returncode != 0:
        raise SystemExit("step failed (%d), the recipe stops here: %s\n%s" % (p.returncode, " ".join(cmd), p.stderr[-2000:]))
    return time.time() - t0, p.stderr


def zip_rates(lines, a, codes="fixed"):
    d = a.workdir
    os.makedirs(d, exist_ok=True)
    src = os.path.join(d, "joint_like.vcf")
    if not os.path.exists(src) or os.path.getsize(src) < a.gb * 1e9:
        joint_like_text(src, a.gb)
    n = os.path.getsize(src)
    cpus = len(os.sched_getaffinity(0))
    lines.append("## bgzfzip, %.2f GB of joint-VCF-like text, %s codes, host route on VARGENO_BGZF_THREADS=%d" % (n / 1e9, codes, min(cpus, 16)))
    res, size = {"host": [], "device": []}, {}
    for rnd in range(a.rounds):
        for route in ("host", "device"):
            dst = os.path.join(d, "out.%s.vcf.gz" % route)
            env = dict(os.environ, VARGENO_VCF_BGZF=route, VARGENO_VCF_CODES=codes, VARGENO_BGZF_THREADS=str(min(cpus, 16)), VARGENO_VERBOSE="1")
            s, err = timed([BIN, "bgzfzip", src, dst], env, a.leg_timeout)
            res[route].append(round(n / 1e9 / s, 3))
            size[route] = os.path.getsize(dst)
            lines.append(json.dumps(dict(round=rnd, route=route, codes=codes, wall_s=round(s, 3), text_GBps=res[route][-1], said=[ln for ln in err.splitlines() if "bgzfzip" in ln][:1])))
            print(lines[-1], flush=True)
    same = subprocess.run(["cmp", os.path.join(d, "out.host.vcf.gz"), os.path.join(d, "out.device.vcf.gz")]).returncode == 0
    lines.append("files identical: %s; %d bytes, ratio %.3f" % (same, size["host"], size["host"] / n))
    lines.append("median text GB/s: host %.3f, device %.3f" % (statistics.median(res["host"]), statistics.median(res["device"])))
    assert same


KERNEL_STEP = """
import sys
import numpy as np
sys.path.insert(0, %r)
from vargeno_amd import api
import time
text = open(%r, "rb").read(196439600)
for codes in %r:
    for _ in range(3):
        api.bgzf_deflate(text, device=0, codes=codes)
if "dynamic" in %r:
    # histograms of the text's own kind: byte counts of its blocks, a few length symbols, the end-of-block symbol
    a = np.frombuffer(text, dtype=np.uint8)[:3000 * 65280].reshape(3000, 65280)
    h = np.zeros((3000, 286), dtype=np.uint32)
    for i in range(3000):
        h[i, :256] = np.bincount(a[i], minlength=256)
    h[:, 256] = 1
    h[:, 258:286] = (np.arange(28) * 37 %% 23 + 1)[None, :]
    big = np.tile(h, (10, 1))
    for name, f in (("3000", h), ("30000", big)):
        api.deflate_code_lengths(f, device=0)
        t = []
        for _ in range(3):
            t0 = time.perf_counter(); api.deflate_code_lengths(f, device=0); t.append(time.perf_counter() - t0)
        sys.stderr.write("code lengths alone, %%s histograms of 286 symbols, copies included: %%s ms\\n" %% (name, ", ".join("%%.3f" %% (x * 1e3) for x in t)))
"""


def kernel_clock(lines, a, codes):
    src = os.path.join(a.workdir, "joint_like.vcf")
    if not os.path.exists(src) or os.path.getsize(src) < 196439600:
        os.makedirs(a.workdir, exist_ok=True)
        joint_like_text(src, 0.2)
    lines.append("## the deflate kernels by their own clock: VG_VERBOSE=1, api.bgzf_deflate(text, device=0, codes=...) three times each on 196 439 600 bytes of the --zip text")
    _, err = timed([sys.executable, "-c", KERNEL_STEP % (ROOT, src, tuple(codes), tuple(codes))], dict(os.environ, VG_VERBOSE="1"), a.leg_timeout)
    lines.extend(ln for ln in err.splitlines() if "bgzf deflate:" in ln or "code lengths alone" in ln)


def geno_walls(lines, a):
    from profiles.cohort_bench import write_fastq_fixed
    from vargeno_amd import synth

    d = a.workdir
    os.makedirs(d, exist_ok=True)
    if not os.path.exists(d + "/idx.done"):
        g, s, r = synth.chr22_scale(n_reads=a.reads)
        synth.write_fasta(d + "/ref.fa", g)
        synth.write_vcf(d + "/snps.vcf", g, s)
        subprocess.check_call([BIN, "index", "ref.fa", "snps.vcf", "idx"], cwd=d, env=dict(os.environ, VARGENO_NO_LITE="1"), stdout=subprocess.DEVNULL)
        write_fastq_fixed(d + "/reads.fq", r, 0, a.reads)
        open(d + "/idx.done", "w").close()
    lines.append("## geno at chr22 scale, %d reads: wall seconds, and the call/VCF phase of the verbose report" % a.reads)
    res = {"unset": [], "host": [], "device": []}
    for rnd in range(a.rounds):
        for route in res:
            env = dict({k: v for k, v in os.environ.items() if k != "VARGENO_VCF_BGZF"}, VARGENO_MAX_DEVICE_GB="10", VARGENO_VERBOSE="1")
            if route != "unset":
                env["VARGENO_VCF_BGZF"] = route
            s, err = timed([BIN, "geno", d + "/idx", d + "/reads.fq", d + "/snps.vcf", d + "/out.%s.vcf" % route], env, a.leg_timeout)
            vcf = [float(ln.split("call/VCF")[1].split()[0]) for ln in err.splitlines() if "call/VCF" in ln]
            res[route].append(dict(wall_s=round(s, 3), call_vcf_s=vcf[0] if vcf else None))
            lines.append(json.dumps(dict(round=rnd, route=route, **res[route][-1])))
            print(lines[-1], flush=True)
    plain = open(d + "/out.unset.vcf", "rb").read()
    for route in ("host", "device"):
        assert gzip.decompress(open(d + "/out.%s.vcf" % route, "rb").read()) == plain, route
    lines.append("both BGZF files inflate to the plain file; median wall s: " + json.dumps({k: statistics.median(x["wall_s"] for x in v) for k, v in res.items()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ratio", action="store_true")
    ap.add_argument("--zip", action="store_true")
    ap.add_argument("--geno", action="store_true")
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--codes", choices=["fixed", "dynamic", "both"], default="fixed")
    ap.add_argument("--gb", type=float, default=2.0)
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--leg-timeout", type=float, default=240.0)
    ap.add_argument("--workdir", default="/dev/shm/vg_vcf_bgzf")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vcf_bgzf.txt"))
    a = ap.parse_args()
    lines = ["# profiles/vcf_bgzf.py %s, %s" % (" ".join(sys.argv[1:]), time.strftime("%Y-%m-%d"))]
    try:
        codes = ("fixed", "dynamic") if a.codes == "both" else (a.codes,)
        if a.ratio:
            ratio(lines, codes)
        if a.zip:
            for c in codes:
                zip_rates(lines, a, c)
        if a.kernel:
            kernel_clock(lines, a, codes)
        if a.geno:
            geno_walls(lines, a)
    finally:
        text = "\n".join(lines) + "\n"
        print(text)
        with open(a.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""BAM ingest against text and BGZF FASTQ (writes profiles/bam_ingest.txt).  NOT RUN YET: nothing about the speed of the BAM routes
has been measured; whoever next has a device lease runs this, and the default route for BAM stays `host` until its record exists.

    python3 profiles/bam_ingest.py [--reads 1000000] [--workdir DIR] [--out profiles/bam_ingest.txt]

The chr22-scale index (BASELINE.json configs[1]: 40 Mbp, 1 M SNPs) under a 10 GB device budget -- the set-up of
profiles/bgzf_ingest.py --, and the SAME `--reads` reads of 150 bp as FASTQ text, as BGZF FASTQ, and as unaligned BAM in both writer
styles: `aligned` (no record straddles a BGZF block: htslib) and `spanning` (blocks of 65 280 bytes cut regardless of records:
htsjdk).  Three rounds, alternated, every leg under its own time limit, `vargeno geno` on
  a  the text file
  b  the BGZF FASTQ, VARGENO_BGZF=device            c  the BGZF FASTQ, VARGENO_BGZF=host
  d  the aligned BAM, VARGENO_BGZF=device           e  the aligned BAM, VARGENO_BGZF=host
  f  the spanning BAM, VARGENO_BGZF=device          g  the spanning BAM, VARGENO_BGZF=host
Recorded per leg: wall, the verbose "FASTQ->counters" seconds, reads/s, and the route's own "ingest" line (for BAM: records kept,
skipped, window repairs).  All VCFs must be identical.  The comparison that matters is d / f against b, in the same run: BAM on the
device against the parent feature's BGZF FASTQ on the device.  No threshold is set.
Then the kernels alone, in a process of their own: vg_bam_frame_device on the whole blocks of the first 24 MiB of the spanning BAM
file (compressed bytes) with VG_VERBOSE set, whose HIP events give TWO times, which are written into the record: the inflate
kernel's, and "framing + gather" -- walk, confirm, repair, lengths, the scans and gather together.  This script does NOT split the
second figure into walk and gather, and the record it writes says so: that split is the profiler's,
`rocprofv3 --kernel-trace --stats -- python3 profiles/bam_ingest.py --kernel-only`, a run of its own (vg_bgzf_inflate_kernel,
vg_bam_walk_windows, vg_bam_gather), whose table is to be appended to profiles/bam_ingest.txt by hand."""
import argparse
import json
import os
import statistics
import struct
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vargeno_amd import synth  # noqa: E402

BIN = os.path.join(ROOT, "vargeno_amd", "csrc", "vargeno")
CODE = {c: i for i, c in enumerate("=ACMGRSVTWYHKDBN")}
PAIR = {(a + b).encode(): bytes([CODE[a] << 4 | CODE[b]]) for a in CODE for b in CODE}


def bam_header():
    text = b"@HD\tVN:1.6\tSO:unsorted\n"
    return b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", 0)


def bam_records(fq_path):
    """One unaligned record (flag 4) per FASTQ record, as `samtools import` would make it."""
    with open(fq_path, "rb") as f:
        while True:
            name = f.readline()
            if not name:
                return
            seq, _, qual = f.readline().rstrip(b"\n").upper(), f.readline(), f.readline().rstrip(b"\n")
            name = name[1:].rstrip(b"\n") + b"\x00"
            padded = seq + b"=" if len(seq) & 1 else seq
            packed = b"".join(PAIR[padded[i:i + 2]] for i in range(0, len(padded), 2))
            body = struct.pack("<iiBBHHHiiii", -1, -1, len(name), 0, 4680, 0, 4, len(seq), -1, -1, 0) + name + packed + bytes(c - 33 for c in qual)
            yield struct.pack("<I", len(body)) + body


def _block(piece):
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    return synth.bgzf_block(co.compress(piece) + co.flush(), zlib.crc32(piece), len(piece))


def write_bam(fq_path, out_path, style):
    with open(out_path, "wb") as out:
        cur = bam_header()
        if style == "aligned":
            out.write(_block(cur))
            cur = b""
        for r in bam_records(fq_path):
            if style == "aligned":
                if len(cur) + len(r) > 65280:
                    out.write(_block(cur))
                    cur = b""
                cur += r
            else:
                cur += r
                while len(cur) >= 65280:
                    out.write(_block(cur[:65280]))
                    cur = cur[65280:]
        if cur:
            out.write(_block(cur))
        out.write(synth.BGZF_EOF)


def kernels_alone(bam_path, lines):
    """--kernel-only: frames the whole blocks of the file's first 24 MiB; the library's timing line goes to stderr."""
    from vargeno_amd import api

    data = open(bam_path, "rb").read(24 << 20)
    blocks, used, _ = api.bgzf_scan(data)
    os.environ["VG_VERBOSE"] = "1"
    off, bases, gate, stats, bad = api.bam_frame(data[:used] + synth.BGZF_EOF, device=0)      # (the file is cut at a block: its last record may be cut)
    lines.append("kernels alone: %d blocks, %d inflated bytes, %d records, %d repairs" % (len(blocks), sum(b[4] for b in blocks), len(gate), stats[3]))


def kernels_alone_record(workdir, lines, timeout):
    """The --kernel-only leg as a child process, its figures and the library's timing line copied into the record."""
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--kernel-only", "--workdir", workdir], capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-2000:]
    lines.extend(ln for ln in p.stdout.splitlines() if ln.startswith("kernels alone"))
    lines.extend(ln for ln in p.stderr.splitlines() if "bam frame:" in ln)
    lines.append("(HIP events: the inflate kernel, and framing + gather as ONE figure.  The split into walk and gather is not in this record: "
                 "it needs `rocprofv3 --kernel-trace --stats -- python3 profiles/bam_ingest.py --kernel-only`, a run of its own.)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--workdir", default="/tmp/vg_bam_bench")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bam_ingest.txt"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--leg-timeout", type=float, default=240.0)
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    d = a.workdir
    os.makedirs(d, exist_ok=True)
    lines = ["# profiles/bam_ingest.py --reads %d, %s" % (a.reads, time.strftime("%Y-%m-%d"))]
    t0 = time.time()
    fq, bz = d + "/reads.fq", d + "/reads.fq.gz"
    bams = {"aligned": d + "/reads.aligned.bam", "spanning": d + "/reads.spanning.bam"}
    if not os.path.exists(d + "/idx.done"):
        from profiles.bgzf_ingest import write_bgzf
        from profiles.cohort_bench import write_fastq_fixed

        g, s, r = synth.chr22_scale(n_reads=a.reads)
        synth.write_fasta(d + "/ref.fa", g)
        synth.write_vcf(d + "/snps.vcf", g, s)
        subprocess.check_call([BIN, "index", "ref.fa", "snps.vcf", "idx"], cwd=d, env=dict(os.environ, VARGENO_NO_LITE="1"), stdout=subprocess.DEVNULL)
        write_fastq_fixed(fq, r, 0, a.reads)
        del g, s, r
        write_bgzf(fq, bz)
        for style, path in bams.items():
            write_bam(fq, path, style)
        open(d + "/idx.done", "w").close()
    lines.append("# set-up %.0f s: %d reads, %.2f GB of text, %.2f GB as BGZF FASTQ, %.2f / %.2f GB as BAM (aligned / spanning)" % (
        time.time() - t0, a.reads, os.path.getsize(fq) / 1e9, os.path.getsize(bz) / 1e9, os.path.getsize(bams["aligned"]) / 1e9, os.path.getsize(bams["spanning"]) / 1e9))
    if a.kernel_only:
        kernels_alone(bams["spanning"], lines)
        print("\n".join(lines))
        return
    env = dict(os.environ, VARGENO_MAX_DEVICE_GB="10", VARGENO_VERBOSE="1")
    legs = [("a_text", fq, {}), ("b_bgzf_device", bz, {"VARGENO_BGZF": "device"}), ("c_bgzf_host", bz, {"VARGENO_BGZF": "host"}),
            ("d_bam_aligned_device", bams["aligned"], {"VARGENO_BGZF": "device"}), ("e_bam_aligned_host", bams["aligned"], {"VARGENO_BGZF": "host"}),
            ("f_bam_spanning_device", bams["spanning"], {"VARGENO_BGZF": "device"}), ("g_bam_spanning_host", bams["spanning"], {"VARGENO_BGZF": "host"})]
    res = {name: [] for name, _, _ in legs}
    vcfs = {}
    for rnd in range(a.rounds):
        for name, path, extra in legs:
            out = d + "/%s.vcf" % name
            t1 = time.time()
            p = subprocess.run([BIN, "geno", d + "/idx", path, d + "/snps.vcf", out], env=dict(env, **extra), capture_output=True, text=True, timeout=a.leg_timeout)
            wall = time.time() - t1
            assert p.returncode == 0, (name, p.stderr[-2000:])
            f2c = [float(ln.split("FASTQ->counters")[1].split()[0]) for ln in p.stderr.splitlines() if "FASTQ->counters" in ln]
            ingest = [ln for ln in p.stderr.splitlines() if ln.startswith("ingest")]
            res[name].append(dict(wall_s=round(wall, 3), fastq_to_counters_s=f2c[0] if f2c else None, reads_per_s=round(a.reads / f2c[0]) if f2c and f2c[0] else None, ingest=ingest[:1]))
            vcfs[name] = open(out, "rb").read()
            lines.append(json.dumps(dict(round=rnd, leg=name, **res[name][-1])))
            print(lines[-1], flush=True)
    same = all(v == vcfs["a_text"] for v in vcfs.values())
    lines.append("all VCFs identical: %s" % same)
    med = {k: statistics.median(x["fastq_to_counters_s"] for x in v) for k, v in res.items()}
    lines.append("median FASTQ->counters s: " + json.dumps(med))
    lines.append("BAM on the device against BGZF FASTQ on the device (same run): aligned %.3f s, spanning %.3f s, BGZF FASTQ %.3f s" % (med["d_bam_aligned_device"], med["f_bam_spanning_device"], med["b_bgzf_device"]))
    kernels_alone_record(d, lines, a.leg_timeout)
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.out, "w") as f:
        f.write(text)
    assert same


if __name__ == "__main__":
    main()

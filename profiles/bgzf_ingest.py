#!/usr/bin/env python3
"""BGZF ingest against text and against `<(zcat file)` (writes profiles/bgzf_ingest.txt).

    python3 profiles/bgzf_ingest.py [--reads 50000000] [--workdir DIR] [--parent-bin PATH] [--out profiles/bgzf_ingest.txt]

The chr22-scale index (BASELINE.json configs[1]: 40 Mbp, 1 M SNPs) under a 10 GB device budget -- the set-up of
profiles/cohort_bench.py --, `--reads` reads of 150 bp as FASTQ text and as BGZF (vargeno_amd.synth.bgzf_bytes on 16 processes).
Three rounds, alternated, every leg under its own time limit:
  a  `vargeno geno` on the text file
  b  on the BGZF file, VARGENO_BGZF=device
  c  on the BGZF file, VARGENO_BGZF=host
  d  `geno ... <(zcat file)` with the binary of the parent commit (--parent-bin: a build of the parent beside this tree; it knows
     no other way to read a .gz), and the parent's `geno` on the text file (a'), for the text route's own before / after
Recorded per leg: wall and the verbose "FASTQ->counters" seconds; all VCFs must be identical.  Then the inflate kernel alone:
vg_bgzf_inflate_device on 256 MiB of text with VG_VERBOSE set (HIP events around the warmed kernel), beside vg_link_rate.
(`rocprofv3 --kernel-trace --stats -- python3 profiles/bgzf_ingest.py --kernel-only` is the profiler's view, a run of its own.)
The default of VARGENO_BGZF is whichever of b and c has the lower median FASTQ->counters time; it must not be slower than d."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vargeno_amd import synth  # noqa: E402

BIN = os.path.join(ROOT, "vargeno_amd", "csrc", "vargeno")


def _compress_piece(args):
    path, lo, hi = args
    with open(path, "rb") as f:
        f.seek(lo)
        return synth.bgzf_bytes(f.read(hi - lo), eof=False)


def write_bgzf(text_path, out_path, piece=64 * 65280, workers=16):
    n = os.path.getsize(text_path)
    jobs = [(text_path, lo, min(n, lo + piece)) for lo in range(0, n, piece)]
    with ProcessPoolExecutor(workers) as ex, open(out_path, "wb") as out:
        for blob in ex.map(_compress_piece, jobs, chunksize=4):
            out.write(blob)
        out.write(synth.BGZF_EOF)


def kernel_alone(text_path, lines):
    from vargeno_amd import api
    from vargeno_amd._lib import lib

    with open(text_path, "rb") as f:
        text = f.read(256 << 20)
    data = b"".join(synth.bgzf_bytes(text[a:a + (8 << 20)], eof=False) for a in range(0, len(text), 8 << 20))
    os.environ["VG_VERBOSE"] = "1"
    got, used, bad = api.bgzf_inflate(data, device=0)              # (the kernel's line goes to stderr: 3 rounds, the last is reported)
    assert bad is None and got == text
    lines.append("kernel alone: %d bytes of text, %d compressed; link rate %.2f GB/s (vg_link_rate); the kernel's own line is on stderr" % (len(text), len(data), lib().vg_link_rate(0) / 1e9))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("--workdir", default="/tmp/vg_bgzf_bench")
    ap.add_argument("--parent-bin", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bgzf_ingest.txt"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--leg-timeout", type=float, default=240.0)
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    d = a.workdir
    os.makedirs(d, exist_ok=True)
    lines = ["# profiles/bgzf_ingest.py --reads %d, %s" % (a.reads, time.strftime("%Y-%m-%d"))]
    t0 = time.time()
    fq, bz = d + "/reads.fq", d + "/reads.fq.gz"
    if not os.path.exists(d + "/idx.done") or not os.path.exists(bz):
        from profiles.cohort_bench import write_fastq_fixed

        g, s, r = synth.chr22_scale(n_reads=a.reads)
        synth.write_fasta(d + "/ref.fa", g)
        synth.write_vcf(d + "/snps.vcf", g, s)
        subprocess.check_call([BIN, "index", "ref.fa", "snps.vcf", "idx"], cwd=d, env=dict(os.environ, VARGENO_NO_LITE="1"), stdout=subprocess.DEVNULL)
        write_fastq_fixed(fq, r, 0, a.reads)
        del g, s, r
        write_bgzf(fq, bz)
        open(d + "/idx.done", "w").close()
    lines.append("# set-up %.0f s: %d reads, %.2f GB of text, %.2f GB as BGZF" % (time.time() - t0, a.reads, os.path.getsize(fq) / 1e9, os.path.getsize(bz) / 1e9))
    if a.kernel_only:
        kernel_alone(fq, lines)
        print("\n".join(lines))
        return
    env = dict(os.environ, VARGENO_MAX_DEVICE_GB="10", VARGENO_VERBOSE="1")
    legs = [("a_text", BIN, fq, {}), ("b_bgzf_device", BIN, bz, {"VARGENO_BGZF": "device"}), ("c_bgzf_host", BIN, bz, {"VARGENO_BGZF": "host"})]
    if a.parent_bin:
        legs += [("d_parent_zcat", a.parent_bin, None, {}), ("a_parent_text", a.parent_bin, fq, {})]
    res = {name: [] for name, _, _, _ in legs}
    vcfs = {}
    for rnd in range(a.rounds):
        for name, binary, path, extra in legs:
            out = d + "/%s.vcf" % name
            if path is None:
                cmd = ["bash", "-c", '"$0" geno "$1" <(zcat "$2") "$3" "$4"', binary, d + "/idx", bz, d + "/snps.vcf", out]
            else:
                cmd = [binary, "geno", d + "/idx", path, d + "/snps.vcf", out]
            t1 = time.time()
            p = subprocess.run(cmd, env=dict(env, **extra), capture_output=True, text=True, timeout=a.leg_timeout)
            wall = time.time() - t1
            assert p.returncode == 0, (name, p.stderr[-2000:])
            f2c = [float(ln.split("FASTQ->counters")[1].split()[0]) for ln in p.stderr.splitlines() if "FASTQ->counters" in ln]
            ingest = [ln for ln in p.stderr.splitlines() if ln.startswith("ingest")]
            res[name].append(dict(wall_s=round(wall, 3), fastq_to_counters_s=f2c[0] if f2c else None, ingest=ingest[:1]))
            vcfs[name] = open(out, "rb").read()
            lines.append(json.dumps(dict(round=rnd, leg=name, **res[name][-1])))
            print(lines[-1], flush=True)
    same = all(v == vcfs["a_text"] for v in vcfs.values())
    lines.append("all VCFs identical: %s" % same)
    med = {k: statistics.median(x["fastq_to_counters_s"] for x in v) for k, v in res.items()}
    lines.append("median FASTQ->counters s: " + json.dumps(med))
    pick = "device" if med["b_bgzf_device"] <= med["c_bgzf_host"] else "host"
    lines.append("VARGENO_BGZF default by this record: %s (b: %s; c: %s)" % (pick, [x["fastq_to_counters_s"] for x in res["b_bgzf_device"]], [x["fastq_to_counters_s"] for x in res["c_bgzf_host"]]))
    if a.parent_bin:
        chosen = med["b_bgzf_device" if pick == "device" else "c_bgzf_host"]
        lines.append("chosen route %.3f s against the parent's <(zcat) %.3f s: %s" % (chosen, med["d_parent_zcat"], "not slower" if chosen <= med["d_parent_zcat"] else "SLOWER: the feature has failed its purpose"))
        lines.append("text route, this tree %.3f s against the parent %.3f s" % (med["a_text"], med["a_parent_text"]))
    kernel_alone(fq, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.out, "w") as f:
        f.write(text)
    assert same


if __name__ == "__main__":
    main()

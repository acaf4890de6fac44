#!/usr/bin/env python3
"""Plain gzip ingest against text, `<(zcat file)` and BGZF (writes profiles/gzip_ingest.txt).  Not run yet: DESIGN.md §7.

    python3 profiles/gzip_ingest.py [--reads 50000000] [--workdir DIR] [--chunks 8192,16384,32768,65536] [--out profiles/gzip_ingest.txt]

The chr22-scale index (BASELINE.json configs[1]: 40 Mbp, 1 M SNPs) under a 10 GB device budget -- the set-up of
profiles/bgzf_ingest.py, whose work directory it can share --, `--reads` reads of 150 bp as FASTQ text, as one gzip -6 member
(`gzip -6 -c`, what sequencers and archives write) and as BGZF.  Three rounds, alternated, every leg under its own time limit:
  a  `vargeno geno` on the text file
  b  `geno ... <(zcat file)`: the only way in before VARGENO_GZIP, the baseline
  c  on the gzip file, VARGENO_GZIP=host
  d  on the gzip file, VARGENO_GZIP=device, once per VG_GZ_CHUNK value of --chunks
  e  on the BGZF file, VARGENO_BGZF=device
Recorded per leg: wall and the verbose "FASTQ->counters" seconds, the route's "ingest" line (the stream's statistics for d); all
VCFs must be identical.  The record then names the chunk value with the lowest median for d, d and c against b with the spread of
the rounds, and which VARGENO_GZIP value a follow-up should make the default (none, if neither beats b).
The kernels' own times are a run of their own, with the program that does the GPU work itself behind the profiler's `--`:
`--kernels-only` prepares the files and prints that command (one `geno` with VARGENO_GZIP=device at the default chunk), to be
run as
    VARGENO_GZIP=device VARGENO_MAX_DEVICE_GB=10 rocprofv3 --kernel-trace --stats -- <the printed command>
(the profiler's table has the vg_gz_* rows)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vargeno_amd import synth  # noqa: E402

BIN = os.path.join(ROOT, "vargeno_amd", "csrc", "vargeno")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("--workdir", default="/tmp/vg_gzip_bench")
    ap.add_argument("--chunks", default="8192,16384,32768,65536")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gzip_ingest.txt"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--leg-timeout", type=float, default=600.0)
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    d = a.workdir
    os.makedirs(d, exist_ok=True)
    lines = ["# profiles/gzip_ingest.py --reads %d, %s" % (a.reads, time.strftime("%Y-%m-%d"))]
    t0 = time.time()
    fq, gz, bz = d + "/reads.fq", d + "/reads.plain.fq.gz", d + "/reads.fq.gz"
    if not os.path.exists(d + "/idx.done"):
        from profiles.cohort_bench import write_fastq_fixed

        g, s, r = synth.chr22_scale(n_reads=a.reads)
        synth.write_fasta(d + "/ref.fa", g)
        synth.write_vcf(d + "/snps.vcf", g, s)
        subprocess.check_call([BIN, "index", "ref.fa", "snps.vcf", "idx"], cwd=d, env=dict(os.environ, VARGENO_NO_LITE="1"), stdout=subprocess.DEVNULL)
        write_fastq_fixed(fq, r, 0, a.reads)
        del g, s, r
        open(d + "/idx.done", "w").close()
    if not os.path.exists(gz):
        with open(gz + ".tmp", "wb") as out:
            subprocess.check_call(["gzip", "-6", "-c", fq], stdout=out)
        os.rename(gz + ".tmp", gz)
    if not os.path.exists(bz):
        from profiles.bgzf_ingest import write_bgzf

        write_bgzf(fq, bz)
    lines.append("# set-up %.0f s: %d reads, %.2f GB of text, %.2f GB as gzip -6, %.2f GB as BGZF" % (time.time() - t0, a.reads, os.path.getsize(fq) / 1e9, os.path.getsize(gz) / 1e9, os.path.getsize(bz) / 1e9))
    env = dict(os.environ, VARGENO_MAX_DEVICE_GB="10", VARGENO_VERBOSE="1")
    env.pop("VARGENO_GZIP", None)
    if a.kernels_only:
        print("\n".join(lines))
        print(" ".join([BIN, "geno", d + "/idx", gz, d + "/snps.vcf", d + "/kernels.vcf"]))
        return
    chunks = [int(c) for c in a.chunks.split(",")]
    legs = [("a_text", fq, {}), ("b_zcat", None, {}), ("c_gzip_host", gz, {"VARGENO_GZIP": "host"})]
    legs += [("d_gzip_device_%d" % c, gz, {"VARGENO_GZIP": "device", "VG_GZ_CHUNK": str(c)}) for c in chunks]
    legs += [("e_bgzf_device", bz, {"VARGENO_BGZF": "device"})]
    res = {name: [] for name, _, _ in legs}
    vcfs = {}
    for rnd in range(a.rounds):
        for name, path, extra in legs:
            out = d + "/%s.vcf" % name
            if path is None:
                cmd = ["bash", "-c", '"$0" geno "$1" <(zcat "$2") "$3" "$4"', BIN, d + "/idx", gz, d + "/snps.vcf", out]
            else:
                cmd = [BIN, "geno", d + "/idx", path, d + "/snps.vcf", out]
            t1 = time.time()
            p = subprocess.run(cmd, env=dict(env, **extra), capture_output=True, text=True, timeout=a.leg_timeout)
            wall = time.time() - t1
            assert p.returncode == 0, (name, p.stderr[-2000:])
            f2c = [float(ln.split("FASTQ->counters")[1].split()[0]) for ln in p.stderr.splitlines() if "FASTQ->counters" in ln]
            ingest = [ln for ln in p.stderr.splitlines() if ln.startswith("ingest")]
            res[name].append(dict(wall_s=round(wall, 3), fastq_to_counters_s=f2c[0] if f2c else None, ingest=ingest[:2]))
            vcfs[name] = open(out, "rb").read()
            lines.append(json.dumps(dict(round=rnd, leg=name, **res[name][-1])))
            print(lines[-1], flush=True)
    same = all(v == vcfs["a_text"] for v in vcfs.values())
    lines.append("all VCFs identical: %s" % same)
    times = {k: [x["fastq_to_counters_s"] for x in v] for k, v in res.items()}
    med = {k: statistics.median(v) for k, v in times.items()}
    lines.append("median FASTQ->counters s: " + json.dumps(med))
    lines.append("spread of the rounds (min, max): " + json.dumps({k: (min(v), max(v)) for k, v in times.items()}))
    best = min(chunks, key=lambda c: med["d_gzip_device_%d" % c])
    d_best = med["d_gzip_device_%d" % best]
    lines.append("VG_GZ_CHUNK with the lowest median for leg d: %d (%.3f s)" % (best, d_best))
    lines.append("d / b = %.2f, c / b = %.2f (below 1: faster than <(zcat file))" % (d_best / med["b_zcat"], med["c_gzip_host"] / med["b_zcat"]))
    route, t = min((("device", d_best), ("host", med["c_gzip_host"])), key=lambda x: x[1])
    lines.append("VARGENO_GZIP default a follow-up should make: %s" % (route if t < med["b_zcat"] else "none -- neither route beats <(zcat file) here"))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.out, "w") as f:
        f.write(text)
    assert same


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What `vargeno cohort` buys over one `vargeno geno` per sample (profiles/cohort_r08.txt).

    python3 profiles/cohort_bench.py [--samples 8] [--reads 1000000] [--workdir DIR] [--out FILE]

The chr22-scale index (BASELINE.json configs[1]: 40 Mbp, 1 M SNPs) under a 10 GB device budget, `--samples` samples of `--reads`
150 bp reads each, as files.
  A  one `vargeno geno` per sample, one after the other: every run opens the index (the only way before sample planes)
  B  one `vargeno cohort` with VARGENO_COHORT_INFLIGHT = 1, 4 and the number of samples
  C  the samples through FIFOs throttled to ~300 MB/s each (a decompressor's rate): `geno` per sample one after the other, and one
     `cohort` with every sample in flight
Every variant must write the same VCFs.  One JSON object per variant on stdout and in --out."""
import argparse
import json
import os
import subprocess
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vargeno_amd import synth  # noqa: E402

BIN = os.path.join(ROOT, "vargeno_amd", "csrc", "vargeno")


def write_fastq_fixed(path, r, lo, hi):
    """Reads [lo, hi) of r, all of one length, as FASTQ text (built as one byte matrix: a Python loop per read takes minutes)."""
    o = r.offsets.astype(np.int64)
    n, L = hi - lo, int(o[lo + 1] - o[lo])
    assert np.all(o[lo + 1:hi + 1] - o[lo:hi] == L)
    ids = np.frombuffer(b"".join(b"@r%08d\n" % i for i in range(n)), dtype=np.uint8).reshape(n, 11)
    rec = np.empty((n, 11 + L + 3 + L + 1), np.uint8)
    rec[:, :11] = ids
    rec[:, 11:11 + L] = r.bases[o[lo]:o[hi]].reshape(n, L)
    rec[:, 11 + L:14 + L] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    rec[:, 14 + L:14 + 2 * L] = r.quals[o[lo]:o[hi]].reshape(n, L)
    rec[:, -1] = 10
    with open(path, "wb") as f:
        f.write(rec.tobytes())


def throttled_feeder(src, fifo, rate):
    def run():
        piece = 1 << 20
        t0, sent = time.time(), 0
        try:
            with open(src, "rb") as f, open(fifo, "wb", buffering=0) as w:
                while True:
                    b = f.read(piece)
                    if not b:
                        break
                    w.write(b)
                    sent += len(b)
                    ahead = sent / rate - (time.time() - t0)
                    if ahead > 0:
                        time.sleep(ahead)
        except BrokenPipeError:
            pass
    t = threading.Thread(target=run)
    t.start()
    return t


def sample_seconds(stderr):
    out = {}
    for ln in stderr.splitlines():
        if ln.startswith("sample, line"):
            out[int(ln.split()[2].rstrip(":"))] = float(ln.split("open -> VCF:")[1].split()[0])
    return [out[k] for k in sorted(out)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--workdir", default="/tmp/vg_cohort_bench")
    ap.add_argument("--out", default=None)
    ap.add_argument("--fifo-rate", type=float, default=300e6, help="bytes per second of each throttled FIFO")
    a = ap.parse_args()
    d, S = a.workdir, a.samples
    os.makedirs(d, exist_ok=True)
    t0 = time.time()
    g, s, r = synth.chr22_scale(n_reads=S * a.reads)
    if not os.path.exists(d + "/idx.done"):
        synth.write_fasta(d + "/ref.fa", g)
        synth.write_vcf(d + "/snps.vcf", g, s)
        subprocess.check_call([BIN, "index", "ref.fa", "snps.vcf", "idx"], cwd=d, env=dict(os.environ, VARGENO_NO_LITE="1"), stdout=subprocess.DEVNULL)
        open(d + "/idx.done", "w").close()
    fq = [d + "/s%d.fq" % i for i in range(S)]
    for i in range(S):
        write_fastq_fixed(fq[i], r, i * a.reads, (i + 1) * a.reads)
    del g, s, r
    print("# set-up %.0f s: index + %d samples of %d reads (%.0f MB each)" % (time.time() - t0, S, a.reads, os.path.getsize(fq[0]) / 1e6), flush=True)
    env = dict(os.environ, VARGENO_MAX_DEVICE_GB="10", VARGENO_VERBOSE="1")
    rows = []

    def vcfs(tag):
        return [d + "/%s_%d.vcf" % (tag, i) for i in range(S)]

    def geno_each(tag, inputs, feeders=None):
        per, t_all = [], time.time()
        for i in range(S):
            t = feeders(i) if feeders else None
            t1 = time.time()
            p = subprocess.run([BIN, "geno", d + "/idx", inputs[i], d + "/snps.vcf", vcfs(tag)[i]], env=env, capture_output=True, text=True)
            per.append(time.time() - t1)
            if t:
                t.join()
            assert p.returncode == 0, p.stderr
        return dict(variant=tag, wall_s=round(time.time() - t_all, 3), per_sample_s=[round(x, 3) for x in per])

    def cohort(tag, inflight, inputs, feeders=None):
        man = d + "/%s.tsv" % tag
        with open(man, "w") as f:
            for i in range(S):
                f.write("%s\t%s\n" % (inputs[i], vcfs(tag)[i]))
        ts = [feeders(i) for i in range(S)] if feeders else []
        t1 = time.time()
        p = subprocess.run([BIN, "cohort", d + "/idx", man, d + "/snps.vcf"], env=dict(env, VARGENO_COHORT_INFLIGHT=str(inflight)), capture_output=True, text=True)
        wall = time.time() - t1
        for t in ts:
            t.join()
        assert p.returncode == 0, p.stderr
        job = [ln for ln in p.stderr.splitlines() if ln.startswith("cohort:")]
        return dict(variant=tag, inflight=inflight, wall_s=round(wall, 3), per_sample_s=sample_seconds(p.stderr), job_line=job[0] if job else "")

    rows.append(geno_each("A_geno_each", fq))
    for k in sorted({1, min(4, S), S}):
        rows.append(cohort("B_cohort_inflight%d" % k, k, fq))
    fifos = [d + "/s%d.fifo" % i for i in range(S)]
    for f in fifos:
        if os.path.exists(f):
            os.remove(f)
        os.mkfifo(f)
    feed = lambda i: throttled_feeder(fq[i], fifos[i], a.fifo_rate)
    rows.append(geno_each("C_geno_each_fifo", fifos, feed))
    rows.append(cohort("C_cohort_fifo_inflight%d" % S, S, fifos, feed))
    want = [open(p, "rb").read() for p in vcfs(rows[0]["variant"])]
    for row in rows:
        row["vcfs_identical_to_A"] = all(open(p, "rb").read() == w for p, w in zip(vcfs(row["variant"]), want))
    assert len(set(want)) == S, "the samples' VCFs should differ from each other"
    text = "\n".join(json.dumps(row) for row in rows)
    print(text, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")
    assert all(row["vcfs_identical_to_A"] for row in rows)


if __name__ == "__main__":
    main()

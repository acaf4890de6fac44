#!/usr/bin/env python3
"""The joint VCF's text routes against each other (writes profiles/joint_text.txt).  NOT RUN YET: nothing about the speed of
VARGENO_JOINT_TEXT=device has been measured; whoever next has a device lease runs this, and the default stays `host` whatever it
shows -- changing it is a change of its own, with this file's output in hand.

    python3 profiles/joint_text.py [--records 1000000] [--samples 8,64,512] [--workdir DIR] [--out profiles/joint_text.txt]

Synthetic calls: a counts table of `--records` sites on one chromosome in eight variants (a sample's table is variant s % 8, so a
512-sample leg reads eight files, not 512), an eight-column SNP list with one record per site, and the hidden `vargeno jointvcf`,
which runs the joint writer with the host caller and no index.  Per number of samples, in ONE process order, three rounds:
  a  VARGENO_JOINT_TEXT unset (host)          b  planned          c  device             -- plain text
  d  host, VARGENO_VCF_BGZF=device            e  planned, ...     f  device, ... (the handle's BGZF stream: text never crosses the link)
Recorded per leg: wall time of the command (it includes reading the counts tables and the host caller, the same for every leg: leg
`z`, a run whose SNP list is only the header, measures that share), the route's own "joint text:" seconds (planned and device; the host
route has no such line: its writer's time is a - z), and with VG_VERBOSE the kernels' own lines: "[vargeno_hip] joint text:" (lengths +
scan, write, GB/s of text) and "[vargeno_hip] joint text stream:" / "bgzf deflate:" (the deflate kernels).  All plain files must be
identical, and all BGZF files.  The comparison that matters is c against a and f against d, from the same run on the same box.  No
threshold is set.  The legs use VARGENO_THREADS=12 and VARGENO_BGZF_THREADS=12: fewer than 16 CPUs' worth of threads."""
import argparse
import hashlib
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vargeno_amd", "csrc", "vargeno")
HEADER8 = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"
LEGS = [("a", "", ""), ("b", "planned", ""), ("c", "device", ""), ("d", "", "device"), ("e", "planned", "device"), ("f", "device", "device")]


def make_inputs(d, n_records):
    rng = random.Random(20261020)
    length = 40 * n_records
    with open(os.path.join(d, "chrlens"), "w") as f:
        f.write("chr1 %d\n" % length)
    pos = sorted(rng.sample(range(1, length), n_records))
    with open(os.path.join(d, "snps.vcf"), "w") as f:
        f.write("##fileformat=VCFv4.0\n" + HEADER8 + "\n")
        f.writelines("1\t%d\trs%d\tA\tC\t.\t.\tRS=%d;VC=SNV\n" % (p, i, i) for i, p in enumerate(pos))
    with open(os.path.join(d, "header_only.vcf"), "w") as f:
        f.write("##fileformat=VCFv4.0\n" + HEADER8 + "\n")
    kinds = [(20, 0), (0, 20), (10, 10), (0, 0), (3, 1), (63, 0), (7, 9), (0, 0)]
    for v in range(8):
        with open(os.path.join(d, "counts%d.txt" % v), "w") as f:
            f.writelines("%d %d %d %d %d\n" % ((p, 230, 25) + rng.choice(kinds)) for p in pos)


def run_leg(d, n_samples, text, bgzf, snps="snps.vcf"):
    out = os.path.join(d, "out.%s.%s" % (text or "host", bgzf or "plain"))
    env = dict(os.environ, VARGENO_VERBOSE="1", VG_VERBOSE="1", VARGENO_THREADS="12", VARGENO_BGZF_THREADS="12")
    for k, v in (("VARGENO_JOINT_TEXT", text), ("VARGENO_VCF_BGZF", bgzf)):
        env.pop(k, None)
        if v:
            env[k] = v
    args = [BIN, "jointvcf", os.path.join(d, "chrlens"), os.path.join(d, snps), out] + ["s%d=%s" % (s, os.path.join(d, "counts%d.txt" % (s % 8))) for s in range(n_samples)]
    t0 = time.time()
    p = subprocess.run(args, env=env, capture_output=True, text=True, timeout=1800)
    wall = time.time() - t0
    if p.returncode != 0:
        raise SystemExit("leg failed: %s\n%s" % (" ".join(args[:5]), p.stderr[-2000:]))
    own = [ln for ln in p.stderr.splitlines() if ln.startswith("joint text:") or ln.startswith("[vargeno_hip] joint text") or ln.startswith("[vargeno_hip] bgzf deflate")]
    with open(out, "rb") as f:
        digest = hashlib.sha256(f.read()).hexdigest()[:16]
    size = os.path.getsize(out)
    os.remove(out)
    return wall, own, digest, size


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--samples", default="8,64,512")
    ap.add_argument("--workdir", default="/dev/shm/joint_text")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "joint_text.txt"))
    a = ap.parse_args()
    os.makedirs(a.workdir, exist_ok=True)
    make_inputs(a.workdir, a.records)
    rows = ["joint text routes: %d records, VARGENO_THREADS=12, three rounds, medians; wall includes reading the counts tables and the host caller (leg z)" % a.records]
    for n in [int(x) for x in a.samples.split(",")]:
        walls, lines, digests, sizes = {k: [] for k, _, _ in LEGS}, {}, {}, {}
        z = [run_leg(a.workdir, n, "", "", snps="header_only.vcf")[0] for _ in range(2)]
        for _ in range(3):
            for key, text, bgzf in LEGS:
                wall, own, digest, size = run_leg(a.workdir, n, text, bgzf)
                walls[key].append(wall)
                lines[key], digests[key], sizes[key] = own, digest, size
        assert len({digests[k] for k in "abc"}) == 1 and len({digests[k] for k in "def"}) == 1, digests
        rows.append("")
        rows.append("%d samples: text %d bytes, BGZF %d bytes; load + call alone (z) %.3f s" % (n, sizes["a"], sizes["d"], min(z)))
        for key, text, bgzf in LEGS:
            rows.append("  %s  %-7s %-12s wall %.3f s (%s)" % (key, text or "host", "BGZF device" if bgzf else "plain", statistics.median(walls[key]), ", ".join("%.3f" % w for w in walls[key])))
            rows.extend("       " + ln for ln in lines[key])
    with open(a.out, "w") as f:
        f.write("\n".join(rows) + "\n")
    print("\n".join(rows))


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""The tabix index beside BGZF output: what VARGENO_VCF_INDEX=tbi costs (writes profiles/vcf_index.txt).

    python3 profiles/vcf_index.py [--gb 2] [--rounds 3] [--out profiles/vcf_index.txt]

The text is the joint-VCF-like text of profiles/vcf_bgzf.py with one change: that recipe writes one 64 MB unit of records again and
again, so its positions start over at every copy and the index would be refused at the second one (unsorted positions) -- here
every copy is a chromosome of its own (chr1, chr2, ...), the same bytes but for that name.  `vargeno bgzfzip` from a file in memory
(/dev/shm) to one, per round the four legs host / host + index / device / device + index, alternated; every leg a process of its own
under `timeout -k 10`, the recipe stops at the first that fails.  Recorded: wall time per leg and the medians, that the .vcf.gz is
the same file with and without the switch, the .tbi size, the "vcf index:" line of VARGENO_VERBOSE, and from one more device leg
with VG_VERBOSE set (not timed: its events synchronise) the scan kernels' own time summed over the spans.  Where `tabix` is on the
PATH: the wall time of `tabix -p vcf` on the same file, and whether `tabix -l` and a few region queries answer the same from our
index and from its own; otherwise the record says that this was not checked."""
import argparse
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import vcf_bgzf as VB  # noqa: E402


def sorted_text(path, gb):
    unit_path = path + ".unit"
    VB.joint_like_text(unit_path, 0.0)                                # the header and one unit
    raw = open(unit_path, "rb").read()
    os.remove(unit_path)
    at = raw.index(b"\nchr22\t") + 1
    header, unit = raw[:at], raw[at:]
    with open(path, "wb") as f:
        f.write(header)
        for k in range(max(1, int(gb * 1e9 / len(unit)))):
            f.write(unit.replace(b"chr22\t", b"chr%d\t" % (k + 1)))
    return os.path.getsize(path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=2.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--leg-timeout", type=float, default=240.0)
    ap.add_argument("--workdir", default="/dev/shm/vg_vcf_index")
    ap.add_argument("--out", default=os.path.join(VB.ROOT, "profiles", "vcf_index.txt"))
    a = ap.parse_args()
    os.makedirs(a.workdir, exist_ok=True)
    src = os.path.join(a.workdir, "sorted_joint_like.vcf")
    if not os.path.exists(src) or os.path.getsize(src) < a.gb * 0.9e9:
        sorted_text(src, a.gb)
    n = os.path.getsize(src)
    cpus = min(16, len(os.sched_getaffinity(0)))
    lines = ["# VARGENO_VCF_INDEX=tbi: bgzfzip on %.2f GB of sorted joint-VCF-like text, fixed codes, VARGENO_BGZF_THREADS=%d, %s" % (n / 1e9, cpus, time.strftime("%Y-%m-%d"))]
    wall = {}
    said = {}
    for rnd in range(a.rounds):
        for route in ("host", "device"):
            for index in (False, True):
                leg = route + (" + index" if index else "")
                dst = os.path.join(a.workdir, "out.%s.%d.vcf.gz" % (route, index))
                env = dict(os.environ, VARGENO_VCF_BGZF=route, VARGENO_BGZF_THREADS=str(cpus), VARGENO_VERBOSE="1")
                env.pop("VG_VERBOSE", None)
                if index:
                    env["VARGENO_VCF_INDEX"] = "tbi"
                s, err = VB.timed([VB.BIN, "bgzfzip", src, dst], env, a.leg_timeout)
                wall.setdefault(leg, []).append(s)
                said[leg] = [ln for ln in err.splitlines() if ln.startswith("vcf index:")]
                lines.append(json.dumps(dict(round=rnd, leg=leg, wall_s=round(s, 3), text_GBps=round(n / 1e9 / s, 3), said=said[leg])))
                print(lines[-1], flush=True)
    for route in ("host", "device"):
        same = subprocess.run(["cmp", os.path.join(a.workdir, "out.%s.0.vcf.gz" % route), os.path.join(a.workdir, "out.%s.1.vcf.gz" % route)]).returncode == 0
        lines.append("%s route: the .vcf.gz is the same file with and without the switch: %s" % (route, same))
        assert same
    same = subprocess.run(["cmp", os.path.join(a.workdir, "out.host.1.vcf.gz.tbi"), os.path.join(a.workdir, "out.device.1.vcf.gz.tbi")]).returncode == 0
    lines.append("the .tbi of the two routes is the same file: %s; %d bytes beside %d bytes of .vcf.gz" % (same, os.path.getsize(os.path.join(a.workdir, "out.host.1.vcf.gz.tbi")), os.path.getsize(os.path.join(a.workdir, "out.host.1.vcf.gz"))))
    assert same
    lines.append("median wall s: " + ", ".join("%s %.3f" % (leg, statistics.median(v)) for leg, v in wall.items()))
    # the scan kernels by their own clock
    env = dict(os.environ, VARGENO_VCF_BGZF="device", VARGENO_VCF_INDEX="tbi", VARGENO_BGZF_THREADS=str(cpus), VG_VERBOSE="1")
    _, err = VB.timed([VB.BIN, "bgzfzip", src, os.path.join(a.workdir, "out.clock.vcf.gz")], env, a.leg_timeout)
    ms = [float(m) for m in re.findall(r"vcf index scan: .*? ([0-9.]+) ms kernels", err)]
    recs = [int(m) for m in re.findall(r"vcf index scan: .*? lines, (\d+) records", err)]
    lines.append("scan kernels' own time (VG_VERBOSE, one device leg): %d spans, %.3f ms in all, %.2f GB/s of text, %d records crossed the link" % (len(ms), sum(ms), n / 1e6 / max(1e-9, sum(ms)), sum(recs)))
    tabix = shutil.which("tabix")
    if not tabix:
        lines.append("tabix is not on this machine: our index was NOT compared with one made by `tabix -p vcf`, and that pass was not timed")
    else:
        ours = os.path.join(a.workdir, "out.host.1.vcf.gz")
        theirs = os.path.join(a.workdir, "theirs.vcf.gz")
        shutil.copyfile(ours, theirs)
        t0 = time.time()
        subprocess.check_call([tabix, "-p", "vcf", theirs])
        lines.append("tabix -p vcf on the same file: %.3f s" % (time.time() - t0))
        agree = subprocess.check_output([tabix, "-l", ours]) == subprocess.check_output([tabix, "-l", theirs])
        for region in ("chr1:1-100000", "chr7:5000000-5100000", "chr22:1-20000", "chr3:99999999-100000000"):
            agree = agree and subprocess.check_output([tabix, ours, region]) == subprocess.check_output([tabix, theirs, region])
        lines.append("tabix -l and four region queries answer the same from both indexes: %s" % agree)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-6:]))


if __name__ == "__main__":
    main()

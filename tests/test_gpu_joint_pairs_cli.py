"""`vargeno joint` with VARGENO_JOINT_PAIRS: the joint VCF stays the same bytes, and the pair table is the text that
tests/pairs_cases.py formats from the oracle over GenoIndex.calls() of each sample alone -- at the default threshold, at a
VARGENO_PAIRS_MIN_GQ inside the samples' GQ range, and with two replicas sharing the device."""
import os
import subprocess

import numpy as np
import pytest

import pairs_cases as PC
from conftest import BIN
from vargeno_amd.api import GenoIndex

pytestmark = pytest.mark.gpu

BASE = dict(VARGENO_CHUNK_MB="1", VARGENO_BATCH="900", VARGENO_PACK_THREADS="2", VARGENO_SHARE_DEVICES="1", VARGENO_VERBOSE="1", VARGENO_COHORT_INFLIGHT="2")
NAMES = ["third0", "third1", "third2", "again0"]


@pytest.fixture(scope="module")
def cohort(ftiny_dir, ftiny_reads, tmp_path_factory):
    """Three samples from disjoint thirds of F-tiny's reads and a fourth that repeats the first; each sample's calls from a handle
    of its own; the joint VCF of the plain run.  Made once, read by every test."""
    d = tmp_path_factory.mktemp("pairs_in")
    prefix = os.path.join(ftiny_dir, "idx")
    lines = open(os.path.join(ftiny_dir, "reads.fq"), "rb").read().split(b"\n")[:-1]
    n = len(lines) // 4
    cuts = [(0, n // 3), (n // 3, 2 * n // 3), (2 * n // 3, n), (0, n // 3)]
    gts, gqs, rows = [], [], []
    with GenoIndex.open(prefix, device=0) as gx:
        for name, (lo, hi) in zip(NAMES, cuts):
            fq = d / (name + ".fq")
            fq.write_bytes(b"\n".join(lines[4 * lo:4 * hi]) + b"\n")
            rows.append("%s\t%s\n" % (fq, name))
            r = ftiny_reads.slice(lo, hi)
            gx.reset()
            gx.submit(r.bases, r.quals, r.offsets)
            gt, gq = gx.calls()
            gts.append(gt.copy()); gqs.append(gq.copy())
    manifest = d / "manifest.tsv"
    manifest.write_text("".join(rows))
    plain = d / "plain.vcf"
    p = subprocess.run([BIN, "joint", prefix, str(manifest), os.path.join(ftiny_dir, "snps.vcf"), str(plain)], env=dict(os.environ, **BASE), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    return dict(prefix=prefix, snps=os.path.join(ftiny_dir, "snps.vcf"), manifest=str(manifest), gt=np.stack(gts), gq=np.stack(gqs), plain=plain.read_bytes(), rows=rows)


def run_joint(cohort, tmp_path, **env):
    out, table = tmp_path / "joint.vcf", tmp_path / "pairs.tsv"
    p = subprocess.run([BIN, "joint", cohort["prefix"], cohort["manifest"], cohort["snps"], str(out)],
                       env=dict(os.environ, VARGENO_JOINT_PAIRS=str(table), **BASE, **env), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert "host loop" not in p.stderr, p.stderr                     # the table came from the device
    assert out.read_bytes() == cohort["plain"]
    return table.read_text()


def test_table_at_the_default_threshold(cohort, tmp_path):
    text = run_joint(cohort, tmp_path)
    want = PC.oracle(cohort["gt"], cohort["gq"], 0)
    assert text == PC.table_text(NAMES, cohort["gt"].shape[1], 0, want)
    assert want[0, 0, 0] > 100 and want[0, 1, 0] > 0                   # the samples do share called sites
    dup = [ln.split("\t") for ln in text.splitlines() if ln.startswith("third0\tagain0\t")]
    assert len(dup) == 1 and dup[0][3] == "0" and dup[0][8] == "1.000000" and dup[0][2] == str(int(want[0, 0, 0]))


def test_table_at_a_threshold_inside_the_gq_range(cohort, tmp_path):
    called = cohort["gq"][cohort["gt"] != 0]
    min_gq = int(np.median(called))
    assert called.min() < min_gq <= called.max()
    text = run_joint(cohort, tmp_path, VARGENO_PAIRS_MIN_GQ=str(min_gq))
    want = PC.oracle(cohort["gt"], cohort["gq"], min_gq)
    assert text == PC.table_text(NAMES, cohort["gt"].shape[1], min_gq, want)
    assert 0 < want[0, 0, 0] < PC.oracle(cohort["gt"], cohort["gq"], 0)[0, 0, 0]
    dup = [ln.split("\t") for ln in text.splitlines() if ln.startswith("third0\tagain0\t")]
    assert dup[0][3] == "0" and dup[0][8] == "1.000000"


def test_two_replicas_sharing_the_device_give_the_same_table(cohort, tmp_path):
    text = run_joint(cohort, tmp_path, VARGENO_GPUS="2")
    assert text == PC.table_text(NAMES, cohort["gt"].shape[1], 0, PC.oracle(cohort["gt"], cohort["gq"], 0))


def test_a_single_sample_gives_the_header_and_no_pair(cohort, tmp_path):
    manifest = tmp_path / "one.tsv"
    manifest.write_text(cohort["rows"][0])
    out, table = tmp_path / "one.vcf", tmp_path / "one_pairs.tsv"
    p = subprocess.run([BIN, "joint", cohort["prefix"], str(manifest), cohort["snps"], str(out)], env=dict(os.environ, VARGENO_JOINT_PAIRS=str(table), **BASE), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert table.read_text() == PC.table_text(NAMES[:1], cohort["gt"].shape[1], 0, PC.oracle(cohort["gt"][:1], cohort["gq"][:1], 0))

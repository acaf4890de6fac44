"""`vargeno geno` / `cohort` / `joint` on BAM input: the golden VCFs of the equivalent text, byte for byte, on both routes --
VARGENO_BGZF=device (compressed bytes to the device, inflated and framed there; after a refusal the host converts the rest) and
VARGENO_BGZF=host (host threads inflate and convert into a pipe, the once-only route takes it from there).  Inputs: tests/bam_cases.py."""
import gzip
import os
import subprocess

import pytest

import bam_cases as B
from conftest import BIN, GOLDEN

pytestmark = pytest.mark.gpu
ROUTES = ["device", "host"]


def _env(route, **env):
    e = dict(os.environ, VARGENO_BGZF=route, VARGENO_CHUNK_MB="1", VARGENO_BATCH="900", VARGENO_PACK_THREADS="2", VARGENO_BGZF_THREADS="3",
             VG_BGZF_SLOT_TEXT="200000")                             # (device route: slots of 200 kB, so that records are carried and a refusal falls behind framed slots)
    e.update(env)
    return e


def _geno(ftiny_dir, reads, out, route, timeout=120, **env):
    return subprocess.run([BIN, "geno", os.path.join(ftiny_dir, "idx"), str(reads), os.path.join(ftiny_dir, "snps.vcf"), str(out)], env=_env(route, **env), capture_output=True, text=True, timeout=timeout)


def _golden(name):
    return gzip.open(os.path.join(GOLDEN, name), "rb").read()


@pytest.mark.parametrize("style", ["aligned", "ragged"])
@pytest.mark.parametrize("route", ROUTES)
def test_geno_on_bam_writes_the_golden_vcf(ftiny_dir, tmp_path, route, style):
    bam = tmp_path / "reads.bam"
    bam.write_bytes(B.ftiny_bam(style)[0])
    p = _geno(ftiny_dir, bam, tmp_path / "out.vcf", route, VARGENO_VERBOSE="1")
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "out.vcf").read_bytes() == _golden("ftiny.out.vcf.gz")
    assert "reads: 4000 " in p.stderr, p.stderr
    line = [ln for ln in p.stderr.splitlines() if "BAM inflated and" in ln]
    assert len(line) == 1 and ("framed on the device" if route == "device" else "converted by host threads") in line[0], p.stderr
    assert "4000 records kept, 200 skipped by flag, 0 skipped empty" in line[0] and "window repairs" in line[0]


@pytest.mark.parametrize("route", ROUTES)
def test_two_replicas_on_bam_write_the_golden_vcf(ftiny_dir, tmp_path, route):
    bam = tmp_path / "reads.bam"
    bam.write_bytes(B.ftiny_bam("spanning")[0])
    p = _geno(ftiny_dir, bam, tmp_path / "out.vcf", route, VARGENO_GPUS="2", VARGENO_SHARE_DEVICES="1")
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "out.vcf").read_bytes() == _golden("ftiny.out.vcf.gz")


def test_cohort_and_joint_with_a_bam_sample(ftiny_dir, tmp_path):
    (tmp_path / "a.bam").write_bytes(B.ftiny_bam("spanning")[0])
    idx, snps, fq = os.path.join(ftiny_dir, "idx"), os.path.join(ftiny_dir, "snps.vcf"), os.path.join(ftiny_dir, "reads.fq")
    env = _env("host", VARGENO_COHORT_INFLIGHT="2", VARGENO_BGZF_THREADS="2")
    manifest = tmp_path / "manifest.tsv"
    manifest.write_text("%s\t%s\n%s\t%s\n" % (tmp_path / "a.bam", tmp_path / "a.vcf", fq, tmp_path / "b.vcf"))
    p = subprocess.run([BIN, "cohort", idx, str(manifest), snps], env=env, capture_output=True, text=True, timeout=180)
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "a.vcf").read_bytes() == _golden("ftiny.out.vcf.gz")
    assert (tmp_path / "b.vcf").read_bytes() == _golden("ftiny.out.vcf.gz")
    # joint: a BAM sample's column is the text sample's
    outs = []
    for name, reads in (("bam", tmp_path / "a.bam"), ("text", fq)):
        man = tmp_path / ("joint_%s.tsv" % name)
        man.write_text("%s\tS1\n%s\tS2\n" % (reads, fq))
        out = tmp_path / ("joint_%s.vcf" % name)
        p = subprocess.run([BIN, "joint", idx, str(man), snps, str(out)], env=env, capture_output=True, text=True, timeout=180)
        assert p.returncode == 0, p.stderr
        outs.append(out.read_bytes())
    assert outs[0] == outs[1] and outs[0].count(b"\n") > 2000


@pytest.fixture(scope="module")
def long_read_job(ftiny_dir, tmp_path_factory):
    """bam_cases.long_read_bam as a file, and what the same binary makes of the Python-converted text: (BAM path, the text job's
    read count, its VCF).  The text job is run once: VARGENO_BGZF says nothing to a text file."""
    d = tmp_path_factory.mktemp("long_read")
    data, raw = B.long_read_bam()
    (d / "long.bam").write_bytes(data)
    (d / "long.fq").write_bytes(B.to_fastq(raw)[0])
    p0 = _geno(ftiny_dir, d / "long.fq", d / "text.vcf", "host", VARGENO_PACK_THREADS="0", VARGENO_VERBOSE="1")
    assert p0.returncode == 0, p0.stderr
    return d / "long.bam", [ln for ln in p0.stderr.splitlines() if ln.startswith("reads: ")][0].split()[1], (d / "text.vcf").read_bytes()


@pytest.mark.parametrize("route", ROUTES)
def test_a_long_read_in_the_middle_of_a_bam_goes_on_through_the_host(ftiny_dir, tmp_path, long_read_job, route):
    """A 2 000-base read in the middle (and a second one right behind it, which restores the reference's four-line rhythm:
    bam_cases.long_read_bam): the device refuses its chunk (the text route refuses the same text) and the host converts the rest;
    each record is counted once, and the VCF is the same binary's VCF on the Python-converted text."""
    bam, want, text_vcf = long_read_job
    p = _geno(ftiny_dir, bam, tmp_path / "bam.vcf", route, VARGENO_VERBOSE="1")
    assert p.returncode == 0, p.stderr
    assert "reads: %s " % want in p.stderr, p.stderr
    if route == "device":
        assert "the device refused a chunk" in p.stderr, p.stderr
    assert (tmp_path / "bam.vcf").read_bytes() == text_vcf
    assert text_vcf.count(b"\n") > 2000


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("what", ["cut_mid_record", "flipped_bit_block_9"])
def test_damage_ends_the_job_with_its_offset(ftiny_dir, tmp_path, route, what):
    data, info = B.damaged()[what]
    at = B.boundary_before(B.ftiny_bam("spanning")[1], len(info)) if what == "cut_mid_record" else info
    bam = tmp_path / "hurt.bam"
    bam.write_bytes(data)
    p = _geno(ftiny_dir, bam, tmp_path / "out.vcf", route)
    assert p.returncode not in (0, None) and p.returncode > 0, p.stderr
    assert not (tmp_path / "out.vcf").exists()
    assert "offset %d" % at in p.stderr, p.stderr


def test_geno_refuses_cram_by_name(ftiny_dir, tmp_path):
    f = tmp_path / "reads.cram"
    f.write_bytes(B.damaged()["cram"][0])
    p = _geno(ftiny_dir, f, tmp_path / "out.vcf", "device")
    assert p.returncode > 0 and not (tmp_path / "out.vcf").exists()
    assert "CRAM" in p.stderr and "samtools fastq" in p.stderr and "FIFO" in p.stderr

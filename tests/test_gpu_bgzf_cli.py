"""`vargeno geno` / `vargeno cohort` on BGZF-compressed FASTQ: the golden VCFs of the text files, byte for byte, on both routes --
VARGENO_BGZF=device (compressed bytes to the device, inflated there; the host takes over through vg_fastq_stream_bgzf_locate)
and VARGENO_BGZF=host (host threads inflate into a pipe, the once-only route takes it from there)."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import bgzf_cases as BC
from conftest import BIN, GOLDEN
from vargeno_amd import synth

pytestmark = pytest.mark.gpu
ROUTES = ["device", "host"]


def _geno(ftiny_dir, fq, out, route, timeout=120, **env):
    e = dict(os.environ, VARGENO_BGZF=route, VARGENO_CHUNK_MB="1", VARGENO_BATCH="900", VARGENO_PACK_THREADS="2", VARGENO_BGZF_THREADS="3", VARGENO_VERBOSE="1",
             VG_BGZF_SLOT_TEXT="200000")                             # (device route: slots of 200 kB of text, so that a refusal and the truncated tail fall behind framed slots)
    e.update(env)
    return subprocess.run([BIN, "geno", os.path.join(ftiny_dir, "idx"), str(fq), os.path.join(ftiny_dir, "snps.vcf"), str(out)], env=e, capture_output=True, text=True, timeout=timeout)


def _golden(name):
    return gzip.open(os.path.join(GOLDEN, name), "rb").read()


@pytest.mark.parametrize("route", ROUTES)
def test_geno_on_bgzf_writes_the_golden_vcf(ftiny_dir, tmp_path, route):
    fq = tmp_path / "reads.fq.gz"
    fq.write_bytes(BC.ftiny_variants()["level6"])
    p = _geno(ftiny_dir, fq, tmp_path / "out.vcf", route)
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "out.vcf").read_bytes() == _golden("ftiny.out.vcf.gz")
    assert ("BGZF inflated on the device" if route == "device" else "BGZF inflated by 3 host threads") in p.stderr, p.stderr


@pytest.mark.parametrize("route", ROUTES)
def test_truncated_final_record_in_bgzf_matches_the_reference(ftiny_dir, tmp_path, route):
    """The file of test_cli_truncated_final_record_matches_the_reference, as BGZF: the reference's stale line buffers must survive
    the host take-over (device route: the last framed record is found through locate, inflated on the host, and primes them)."""
    lines = BC.ftiny_text().split(b"\n")[:-1]
    k = int(open(os.path.join(GOLDEN, "ftiny.trunc.k")).read())
    fq = tmp_path / "reads_trunc.fq.gz"
    fq.write_bytes(synth.bgzf_bytes(b"\n".join(lines[:4 * k + 3]), block=(311, 4096, 65280), rng=np.random.default_rng(2)))
    p = _geno(ftiny_dir, fq, tmp_path / "out.vcf", route)
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "out.vcf").read_bytes() == _golden("ftiny.trunc.out.vcf.gz")


@pytest.mark.parametrize("route", ROUTES)
def test_long_line_in_the_middle_of_a_bgzf_file_goes_on_through_the_host_reader(ftiny_dir, tmp_path, route):
    """The odd record of test_cli_long_line_in_the_middle_of_the_file_falls_back_to_host_framing: the VCF must equal the same
    binary's on the text file."""
    lines = BC.ftiny_text().split(b"\n")[:-1]
    odd = [b"@" + b"ACGT" * 300, b"ACGT" * 20, b"+", b"ACGT" * 800]
    text = b"\n".join(lines[:4 * 1500] + odd + lines[4 * 1500:]) + b"\n"
    (tmp_path / "long.fq").write_bytes(text)
    (tmp_path / "long.fq.gz").write_bytes(synth.bgzf_bytes(text))
    p0 = _geno(ftiny_dir, tmp_path / "long.fq", tmp_path / "text.vcf", route, VARGENO_PACK_THREADS="0")
    assert p0.returncode == 0, p0.stderr
    p = _geno(ftiny_dir, tmp_path / "long.fq.gz", tmp_path / "bgzf.vcf", route)
    assert p.returncode == 0, p.stderr
    assert "reads: %d " % (len(lines) // 4 + 2) in p.stderr, p.stderr
    assert (tmp_path / "bgzf.vcf").read_bytes() == (tmp_path / "text.vcf").read_bytes()
    assert (tmp_path / "bgzf.vcf").read_bytes().count(b"\n") > 2000


@pytest.mark.parametrize("route", ROUTES)
def test_two_replicas_on_bgzf_write_the_golden_vcf(ftiny_dir, tmp_path, route):
    fq = tmp_path / "reads.fq.gz"
    fq.write_bytes(BC.ftiny_variants()["level1"])
    p = _geno(ftiny_dir, fq, tmp_path / "out.vcf", route, VARGENO_GPUS="2", VARGENO_SHARE_DEVICES="1")
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "out.vcf").read_bytes() == _golden("ftiny.out.vcf.gz")


@pytest.mark.parametrize("route", ROUTES)
def test_a_damaged_block_ends_the_job_with_its_offset(ftiny_dir, tmp_path, route):
    data = bytearray(BC.ftiny_variants()["level6"])
    at = BC.split_blocks(bytes(data))[9][0]
    data[at + 18 + 40] ^= 0x04
    fq = tmp_path / "hurt.fq.gz"
    fq.write_bytes(bytes(data))
    p = _geno(ftiny_dir, fq, tmp_path / "out.vcf", route)
    assert p.returncode not in (0, None) and p.returncode > 0, p.stderr
    assert not (tmp_path / "out.vcf").exists()
    assert "offset %d" % at in p.stderr, p.stderr


def test_geno_refuses_plain_gzip(ftiny_dir, tmp_path):
    fq = tmp_path / "plain.fq.gz"
    fq.write_bytes(gzip.compress(BC.ftiny_text()[:100_000]))
    p = _geno(ftiny_dir, fq, tmp_path / "out.vcf", "device")
    assert p.returncode > 0 and not (tmp_path / "out.vcf").exists()
    assert "only BGZF" in p.stderr and "<(zcat %s)" % fq in p.stderr


@pytest.mark.parametrize("route", ROUTES)
def test_cohort_with_a_bgzf_and_a_text_sample(ftiny_dir, tmp_path, route):
    (tmp_path / "a.fq.gz").write_bytes(BC.ftiny_variants()["level9"])
    manifest = tmp_path / "manifest.tsv"
    manifest.write_text("%s\t%s\n%s\t%s\n" % (tmp_path / "a.fq.gz", tmp_path / "a.vcf", os.path.join(ftiny_dir, "reads.fq"), tmp_path / "b.vcf"))
    env = dict(os.environ, VARGENO_BGZF=route, VARGENO_CHUNK_MB="1", VARGENO_BATCH="900", VARGENO_PACK_THREADS="2", VARGENO_COHORT_INFLIGHT="2", VARGENO_BGZF_THREADS="2")
    p = subprocess.run([BIN, "cohort", os.path.join(ftiny_dir, "idx"), str(manifest), os.path.join(ftiny_dir, "snps.vcf")], env=env, capture_output=True, text=True, timeout=180)
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "a.vcf").read_bytes() == _golden("ftiny.out.vcf.gz")
    assert (tmp_path / "b.vcf").read_bytes() == _golden("ftiny.out.vcf.gz")

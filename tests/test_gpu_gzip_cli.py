"""`vargeno geno` / `cohort` on plain gzip FASTQ, with VARGENO_GZIP=device (the compressed file is streamed to the device, which
inflates it slot by slot and frames the text; the host takes over from a checkpoint where it must) and VARGENO_GZIP=host (one host
thread inflates into a pipe, the once-only route takes it from there): the golden VCFs of the text files, byte for byte."""
import gzip
import os
import subprocess

import pytest

import bgzf_cases as BC
import gzip_cases as GC
from conftest import BIN, GOLDEN
from vargeno_amd import synth

pytestmark = pytest.mark.gpu


ROUTES = ["device", "host"]
DEVICE_LINE = "gzip inflated on the device"


def _geno(ftiny_dir, fq, out, route, timeout=120, **env):
    e = dict(os.environ, VARGENO_GZIP=route, VARGENO_CHUNK_MB="1", VARGENO_BATCH="900", VARGENO_PACK_THREADS="2", VARGENO_VERBOSE="1")
    e.update(env)
    return subprocess.run([BIN, "geno", os.path.join(ftiny_dir, "idx"), str(fq), os.path.join(ftiny_dir, "snps.vcf"), str(out)], env=e, capture_output=True, text=True, timeout=timeout)


def _golden(name):
    return gzip.open(os.path.join(GOLDEN, name), "rb").read()


@pytest.mark.parametrize("route", ROUTES)
def test_geno_on_gzip_writes_the_golden_vcf(ftiny_dir, tmp_path, route):
    fq = tmp_path / "reads.fq.gz"
    fq.write_bytes(synth.gzip_bytes(GC.ftiny_text(), level=6))
    p = _geno(ftiny_dir, fq, tmp_path / "out.vcf", route)
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "out.vcf").read_bytes() == _golden("ftiny.out.vcf.gz")
    if route == "device":                                          # the device inflated it: all 4 000 reads framed there, one member, no slot refused
        assert DEVICE_LINE + ": 4000 reads framed, 1 members" in p.stderr and "0 slots refused" in p.stderr, p.stderr
    else:
        assert "gzip inflated by one host thread: 1 members" in p.stderr and DEVICE_LINE not in p.stderr, p.stderr


@pytest.mark.parametrize("env", [dict(VG_GZ_SLOT="50000", VG_GZ_CHUNK="8192"), dict(VG_GZ_MAX_RATIO="1")], ids=["small_slots", "refused_slot"])
def test_geno_on_the_device_route_with_small_slots_and_with_a_refused_slot(ftiny_dir, tmp_path, env):
    """Slots far smaller than the file: the boundary and the window are carried from slot to slot.  A ratio bound of 1 (this file
    compresses 1.8 : 1): the first slot is refused, and the host inflates the whole file from the checkpoint -- the same VCF."""
    fq = tmp_path / "reads.fq.gz"
    fq.write_bytes(synth.gzip_bytes(GC.ftiny_text(), level=6))
    p = _geno(ftiny_dir, fq, tmp_path / "out.vcf", "device", **env)
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "out.vcf").read_bytes() == _golden("ftiny.out.vcf.gz")
    if "VG_GZ_MAX_RATIO" in env:
        assert DEVICE_LINE + ": 0 reads framed" in p.stderr and "1 slots refused" in p.stderr and "the host inflates the rest" in p.stderr, p.stderr
    else:
        assert DEVICE_LINE + ": 4000 reads framed" in p.stderr and "0 slots refused" in p.stderr, p.stderr


@pytest.mark.parametrize("route", ROUTES)
def test_truncated_final_record_in_gzip_matches_the_reference(ftiny_dir, tmp_path, route):
    """The file of test_cli_truncated_final_record_matches_the_reference, as gzip: the reference's stale line buffers survive."""
    lines = GC.ftiny_text().split(b"\n")[:-1]
    k = int(open(os.path.join(GOLDEN, "ftiny.trunc.k")).read())
    fq = tmp_path / "reads_trunc.fq.gz"
    fq.write_bytes(synth.gzip_bytes(b"\n".join(lines[:4 * k + 3]), level=6))
    p = _geno(ftiny_dir, fq, tmp_path / "out.vcf", route, **(dict(VG_GZ_SLOT="50000") if route == "device" else {}))
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "out.vcf").read_bytes() == _golden("ftiny.trunc.out.vcf.gz")
    assert (DEVICE_LINE in p.stderr) == (route == "device"), p.stderr


@pytest.mark.parametrize("route", ROUTES)
def test_long_line_in_the_middle_of_a_gzip_file_goes_on_through_the_host_reader(ftiny_dir, tmp_path, route):
    """The odd record of the BGZF suite: the VCF must equal the same binary's on the text file."""
    lines = GC.ftiny_text().split(b"\n")[:-1]
    odd = [b"@" + b"ACGT" * 300, b"ACGT" * 20, b"+", b"ACGT" * 800]
    text = b"\n".join(lines[:4 * 1500] + odd + lines[4 * 1500:]) + b"\n"
    (tmp_path / "long.fq").write_bytes(text)
    (tmp_path / "long.fq.gz").write_bytes(synth.gzip_bytes(text))
    p0 = _geno(ftiny_dir, tmp_path / "long.fq", tmp_path / "text.vcf", route, VARGENO_PACK_THREADS="0")
    assert p0.returncode == 0, p0.stderr
    p = _geno(ftiny_dir, tmp_path / "long.fq.gz", tmp_path / "gzip.vcf", route, **(dict(VG_GZ_SLOT="50000") if route == "device" else {}))
    assert (DEVICE_LINE in p.stderr) == (route == "device"), p.stderr
    assert p.returncode == 0, p.stderr
    assert "reads: %d " % (len(lines) // 4 + 2) in p.stderr, p.stderr
    assert (tmp_path / "gzip.vcf").read_bytes() == (tmp_path / "text.vcf").read_bytes()
    assert (tmp_path / "gzip.vcf").read_bytes().count(b"\n") > 2000


@pytest.mark.parametrize("route", ROUTES)
def test_two_replicas_on_gzip_write_the_golden_vcf(ftiny_dir, tmp_path, route):
    fq = tmp_path / "reads.fq.gz"
    fq.write_bytes(synth.gzip_bytes(GC.ftiny_text(), level=1) )
    p = _geno(ftiny_dir, fq, tmp_path / "out.vcf", route, VARGENO_GPUS="2", VARGENO_SHARE_DEVICES="1")
    assert p.returncode == 0, p.stderr
    assert "gzip inflated by one host thread" in p.stderr and DEVICE_LINE not in p.stderr, p.stderr        # several replicas: the host route, whatever was asked for
    assert (tmp_path / "out.vcf").read_bytes() == _golden("ftiny.out.vcf.gz")


@pytest.mark.parametrize("route", ROUTES)
def test_a_flipped_bit_ends_the_job_with_its_offset(ftiny_dir, tmp_path, route):
    data = bytearray(synth.gzip_bytes(GC.ftiny_text(), level=6))
    data[300_000] ^= 0x04
    fq = tmp_path / "hurt.fq.gz"
    fq.write_bytes(bytes(data))
    p = _geno(ftiny_dir, fq, tmp_path / "out.vcf", route)
    assert p.returncode not in (0, None) and p.returncode > 0, p.stderr
    assert not (tmp_path / "out.vcf").exists()
    assert "gzip stream at compressed offset" in p.stderr, p.stderr


def test_unset_the_file_is_refused_as_before(ftiny_dir, tmp_path):
    fq = tmp_path / "plain.fq.gz"
    fq.write_bytes(gzip.compress(GC.ftiny_text()[:100_000]))
    env = {k: v for k, v in os.environ.items() if k != "VARGENO_GZIP"}
    p = subprocess.run([BIN, "geno", os.path.join(ftiny_dir, "idx"), str(fq), os.path.join(ftiny_dir, "snps.vcf"), str(tmp_path / "out.vcf")], env=env, capture_output=True, text=True, timeout=60)
    assert p.returncode > 0 and not (tmp_path / "out.vcf").exists()
    assert "only BGZF" in p.stderr and "<(zcat %s)" % fq in p.stderr and "VARGENO_GZIP=device|host" in p.stderr


@pytest.mark.parametrize("route", ROUTES)
def test_cohort_with_a_gzip_a_bgzf_and_a_text_sample(ftiny_dir, tmp_path, route):
    (tmp_path / "a.fq.gz").write_bytes(synth.gzip_bytes(GC.ftiny_text(), level=9))
    (tmp_path / "b.fq.gz").write_bytes(BC.ftiny_variants()["level6"])
    manifest = tmp_path / "manifest.tsv"
    manifest.write_text("".join("%s\t%s\n" % (fq, tmp_path / out) for fq, out in ((tmp_path / "a.fq.gz", "a.vcf"), (tmp_path / "b.fq.gz", "b.vcf"), (os.path.join(ftiny_dir, "reads.fq"), "c.vcf"))))
    env = dict(os.environ, VARGENO_GZIP=route, VARGENO_CHUNK_MB="1", VARGENO_BATCH="900", VARGENO_PACK_THREADS="2", VARGENO_COHORT_INFLIGHT="2", VARGENO_BGZF_THREADS="2")
    p = subprocess.run([BIN, "cohort", os.path.join(ftiny_dir, "idx"), str(manifest), os.path.join(ftiny_dir, "snps.vcf")], env=env, capture_output=True, text=True, timeout=180)
    assert p.returncode == 0, p.stderr
    for out in ("a.vcf", "b.vcf", "c.vcf"):
        assert (tmp_path / out).read_bytes() == _golden("ftiny.out.vcf.gz"), out

"""BAM on the host: the host build of the record parser (vargeno_amd/csrc/vg_bam.h -- the source the device kernels are compiled
from) through vg_bam_to_fastq_host and the command line's `bamcat`, against the independent Python converter of tests/bam_cases.py;
the damage cases; the parser alone under AddressSanitizer + UBSan (tests/bam_fuzz.cpp); a cohort manifest that names a BAM.
No device is touched."""
import os
import subprocess

import pytest

import bam_cases as B
from conftest import BIN, ROOT
from vargeno_amd import api
from vargeno_amd._lib import VgError

CASES = {"ftiny": B.ftiny_bam, "corner": B.corner_bam, "decoy": lambda style: B.decoy_bam()[:2]}
VALID = [(c, s) for c in ("ftiny", "corner") for s in B.STYLES] + [("decoy", "spanning")]
IDS = ["%s-%s" % cs for cs in VALID]


@pytest.mark.parametrize("case,style", VALID, ids=IDS)
def test_host_conversion_equals_the_python_converter(case, style):
    data, raw = CASES[case](style)
    text, reads, n_flag, n_empty = B.to_fastq(raw)
    got, n, bad = api.bam_to_fastq(data)
    assert bad is None and n == len(reads)
    assert got == text


@pytest.mark.parametrize("case,style", VALID, ids=IDS)
def test_bamcat_writes_the_equivalent_text(case, style, tmp_path):
    data, raw = CASES[case](style)
    f = tmp_path / "reads.bam"
    f.write_bytes(data)
    p = subprocess.run([BIN, "bamcat", str(f)], capture_output=True, timeout=60)
    assert p.returncode == 0, p.stderr
    assert p.stdout == B.to_fastq(raw)[0]


def test_a_missing_end_of_file_marker_is_accepted(tmp_path):
    hdr, recs = B.header(2), [B.record("r%d" % i, "ACGT" * 10, [30] * 40) for i in range(5)]
    data = B.write(hdr, recs, "spanning", eof=False)
    text = B.to_fastq(hdr + b"".join(recs))[0]
    assert api.bam_to_fastq(data) == (text, 5, None)
    f = tmp_path / "reads.bam"
    f.write_bytes(data)
    p = subprocess.run([BIN, "bamcat", str(f)], capture_output=True, timeout=60)
    assert p.returncode == 0 and p.stdout == text


def test_damage_is_reported_with_its_inflated_offset(tmp_path):
    dm = B.damaged()
    raw = B.ftiny_bam("spanning")[1]
    full_text, reads, _, _ = B.to_fastq(raw)

    def bamcat(data):
        f = tmp_path / "damaged.bam"
        f.write_bytes(data)
        return subprocess.run([BIN, "bamcat", str(f)], capture_output=True, timeout=60)

    # cut mid-record: the text of the records before it, and the offset of the record the stream ends inside
    data, cut_raw = dm["cut_mid_record"]
    at = B.boundary_before(raw, len(cut_raw))
    got, n, bad = api.bam_to_fastq(data)
    assert bad == at and at < len(cut_raw) and got == _text_of(reads, full_text, at)
    p = bamcat(data)
    assert p.returncode != 0 and b"inside a record" in p.stderr and b"offset %d" % at in p.stderr and p.stdout == got
    # cut mid-header
    data, cut_raw = dm["cut_mid_header"]
    got, n, bad = api.bam_to_fastq(data)
    assert (got, n, bad) == (b"", 0, len(cut_raw))
    p = bamcat(data)
    assert p.returncode != 0 and b"header" in p.stderr and b"offset %d" % len(cut_raw) in p.stderr and p.stdout == b""
    # a block_size of 7
    data, at = dm["block_size_7"]
    got, n, bad = api.bam_to_fastq(data)
    assert bad == at and got == _text_of(reads, full_text, at)
    p = bamcat(data)
    assert p.returncode != 0 and b"block_size" in p.stderr and b"offset %d" % at in p.stderr
    # a flipped deflate bit in block 9: the text stops before that block's records, the block is named by its compressed offset
    data, comp_at = dm["flipped_bit_block_9"]
    got, n, bad = api.bam_to_fastq(data)
    assert bad is not None and bad <= 9 * 65280 and got == _text_of(reads, full_text, bad)
    assert ("compressed offset %d" % comp_at) in api.lib().vg_last_error().decode()
    p = bamcat(data)
    assert p.returncode != 0 and b"compressed offset %d" % comp_at in p.stderr
    # CRAM: refused by name, one line, with the way round it
    with pytest.raises(VgError) as e:
        api.bam_to_fastq(dm["cram"][0])
    assert e.value.code == -2 and "CRAM" in str(e.value)
    f = tmp_path / "reads.cram"
    f.write_bytes(dm["cram"][0])
    for cmd in (["bamcat", str(f)], ["geno", str(tmp_path / "no_such_index"), str(f), str(tmp_path / "snps.vcf"), str(tmp_path / "out.vcf")]):
        p = subprocess.run([BIN] + cmd, capture_output=True, text=True, timeout=60)
        lines = [ln for ln in p.stderr.splitlines() if ln.strip()]
        assert p.returncode != 0 and p.stdout == "" and len(lines) == 1, p.stderr
        assert "CRAM" in lines[0] and "samtools fastq" in lines[0] and "FIFO" in lines[0]
    assert not (tmp_path / "out.vcf").exists()
    # BGZF that is not BAM
    with pytest.raises(VgError) as e:
        api.bam_to_fastq(B.BC.ftiny_variants()["level6"])
    assert e.value.code == -2 and "BAM" in str(e.value)


def _text_of(reads, full_text, before):
    """The equivalent text of the kept records that start before a stream offset."""
    n = sum(1 for r in reads if r[0] < before)
    return b"".join(ln + b"\n" for ln in full_text.split(b"\n")[:4 * n])


def test_record_parser_under_sanitizers(tmp_path):
    """tests/bam_fuzz.cpp: the host build of vg_bam.h alone, built with -fsanitize=address,undefined and run directly: 20 000 seeded
    mutations of record bytes through the field view, the plausibility predicate, the window walk and the header parser, and walks
    started at every offset of a 4 KiB sample, all on exactly-sized heap buffers."""
    exe = tmp_path / "bam_fuzz"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe),
                    os.path.join(ROOT, "tests", "bam_fuzz.cpp")], check=True, timeout=300)
    raw = B.corner_bam("spanning")[1] + B.ftiny_bam("spanning")[1][B.parse_header(B.ftiny_bam("spanning")[1])[0]:][:200_000]
    raw = raw[:B.boundary_before(raw, len(raw))]
    f = tmp_path / "stream.bin"
    f.write_bytes(raw)
    p = subprocess.run([str(exe), str(f), "20000", "12345"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().endswith("ok"), p.stdout


def test_a_cohort_manifest_may_name_a_bam(ftiny_dir, tmp_path):
    """Validation happens before a device is touched and does not look at what the inputs are: a manifest with a BAM and a text
    sample passes it.  Without a device the command then fails the way `geno` does; with one it writes both golden VCFs."""
    import gzip

    from conftest import GOLDEN
    from vargeno_amd import _lib

    bam = tmp_path / "reads.bam"
    bam.write_bytes(B.ftiny_bam("aligned")[0])
    man = tmp_path / "manifest.tsv"
    man.write_text("%s\t%s\n%s\t%s\n" % (bam, tmp_path / "a.vcf", os.path.join(ftiny_dir, "reads.fq"), tmp_path / "b.vcf"))
    p = subprocess.run([BIN, "cohort", os.path.join(ftiny_dir, "idx"), str(man), os.path.join(ftiny_dir, "snps.vcf")], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert "manifest.tsv line" not in p.stderr, p.stderr
    if _lib.lib().vg_device_count() <= 0:
        assert p.returncode == 1 and "no HIP device found" in p.stderr
        assert not (tmp_path / "a.vcf").exists()
    else:
        assert p.returncode == 0, p.stderr
        golden = gzip.open(os.path.join(GOLDEN, "ftiny.out.vcf.gz"), "rb").read()
        assert (tmp_path / "a.vcf").read_bytes() == golden and (tmp_path / "b.vcf").read_bytes() == golden

"""The device caller behind the command line: `VARGENO_CALLER=device vargeno geno|cohort` must write the very bytes of the host
call loop (the reference's golden VCFs), and `vargeno joint` one multi-sample VCF whose columns are, sample by sample, what
the oracle's caller gives on that sample's reads alone."""
import gzip
import os
import subprocess

import pytest

from conftest import BIN, GOLDEN
from oracle import oracle as O
from vargeno_amd import index_io

pytestmark = pytest.mark.gpu

BASE = dict(VARGENO_CHUNK_MB="1", VARGENO_BATCH="900", VARGENO_PACK_THREADS="2", VARGENO_SHARE_DEVICES="1", VARGENO_VERBOSE="1")
MISSING = "./.:."


@pytest.fixture(scope="module")
def inputs(ftiny_dir, ftiny_reads, tmp_path_factory):
    """The samples' FASTQ files and what the oracle calls on each: written and computed once, read by every test."""
    d = tmp_path_factory.mktemp("joint_in")
    prefix = os.path.join(ftiny_dir, "idx")
    whole_path = os.path.join(ftiny_dir, "reads.fq")
    lines = open(whole_path, "rb").read().split(b"\n")[:-1]
    k = int(open(os.path.join(GOLDEN, "ftiny.trunc.k")).read())
    trunc = d / "trunc.fq"
    trunc.write_bytes(b"\n".join(lines[:4 * k + 3]))
    chrlens = index_io.read_chrlens(prefix + ".chrlens")

    def oracle_calls(r):
        ox = O.OracleIndex.load(prefix)
        ox.process(r.bases, r.quals, r.offsets)
        return O.calls_by_key(ox.sites(), chrlens)

    samples = [("whole", whole_path, oracle_calls(ftiny_reads))]
    for n, (lo, hi) in enumerate(((0, 1333), (1333, 2666))):
        fq = d / ("third%d.fq" % n)
        fq.write_bytes(b"\n".join(lines[4 * lo:4 * hi]) + b"\n")
        samples.append(("third%d" % n, str(fq), oracle_calls(ftiny_reads.slice(lo, hi))))
    bad = list(lines[:4 * 200])
    at = next(i for i in range(1, len(bad), 4) if len(bad[i]) >= 64 and b"N" not in bad[i].upper())
    bad[at] = bad[at][:7] + b"X" + bad[at][8:]
    bad_fq = d / "bad.fq"
    bad_fq.write_bytes(b"\n".join(bad) + b"\n")
    return dict(prefix=prefix, snps=os.path.join(ftiny_dir, "snps.vcf"), whole=whole_path, trunc=str(trunc), samples=samples, bad=str(bad_fq),
                golden_whole=gzip.open(os.path.join(GOLDEN, "ftiny.out.vcf.gz"), "rb").read(), golden_trunc=gzip.open(os.path.join(GOLDEN, "ftiny.trunc.out.vcf.gz"), "rb").read())


def test_geno_with_the_device_caller_writes_the_golden_bytes(inputs, tmp_path):
    env = dict(os.environ, VARGENO_CALLER="device", **BASE)
    for name, fq, want in (("whole", inputs["whole"], inputs["golden_whole"]), ("trunc", inputs["trunc"], inputs["golden_trunc"])):
        out = tmp_path / (name + ".vcf")
        p = subprocess.run([BIN, "geno", inputs["prefix"], fq, inputs["snps"], str(out)], env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        assert "caller: device" in p.stderr, p.stderr                    # the calls did come from the kernel
        assert out.read_bytes() == want, name


def test_cohort_with_the_device_caller_writes_the_golden_bytes(inputs, tmp_path):
    env = dict(os.environ, VARGENO_CALLER="device", VARGENO_COHORT_INFLIGHT="2", **BASE)
    a, b = tmp_path / "a.vcf", tmp_path / "b.vcf"
    manifest = tmp_path / "manifest.tsv"
    manifest.write_text("%s\t%s\n%s\t%s\n" % (inputs["whole"], a, inputs["trunc"], b))
    p = subprocess.run([BIN, "cohort", inputs["prefix"], str(manifest), inputs["snps"]], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert p.stderr.count("caller: device") == 2, p.stderr
    assert a.read_bytes() == inputs["golden_whole"] and b.read_bytes() == inputs["golden_trunc"]


def test_joint_with_the_single_sample_donor_is_the_geno_vcf(inputs, tmp_path):
    manifest = tmp_path / "manifest.tsv"
    manifest.write_text("%s\tDONOR\n" % inputs["whole"])
    out = tmp_path / "joint.vcf"
    p = subprocess.run([BIN, "joint", inputs["prefix"], str(manifest), inputs["snps"], str(out)], env=dict(os.environ, **BASE), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert "caller: device" in p.stderr, p.stderr
    assert out.read_bytes() == inputs["golden_whole"]


_three_sample_runs = {}                                                  # (inflight, replicas) -> the joint file's bytes, for the comparison between the runs


@pytest.mark.parametrize("inflight,replicas", [("1", "1"), ("3", "1"), ("3", "2")])
def test_joint_with_three_samples(inputs, tmp_path, inflight, replicas):
    """One plane serving the samples in turn, three planes at once, and two replicas that share the device: column by column the
    oracle's calls on each sample alone, the union of their records, and the same bytes from every run."""
    manifest = tmp_path / "manifest.tsv"
    manifest.write_text("".join("%s\t%s\n" % (fq, name) for name, fq, _ in inputs["samples"]))
    out = tmp_path / "joint.vcf"
    env = dict(os.environ, VARGENO_COHORT_INFLIGHT=inflight, VARGENO_GPUS=replicas, **BASE)
    p = subprocess.run([BIN, "joint", inputs["prefix"], str(manifest), inputs["snps"], str(out)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert p.stderr.count("caller: device") == 3, p.stderr
    _three_sample_runs[(inflight, replicas)] = out.read_bytes()
    for other in _three_sample_runs.values():
        assert other == out.read_bytes()
    text = out.read_bytes().decode()
    head = [ln for ln in text.split("\n") if ln.startswith("#")]
    assert head[-1].split("\t")[8:] == ["FORMAT"] + [name for name, _, _ in inputs["samples"]]
    want = [calls for _, _, calls in inputs["samples"]]
    seen = set()
    for ln in text.split("\n"):
        if not ln or ln[0] == "#":
            continue
        c = ln.split("\t")
        assert len(c) == 9 + 3 and c[8] == "GT:GQ"
        key = "%s$%s" % (c[0] if c[0].startswith("c") else "chr" + c[0], c[1])
        seen.add(key)
        for col, calls in zip(c[9:], want):
            assert col == ("%s:%d" % calls[key] if key in calls else MISSING), (key, col)
        assert any(col != MISSING for col in c[9:])
    # the record set is the union: every key some sample has called is a record of F-tiny's SNP list
    union = set().union(*[set(w) for w in want])
    assert seen == union and len(union) > 2000


def test_joint_with_a_sample_the_reference_aborts_on_writes_no_file(inputs, tmp_path):
    manifest = tmp_path / "manifest.tsv"
    manifest.write_text("%s\tgood\n%s\tbad\n" % (inputs["samples"][1][1], inputs["bad"]))
    out = tmp_path / "joint.vcf"
    p = subprocess.run([BIN, "joint", inputs["prefix"], str(manifest), inputs["snps"], str(out)], env=dict(os.environ, VARGENO_COHORT_INFLIGHT="2", **BASE), capture_output=True, text=True, timeout=300)
    assert p.returncode == 1, p.stderr
    assert not out.exists()
    named = [ln for ln in p.stderr.splitlines() if "character other than ACGTN" in ln]
    assert len(named) == 1 and "line 2:" in named[0] and "no joint file" in named[0], p.stderr

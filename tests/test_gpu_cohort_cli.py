"""`vargeno cohort`: six samples against one resident index, in one process -- the reference's golden VCFs byte for byte where it
has one, the oracle's calls for the samples that are parts of F-tiny, and `vargeno geno` itself (unchanged code, pinned to the
reference by test_gpu_fastq.py) for the file that needs the host reader in its middle."""
import gzip
import os
import subprocess
import threading

import pytest

from conftest import BIN, GOLDEN
from oracle import oracle as O
from vargeno_amd import index_io

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cohort_inputs(ftiny_dir, ftiny_reads, tmp_path_factory):
    """The samples' FASTQ files and what each must give: written and computed once for the four parametrised cases."""
    d = tmp_path_factory.mktemp("cohort_in")
    prefix = os.path.join(ftiny_dir, "idx")
    whole = open(os.path.join(ftiny_dir, "reads.fq"), "rb").read()
    lines = whole.split(b"\n")[:-1]
    k = int(open(os.path.join(GOLDEN, "ftiny.trunc.k")).read())
    trunc = b"\n".join(lines[:4 * k + 3])
    chrlens = index_io.read_chrlens(prefix + ".chrlens")
    thirds = []
    for n, (lo, hi) in enumerate(((0, 1333), (1333, 2666))):
        fq = d / ("third%d.fq" % n)
        fq.write_bytes(b"\n".join(lines[4 * lo:4 * hi]) + b"\n")
        r = ftiny_reads.slice(lo, hi)
        ox = O.OracleIndex.load(prefix)
        ox.process(r.bases, r.quals, r.offsets)
        thirds.append((str(fq), O.calls_by_key(ox.sites(), chrlens)))
    # a record with lines beyond fgets' 1023 characters in the middle of the file (test_gpu_fastq.py has the story of its four lines)
    odd = [b"@" + b"ACGT" * 300, b"ACGT" * 20, b"+", b"ACGT" * 800]
    long_fq = d / "long.fq"
    long_fq.write_bytes(b"\n".join(lines[:4 * 1500] + odd + lines[4 * 1500:]) + b"\n")
    # a read the reference aborts on
    bad = list(lines[:4 * 200])
    at = next(i for i in range(1, len(bad), 4) if len(bad[i]) >= 64 and b"N" not in bad[i].upper())
    bad[at] = bad[at][:7] + b"X" + bad[at][8:]
    bad_fq = d / "bad.fq"
    bad_fq.write_bytes(b"\n".join(bad) + b"\n")
    return dict(prefix=prefix, snps=os.path.join(ftiny_dir, "snps.vcf"), whole=os.path.join(ftiny_dir, "reads.fq"), trunc=trunc, thirds=thirds, long=str(long_fq), bad=str(bad_fq),
                golden_whole=gzip.open(os.path.join(GOLDEN, "ftiny.out.vcf.gz"), "rb").read(), golden_trunc=gzip.open(os.path.join(GOLDEN, "ftiny.trunc.out.vcf.gz"), "rb").read())


@pytest.mark.parametrize("inflight,replicas", [("1", "1"), ("3", "1"), ("1", "2"), ("3", "2")])
def test_cohort_of_six_samples(cohort_inputs, tmp_path, inflight, replicas):
    """INFLIGHT=1: plane 0 serves the six samples in turn (the reset between them); 3: three planes, three samples in flight
    together.  Two replicas share the device: a sample's batches go round robin over them, its planes are summed with RCCL."""
    ci = cohort_inputs
    env = dict(os.environ, VARGENO_CHUNK_MB="1", VARGENO_BATCH="900", VARGENO_PACK_THREADS="2", VARGENO_COHORT_INFLIGHT=inflight, VARGENO_GPUS=replicas, VARGENO_SHARE_DEVICES="1", VARGENO_VERBOSE="1")
    fifo = str(tmp_path / "trunc.fifo")
    os.mkfifo(fifo)
    out = {c: tmp_path / ("%s.vcf" % c) for c in "abcdef"}
    manifest = tmp_path / "manifest.tsv"
    manifest.write_text("%s\t%s\n%s\t%s\n%s\t%s\n%s\t%s\n%s\t%s\n%s\t%s\n" % (
        ci["whole"], out["a"], fifo, out["b"], ci["thirds"][0][0], out["c"], ci["thirds"][1][0], out["d"], ci["long"], out["e"], ci["bad"], out["f"]))
    bad_line = 6

    def feed():
        try:
            with open(fifo, "wb", buffering=0) as w:
                for a in range(0, len(ci["trunc"]), 300_000):
                    w.write(ci["trunc"][a:a + 300_000])
        except BrokenPipeError:
            pass
    t = threading.Thread(target=feed)
    t.start()
    p = subprocess.run([BIN, "cohort", ci["prefix"], str(manifest), ci["snps"]], env=env, capture_output=True, text=True, timeout=300)
    if t.is_alive():                                                     # the command never opened the FIFO: let the feeder go
        os.close(os.open(fifo, os.O_RDONLY | os.O_NONBLOCK))
    t.join()
    assert p.returncode == 1, p.stderr                                   # because of (f), and only because of it
    assert out["a"].read_bytes() == ci["golden_whole"], p.stderr
    assert out["b"].read_bytes() == ci["golden_trunc"], p.stderr
    for c, (_, want) in zip("cd", ci["thirds"]):
        assert O.parse_vcf_calls(str(out[c])) == want, (c, p.stderr)
    g_out = tmp_path / "geno_long.vcf"
    g = subprocess.run([BIN, "geno", ci["prefix"], ci["long"], ci["snps"], str(g_out)], env=env, capture_output=True, text=True, timeout=300)
    assert g.returncode == 0, g.stderr
    assert out["e"].read_bytes() == g_out.read_bytes() and g_out.read_bytes().count(b"\n") > 2000, p.stderr
    assert not out["f"].exists()
    named = [ln for ln in p.stderr.splitlines() if "character other than ACGTN" in ln]
    assert len(named) == 1 and "line %d:" % bad_line in named[0] and "1 reads" in named[0], p.stderr
    assert sum(ln.startswith("sample, line") for ln in p.stderr.splitlines()) == 5 and "cohort: samples: 6" in p.stderr, p.stderr
    # without (f) the exit status is 0
    manifest.write_text("%s\t%s\n%s\t%s\n" % (ci["thirds"][0][0], tmp_path / "c2.vcf", ci["thirds"][1][0], tmp_path / "d2.vcf"))
    p = subprocess.run([BIN, "cohort", ci["prefix"], str(manifest), ci["snps"]], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "c2.vcf").read_bytes() == out["c"].read_bytes() and (tmp_path / "d2.vcf").read_bytes() == out["d"].read_bytes()

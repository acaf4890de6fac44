"""VARGENO_VCF_INDEX=tbi behind the command line on F-tiny: `geno`, `cohort` and `joint` write <path>.tbi beside every BGZF VCF -- the
bytes of the definition (tests/tbi_cases.py) over the file's text -- on the device route, the host route and the joint text stream;
the VCF and the pair table are the bytes of the run without the switch."""
import gzip
import os
import subprocess

import pytest

import tbi_cases as T
from conftest import BIN, GOLDEN
from vargeno_amd import api

pytestmark = pytest.mark.gpu

BASE = dict(VARGENO_CHUNK_MB="1", VARGENO_BATCH="900", VARGENO_PACK_THREADS="2", VARGENO_SHARE_DEVICES="1", VARGENO_VERBOSE="1", VARGENO_BGZF_THREADS="3", VARGENO_COHORT_INFLIGHT="2")


def _env(route, index=True, **more):
    e = {k: v for k, v in os.environ.items() if k not in ("VARGENO_VCF_BGZF", "VARGENO_VCF_INDEX", "VARGENO_JOINT_TEXT")}
    e.update(BASE, VARGENO_VCF_BGZF=route)
    if index:
        e["VARGENO_VCF_INDEX"] = "tbi"
    e.update(more)
    return e


def _tbi(path):
    return api.bgzf_inflate(open(str(path) + ".tbi", "rb").read(), device=None)[0]


def _definition(text):
    z, want = T.expected(text)
    assert not isinstance(want, T.Refused), want
    return z, want


@pytest.fixture(scope="module")
def cohort(ftiny_dir, tmp_path_factory):
    d = tmp_path_factory.mktemp("index_cohort")
    whole = os.path.join(ftiny_dir, "reads.fq")
    lines = open(whole, "rb").read().split(b"\n")[:-1]
    samples = [("whole", whole)]
    for n, (lo, hi) in enumerate(((0, 1333), (1333, 2666))):
        fq = d / ("third%d.fq" % n)
        fq.write_bytes(b"\n".join(lines[4 * lo:4 * hi]) + b"\n")
        samples.append(("third%d" % n, str(fq)))
    return dict(prefix=os.path.join(ftiny_dir, "idx"), snps=os.path.join(ftiny_dir, "snps.vcf"), samples=samples)


@pytest.mark.parametrize("route", ["device", "host"])
def test_geno_writes_the_index_of_the_golden_text(ftiny_dir, tmp_path, route):
    golden = gzip.open(os.path.join(GOLDEN, "ftiny.out.vcf.gz"), "rb").read()
    z, want = _definition(golden)
    out = tmp_path / "out.vcf.gz"
    p = subprocess.run([BIN, "geno", os.path.join(ftiny_dir, "idx"), os.path.join(ftiny_dir, "reads.fq"), os.path.join(ftiny_dir, "snps.vcf"), str(out)], env=_env(route), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert out.read_bytes() == z
    assert _tbi(out) == want
    said = [ln for ln in p.stderr.splitlines() if ln.startswith("vcf index: ")]
    assert len(said) == 1 and said[0].startswith("vcf index: %s, %d data lines, 2 chromosomes" % (route, len(T.data_lines(golden)))), p.stderr


@pytest.mark.parametrize("route", ["device", "host"])
def test_cohort_writes_one_index_per_sample(cohort, tmp_path, route):
    outs = [tmp_path / ("%s.vcf.gz" % name) for name, _ in cohort["samples"]]
    manifest = tmp_path / "manifest.tsv"
    manifest.write_text("".join("%s\t%s\n" % (fq, out) for (_, fq), out in zip(cohort["samples"], outs)))
    p = subprocess.run([BIN, "cohort", cohort["prefix"], str(manifest), cohort["snps"]], env=_env(route), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    for out in outs:
        text = gzip.decompress(out.read_bytes())
        z, want = _definition(text)
        assert out.read_bytes() == z and _tbi(out) == want, out


def _joint(cohort, out, env):
    manifest = out.parent / (out.name + ".manifest.tsv")
    manifest.write_text("".join("%s\t%s\n" % (fq, name) for name, fq in cohort["samples"]))
    p = subprocess.run([BIN, "joint", cohort["prefix"], str(manifest), cohort["snps"], str(out)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    return p.stderr


def test_joint_stream_and_host_text_write_the_same_file_and_the_same_index(cohort, tmp_path):
    """VARGENO_JOINT_TEXT=device + VARGENO_VCF_BGZF=device (the rendered text is scanned on the device, where alone it is) against
    VARGENO_JOINT_TEXT=host on both compressing routes, and against the run without the switch; the pair table is left alone."""
    base, tsv0 = tmp_path / "base.vcf.gz", tmp_path / "pairs0.tsv"
    _joint(cohort, base, _env("device", index=False, VARGENO_JOINT_PAIRS=str(tsv0)))
    assert not os.path.exists(str(base) + ".tbi")
    z, want = _definition(gzip.decompress(base.read_bytes()))
    assert base.read_bytes() == z
    runs = {"stream": _env("device", VARGENO_JOINT_TEXT="device", VARGENO_JOINT_TEXT_LINES="97"), "host text, device": _env("device", VARGENO_JOINT_TEXT="host"),
            "host text, host": _env("host", VARGENO_JOINT_TEXT="host")}
    for name, env in runs.items():
        out, tsv = tmp_path / (name.replace(", ", "_").replace(" ", "_") + ".vcf.gz"), tmp_path / "pairs.tsv"
        err = _joint(cohort, out, dict(env, VARGENO_JOINT_PAIRS=str(tsv)))
        assert out.read_bytes() == z, name
        assert _tbi(out) == want, name
        assert tsv.read_bytes() == tsv0.read_bytes() and not os.path.exists(str(tsv) + ".tbi"), name
        assert ("vcf index: device stream" in err) == (name == "stream"), err

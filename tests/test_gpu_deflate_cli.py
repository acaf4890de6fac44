"""VARGENO_VCF_BGZF behind the command line: `geno`, `cohort` and `joint` write their VCF as BGZF -- the very bytes of
vg_bgzf_deflate_host over the whole text, on the `device` route and on the `host` route -- and what the file inflates to is the
VCF the same job writes as plain text.  The pair table is not touched by it."""
import gzip
import os
import subprocess

import pytest

from conftest import BIN, GOLDEN
from vargeno_amd import api

pytestmark = pytest.mark.gpu

BASE = dict(VARGENO_CHUNK_MB="1", VARGENO_BATCH="900", VARGENO_PACK_THREADS="2", VARGENO_SHARE_DEVICES="1", VARGENO_VERBOSE="1", VARGENO_BGZF_THREADS="3")
ROUTES = ["device", "host"]


def _env(route=None, **more):
    e = {k: v for k, v in os.environ.items() if k != "VARGENO_VCF_BGZF"}
    e.update(BASE)
    if route:
        e["VARGENO_VCF_BGZF"] = route
    e.update(more)
    return e


@pytest.fixture(scope="module")
def cohort(ftiny_dir, tmp_path_factory):
    """The small cohort of tests/test_gpu_joint_cli.py: F-tiny's reads whole and two thirds of them, as three samples."""
    d = tmp_path_factory.mktemp("deflate_cohort")
    whole = os.path.join(ftiny_dir, "reads.fq")
    lines = open(whole, "rb").read().split(b"\n")[:-1]
    samples = [("whole", whole)]
    for n, (lo, hi) in enumerate(((0, 1333), (1333, 2666))):
        fq = d / ("third%d.fq" % n)
        fq.write_bytes(b"\n".join(lines[4 * lo:4 * hi]) + b"\n")
        samples.append(("third%d" % n, str(fq)))
    return dict(prefix=os.path.join(ftiny_dir, "idx"), snps=os.path.join(ftiny_dir, "snps.vcf"), samples=samples)


def test_geno_writes_the_golden_vcf_as_bgzf_on_both_routes(ftiny_dir, tmp_path):
    golden = gzip.open(os.path.join(GOLDEN, "ftiny.out.vcf.gz"), "rb").read()
    want = api.bgzf_deflate(golden, device=None)
    for route in ROUTES:
        out = tmp_path / (route + ".vcf.gz")
        p = subprocess.run([BIN, "geno", os.path.join(ftiny_dir, "idx"), os.path.join(ftiny_dir, "reads.fq"), os.path.join(ftiny_dir, "snps.vcf"), str(out)],
                           env=_env(route), capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        data = out.read_bytes()
        assert gzip.decompress(data) == golden, route
        assert data == want, route


def _joint(cohort, out, env):
    manifest = out.parent / (out.name + ".manifest.tsv")
    manifest.write_text("".join("%s\t%s\n" % (fq, name) for name, fq in cohort["samples"]))
    p = subprocess.run([BIN, "joint", cohort["prefix"], str(manifest), cohort["snps"], str(out)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    return out.read_bytes()


@pytest.fixture(scope="module")
def plain_joint(cohort, tmp_path_factory):
    """What the job writes without the variable: the joint VCF and the pair table."""
    d = tmp_path_factory.mktemp("plain_joint")
    vcf = _joint(cohort, d / "joint.vcf", _env(VARGENO_JOINT_PAIRS=str(d / "pairs.tsv")))
    assert vcf.startswith(b"##") and vcf.count(b"\n") > 2000
    return vcf, (d / "pairs.tsv").read_bytes()


@pytest.mark.parametrize("route", ROUTES)
def test_joint_writes_the_same_vcf_as_bgzf(cohort, plain_joint, tmp_path, route):
    data = _joint(cohort, tmp_path / "joint.vcf.gz", _env(route))
    assert gzip.decompress(data) == plain_joint[0]
    assert data == api.bgzf_deflate(plain_joint[0], device=None)


def test_joint_with_the_pair_table_leaves_the_table_alone(cohort, plain_joint, tmp_path):
    table = tmp_path / "pairs.tsv"
    data = _joint(cohort, tmp_path / "joint.vcf.gz", _env("device", VARGENO_JOINT_PAIRS=str(table)))
    assert gzip.decompress(data) == plain_joint[0]
    assert table.read_bytes() == plain_joint[1] and plain_joint[1].startswith(b"##sites")


@pytest.mark.parametrize("route", ROUTES)
def test_cohort_writes_every_samples_vcf_as_bgzf(cohort, tmp_path, route):
    def run(tag, env):
        outs = [tmp_path / ("%s.%s.vcf" % (name, tag)) for name, _ in cohort["samples"]]
        manifest = tmp_path / (tag + ".manifest.tsv")
        manifest.write_text("".join("%s\t%s\n" % (fq, out) for (_, fq), out in zip(cohort["samples"], outs)))
        p = subprocess.run([BIN, "cohort", cohort["prefix"], str(manifest), cohort["snps"]], env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        return [o.read_bytes() for o in outs]

    plain = run("plain", _env(VARGENO_COHORT_INFLIGHT="2"))
    packed = run("bgzf", _env(route, VARGENO_COHORT_INFLIGHT="2"))
    for text, data in zip(plain, packed):
        assert text.startswith(b"##") and gzip.decompress(data) == text
        assert data == api.bgzf_deflate(text, device=None)


def test_bgzfzip_on_the_device_route(tmp_path):
    """The sink's device route over more than one span (16 MiB of text each), cut where the blocks are."""
    text = gzip.open(os.path.join(GOLDEN, "fdense.out.vcf.gz"), "rb").read() * 9
    src, dst = tmp_path / "in.vcf", tmp_path / "out.vcf.gz"
    src.write_bytes(text)
    p = subprocess.run([BIN, "bgzfzip", str(src), str(dst)], env=_env("device"), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert "device route" in p.stderr, p.stderr
    assert dst.read_bytes() == api.bgzf_deflate(text, device=None)

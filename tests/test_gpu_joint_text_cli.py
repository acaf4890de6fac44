"""`VARGENO_JOINT_TEXT=device` behind the command line: `vargeno joint` on F-tiny with the three samples of test_gpu_joint_cli.py,
and the hidden `jointvcf` over the scenarios of test_joint_text_cpu.py, must write the very bytes of the run without the variable
(the present writer), as plain text and through the handle's BGZF stream."""
import gzip
import os
import subprocess

import pytest

import test_joint_text_cpu as CPU
from conftest import BIN, GOLDEN

pytestmark = pytest.mark.gpu

BASE = dict(VARGENO_CHUNK_MB="1", VARGENO_BATCH="900", VARGENO_PACK_THREADS="2", VARGENO_SHARE_DEVICES="1", VARGENO_VERBOSE="1", VARGENO_COHORT_INFLIGHT="3")
OUTPUTS = {"plain": {}, "fixed": {"VARGENO_VCF_BGZF": "device", "VARGENO_VCF_CODES": "fixed"}, "dynamic": {"VARGENO_VCF_BGZF": "device", "VARGENO_VCF_CODES": "dynamic"}}


def _joint(inputs, manifest, out, env):
    p = subprocess.run([BIN, "joint", inputs["prefix"], str(manifest), inputs["snps"], str(out)], env=dict(os.environ, **dict(BASE, **env)), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    return p.stderr


@pytest.fixture(scope="module")
def inputs(ftiny_dir, tmp_path_factory):
    """The three samples' FASTQ files, and the joint file of the run without VARGENO_JOINT_TEXT in every output mode: made once."""
    d = tmp_path_factory.mktemp("joint_text_in")
    whole = os.path.join(ftiny_dir, "reads.fq")
    lines = open(whole, "rb").read().split(b"\n")[:-1]
    manifest = d / "manifest.tsv"
    rows = ["%s\twhole\n" % whole]
    for n, (lo, hi) in enumerate(((0, 1333), (1333, 2666))):
        fq = d / ("third%d.fq" % n)
        fq.write_bytes(b"\n".join(lines[4 * lo:4 * hi]) + b"\n")
        rows.append("%s\tthird%d\n" % (fq, n))
    manifest.write_text("".join(rows))
    donor = d / "donor.tsv"
    donor.write_text("%s\tDONOR\n" % whole)
    inp = dict(prefix=os.path.join(ftiny_dir, "idx"), snps=os.path.join(ftiny_dir, "snps.vcf"), manifest=manifest, donor=donor, base={})
    for how, env in OUTPUTS.items():
        out = d / ("base.%s" % how)
        assert "joint text" not in _joint(inp, manifest, out, env)
        inp["base"][how] = out.read_bytes()
    assert inp["base"]["plain"].count(b"\tGT:GQ\t") > 2000
    for how in ("fixed", "dynamic"):
        assert gzip.decompress(inp["base"][how]) == inp["base"]["plain"]
    return inp


@pytest.mark.parametrize("lines", ["97", None])
@pytest.mark.parametrize("how", list(OUTPUTS))
def test_joint_on_the_device_writes_the_present_writers_bytes(inputs, tmp_path, how, lines):
    env = dict(OUTPUTS[how], VARGENO_JOINT_TEXT="device")
    if lines:
        env["VARGENO_JOINT_TEXT_LINES"] = lines
    out = tmp_path / "joint.out"
    err = _joint(inputs, inputs["manifest"], out, env)
    assert "joint text: device" in err, err
    assert ("(BGZF stream)" in err) == (how != "plain"), err
    got = out.read_bytes()
    assert got == inputs["base"][how]
    if how != "plain":
        assert gzip.decompress(got) == inputs["base"]["plain"]
    said = [ln for ln in err.splitlines() if ln.startswith("joint text: device")][0]
    assert "%d lines written" % inputs["base"]["plain"].count(b"\tGT:GQ\t") in said and "%d text bytes" % sum(len(ln) + 1 for ln in inputs["base"]["plain"].split(b"\n") if ln and ln[:1] != b"#") in said, said


def test_the_single_sample_donor_is_the_references_file(inputs, tmp_path):
    out = tmp_path / "donor.vcf"
    err = _joint(inputs, inputs["donor"], out, {"VARGENO_JOINT_TEXT": "device"})
    assert "joint text: device" in err, err
    assert out.read_bytes() == gzip.open(os.path.join(GOLDEN, "ftiny.out.vcf.gz"), "rb").read()


def test_the_pair_table_is_unchanged(inputs, tmp_path):
    tables = []
    for k, env in enumerate(({}, {"VARGENO_JOINT_TEXT": "device"})):
        out, tsv = tmp_path / ("joint%d.vcf" % k), tmp_path / ("pairs%d.tsv" % k)
        _joint(inputs, inputs["manifest"], out, dict(env, VARGENO_JOINT_PAIRS=str(tsv)))
        assert out.read_bytes() == inputs["base"]["plain"]
        tables.append(tsv.read_bytes())
    assert tables[0] == tables[1] and tables[0].count(b"\n") > 5


SCENARIOS = ["one sample", "three samples", "chr names", "repeated records", "one name twice", "header lines in the data", "crlf", "no final newline", "no final newline, short line",
             "declared, with sample columns"]


@pytest.mark.parametrize("name", SCENARIOS)
def test_jointvcf_on_the_device_over_the_cpu_scenarios(tmp_path, name):
    """Plain text in spans of 97 records and of the default size (the small lists also a record per span), and the BGZF stream in
    both coding modes."""
    scenarios = CPU._scenarios(tmp_path)
    assert sorted(scenarios) == sorted(SCENARIOS)
    chrlens, src, samples, env = scenarios[name]
    small = os.path.getsize(src) < 20_000
    for how, out_env in OUTPUTS.items():
        base, out = str(tmp_path / "base.out"), str(tmp_path / "dev.out")
        p = CPU._jointvcf(chrlens, src, samples, base, dict(env, **out_env))
        assert p.returncode == 0, (name, how, p.stderr)
        for lines in ((("1",) if small else ()) + ("97", None) if how == "plain" else ("97",)):
            e = dict(env, VARGENO_JOINT_TEXT="device", VARGENO_VERBOSE="1", **out_env)
            if lines:
                e["VARGENO_JOINT_TEXT_LINES"] = lines
            p = CPU._jointvcf(chrlens, src, samples, out, e)
            assert p.returncode == 0 and "joint text: device" in p.stderr, (name, how, lines, p.stderr)
            assert open(out, "rb").read() == open(base, "rb").read(), (name, how, lines)

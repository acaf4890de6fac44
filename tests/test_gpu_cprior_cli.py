"""`VARGENO_JOINT_PRIOR=cohort` behind the command line on F-tiny with the three samples of test_gpu_joint_info_cli.py: `vargeno joint`
re-calls the columns on the device and writes the bytes of VARGENO_JOINT_PRIOR_ROUTE=host, which differ from the file without the
variable; and the device text route with the INFO counts takes the re-called columns as the host text route does."""
import os
import subprocess

import pytest

from conftest import BIN

pytestmark = pytest.mark.gpu

BASE = dict(VARGENO_CHUNK_MB="1", VARGENO_BATCH="900", VARGENO_PACK_THREADS="2", VARGENO_SHARE_DEVICES="1", VARGENO_VERBOSE="1", VARGENO_COHORT_INFLIGHT="3", VARGENO_BGZF_THREADS="3")
PRIOR = {"VARGENO_JOINT_PRIOR": "cohort"}
HEADER_LINE = b"##vargenoPrior=cohort,iters=8,pseudo=2\n"
OURS = ("VARGENO_VCF_BGZF", "VARGENO_VCF_INDEX", "VARGENO_JOINT_TEXT", "VARGENO_JOINT_INFO", "VARGENO_JOINT_PRIOR", "VARGENO_JOINT_PRIOR_ROUTE", "VARGENO_JOINT_PAIRS")


def _joint(inputs, out, env):
    e = {k: v for k, v in os.environ.items() if k not in OURS}
    p = subprocess.run([BIN, "joint", inputs["prefix"], str(inputs["manifest"]), inputs["snps"], str(out)], env=dict(e, **dict(BASE, **env)), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    return p.stderr


@pytest.fixture(scope="module")
def inputs(ftiny_dir, tmp_path_factory):
    """The three samples, the file without the variable and the file of the host route."""
    d = tmp_path_factory.mktemp("joint_prior_in")
    whole = os.path.join(ftiny_dir, "reads.fq")
    lines = open(whole, "rb").read().split(b"\n")[:-1]
    rows = ["%s\twhole\n" % whole]
    for n, (lo, hi) in enumerate(((0, 1333), (1333, 2666))):
        fq = d / ("third%d.fq" % n)
        fq.write_bytes(b"\n".join(lines[4 * lo:4 * hi]) + b"\n")
        rows.append("%s\tthird%d\n" % (fq, n))
    manifest = d / "manifest.tsv"
    manifest.write_text("".join(rows))
    inp = dict(prefix=os.path.join(ftiny_dir, "idx"), snps=os.path.join(ftiny_dir, "snps.vcf"), manifest=manifest)
    assert "cohort prior" not in _joint(inp, d / "plain.vcf", {})
    err = _joint(inp, d / "host.vcf", dict(PRIOR, VARGENO_JOINT_PRIOR_ROUTE="host"))
    assert "cohort prior: host (" in err and "cohort prior: device" not in err, err
    inp["plain"], inp["host"] = (d / "plain.vcf").read_bytes(), (d / "host.vcf").read_bytes()
    return inp


def _cells(text):
    return {tuple(ln.split(b"\t")[:2]): ln.split(b"\t")[9:] for ln in text.split(b"\n") if ln and ln[:1] != b"#"}


def test_the_device_route_writes_the_host_routes_bytes_and_other_cells_than_before(inputs, tmp_path):
    out = tmp_path / "device.vcf"
    err = _joint(inputs, out, PRIOR)
    assert "cohort prior: device, " in err and " 3 samples, " in err and "cohort prior: host" not in err, err
    got = out.read_bytes()
    assert got == inputs["host"]
    assert got.count(HEADER_LINE) == 1 and got.index(HEADER_LINE) + len(HEADER_LINE) == got.index(b"#CHROM") and HEADER_LINE not in inputs["plain"]
    old, new = _cells(inputs["plain"]), _cells(got)
    assert old.keys() == new.keys() and len(new) > 2000                         # the same sites are called ...
    assert sum(1 for k in new if new[k] != old[k]) >= 1                         # ... and at least one cell is another


def test_the_device_text_route_with_the_counts_takes_the_recalled_columns(inputs, tmp_path):
    host, dev = tmp_path / "host_text.vcf", tmp_path / "device_text.vcf"
    info = dict(PRIOR, VARGENO_JOINT_INFO="counts")
    _joint(inputs, host, dict(info, VARGENO_JOINT_PRIOR_ROUTE="host"))
    err = _joint(inputs, dev, dict(info, VARGENO_JOINT_TEXT="device", VARGENO_JOINT_PAIRS=str(tmp_path / "pairs.tsv")))
    assert "cohort prior: device, " in err and "joint text: device, info counts, " in err, err
    got = dev.read_bytes()
    assert got == host.read_bytes() and got.count(HEADER_LINE) == 1 and got.count(b";AF=") + got.count(b"\tNS=") > 2000
    assert _cells(got) == _cells(inputs["host"])
    assert (tmp_path / "pairs.tsv").read_bytes().count(b"\n") > 5

"""`VARGENO_JOINT_INFO=counts` behind the command line on F-tiny with the three samples of test_gpu_joint_text_cli.py: `vargeno joint`
with VARGENO_JOINT_TEXT=device writes the bytes of the `host` route, as plain text and through the handle's BGZF stream, whose .tbi
is the `host` route's."""
import gzip
import os
import subprocess

import pytest

import jinfo_cases as JI
from conftest import BIN

pytestmark = pytest.mark.gpu

BASE = dict(VARGENO_CHUNK_MB="1", VARGENO_BATCH="900", VARGENO_PACK_THREADS="2", VARGENO_SHARE_DEVICES="1", VARGENO_VERBOSE="1", VARGENO_COHORT_INFLIGHT="3", VARGENO_BGZF_THREADS="3")
INFO = {"VARGENO_JOINT_INFO": "counts"}


def _joint(inputs, out, env):
    e = {k: v for k, v in os.environ.items() if k not in ("VARGENO_VCF_BGZF", "VARGENO_VCF_INDEX", "VARGENO_JOINT_TEXT", "VARGENO_JOINT_INFO")}
    p = subprocess.run([BIN, "joint", inputs["prefix"], str(inputs["manifest"]), inputs["snps"], str(out)], env=dict(e, **dict(BASE, **env)), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    return p.stderr


@pytest.fixture(scope="module")
def inputs(ftiny_dir, tmp_path_factory):
    """The three samples, and the `host` route's file with the variable set: BGZF with its index, and the text it holds."""
    d = tmp_path_factory.mktemp("joint_info_in")
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
    z = d / "host.vcf.gz"
    assert "joint text" not in _joint(inp, z, dict(INFO, VARGENO_VCF_BGZF="host", VARGENO_VCF_INDEX="tbi"))
    inp["plain"], inp["tbi"] = gzip.decompress(z.read_bytes()), open(str(z) + ".tbi", "rb").read()      # (one run: the text is what the file inflates to)
    return inp


def test_joint_on_the_device_writes_the_host_routes_counted_bytes(inputs, tmp_path):
    out = tmp_path / "device.vcf"
    err = _joint(inputs, out, dict(INFO, VARGENO_JOINT_TEXT="device", VARGENO_JOINT_TEXT_LINES="97"))
    assert "joint text: device, info counts, " in err, err
    got = out.read_bytes()
    assert got == inputs["plain"]
    # the host route's file is the counted one: every line's tag holds the line's own counts (test_joint_info_cpu.py has the rest)
    _, found = JI.strip_info(got)
    assert len(found) == got.count(b"\tGT:GQ\t") > 2000 and all(got.count(d) == 1 for d in JI.INFO_DECL)
    assert all((ns, an, ac) == JI.cells_counts(ln) and af == JI.af_text(ac, an).encode() for ln, ns, an, ac, af in found)
    assert len({ns for _, ns, _, _, _ in found}) >= 2                          # lines that differ in how many samples are called


def test_the_stream_inflates_to_those_bytes_and_its_index_is_the_host_routes(inputs, tmp_path):
    out = tmp_path / "stream.vcf.gz"
    err = _joint(inputs, out, dict(INFO, VARGENO_JOINT_TEXT="device", VARGENO_VCF_BGZF="device", VARGENO_VCF_INDEX="tbi", VARGENO_JOINT_PAIRS=str(tmp_path / "pairs.tsv")))
    assert "joint text: device (BGZF stream), info counts, " in err and "vcf index: device stream" in err, err
    assert gzip.decompress(out.read_bytes()) == inputs["plain"]
    assert open(str(out) + ".tbi", "rb").read() == inputs["tbi"]
    assert (tmp_path / "pairs.tsv").read_bytes().count(b"\n") > 5

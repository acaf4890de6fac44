"""VARGENO_VCF_CODES=dynamic behind the command line: `geno` writes its VCF as BGZF with dynamic Huffman codes -- the very bytes of
vg_bgzf_deflate_host_coded(..., VG_DEFLATE_DYNAMIC, ...) over the whole text -- on the `device` route and on the `host` route, and
`bgzfzip` does on the device route over more than one span."""
import gzip
import os
import subprocess

import pytest

from conftest import BIN, GOLDEN
from vargeno_amd import api

pytestmark = pytest.mark.gpu

BASE = dict(VARGENO_CHUNK_MB="1", VARGENO_BATCH="900", VARGENO_PACK_THREADS="2", VARGENO_SHARE_DEVICES="1", VARGENO_VERBOSE="1", VARGENO_BGZF_THREADS="3")


def _env(route, codes):
    e = {k: v for k, v in os.environ.items() if k not in ("VARGENO_VCF_BGZF", "VARGENO_VCF_CODES")}
    e.update(BASE, VARGENO_VCF_BGZF=route, VARGENO_VCF_CODES=codes)
    return e


def test_geno_writes_the_golden_vcf_with_dynamic_codes_on_both_routes(ftiny_dir, tmp_path):
    golden = gzip.open(os.path.join(GOLDEN, "ftiny.out.vcf.gz"), "rb").read()
    want = api.bgzf_deflate(golden, device=None, codes="dynamic")
    assert want != api.bgzf_deflate(golden, device=None)
    for route in ("device", "host"):
        out = tmp_path / (route + ".vcf.gz")
        p = subprocess.run([BIN, "geno", os.path.join(ftiny_dir, "idx"), os.path.join(ftiny_dir, "reads.fq"), os.path.join(ftiny_dir, "snps.vcf"), str(out)],
                           env=_env(route, "dynamic"), capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        data = out.read_bytes()
        assert gzip.decompress(data) == golden, route
        assert data == want, route


def test_bgzfzip_on_the_device_route_with_dynamic_codes(tmp_path):
    """The sink's device route over more than one span (16 MiB of text each), cut where the blocks are."""
    text = gzip.open(os.path.join(GOLDEN, "fdense.out.vcf.gz"), "rb").read() * 9
    src, dst = tmp_path / "in.vcf", tmp_path / "out.vcf.gz"
    src.write_bytes(text)
    p = subprocess.run([BIN, "bgzfzip", str(src), str(dst)], env=_env("device", "dynamic"), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert "device route, dynamic codes" in p.stderr, p.stderr
    assert dst.read_bytes() == api.bgzf_deflate(text, device=None, codes="dynamic")

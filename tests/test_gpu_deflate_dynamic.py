"""The dynamic mode's kernel (vg_bgzf_deflate_dyn_kernel: one wave per BGZF block; vg_deflate_block_dyn under its wave policy) and
the code-length builder's kernel against the host build of the same core: the device's bytes ARE the host's bytes.  That the
host's bytes are right is tests/test_deflate_dynamic_cpu.py's business."""
import numpy as np
import pytest

import deflate_cases as DC
import deflate_dyn_cases as DD
from vargeno_amd import api

pytestmark = pytest.mark.gpu

TEXT = dict(DC.cases() + DD.new_cases())
SHARED = [n for n, _ in DD.new_cases()] + ["len_311", "periods_2_3_5", "distance_32768", "high_bytes", "random_65280", "ftiny.out.vcf.gz", "fquirk.out.vcf.gz"]
CASES = [(n, b) for n in SHARED for b in (311, 4096, 65280)] + [("ftiny_reads", 311), ("len_8", 1)]


@pytest.fixture(scope="module")
def host_files():
    """The host's dynamic files, made once"""
    return {(n, b): api.bgzf_deflate(TEXT[n], device=None, block=b, codes="dynamic") for n, b in CASES}


@pytest.mark.parametrize("name,block", CASES, ids=["%s-%d" % c for c in CASES])
def test_device_bytes_are_the_host_bytes(name, block, host_files):
    """Among them: blocks of one group of positions and of one more byte, a block that is stored, one with every symbol in use (the
    largest header), one with a token that straddles three words of the window, and F-tiny's reads at 311 bytes a block (some 3 400
    waves, far more than the device has CUs)."""
    assert api.bgzf_deflate(TEXT[name], device=0, block=block, codes="dynamic") == host_files[(name, block)]


def test_the_fixed_mode_on_the_device_is_unchanged():
    text = TEXT["ftiny.out.vcf.gz"]
    want = api.bgzf_deflate(text, device=None)
    assert api.bgzf_deflate(text, device=0) == want and api.bgzf_deflate(text, device=0, codes="fixed") == want
    assert want != api.bgzf_deflate(text, device=None, codes="dynamic")


def test_device_to_device(host_files):
    text = TEXT["ftiny.out.vcf.gz"]
    out = api.bgzf_deflate(text, device=0, codes="dynamic")
    assert out == host_files[("ftiny.out.vcf.gz", 65280)]
    got, consumed, bad = api.bgzf_inflate(out, device=0)
    assert bad is None and consumed == len(out)
    assert got == text


def test_without_the_marker_and_in_pieces(host_files):
    text = TEXT["ftiny.out.vcf.gz"]
    whole = host_files[("ftiny.out.vcf.gz", 4096)]
    z = lambda t, **kw: api.bgzf_deflate(t, device=0, block=4096, codes="dynamic", **kw)
    assert z(text, eof=False) + DC.EOF_MARKER == whole
    cut = 3 * 4096
    assert z(text[:cut], eof=False) + z(text[cut:]) == whole


def test_more_text_than_one_chunk_of_the_device_call():
    """The device call works through chunks of 64 MiB of text (1 028 blocks of 65 280 bytes): 70 MB is two of them."""
    text = TEXT["fdense.out.vcf.gz"] * 31 + b"tail\n"
    assert len(text) > 1028 * 65280 + 65280
    assert api.bgzf_deflate(text, device=0, codes="dynamic") == api.bgzf_deflate(text, device=None, codes="dynamic")


@pytest.mark.parametrize("limit", [7, 15])
def test_code_lengths_on_the_device_are_the_hosts(limit):
    """One wave per histogram; the histograms of the CPU tests, Fibonacci counts (which need the limit) among them, in one call per
    alphabet size."""
    by_size = {}
    for name, freq in DD.histograms():
        if len(freq) <= 1 << limit:
            by_size.setdefault(len(freq), []).append(freq)
    assert len(by_size) >= 5
    for n_sym, rows in by_size.items():
        f = np.array(rows, dtype=np.uint32)
        dev = api.deflate_code_lengths(f, limit=limit, device=0)
        assert dev.shape == f.shape and (dev == api.deflate_code_lengths(f, limit=limit, device=None)).all(), n_sym

"""The deflate kernel (one wave per BGZF block; vargeno_amd/csrc/vg_deflate.h under its wave policy) against the host build of the
same core: the device's bytes ARE the host's bytes, for every text and block length of tests/deflate_cases.py.  That the host's
bytes are right is tests/test_deflate_cpu.py's business (Python's zlib and the host inflater read them back)."""
import gzip
import os

import pytest

import deflate_cases as DC
from conftest import GOLDEN
from vargeno_amd import api

pytestmark = pytest.mark.gpu

CASES = DC.cases()
NAMES = DC.names()


@pytest.mark.parametrize("block", DC.BLOCK_SIZES)
@pytest.mark.parametrize("case", range(len(CASES)), ids=NAMES)
def test_device_bytes_are_the_host_bytes(case, block):
    """Among them: no block and one, two blocks, blocks of one group of positions and of 1 020, F-tiny's reads at 311 bytes a
    block (some 3 400 waves, far more than the device has CUs), and at one byte a block (a million waves in sixteen launches)."""
    text = CASES[case][1]
    assert api.bgzf_deflate(text, device=0, block=block) == api.bgzf_deflate(text, device=None, block=block)


def test_without_the_marker_and_in_pieces():
    text = dict(CASES)["ftiny_reads"]
    whole = api.bgzf_deflate(text, device=None, block=4096)
    assert api.bgzf_deflate(text, device=0, block=4096, eof=False) + DC.EOF_MARKER == whole
    cut = 3 * 4096
    assert api.bgzf_deflate(text[:cut], device=0, block=4096, eof=False) + api.bgzf_deflate(text[cut:], device=0, block=4096) == whole


def test_more_text_than_one_chunk_of_the_device_call():
    """The device call works through chunks of 64 MiB of text (1 028 blocks of 65 280 bytes): 70 MB is two of them."""
    text = dict(CASES)["fdense.out.vcf.gz"] * 31 + b"tail\n"
    assert len(text) > 1028 * 65280 + 65280
    out = api.bgzf_deflate(text, device=0)
    assert out == api.bgzf_deflate(text, device=None)


def test_device_to_device():
    text = gzip.open(os.path.join(GOLDEN, "ftiny.out.vcf.gz"), "rb").read()
    out = api.bgzf_deflate(text, device=0)
    got, consumed, bad = api.bgzf_inflate(out, device=0)
    assert bad is None and consumed == len(out)
    assert got == text


def test_capacity_one_byte_short_is_refused_and_nothing_is_written():
    import ctypes as C

    import numpy as np

    from vargeno_amd import _lib

    text = dict(CASES)["ftiny.out.vcf.gz"]
    want = api.bgzf_deflate(text, device=None)
    a = np.frombuffer(text, dtype=np.uint8)
    for cap, code in ((len(want), "ok"), (len(want) - 1, "VG_ETOOBIG")):
        buf = np.full(cap + 4096, 0xA5, dtype=np.uint8)
        n = C.c_uint64()
        rc = _lib.lib().vg_bgzf_deflate_device(0, a.ctypes.data, len(text), 0, 1, buf.ctypes.data, cap, C.byref(n))
        if code == "ok":
            assert rc == 0 and buf[:cap].tobytes() == want and (buf[cap:] == 0xA5).all()
        else:
            assert _lib.VG_ERRORS[rc] == code and (buf == 0xA5).all()

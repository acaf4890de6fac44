"""BGZF on the host: the header walk, the host build of the inflate core (vargeno_amd/csrc/vg_inflate.h -- the source the device
kernel is compiled from), the command line's `bgzfcat`, and the core alone under AddressSanitizer + UBSan (tests/inflate_fuzz.cpp).
No device is touched.  Expected text is always what the inputs were made from / what Python's zlib says, never the code under test."""
import os
import subprocess

import numpy as np
import pytest

import bgzf_cases as BC
from conftest import BIN, ROOT
from vargeno_amd import api

VALID = BC.valid_cases()
DAMAGED = BC.damaged_cases()


@pytest.mark.parametrize("case", range(len(VALID)), ids=[c[0] for c in VALID])
def test_host_inflate_is_byte_exact(case):
    _, data, text = VALID[case]
    got, consumed, bad = api.bgzf_inflate(data, device=None)
    assert bad is None and consumed == len(data)
    assert got == text


@pytest.mark.parametrize("case", range(len(VALID)), ids=[c[0] for c in VALID])
def test_bgzfcat_writes_the_text(case, tmp_path):
    _, data, text = VALID[case]
    f = tmp_path / "in.fq.gz"
    f.write_bytes(data)
    p = subprocess.run([BIN, "bgzfcat", str(f)], capture_output=True, timeout=60)
    assert p.returncode == 0, p.stderr
    assert p.stdout == text


@pytest.mark.parametrize("case", range(len(VALID)), ids=[c[0] for c in VALID])
def test_scan_through_arbitrary_cuts_reports_the_same_blocks(case):
    """The header walk over bytes cut anywhere: pieces of 1, 2, 17, 18, 19 and 4 096 bytes are appended to what the walk left
    unconsumed, as the library's stream does; the blocks found must be those of one walk over the whole file."""
    _, data, _ = VALID[case]
    whole, used, bad = api.bgzf_scan(data)
    assert bad is None and used == len(data)
    assert [b[0] for b in whole] == [off for off, _ in BC.split_blocks(data)]
    for step in (1, 2, 17, 18, 19, 4096):
        if step < 17 and len(data) > 40_000:
            part = data[:40_000]                                  # (tiny steps over the head of a large file: each step walks the carry again)
            want = [b for b in whole if b[2] + b[3] + 8 <= len(part)]
        else:
            part, want = data, whole
        found, carry, base, text_base = [], b"", 0, 0
        for at in range(0, len(part), step):
            carry += part[at:at + step]
            blocks, used, bad = api.bgzf_scan(carry)
            assert bad is None
            for (c, t, po, pl, isz, crc) in blocks:
                found.append((base + c, text_base + t, base + po, pl, isz, crc))
            if blocks:
                text_base += blocks[-1][1] + blocks[-1][4]
            base += used
            carry = carry[used:]
        assert found == want, step
        assert carry == part[base:] and (part is not data or carry == b"")


def test_header_errors_are_reported_with_their_offset():
    good = VALID[0][1]
    blocks = BC.split_blocks(good)
    at = blocks[2][0]
    for name, bad_bytes in (("magic", b"\x1f\x8b\x08\x00"), ("flg", b"\x1f\x8b\x08\x0c")):
        data = good[:at] + bad_bytes + good[at + 4:]
        found, used, bad = api.bgzf_scan(data)
        assert (len(found), used, bad) == (2, at, at), name
        text, consumed, bad = api.bgzf_inflate(data, device=None)
        assert bad == at and text == VALID[0][2][:len(text)] and len(text) == sum(b[4] for b in found)
    # no BC subfield; a subfield that runs past XLEN; BSIZE smaller than header + trailer; ISIZE beyond 64 KiB
    blk = blocks[0][1]
    for name, b in (("no_bc", blk[:12] + b"BX" + blk[14:]), ("subfield_overrun", blk[:14] + b"\x07\x00" + blk[16:]),
                    ("bsize_small", blk[:16] + b"\x19\x00" + blk[18:]), ("isize_big", blk[:-4] + (65537).to_bytes(4, "little"))):
        found, used, bad = api.bgzf_scan(b + good)
        assert (found, used, bad) == ([], 0, 0), name


@pytest.mark.parametrize("base", sorted(DAMAGED))
def test_damaged_blocks_fail_or_agree_with_zlib(base):
    """Every damaged block returns an error, or succeeds only where Python's zlib accepts the same bytes with the same CRC and
    length.  Nothing is written beyond text_cap: the buffer carries a canary behind it."""
    good = VALID[3][1][:BC.split_blocks(VALID[3][1])[0][1].__len__()]        # one valid block in front
    good_text = VALID[3][2][:65280]
    for name, block, verdict in DAMAGED[base]:
        data = good + block + good
        isize = int.from_bytes(block[-4:], "little")
        cap = 2 * len(good_text) + isize
        buf = np.full(cap + 4096, 0xA5, dtype=np.uint8)
        text, consumed, bad = api.bgzf_inflate(data, device=None, out=buf, text_cap=cap)
        assert (buf[cap:] == 0xA5).all(), name
        if bad is None:
            assert verdict is not None, name
            assert text == good_text + verdict + good_text and consumed == len(data), name
        else:
            assert bad == len(good) and consumed == len(good) and text == good_text, name
    # a BSIZE that points past the data: the block is incomplete, not decoded, and not consumed
    block = DAMAGED[base][0][1]
    text, consumed, bad = api.bgzf_inflate(good + BC.bsize_past_the_data(block), device=None)
    assert (text, consumed, bad) == (good_text, len(good), None)


def test_text_that_does_not_fit_is_refused_before_anything_is_written():
    from vargeno_amd._lib import VgError

    _, data, text = VALID[3]
    buf = np.full(len(text), 0xA5, dtype=np.uint8)
    with pytest.raises(VgError) as e:
        api.bgzf_inflate(data, device=None, out=buf, text_cap=100_000)      # one block fits, the second does not
    assert e.value.code == -5
    assert (buf[100_000:] == 0xA5).all()


def test_plain_gzip_is_refused_by_name(tmp_path):
    """gzip magic without the BC subfield: one line that says only BGZF is inflated and that <(zcat FILE) works, a non-zero
    status, nothing on stdout -- before any device is asked for (`geno` says the same: tests/test_gpu_bgzf_cli.py)."""
    import gzip

    f = tmp_path / "plain.fq.gz"
    f.write_bytes(gzip.compress(BC.ftiny_text()[:5000]))
    for cmd in (["bgzfcat", str(f)], ["geno", str(tmp_path / "no_such_index"), str(f), str(tmp_path / "snps.vcf"), str(tmp_path / "out.vcf")]):
        p = subprocess.run([BIN] + cmd, capture_output=True, text=True, timeout=60)
        assert p.returncode != 0 and p.stdout == ""
        lines = [ln for ln in p.stderr.splitlines() if ln.strip()]
        assert len(lines) == 1 and "BGZF" in lines[0] and "<(zcat %s)" % f in lines[0], p.stderr
    assert not (tmp_path / "out.vcf").exists()


def test_inflate_core_under_sanitizers(tmp_path):
    """tests/inflate_fuzz.cpp: the host build of the core alone, built with -fsanitize=address,undefined and run directly, on
    20 000 seeded mutations (bit flips, truncations, length-field edits) of valid blocks with exactly-sized heap buffers."""
    exe = tmp_path / "inflate_fuzz"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe),
                    os.path.join(ROOT, "tests", "inflate_fuzz.cpp")], check=True, timeout=300)
    t = BC.ftiny_text()
    parts = [d for name, d, _ in VALID if name in ("ftiny_full_flush", "distance_32768", "isize_max", "short_periods", "random_stored")]
    parts += [BC.synth.bgzf_bytes(t[:200_000], **kw) for kw in (dict(level=0, block=65000), dict(strategy=BC.zlib.Z_FIXED), dict(level=6), dict(level=9))]
    f = tmp_path / "blocks.bgzf"
    f.write_bytes(b"".join(parts))
    p = subprocess.run([str(exe), str(f), "20000", "12345"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().endswith("ok"), p.stdout

"""BGZF output on the CPU: the host build of the compressor (vargeno_amd/csrc/vg_deflate.h, the one the device kernel is compiled
from) behind vg_bgzf_deflate_host, the command line's `bgzfzip` and VARGENO_VCF_BGZF, and the core alone under AddressSanitizer +
UBSan (tests/deflate_fuzz.cpp).  No device is touched.  What a file must inflate to is the text it was made from, and the judges
are Python's zlib and the library's own host inflater, never the compressor."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import deflate_cases as DC
from conftest import BIN, ROOT
from vargeno_amd import _lib, api

CASES = DC.cases()
NAMES = DC.names()


def _raw_host(text, block, eof, threads, cap, canary=0xA5, tail=4096):
    """vg_bgzf_deflate_host into a canary-filled buffer of cap + tail bytes: (return code, bytes written, the buffer)"""
    a = np.frombuffer(text, dtype=np.uint8) if text else np.zeros(1, dtype=np.uint8)
    buf = np.full(cap + tail, canary, dtype=np.uint8)
    n = C.c_uint64(12345)
    rc = _lib.lib().vg_bgzf_deflate_host(a.ctypes.data, len(text), block, eof, threads, buf.ctypes.data, cap, C.byref(n))
    return rc, int(n.value), buf


@pytest.mark.parametrize("block", DC.BLOCK_SIZES)
@pytest.mark.parametrize("case", range(len(CASES)), ids=NAMES)
def test_round_trip_by_two_independent_inflaters(case, block):
    """Every text at every block length: Python's zlib reads the file back block by block (header fields, BSIZE, ISIZE, CRC32, the
    end-of-file marker: deflate_cases.check_file), and so does vg_bgzf_inflate_host; the file fits vg_bgzf_deflate_bound."""
    text = CASES[case][1]
    out = api.bgzf_deflate(text, block=block)
    assert len(out) <= _lib.lib().vg_bgzf_deflate_bound(len(text), block)
    DC.check_file(out, text, block)
    got, consumed, bad = api.bgzf_inflate(out, device=None, text_cap=len(text))
    assert bad is None and consumed == len(out)
    assert got == text


def test_empty_text_is_the_marker_alone_or_nothing():
    assert api.bgzf_deflate(b"", eof=True) == DC.EOF_MARKER
    assert api.bgzf_deflate(b"", eof=False) == b""
    for name in ("len_311", "ftiny.out.vcf.gz"):
        text = dict(CASES)[name]
        with_eof, without = api.bgzf_deflate(text, eof=True), api.bgzf_deflate(text, eof=False)
        assert with_eof == without + DC.EOF_MARKER
        DC.check_file(without, text, 0, eof=False)


def test_random_bytes_come_out_stored():
    text = dict(CASES)["random_65280"]
    out = api.bgzf_deflate(text, eof=False)
    assert len(out) == 18 + 5 + 65280 + 8
    assert out[18] == 0x01 and out[19:23] == bytes.fromhex("00ffff00")      # BFINAL, BTYPE 00; LEN 65280, NLEN
    assert out[23:-8] == text


def test_a_repeat_at_the_windows_edge_is_used_and_one_byte_beyond_it_is_not():
    """A 300-byte repeat at distance 32 768 is coded as matches: the block is some hundred bytes shorter than with noise in the
    repeat's place.  At 32 769 the format has no distance for it: the block is as long as with noise there (300 random bytes cost
    8 or 9 bits each whatever they are: a few bytes of difference), and both inflaters read it (zlib refuses a distance beyond the
    window: test_round_trip_by_two_independent_inflaters)."""
    size = {(d, rep): len(api.bgzf_deflate(DC.far_repeat(d, rep), eof=False)) for d in (32768, 32769) for rep in (True, False)}
    assert all(s < 60000 for s in size.values()), size                       # coded, not stored
    assert size[(32768, True)] <= size[(32768, False)] - 250, size
    assert size[(32769, True)] >= size[(32769, False)] - 16, size


@pytest.mark.parametrize("name", [n for n in NAMES if n.endswith(".out.vcf.gz")])
def test_the_compressor_finds_matches(name):
    """Smaller than zlib's Z_HUFFMAN_ONLY over the same 65 280-byte blocks (plus 26 bytes each): no literal-only coder gets there."""
    text = dict(CASES)[name]
    out = api.bgzf_deflate(text)
    limit = DC.huffman_only_size(text)
    print("%s: %d bytes of text, %d as BGZF, %d by Z_HUFFMAN_ONLY" % (name, len(text), len(out), limit))
    assert len(out) < limit


@pytest.mark.parametrize("name,block", [("ftiny.out.vcf.gz", 0), ("ftiny_reads", 311), ("len_65281", 0), ("one_byte", 1)])
def test_capacity_one_byte_short_is_refused_and_nothing_is_written(name, block):
    text = dict(CASES)[name]
    want = api.bgzf_deflate(text, block=block)
    rc, n, buf = _raw_host(text, block, 1, 2, len(want))
    assert rc == 0 and n == len(want) and buf[:n].tobytes() == want and (buf[n:] == 0xA5).all()
    rc, n, buf = _raw_host(text, block, 1, 2, len(want) - 1)
    assert _lib.VG_ERRORS[rc] == "VG_ETOOBIG"
    assert (buf == 0xA5).all()
    assert b"fit" in _lib.lib().vg_last_error()


@pytest.mark.parametrize("name,block", [("ftiny_reads", 311), ("fsmall.out.vcf.gz", 0), ("run_131072", 4096), ("periods_2_3_5", 7)])
def test_the_bytes_do_not_depend_on_the_number_of_threads(name, block):
    text = dict(CASES)[name]
    assert api.bgzf_deflate(text, block=block, threads=1) == api.bgzf_deflate(text, block=block, threads=5)


@pytest.mark.parametrize("name,block", [("ftiny_reads", 311), ("ftiny_reads", 4096), ("fdense.out.vcf.gz", 0), ("run_131072", 4096), ("len_8", 1)])
def test_the_bytes_do_not_depend_on_how_the_text_is_cut_into_calls(name, block):
    """Three blocks with eof = 0, then the rest: the concatenation is the one call's file."""
    text = dict(CASES)[name]
    cut = 3 * (block or DC.MAX_BLOCK)
    assert len(text) > cut
    assert api.bgzf_deflate(text[:cut], block=block, eof=False) + api.bgzf_deflate(text[cut:], block=block) == api.bgzf_deflate(text, block=block)


def test_error_codes():
    L = _lib.lib()
    text = np.frombuffer(b"some text\n" * 10, dtype=np.uint8)
    buf = np.zeros(4096, dtype=np.uint8)
    n = C.c_uint64()
    args = lambda **kw: [kw.get("text", text.ctypes.data), len(text), kw.get("block", 0), 1, 1, kw.get("buf", buf.ctypes.data), len(buf), kw.get("n", C.byref(n))]
    assert L.vg_bgzf_deflate_host(*args()) == 0
    for name, kw in (("text", dict(text=None)), ("bgzf", dict(buf=None)), ("bgzf_len", dict(n=None)), ("block", dict(block=65281))):
        assert _lib.VG_ERRORS[L.vg_bgzf_deflate_host(*args(**kw))] == "VG_EINVAL", name
        dev = args(**kw)
        del dev[4]                                                    # (no `threads`)
        assert _lib.VG_ERRORS[L.vg_bgzf_deflate_device(0, *dev)] == "VG_EINVAL", name
    assert L.vg_bgzf_deflate_bound(100, 65281) == 0
    assert L.vg_bgzf_deflate_bound(0, 0) == 28 and L.vg_bgzf_deflate_bound(65281, 0) == 65281 + 2 * 31 + 28


def test_the_device_call_never_falls_back():
    """Without a device vg_bgzf_deflate_device is VG_ENODEV and says so; with one it writes the host's bytes."""
    L = _lib.lib()
    text = dict(CASES)["len_311"]
    if L.vg_device_count() > 0:
        assert api.bgzf_deflate(text, device=0) == api.bgzf_deflate(text)
        return
    with pytest.raises(_lib.VgError) as e:
        api.bgzf_deflate(text, device=0)
    assert _lib.VG_ERRORS[e.value.code] == "VG_ENODEV"
    assert L.vg_last_error() != b""


@pytest.mark.parametrize("name,block", [("ftiny.out.vcf.gz", None), ("ftiny.out.vcf.gz", 311), ("fdense.out.vcf.gz", 0), ("empty", None), ("run_131072", 65280)])
def test_bgzfzip_writes_the_librarys_bytes_and_bgzfcat_reads_them_back(name, block, tmp_path):
    text = dict(CASES)[name]
    src, dst = tmp_path / "in.vcf", tmp_path / "out.vcf.gz"
    src.write_bytes(text)
    env = {k: v for k, v in os.environ.items() if k != "VARGENO_VCF_BGZF"}
    p = subprocess.run([BIN, "bgzfzip", str(src), str(dst)] + ([] if block is None else [str(block)]), capture_output=True, env=env, timeout=120)
    assert p.returncode == 0, p.stderr
    assert dst.read_bytes() == api.bgzf_deflate(text, block=block or 0)
    p = subprocess.run([BIN, "bgzfcat", str(dst)], capture_output=True, env=env, timeout=120)
    assert p.returncode == 0, p.stderr
    assert p.stdout == text


def test_bgzfzip_cuts_its_spans_at_block_boundaries(tmp_path):
    """More text than one span of the sink (16 MiB) holds, and no multiple of it: the file is still the one call's."""
    text = dict(CASES)["fdense.out.vcf.gz"] * 9
    src, dst = tmp_path / "in.vcf", tmp_path / "out.vcf.gz"
    src.write_bytes(text)
    env = dict({k: v for k, v in os.environ.items() if k != "VARGENO_VCF_BGZF"}, VARGENO_VCF_BGZF="host", VARGENO_BGZF_THREADS="3")
    p = subprocess.run([BIN, "bgzfzip", str(src), str(dst)], capture_output=True, env=env, timeout=120)
    assert p.returncode == 0, p.stderr
    assert dst.read_bytes() == api.bgzf_deflate(text)


@pytest.mark.parametrize("cmd", ["geno", "cohort", "joint", "bgzfzip"])
def test_a_value_that_is_neither_device_nor_host_is_refused_in_one_line(cmd, tmp_path):
    """Before the index, the reads or a device are looked at: none of the files exists, and this machine may have no GPU."""
    n_args = {"geno": 4, "cohort": 3, "joint": 4, "bgzfzip": 2}[cmd]
    args = [str(tmp_path / ("no_such_file_%d" % i)) for i in range(n_args)]
    p = subprocess.run([BIN, cmd] + args, capture_output=True, text=True, env=dict(os.environ, VARGENO_VCF_BGZF="zip"), timeout=60)
    assert p.returncode != 0 and p.stdout == ""
    lines = [ln for ln in p.stderr.splitlines() if ln.strip()]
    assert len(lines) == 1 and "VARGENO_VCF_BGZF=zip" in lines[0] and "`device`" in lines[0] and "`host`" in lines[0], p.stderr
    assert not os.path.exists(args[-1])


def test_deflate_core_under_sanitizers(tmp_path):
    """tests/deflate_fuzz.cpp: the host build of the core alone, built with -fsanitize=address,undefined and run directly: seeded
    texts and the edge cases through exactly-sized heap buffers, read back by the host inflater, CRC32 recomputed bit by bit."""
    exe = tmp_path / "deflate_fuzz"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe),
                    os.path.join(ROOT, "tests", "deflate_fuzz.cpp")], check=True, timeout=300)
    p = subprocess.run([str(exe), "150", "12345"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().endswith("ok"), p.stdout

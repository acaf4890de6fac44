"""BGZF output with dynamic Huffman codes on the CPU: the host build of the compressor's second coding mode
(vargeno_amd/csrc/vg_deflate.h: vg_deflate_block_dyn, vg_def_code_lengths) behind vg_bgzf_deflate_host_coded and
vg_deflate_code_lengths_host, the command line's VARGENO_VCF_CODES, and the core alone under AddressSanitizer + UBSan
(tests/deflate_dyn_fuzz.cpp).  No device is touched.  What a file must inflate to is the text it was made from; the judges are
Python's zlib, the library's own host inflater, a header reader and a Huffman tree written in tests/deflate_dyn_cases.py -- never
the compressor.  The fixed mode is pinned to the bytes it wrote before this mode existed (tests/golden/deflate_fixed.sha256)."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import deflate_cases as DC
import deflate_dyn_cases as DD
from conftest import BIN, GOLDEN, ROOT
from vargeno_amd import _lib, api

CASES = DC.cases() + DD.new_cases()
NAMES = [c[0] for c in CASES]
TEXT = dict(CASES)


@pytest.mark.parametrize("block", DC.BLOCK_SIZES)
@pytest.mark.parametrize("case", range(len(CASES)), ids=NAMES)
def test_round_trip_and_never_larger_than_fixed(case, block):
    """Every text at every block length in dynamic mode: Python's zlib reads the file back block by block (deflate_cases.check_file)
    and so does vg_bgzf_inflate_host; block for block the file is no larger than the fixed mode's, and a block in the stored or the
    fixed form is the fixed mode's block.  At block lengths 1 and 7 nothing can shrink: the two files are identical."""
    text = CASES[case][1]
    out = api.bgzf_deflate(text, block=block, codes="dynamic")
    fixed = api.bgzf_deflate(text, block=block)
    assert len(out) <= _lib.lib().vg_bgzf_deflate_bound(len(text), block)
    DC.check_file(out, text, block)
    got, consumed, bad = api.bgzf_inflate(out, device=None, text_cap=len(text))
    assert bad is None and consumed == len(out)
    assert got == text
    if block in (1, 7):
        assert out == fixed
    elif DC.n_blocks(len(text), block) <= 20000:
        mine, theirs = DC.split_blocks(out), DC.split_blocks(fixed)
        assert len(mine) == len(theirs)
        for (_, a), (_, b) in zip(mine, theirs):
            assert len(a) <= len(b)
            assert DD.block_form(a[18:]) == 2 or a == b
    else:
        assert len(out) <= len(fixed)


def test_the_edge_cases_are_what_they_are_meant_to_be():
    """The header reader of deflate_dyn_cases on the new cases' blocks: what each was built to hold is there."""
    def header(name):
        (payload, isize), _ = DD.block_payloads(api.bgzf_deflate(TEXT[name], codes="dynamic"))
        assert isize == len(TEXT[name]) and DD.block_form(payload) == 2, name
        return DD.dynamic_header(payload)
    ll, dl, _, _ = header("every_symbol")
    assert all(ll[:257]) and ll[257] == 0 and all(ll[258:286]) and len(ll) == 286       # (the finder takes no match of three bytes)
    assert all(dl) and len(dl) == 30
    ll, dl, _, _ = header("one_byte_300")
    assert [s for s, l in enumerate(ll) if l] == [ord("Q"), 256, 284] and [l for l in dl if l] == [1, 1]      # one literal, one distance and its padding
    ll, dl, _, _ = header("wide_token")
    assert ll[284] + 5 + dl[29] + 13 > 32                              # the match of 240 bytes some 30 000 back: a token that straddles three words
    assert max(ll) <= 15 and max(dl) <= 15
    (payload, _), _ = DD.block_payloads(api.bgzf_deflate(TEXT["no_match_256"], codes="dynamic"))
    assert DD.block_form(payload) == 0                                 # 256 distinct bytes: nothing to gain, stored
    for name in ("block_of_64", "block_of_65"):
        assert len(header(name)[0]) >= 257


GOLDEN_VCFS = [n for n in NAMES if n.endswith(".vcf.gz")]


def test_golden_vcfs_come_out_smaller_than_fixed_and_together_smaller_than_zlib_level_1():
    assert len(GOLDEN_VCFS) == 12
    total = {"text": 0, "fixed": 0, "dynamic": 0, "zlib1": 0}
    for name in GOLDEN_VCFS:
        text = TEXT[name]
        fixed, dyn = len(api.bgzf_deflate(text)), len(api.bgzf_deflate(text, codes="dynamic"))
        z = DD.zlib_level1_size(text) + len(DC.EOF_MARKER)
        print("%s: %d bytes of text, fixed %d, dynamic %d, zlib level 1 %d" % (name, len(text), fixed, dyn, z))
        assert dyn < fixed, name
        for k, v in (("text", len(text)), ("fixed", fixed), ("dynamic", dyn), ("zlib1", z)):
            total[k] += v
    print("all twelve: fixed %.4f, dynamic %.4f, zlib level 1 %.4f of the text" % tuple(total[k] / total["text"] for k in ("fixed", "dynamic", "zlib1")))
    assert total["dynamic"] < total["zlib1"]


@pytest.mark.parametrize("name,block", [("ftiny_reads", 311), ("fsmall.out.vcf.gz", 0), ("run_131072", 4096), ("every_symbol", 4096)])
def test_the_bytes_do_not_depend_on_the_number_of_threads(name, block):
    assert api.bgzf_deflate(TEXT[name], block=block, threads=1, codes="dynamic") == api.bgzf_deflate(TEXT[name], block=block, threads=5, codes="dynamic")


@pytest.mark.parametrize("name,block", [("ftiny_reads", 311), ("ftiny_reads", 4096), ("fdense.out.vcf.gz", 0), ("run_131072", 4096), ("len_8", 1)])
def test_the_bytes_do_not_depend_on_how_the_text_is_cut_into_calls(name, block):
    """Three blocks with eof = 0, then the rest: the concatenation is the one call's file."""
    text = TEXT[name]
    cut = 3 * (block or DC.MAX_BLOCK)
    assert len(text) > cut
    z = lambda t, **kw: api.bgzf_deflate(t, block=block, codes="dynamic", **kw)
    assert z(text[:cut], eof=False) + z(text[cut:]) == z(text)


def _raw_host_coded(text, block, eof, threads, codes, cap, canary=0xA5, tail=4096):
    a = np.frombuffer(text, dtype=np.uint8) if text else np.zeros(1, dtype=np.uint8)
    buf = np.full(cap + tail, canary, dtype=np.uint8)
    n = C.c_uint64(12345)
    rc = _lib.lib().vg_bgzf_deflate_host_coded(a.ctypes.data, len(text), block, eof, threads, codes, buf.ctypes.data, cap, C.byref(n))
    return rc, int(n.value), buf


@pytest.mark.parametrize("name,block", [("ftiny.out.vcf.gz", 0), ("ftiny_reads", 311), ("len_65281", 0), ("one_byte", 1)])
def test_capacity_one_byte_short_is_refused_and_nothing_is_written(name, block):
    text = TEXT[name]
    want = api.bgzf_deflate(text, block=block, codes="dynamic")
    rc, n, buf = _raw_host_coded(text, block, 1, 2, 1, len(want))
    assert rc == 0 and n == len(want) and buf[:n].tobytes() == want and (buf[n:] == 0xA5).all()
    rc, n, buf = _raw_host_coded(text, block, 1, 2, 1, len(want) - 1)
    assert _lib.VG_ERRORS[rc] == "VG_ETOOBIG"
    assert (buf == 0xA5).all()


def test_a_codes_value_that_is_neither_mode_is_refused():
    text = TEXT["len_311"]
    for codes in (2, -1, 7):
        rc, _, buf = _raw_host_coded(text, 0, 1, 1, codes, 4096)
        assert _lib.VG_ERRORS[rc] == "VG_EINVAL" and (buf == 0xA5).all()
        a, n = np.frombuffer(text, dtype=np.uint8), C.c_uint64()
        assert _lib.VG_ERRORS[_lib.lib().vg_bgzf_deflate_device_coded(0, a.ctypes.data, len(text), 0, 1, codes, buf.ctypes.data, 4096, C.byref(n))] == "VG_EINVAL"
    for codes in ("Dynamic", "", None, 1, b"fixed"):
        with pytest.raises(ValueError):
            api.bgzf_deflate(text, codes=codes)


@pytest.mark.parametrize("block", [0, 311])
def test_fixed_mode_is_what_it_was(block):
    """The default, codes="fixed", the coded call with VG_DEFLATE_FIXED and vg_bgzf_deflate_host write the same file."""
    for name, text in DC.cases():
        if DC.n_blocks(len(text), block) > 20000:
            continue
        want = api.bgzf_deflate(text, block=block)
        assert api.bgzf_deflate(text, block=block, codes="fixed") == want, name
        cap = int(_lib.lib().vg_bgzf_deflate_bound(len(text), block))
        a = np.frombuffer(text, dtype=np.uint8) if text else np.zeros(1, dtype=np.uint8)
        buf, n = np.zeros(max(1, cap), dtype=np.uint8), C.c_uint64()
        assert _lib.lib().vg_bgzf_deflate_host(a.ctypes.data, len(text), block, 1, 3, buf.ctypes.data, cap, C.byref(n)) == 0
        assert buf[:n.value].tobytes() == want, name


def test_fixed_mode_writes_the_bytes_it_wrote_before_the_dynamic_mode_existed():
    """tests/golden/deflate_fixed.sha256: one sha256 per (case, block length) of the files the commit before this mode wrote, made
    from that commit's build.  The default path still writes them."""
    want = {}
    with open(os.path.join(GOLDEN, "deflate_fixed.sha256")) as f:
        for ln in f:
            digest, name, block = ln.split()
            want[(name, int(block))] = digest
    cases = DC.cases()
    assert len(want) == len(cases) * len(DC.BLOCK_SIZES)
    for name, text in cases:
        for block in DC.BLOCK_SIZES:
            assert hashlib.sha256(api.bgzf_deflate(text, block=block)).hexdigest() == want[(name, block)], (name, block)


HISTOGRAMS = DD.histograms()


@pytest.mark.parametrize("limit", [7, 15])
def test_code_lengths_on_the_host(limit):
    """Kraft sum exactly 1, nothing above the limit, length 0 exactly where the count is 0 (but for the two-symbol padding), cost no
    less than an unlimited Huffman tree's and equal to it where that tree is within the limit; Fibonacci counts need the limit."""
    n_checked = 0
    for name, freq in HISTOGRAMS:
        if len(freq) > 1 << limit:
            continue
        lens = api.deflate_code_lengths(np.array(freq, dtype=np.uint32), limit=limit)
        DD.check_lengths(freq, lens, limit)
        if name.startswith("fibonacci") or name == "powers_of_two":
            assert DD.huffman(freq)[1] > limit and int(lens.max()) == limit, name
        n_checked += 1
    assert n_checked > 100
    # many histograms in one call are the single calls' rows
    rows = [f for _, f in HISTOGRAMS if len(f) == 30]
    many = api.deflate_code_lengths(np.array(rows, dtype=np.uint32), limit=limit)
    assert many.shape == (len(rows), 30)
    for row, lens in zip(rows, many):
        assert (lens == api.deflate_code_lengths(np.array(row, dtype=np.uint32), limit=limit)).all()


def test_code_lengths_arguments():
    L = _lib.lib()
    f, out = np.ones(20, dtype=np.uint32), np.zeros(300, dtype=np.uint8)
    call = lambda fn, *a: _lib.VG_ERRORS.get(fn(*a), 0)
    for fn, dev in ((L.vg_deflate_code_lengths_host, ()), (L.vg_deflate_code_lengths_device, (0,))):
        assert call(fn, *dev, None, 1, 20, 15, out.ctypes.data) == "VG_EINVAL"
        assert call(fn, *dev, f.ctypes.data, 1, 20, 15, None) == "VG_EINVAL"
        assert call(fn, *dev, f.ctypes.data, 1, 20, 16, out.ctypes.data) == "VG_EINVAL"
        assert call(fn, *dev, f.ctypes.data, 1, 20, 4, out.ctypes.data) == "VG_EINVAL"          # 20 symbols have no code of 4 bits
        assert call(fn, *dev, f.ctypes.data, 1, 1, 15, out.ctypes.data) == "VG_EINVAL"
        big = np.full(289, 1, dtype=np.uint32)
        assert call(fn, *dev, big.ctypes.data, 1, 289, 15, out.ctypes.data) == "VG_EINVAL"
        huge = np.full(2, 1 << 31, dtype=np.uint32)
        assert call(fn, *dev, huge.ctypes.data, 1, 2, 15, out.ctypes.data) == "VG_EINVAL"       # the counts' sum must fit 32 bits
    assert call(L.vg_deflate_code_lengths_host, f.ctypes.data, 1, 20, 15, out.ctypes.data) == 0
    if L.vg_device_count() <= 0:
        assert call(L.vg_deflate_code_lengths_device, 0, f.ctypes.data, 1, 20, 15, out.ctypes.data) == "VG_ENODEV"


def _env(**kw):
    return dict({k: v for k, v in os.environ.items() if k not in ("VARGENO_VCF_BGZF", "VARGENO_VCF_CODES")}, **kw)


@pytest.mark.parametrize("name,block", [("ftiny.out.vcf.gz", None), ("ftiny.out.vcf.gz", 311), ("fdense.out.vcf.gz", 0), ("empty", None), ("every_symbol", 4096)])
def test_bgzfzip_in_dynamic_mode_writes_the_librarys_bytes_and_bgzfcat_reads_them_back(name, block, tmp_path):
    text = TEXT[name]
    src, dst = tmp_path / "in.vcf", tmp_path / "out.vcf.gz"
    src.write_bytes(text)
    p = subprocess.run([BIN, "bgzfzip", str(src), str(dst)] + ([] if block is None else [str(block)]), capture_output=True, timeout=120,
                       env=_env(VARGENO_VCF_BGZF="host", VARGENO_VCF_CODES="dynamic", VARGENO_VERBOSE="1", VARGENO_BGZF_THREADS="3"))
    assert p.returncode == 0, p.stderr
    assert b"dynamic codes" in p.stderr
    assert dst.read_bytes() == api.bgzf_deflate(text, block=block or 0, codes="dynamic")
    p = subprocess.run([BIN, "bgzfcat", str(dst)], capture_output=True, env=_env(), timeout=120)
    assert p.returncode == 0, p.stderr
    assert p.stdout == text


def test_bgzfzip_with_the_variable_unset_empty_or_fixed_writes_the_fixed_file(tmp_path):
    text = TEXT["ftiny.out.vcf.gz"]
    src = tmp_path / "in.vcf"
    src.write_bytes(text)
    for i, env in enumerate((_env(), _env(VARGENO_VCF_CODES=""), _env(VARGENO_VCF_CODES="fixed"))):
        dst = tmp_path / ("out%d.vcf.gz" % i)
        p = subprocess.run([BIN, "bgzfzip", str(src), str(dst)], capture_output=True, env=env, timeout=120)
        assert p.returncode == 0, p.stderr
        assert dst.read_bytes() == api.bgzf_deflate(text)


@pytest.mark.parametrize("cmd", ["geno", "cohort", "joint", "bgzfzip"])
def test_a_value_that_is_neither_fixed_nor_dynamic_is_refused_in_one_line(cmd, tmp_path):
    """Before the index, the reads or a device are looked at: none of the files exists, and the host may have no GPU."""
    n_args = {"geno": 4, "cohort": 3, "joint": 4, "bgzfzip": 2}[cmd]
    args = [str(tmp_path / ("no_such_file_%d" % i)) for i in range(n_args)]
    for route in ({}, {"VARGENO_VCF_BGZF": "host"}):
        p = subprocess.run([BIN, cmd] + args, capture_output=True, text=True, env=_env(VARGENO_VCF_CODES="huffman", **route), timeout=60)
        assert p.returncode != 0 and p.stdout == ""
        lines = [ln for ln in p.stderr.splitlines() if ln.strip()]
        assert len(lines) == 1 and "VARGENO_VCF_CODES=huffman" in lines[0] and "`fixed`" in lines[0] and "`dynamic`" in lines[0], p.stderr
        assert not os.path.exists(args[-1])


def test_dynamic_core_under_sanitizers(tmp_path):
    """tests/deflate_dyn_fuzz.cpp: the host build of the dynamic path alone, built with -fsanitize=address,undefined and run
    directly: seeded texts and the edge cases through exactly-sized heap buffers and poisoned shared state, read back by the host
    inflater and by the program's own token reader, which must meet a token of more than 32 bits; the builder on Fibonacci counts."""
    exe = tmp_path / "deflate_dyn_fuzz"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe),
                    os.path.join(ROOT, "tests", "deflate_dyn_fuzz.cpp")], check=True, timeout=300)
    p = subprocess.run([str(exe), "120", "12345"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().endswith("ok"), p.stdout

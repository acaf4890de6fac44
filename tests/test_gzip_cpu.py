"""Plain gzip on the host: the sequential reference decoder (vg_gunzip_host), the chunked stages -- find, decode, confirm, repair,
resolve: what the device kernels run -- through the host policy (vg_gunzip_chunked_host), the command line's `gzcat`, and the core
alone under AddressSanitizer + UBSan (tests/gzip_fuzz.cpp).  No device is touched.  Expected text is always what Python's zlib
makes of the same bytes (tests/gzip_cases.py), never the code under test."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import gzip_cases as GC
from conftest import BIN, ROOT
from vargeno_amd import api, synth

VALID = GC.valid_cases()
DAMAGED = GC.damaged_cases()
IDS = [c[0] for c in VALID]


def _ratio(name):
    return 300 if name == "ratio_254" else None                  # (the staging must hold 254 symbols per compressed byte there)


def test_the_cases_are_what_they_claim():
    """The generator against Python's gzip module: every kind of damage has survivors that Python rejects, the decoy is a block
    start at the first bit of a chunk's range at every chunk size, and the hand-made references are as far and as long as said."""
    kinds = {n.split("_")[0] + "_" + n.split("_")[1] for n, _ in DAMAGED}
    assert {"flip_magic", "flip_method", "flip_block", "flip_code", "flip_symbols", "flip_crc", "flip_isize", "truncated_in", "truncated_mid", "junk_after"} <= kinds, kinds
    data, text, at = GC.decoy()
    assert all((at - GC.HEADER) % c == 0 for c in GC.CHUNKS) and data[at] & 7 == 4
    assert zlib.decompressobj(-15).decompress(data[at:at + 2000])[:100] == GC.ftiny_text()[500_000:500_100]
    far, far_text = GC.far_references()
    assert far_text[40_000 + 3_000:][:258] == far_text[40_000 + 3_000 - 32768:][:258] and b"Q" * 259 in far_text
    sizes = {name: (len(d), len(t)) for name, d, t in VALID}
    assert 200 < sizes["ratio_254"][1] / sizes["ratio_254"][0] < 260 and sizes["short_file"][0] < 1024


@pytest.mark.parametrize("case", range(len(VALID)), ids=IDS)
def test_sequential_decoder_equals_zlib(case):
    _, data, text = VALID[case]
    buf_cap = len(text)                                           # exactly the text: not a byte more is needed
    r = api.gunzip(data, device=None, text_cap=buf_cap)
    assert r.error is None and r.bad_offset is None and r.consumed == len(data)
    assert r.text == text


@pytest.mark.parametrize("case", range(len(VALID)), ids=IDS)
def test_gzcat_writes_the_text(case, tmp_path):
    _, data, text = VALID[case]
    f = tmp_path / "in.fq.gz"
    f.write_bytes(data)
    p = subprocess.run([BIN, "gzcat", str(f)], capture_output=True, timeout=60)
    assert p.returncode == 0, p.stderr
    assert p.stdout == text


@pytest.mark.parametrize("case", range(len(VALID)), ids=IDS)
def test_chunked_stages_equal_zlib_at_every_setting(case):
    """Chunks of 1 024, 8 192, 32 768 bytes and one chunk for the whole file; slot sizes that cut the file into 1, 4 and 40 slots."""
    name, data, text = VALID[case]
    n = len(data)
    settings = [dict(chunk=c) for c in GC.CHUNKS] + [dict(chunk=n + 1)] + [dict(chunk=1024, slot=-(-n // k) + 16) for k in (1, 4, 40)] + [dict(chunk=8192, slot=-(-n // 4) + 16)]
    for kw in settings:
        r = api.gunzip(data, device=None, chunked=True, ratio=_ratio(name), text_cap=len(text), **kw)
        assert r.error is None and r.stats["slots_refused"] == 0, (kw, r.error, r.stats)
        assert r.consumed == n and r.text == text, kw
        assert r.stats["members"] == (3 if name == "three_members" else 2 if name == "ends_on_chunk_boundary" else 1)
        if name in GC.ORDINARY:                                    # no false guess on these files
            assert r.stats["repaired"] == 0 and r.stats["confirmed"] < r.stats["guessed"], (kw, r.stats)
            if "slot" not in kw:                                   # one member in one slot: every guess but the slot's own entry was confirmed
                assert r.stats["confirmed"] == r.stats["guessed"] - 1, (kw, r.stats)
        if name == "decoy" and "slot" not in kw and kw["chunk"] <= 32768:
            assert r.stats["repaired"] >= 1, (kw, r.stats)


PUSHES = [dict(push=1, chunk=1024, slots=4), dict(push=4099, chunk=8192, slots=40), dict(push=4099, chunk=32768, slots=1), dict(push=1 << 20, chunk=1024, slots=4)]


@pytest.mark.parametrize("case", range(len(VALID)), ids=IDS)
def test_pushes_cut_anywhere_equal_zlib_and_the_whole_file_route(case):
    """The push driver of a gzip stream over the host stages: pushes of 1 byte and of 4 099 bytes (and one push for the whole file),
    the incomplete tail block, a header and a trailer cut short carried from push to push.  The text is zlib's; the slots, and
    with them the statistics, are those of the route that sees the whole file at once."""
    name, data, text = VALID[case]
    n = len(data)
    for st in PUSHES:
        kw = dict(chunk=st["chunk"], slot=-(-n // st["slots"]) + 16, ratio=_ratio(name), text_cap=len(text))
        r = api.gunzip(data, device=None, push=st["push"], **kw)
        assert r.error is None and r.stats["slots_refused"] == 0, (st, r.error, r.stats)
        assert r.consumed == n and r.text == text, st
        assert r.stats == api.gunzip(data, device=None, chunked=True, **kw).stats, st


@pytest.mark.parametrize("push", [1, 4099])
def test_pushes_of_damaged_files_end_as_the_whole_file_route_does(push):
    for name, data in DAMAGED:
        kw = dict(chunk=1024, slot=20_000, text_cap=200_000)
        r = api.gunzip(data, device=None, push=push, **kw)
        h = api.gunzip(data, device=None, chunked=True, **kw)
        assert r.error is not None and (r.error, r.bad_offset, r.consumed, r.text) == (h.error, h.bad_offset, h.consumed, h.text), name
    # and a refused slot: the same boundary
    _, data, text = [c for c in VALID if c[0] == "ratio_254"][0]
    r = api.gunzip(data, device=None, push=push, chunk=8192, ratio=8, text_cap=len(text))
    assert r.error is None and r.stats["slots_refused"] == 1 and r.text == b"" and r.consumed == GC.HEADER and r.stats["resume_bit"] == 8 * GC.HEADER


def test_level6_chunks_have_the_block_starts_the_issue_counted():
    """At level 6 zlib's blocks of this file are 16.5-17.1 KB compressed: chunks of 8 192 bytes leave about every second one
    without a block start, chunks of 32 768 have one each (but the last)."""
    data = dict((n, d) for n, d, _ in VALID)["level6"]
    s8 = api.gunzip(data, device=None, chunked=True, chunk=8192).stats
    s32 = api.gunzip(data, device=None, chunked=True, chunk=32768).stats
    assert s8["guessed"] == 33 + 1 - 1 and 0.4 < s8["guessed"] / s8["chunks"] < 0.6, s8         # 33 non-final block starts, one in chunk 0's range
    assert s32["guessed"] >= s32["chunks"] - 1, s32


def test_a_slot_beyond_the_ratio_bound_is_refused_not_overrun():
    name, data, text = [c for c in VALID if c[0] == "ratio_254"][0]
    buf_cap = len(text)
    r = api.gunzip(data, device=None, chunked=True, chunk=8192, ratio=8, text_cap=buf_cap)
    assert r.error is None and r.stats["slots_refused"] == 1 and r.stats["members"] == 0
    assert r.text == b"" and r.consumed == GC.HEADER and r.stats["resume_bit"] == 8 * GC.HEADER
    # raw deflate from the boundary it names is the member's text
    assert zlib.decompressobj(-15).decompress(data[r.stats["resume_bit"] // 8:]) == text


@pytest.mark.parametrize("case", range(len(DAMAGED)), ids=[c[0] for c in DAMAGED])
def test_damaged_files_end_in_an_error_that_names_an_offset(case):
    """Both decoders: an error with the compressed offset in it (or the CRC / ISIZE error, at the trailer), and only the text of
    the members before the damaged one -- never wrong text with OK.  Nothing is written behind text_cap."""
    name, data = DAMAGED[case]
    good_first = GC.ftiny_text()[:150_000]
    for kw in (dict(), dict(chunked=True, chunk=1024), dict(chunked=True, chunk=8192, slot=20_000)):
        r = api.gunzip(data, device=None, text_cap=200_000, **kw)
        assert r.error is not None and r.bad_offset is not None and r.bad_offset <= len(data), (name, kw)
        assert "offset %d" % r.bad_offset in r.error
        assert r.text in (b"", good_first), (name, kw, len(r.text))
        if "crc" in name:
            assert "CRC" in r.error
        if "isize" in name:
            assert "ISIZE" in r.error
        if name.startswith("truncated"):
            assert "input exhausted" in r.error and r.bad_offset == len(data)
        if name.startswith("junk"):
            assert "not a gzip member header" in r.error and r.text == good_first


def test_gzcat_names_the_offset_of_bad_data(tmp_path):
    for name, data in DAMAGED[::7]:
        f = tmp_path / "bad.fq.gz"
        f.write_bytes(data)
        p = subprocess.run([BIN, "gzcat", str(f)], capture_output=True, text=True, timeout=60)
        want = api.gunzip(data, device=None, text_cap=200_000)
        assert p.returncode != 0, (name, p.stderr)
        # the offset and the reason are the library's (the tool decodes the file piece by piece: the same place all the same)
        assert want.error[want.error.index("gzip stream at compressed offset"):] in p.stderr, (name, want.error, p.stderr)


def test_a_block_larger_than_a_slot_is_said_by_name():
    """A slot that holds no whole block is tried again twice as long (the 40-slot setting above needs that at level 1); where
    VG_GZ_SLOT_MAX ends that, the call fails with the slot's offset -- on the first slot here: the member's first block."""
    _, data, text = VALID[0]
    r = api.gunzip(data, device=None, chunked=True, chunk=1024, slot=4096, slot_max=8192, text_cap=len(text))
    assert r.error is not None and "larger than a slot" in r.error and "offset %d" % GC.HEADER in r.error and r.text == b""
    r = api.gunzip(data, device=None, chunked=True, chunk=1024, slot=4096, text_cap=len(text))
    assert r.error is None and r.text == text


def test_text_that_does_not_fit_is_refused():
    from vargeno_amd._lib import VgError

    _, data, text = VALID[1]
    for kw in (dict(), dict(chunked=True)):
        with pytest.raises(VgError) as e:
            api.gunzip(data, device=None, text_cap=len(text) - 1, **kw)
        assert e.value.code == -5


def test_the_refusal_names_the_switch_and_host_is_the_way_in(tmp_path):
    """Unset (or set to anything else), a plain gzip file is refused with one line, which now names VARGENO_GZIP=device|host; with
    either value the file is no longer refused -- `geno` gets as far as asking for the index."""
    f = tmp_path / "plain.fq.gz"
    f.write_bytes(VALID[1][1][:5000])
    cmd = [BIN, "geno", str(tmp_path / "no_such_index"), str(f), str(tmp_path / "snps.vcf"), str(tmp_path / "out.vcf")]
    env = {k: v for k, v in os.environ.items() if k != "VARGENO_GZIP"}
    for value in (None, "", "zstd"):
        e = dict(env) if value is None else dict(env, VARGENO_GZIP=value)
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=60, env=e)
        lines = [ln for ln in p.stderr.splitlines() if ln.strip()]
        assert p.returncode != 0 and len(lines) == 1 and "VARGENO_GZIP=device|host" in lines[0] and "<(zcat %s)" % f in lines[0] and "only BGZF" in lines[0], p.stderr
    for value in ("host", "device"):
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=60, env=dict(env, VARGENO_GZIP=value))
        assert p.returncode != 0 and "BGZF" not in p.stderr and "no_such_index" in p.stderr, (value, p.stderr)


def test_gunzip_core_under_sanitizers(tmp_path):
    """tests/gzip_fuzz.cpp: the host build of the core alone, built with -fsanitize=address,undefined and run directly, on 20 000
    seeded mutations of a file with dynamic, fixed and stored members, through the sequential decoder and the chunked stages."""
    exe = tmp_path / "gzip_fuzz"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe),
                    os.path.join(ROOT, "tests", "gzip_fuzz.cpp")], check=True, timeout=300)
    t = GC.ftiny_text()
    data = (synth.gzip_bytes(t[:24_000], flush=zlib.Z_FULL_FLUSH, flush_every=4000) + synth.gzip_bytes(t[24_000:27_000], strategy=zlib.Z_FIXED)
            + synth.gzip_bytes(t[27_000:29_000], level=0) + synth.gzip_bytes(t[29_000:45_000], level=9, name=b"x", hcrc=True))
    f = tmp_path / "members.gz"
    f.write_bytes(data)
    p = subprocess.run([str(exe), str(f), "20000", "12345"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().endswith("ok"), p.stdout

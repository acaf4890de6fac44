"""Plain gzip inflated on the device (vg_gz_find / decode / confirm / repair / windows / resolve / crc through vg_gunzip_device):
every inflated byte against Python's zlib at three chunk sizes, the statistics the inputs' structure forces, and the error path;
and the stream (vg_fastq_stream_begin_gzip): gzip bytes pushed in uneven pieces, inflated and framed on the device, against the
oracle's counters.  The inputs are those of tests/test_gzip_cpu.py (tests/gzip_cases.py)."""
import os
import zlib

import numpy as np
import pytest

import gzip_cases as GC
from oracle import oracle as O
from vargeno_amd import api, synth
from vargeno_amd._lib import VgError
from vargeno_amd.api import GenoIndex

pytestmark = pytest.mark.gpu

VALID = GC.valid_cases()
DAMAGED = GC.damaged_cases()
BY_NAME = {name: (data, text) for name, data, text in VALID}


def _ratio(name):
    return 300 if name == "ratio_254" else None                  # (the staging must hold 254 symbols per compressed byte there)


@pytest.mark.parametrize("chunk", GC.CHUNKS)
@pytest.mark.parametrize("case", range(len(VALID)), ids=[c[0] for c in VALID])
def test_device_gunzip_is_byte_exact(case, chunk):
    name, data, text = VALID[case]
    r = api.gunzip(data, device=0, chunk=chunk, ratio=_ratio(name), text_cap=len(text) + 1)
    print(name, chunk, r.stats)
    assert r.error is None and r.bad_offset is None and r.stats["slots_refused"] == 0
    assert r.consumed == len(data)
    assert r.text == text
    # the kernels and the host build of the same stages decide alike
    h = api.gunzip(data, device=None, chunked=True, chunk=chunk, ratio=_ratio(name), text_cap=len(text) + 1)
    assert r.stats == h.stats
    if name in GC.ORDINARY:
        assert r.stats["repaired"] == 0 and r.stats["confirmed"] == r.stats["guessed"] - 1
    if name == "decoy":
        assert r.stats["repaired"] >= 1
    if name == "fixed":                                          # no dynamic block anywhere: chunk 0 walks the whole slot, nothing to repair
        assert (r.stats["guessed"], r.stats["repaired"]) == (1, 0)


@pytest.mark.parametrize("slot", [70_000, 200_000])
def test_slots_carry_the_boundary_and_the_window(slot):
    """Several slots per member: each starts at the bit where the one before stopped, with its last 32 KiB as the window."""
    for name in ("level6", "far_references", "three_members", "sync_flush"):
        data, text = BY_NAME[name]
        r = api.gunzip(data, device=0, chunk=8192, slot=slot, text_cap=len(text) + 1)
        assert r.error is None and r.text == text and r.consumed == len(data), name
        assert r.stats == api.gunzip(data, device=None, chunked=True, chunk=8192, slot=slot, text_cap=len(text) + 1).stats, name


def test_a_slot_grows_to_hold_one_block_and_says_when_it_may_not():
    """Slots of 4 KiB under blocks of 20 KB: each is tried again twice as long until a block fits (the staging grows with it);
    with VG_GZ_SLOT_MAX in the way the call names the slot, as the host build does."""
    data, text = BY_NAME["level1"]
    r = api.gunzip(data, device=0, chunk=1024, slot=4096, text_cap=len(text))
    assert r.error is None and r.text == text and r.consumed == len(data)
    r = api.gunzip(data, device=0, chunk=1024, slot=4096, slot_max=8192, text_cap=len(text))
    assert r.error is not None and "larger than a slot" in r.error and "offset %d" % GC.HEADER in r.error and r.text == b""


def test_a_slot_beyond_the_ratio_bound_is_refused_not_overrun():
    """254 : 1 under a bound of 8: the slot is refused, nothing of it counts, and the call names the block boundary it stands at."""
    data, text = BY_NAME["ratio_254"]
    r = api.gunzip(data, device=0, chunk=8192, ratio=8, text_cap=len(text) + 1)
    assert r.error is None and r.stats["slots_refused"] == 1 and r.stats["members"] == 0
    assert r.text == b"" and r.consumed == GC.HEADER and r.stats["resume_bit"] == 8 * GC.HEADER
    # a second member behind a good one: the text and the boundary of the first stand
    first, first_text = BY_NAME["short_file"]
    r = api.gunzip(first + data, device=0, chunk=8192, ratio=8, text_cap=len(text) + 1000)
    assert r.error is None and r.stats["slots_refused"] == 1 and r.stats["members"] == 1
    assert r.text == first_text and r.consumed == len(first) + GC.HEADER


def test_damaged_files_end_in_an_error_as_on_the_host():
    """Every damaged case: an error that names a compressed offset (or the CRC / ISIZE error at the trailer), the same as the host
    build of the chunked stages gives, never text with OK; nothing is written behind text_cap; a valid call afterwards is exact."""
    cap = 200_000
    for name, data in DAMAGED:
        r = api.gunzip(data, device=0, chunk=8192, text_cap=cap)
        h = api.gunzip(data, device=None, chunked=True, chunk=8192, text_cap=cap)
        assert r.error is not None and r.bad_offset is not None and "offset %d" % r.bad_offset in r.error, name
        assert (r.error, r.bad_offset, r.consumed, r.text) == (h.error, h.bad_offset, h.consumed, h.text), name
        # ... and what the kind of damage says by itself
        assert r.text in (b"", GC.ftiny_text()[:150_000]), name
        if "crc" in name:
            assert "CRC" in r.error, name
        if "isize" in name:
            assert "ISIZE" in r.error, name
        if name.startswith("truncated"):
            assert "input exhausted" in r.error and r.bad_offset == len(data), name
        if name.startswith("junk"):
            assert "not a gzip member header" in r.error and r.text == GC.ftiny_text()[:150_000] and r.bad_offset == r.consumed, name
    data, text = BY_NAME["level6"]
    r = api.gunzip(data, device=0, text_cap=len(text))
    assert r.error is None and r.text == text


# ---- the stream ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_counts(ftiny_dir, ftiny_reads):
    """The oracle's counters for the 4 000 reads, computed once."""
    ox = O.OracleIndex.load(os.path.join(ftiny_dir, "idx"))
    ox.process(ftiny_reads.bases, ftiny_reads.quals, ftiny_reads.offsets)
    so = ox.sites()
    return so["ref_cnt"], so["alt_cnt"]


def _pieces(data, seed, steps=(1, 2, 7, 311, 4099, 65_537)):
    rng, at, out = np.random.default_rng(seed), 0, []
    while at < len(data):
        n = int(rng.choice(steps)) if len(out) < 300 else len(data)       # (the tiny steps at the head of the file)
        out.append(data[at:at + n])
        at += n
    return out


def _inflate_from(data, bit, window):
    """zlib on the raw DEFLATE stream from a bit offset on, the window as its dictionary: the bytes are shifted to a byte boundary."""
    tail = int.from_bytes(data[bit // 8:], "little") >> (bit % 8)
    d = zlib.decompressobj(-15, zdict=window) if window else zlib.decompressobj(-15)
    return d.decompress(tail.to_bytes(len(data) - bit // 8, "little"))


STREAMS = {"one_slot": {}, "slots_of_70000": dict(VG_GZ_SLOT="70000", VG_GZ_CHUNK="8192"), "slots_of_20000": dict(VG_GZ_SLOT="20000", VG_GZ_CHUNK="1024")}


@pytest.mark.parametrize("members", [1, 3])
@pytest.mark.parametrize("setting", list(STREAMS))
def test_gzip_stream_in_uneven_pieces_gives_the_oracles_counters(ftiny_dir, oracle_counts, setting, members, monkeypatch):
    """Pushes cut anywhere (one byte at a time at the head of the file), slots smaller than the file and smaller than a block (the
    slot grows), one member and three (the middle one empty): 4 000 reads, the whole text consumed, the oracle's counters; and every
    checkpoint is a place zlib can inflate on from, with the window it gives."""
    text = GC.ftiny_text()
    data = BY_NAME["level6"][0] if members == 1 else synth.gzip_bytes(text[:400_000]) + synth.gzip_bytes(b"") + synth.gzip_bytes(text[400_000:], level=1)
    for k, v in STREAMS[setting].items():
        monkeypatch.setenv(k, v)
    with GenoIndex.open(os.path.join(ftiny_dir, "idx")) as gx:
        n, used, last, refused = gx.fastq_stream(_pieces(data, 5 + members), gzip=True)
        assert (n, used, refused) == (4000, len(text), False)
        assert text[last:last + 1] == b"@" and text[last:].count(b"\n") == 4
        rc, ac = gx.counts()
        st = gx.gzip_stats()
        marks = [gx.gzip_checkpoint(at) for at in (0, 399_999, 400_000, last, len(text))]
    assert np.array_equal(rc, oracle_counts[0]) and np.array_equal(ac, oracle_counts[1])
    assert st["members"] == members and st["repaired"] == 0 and st["slots_refused"] == 0, st
    if setting != "one_slot":
        assert st["guessed"] - st["confirmed"] > members, st           # more slots than members
    for want, (bit, at, window) in zip((0, 399_999, 400_000, last, len(text)), marks):
        assert at <= want and len(window) == min(32768, at if members == 1 else at - (400_000 if at >= 400_000 else 0)), (want, at, len(window))
        end = len(text) if members == 1 or at >= 400_000 else 400_000   # zlib stops at the member's end
        assert _inflate_from(data, bit, window) == text[at:end], (want, bit, at)
    assert marks[0][1] == 0 and marks[0][2] == b""


def test_a_refused_slot_poisons_the_gzip_stream_and_names_where_to_go_on(ftiny_dir, monkeypatch):
    """254 : 1 under a ratio bound of 8 behind a good member: the good member's reads count, nothing of the refused slot is framed,
    refused is set, and the checkpoint is the refused slot's entry."""
    text = b"\n".join(GC.ftiny_text().split(b"\n", 160)[:160]) + b"\n"             # 40 records
    first = synth.gzip_bytes(text)
    data, big = BY_NAME["ratio_254"]
    monkeypatch.setenv("VG_GZ_MAX_RATIO", "8")
    monkeypatch.setenv("VG_GZ_CHUNK", "8192")
    with GenoIndex.open(os.path.join(ftiny_dir, "idx")) as gx:
        n, used, last, refused = gx.fastq_stream([first[:11], first[11:] + data[:5000], data[5000:]], gzip=True)
        st = gx.gzip_stats()
        bit, at, window = gx.gzip_checkpoint(used)
    assert refused and st["slots_refused"] == 1 and st["members"] == 1, st
    assert (n, used) == (40, len(text))
    assert (bit, at, window) == (8 * (len(first) + GC.HEADER), len(text), b"")
    assert _inflate_from(first + data, bit, b"") == big


def test_bad_data_ends_the_gzip_stream_with_its_offset(ftiny_dir):
    """A flipped CRC, a flipped symbol, a truncated member and junk behind the last member: VG_EIO that names the compressed offset
    the whole-file call names; a valid stream on the same handle afterwards is exact."""
    picks = [c for c in DAMAGED if c[0].startswith(("flip_crc", "flip_symbols", "truncated_mid", "junk_after"))][::2]
    assert len(picks) >= 4
    with GenoIndex.open(os.path.join(ftiny_dir, "idx")) as gx:
        for name, data in picks:
            want = api.gunzip(data, device=None, chunked=True, text_cap=200_000)
            with pytest.raises(VgError) as e:
                gx.fastq_stream([p for p in (data[:1000], data[1000:70_000], data[70_000:]) if p], gzip=True)
            assert e.value.code == -2 and want.error in str(e.value), (name, str(e.value), want.error)
        gx.reset()
        data, text = BY_NAME["level1"]
        n, used, last, refused = gx.fastq_stream([data], gzip=True)
        assert (n, used, refused) == (4000, len(text), False)

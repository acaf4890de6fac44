"""BAM inputs shared by tests/test_bam_cpu.py, tests/test_gpu_bam.py and tests/test_gpu_bam_cli.py (a helper module, not a test
file): a BAM writer on `struct` + vargeno_amd.synth's BGZF blocks, and an INDEPENDENT converter from the inflated BAM stream to the
equivalent FASTQ text -- complement by a table of letters, nothing shared with csrc/vg_bam.h.  Everything is
generated from seeds; nothing compressed is committed.

Three writer styles:
  aligned    the header flushed into blocks of its own, no record straddles a block (what htslib writes)
  spanning   the stream cut every 65 280 bytes regardless of records (what htsjdk writes)
  ragged     block sizes drawn from bgzf_cases.BLOCK_SIZES: records and the header straddle many blocks, empty blocks among them
"""
import functools
import struct
import zlib

import numpy as np

import bgzf_cases as BC
from vargeno_amd import synth

NIB = "=ACMGRSVTWYHKDBN"
CODE = {c: i for i, c in enumerate(NIB)}
COMPLEMENT = {"=": "=", "A": "T", "C": "G", "G": "C", "T": "A", "M": "K", "K": "M", "R": "Y", "Y": "R", "W": "W", "S": "S",
              "V": "B", "B": "V", "H": "D", "D": "H", "N": "N"}
STYLES = ("aligned", "spanning", "ragged")
WINDOW = 65536


# ------------------------------------------------------------------------------------------------ writer
def header(n_ref=0, text=b"@HD\tVN:1.6\tSO:unsorted\n"):
    out = [b"BAM\x01", struct.pack("<i", len(text)), text, struct.pack("<i", n_ref)]
    for i in range(n_ref):
        name = b"ref%d\x00" % i
        out.append(struct.pack("<i", len(name)) + name + struct.pack("<i", 1000 + i))
    return b"".join(out)


def record(name, seq, qual, flag=0, ref_id=-1, pos=-1, mapq=0, cigar=(), next_ref=-1, next_pos=-1, tlen=0, aux=b"", block_size=None):
    """One record as stored: seq is a string over NIB (stored order), qual a sequence of ints (stored order) or None (absent: 0xFF)."""
    name = name.encode() + b"\x00"
    l_seq = len(seq)
    codes = [CODE[c] for c in seq] + [0]
    packed = bytes(codes[2 * i] << 4 | codes[2 * i + 1] for i in range((l_seq + 1) // 2))
    q = b"\xff" * l_seq if qual is None else bytes(qual)
    assert len(q) == l_seq and len(name) <= 255
    body = (struct.pack("<iiBBHHHiiii", ref_id, pos, len(name), mapq, 4680, len(cigar), flag, l_seq, next_ref, next_pos, tlen)
            + name + b"".join(struct.pack("<I", c) for c in cigar) + packed + q + aux)
    return struct.pack("<I", len(body) if block_size is None else block_size) + body


def _block(piece, level=1):
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    return synth.bgzf_block(co.compress(piece) + co.flush(), zlib.crc32(piece), len(piece))


def write(hdr, records, style, seed=1, eof=True):
    """The BAM file's bytes."""
    stream = hdr + b"".join(records)
    if style == "aligned":
        out = [_block(hdr[at:at + 65280]) for at in range(0, len(hdr), 65280)]
        cur = b""
        for r in records:
            assert len(r) <= 65280
            if len(cur) + len(r) > 65280:
                out.append(_block(cur))
                cur = b""
            cur += r
        if cur:
            out.append(_block(cur))
        return b"".join(out) + (synth.BGZF_EOF if eof else b"")
    if style == "spanning":
        return synth.bgzf_bytes(stream, block=65280, level=1, eof=eof)
    assert style == "ragged"
    return synth.bgzf_bytes(stream, block=BC.BLOCK_SIZES, level=1, rng=np.random.default_rng(seed), eof=eof)


# ------------------------------------------------------------------------------------------------ independent converter
def parse_header(raw):
    """(offset of the first record, n_ref)"""
    assert raw[:4] == b"BAM\x01"
    l_text = struct.unpack_from("<i", raw, 4)[0]
    at = 8 + l_text
    n_ref = struct.unpack_from("<i", raw, at)[0]
    at += 4
    for _ in range(n_ref):
        at += 8 + struct.unpack_from("<i", raw, at)[0]
    return at, n_ref


def to_fastq(raw):
    """The equivalent FASTQ text of an inflated BAM stream: (text, reads [(stream offset, bases, quality string)], skipped by flag,
    skipped empty).  The stream must end at a record boundary."""
    at, _ = parse_header(raw)
    out, reads, n_flag, n_empty = [], [], 0, 0
    while at < len(raw):
        block_size, = struct.unpack_from("<I", raw, at)
        ref_id, pos, l_name, mapq, bin_, n_cigar, flag, l_seq = struct.unpack_from("<iiBBHHHi", raw, at + 4)
        assert at + 4 + block_size <= len(raw), "the stream ends inside the record at %d" % at
        p = at + 36
        name = raw[p:p + l_name - 1]
        p += l_name + 4 * n_cigar
        packed = raw[p:p + (l_seq + 1) // 2]
        p += (l_seq + 1) // 2
        q = raw[p:p + l_seq]
        start, at = at, at + 4 + block_size
        if flag & 0x900:
            n_flag += 1
            continue
        if l_seq == 0:
            n_empty += 1
            continue
        seq = "".join(NIB[packed[i >> 1] >> 4 if i % 2 == 0 else packed[i >> 1] & 15] for i in range(l_seq))
        qs = '"' * l_seq if q[0] == 0xFF else "".join(chr(min(v, 93) + 33) for v in q)
        if flag & 0x10:
            seq = "".join(COMPLEMENT[c] for c in reversed(seq))
            qs = qs[::-1]
        out.append(b"@" + name + b"\n" + seq.encode() + b"\n+\n" + qs.encode() + b"\n")
        reads.append((start, seq, qs))
    return b"".join(out), reads, n_flag, n_empty


def boundary_before(raw, n):
    """The largest record boundary of the stream at or below n: where the record that raw[:n] ends inside starts."""
    at, _ = parse_header(raw)
    while at + 4 <= n:
        nxt = at + 4 + struct.unpack_from("<I", raw, at)[0]
        if nxt > n:
            break
        at = nxt
    return at


def expected_batch(reads):
    """The flat batch layout of the equivalent text: (offsets uint64[n + 1], bases uint8, gate uint32[n]) -- gate bit c set iff quality
    character c is below '8', for c < min(len >> 5, 32): vg_fq_gather's rule."""
    offsets = np.zeros(len(reads) + 1, dtype=np.uint64)
    gate = np.zeros(len(reads), dtype=np.uint32)
    for i, (_, seq, qs) in enumerate(reads):
        offsets[i + 1] = offsets[i] + np.uint64(len(seq))
        g = 0
        for c in range(min(len(seq) >> 5, 32)):
            if qs[c] < "8":
                g |= 1 << c
        gate[i] = g
    bases = np.frombuffer("".join(s for _, s, _ in reads).encode(), dtype=np.uint8)
    return offsets, bases, gate


def revcomp(seq):
    return "".join(COMPLEMENT[c] for c in reversed(seq))


# ------------------------------------------------------------------------------------------------ cases
def _ftiny_records(extra=None):
    """F-tiny's 4 000 reads as records: a seeded half stored reverse-complemented with 0x10, 200 secondary / supplementary decoys
    interleaved, some records with CIGARs, aux fields and refID >= 0.  extra: {read index: record bytes} put in front of that read."""
    lines = BC.ftiny_text().split(b"\n")
    rng = np.random.default_rng(41)
    n = len(lines) // 4
    decoy_at = set(int(v) for v in rng.choice(n, 200, replace=False))
    recs = []
    for i in range(n):
        if extra and i in extra:
            recs.append(extra[i])
        name, seq, qs = lines[4 * i][1:].decode(), lines[4 * i + 1].decode().upper(), lines[4 * i + 3].decode()
        if i in decoy_at:
            dl = int(rng.integers(1, 200))
            recs.append(record("decoy%d" % i, "".join(rng.choice(list("ACGT"), dl)), list(rng.integers(0, 60, dl)), flag=int(rng.choice([0x100, 0x800, 0x910])),
                               ref_id=int(rng.integers(0, 300)), pos=int(rng.integers(0, 1000))))
        q = [ord(c) - 33 for c in qs]
        kw = {}
        if rng.random() < 0.5:
            seq, q, kw["flag"] = revcomp(seq), q[::-1], 0x10
        if rng.random() < 0.3:
            kw.update(ref_id=int(rng.integers(0, 300)), pos=int(rng.integers(0, 1000)), cigar=(len(seq) << 4,), mapq=60, next_ref=int(rng.integers(-1, 300)), next_pos=int(rng.integers(-1, 1000)))
        if rng.random() < 0.3:
            kw["aux"] = b"NMC\x03" + b"RGZgrp1\x00" + b"XSi" + struct.pack("<i", int(rng.integers(-5, 5)))
        recs.append(record(name, seq, q, **kw))
    return recs


@functools.lru_cache(maxsize=None)
def ftiny_bam(style):
    """(file bytes, inflated stream) of F-tiny as BAM; the helper asserts that its equivalent text is the fixture's, up to letter
    case (BAM has none; the reference reads a and A alike, util.c:89-111)."""
    hdr, recs = header(300), _ftiny_records()
    raw = hdr + b"".join(recs)
    text, reads, n_flag, n_empty = to_fastq(raw)
    want = BC.ftiny_text().split(b"\n")
    got = text.split(b"\n")
    assert len(got) == len(want) and n_flag == 200 and n_empty == 0
    assert got[0::4] == want[0::4] and got[1::4] == [b.upper() for b in want[1::4]] and got[3::4] == want[3::4]
    return write(hdr, recs, style, seed=3), raw


@functools.lru_cache(maxsize=None)
def corner_bam(style):
    """At most 300 records: l_seq in {0, 1, 31, 32, 33, 63, 64, 65, 1022}, forward and reversed; absent qualities; q > 93; every
    4-bit code; 254-character names."""
    rng = np.random.default_rng(17)
    recs = []
    k = 0
    for l in (0, 1, 31, 32, 33, 63, 64, 65, 1022):
        for rev in (0, 0x10):
            for variant in ("plain", "noqual", "highq", "allcodes", "longname"):
                seq = "".join(rng.choice(list("ACGT"), l))
                q = list(int(v) for v in rng.integers(0, 50, l))
                name = "c%d" % k
                if variant == "noqual":
                    q = None
                elif variant == "highq":
                    q = list(int(v) for v in rng.integers(60, 255, l))          # (never 0xFF first: that means absent)
                elif variant == "allcodes":
                    seq = "".join(NIB[(j + k) % 16] for j in range(l))
                elif variant == "longname":
                    name = ("n%d_" % k).ljust(254, "x")
                recs.append(record(name, seq, q, flag=rev | (0x1 | 0x40 if k % 3 == 0 else 0)))
                k += 1
    assert len(recs) <= 300
    hdr = header(2)
    return write(hdr, recs, style, seed=5), hdr + b"".join(recs)


@functools.lru_cache(maxsize=None)
def decoy_bam():
    """Records with XX:B:C aux arrays whose bytes are three well-formed fake records; padding places a 64 KiB window boundary just
    before the fakes, inside the aux data, so the window's speculative guess (the fakes) is wrong.  Returns (file bytes, inflated
    stream, offsets of the window boundaries that fall right before fakes)."""
    rng = np.random.default_rng(23)
    hdr = header(4)
    fakes = b"".join(record("fake%d" % i, "ACGTACGTAC", [30] * 10, ref_id=1, pos=5) for i in range(3))

    def real(i, pad=0):
        seq = "".join(rng.choice(list("ACGT"), 100))
        aux = b"XXBC" + struct.pack("<I", pad + len(fakes)) + bytes(255 for _ in range(pad)) + fakes       # (0xFF padding: no plausible record inside it)
        return record("real%d" % i, seq, list(int(v) for v in rng.integers(0, 60, 100)), aux=aux)

    recs, at, hits = [], len(hdr), []
    for i in range(900):
        r = real(i)
        fake_at = at + len(r) - len(fakes)                       # where this record's fakes would start without padding
        nxt = (at // WINDOW + 1) * WINDOW
        if fake_at <= nxt < fake_at + 2000 and i > 0:
            r = real(i, pad=nxt - fake_at)
            assert at + len(r) - len(fakes) == nxt
            hits.append(nxt)
        recs.append(r)
        at += len(r)
    assert len(hits) >= 2
    return write(hdr, recs, "spanning"), hdr + b"".join(recs), hits


@functools.lru_cache(maxsize=None)
def long_read_bam(style="spanning"):
    """F-tiny as BAM with a 2 000-base read in the middle (the device route refuses its chunk; the text route does the same with
    the equivalent text): (file bytes, inflated stream).  In the text the read's two long lines are four fgets() lines, which
    shifts the reference's four-line rhythm by two for everything behind it -- quality strings would be taken for reads and the
    job would abort on their characters.  So the read is followed at once by a second one of its kind (twelve fgets() lines in
    all: the rhythm is back), and the qualities of both are 32, 34, 38, 51 -- the letters A, C, G, T -- because the reference takes
    the tail of the first one's quality line for a read."""
    rng = np.random.default_rng(29)
    longs = b"".join(record("long%d" % i, "".join(rng.choice(list("ACGT"), 2000)), [int(v) for v in rng.choice([32, 34, 38, 51], 2000)]) for i in range(2))
    hdr, recs = header(300), _ftiny_records(extra={2000: longs})
    return write(hdr, recs, style, seed=7), hdr + b"".join(recs)


@functools.lru_cache(maxsize=None)
def damaged():
    """name -> (file bytes, what it is).  Built on the spanning F-tiny file."""
    data, raw = ftiny_bam("spanning")
    hdr_end, _ = parse_header(raw)
    _, reads, _, _ = to_fastq(raw)
    out = {}
    # cut mid-record: whole blocks only, the last record of block 5 unfinished
    cut_raw = raw[:6 * 65280]
    last_start = max(s for s, _, _ in reads if s < len(cut_raw))
    out["cut_mid_record"] = (synth.bgzf_bytes(cut_raw, block=65280, level=1, eof=True), cut_raw)
    out["cut_mid_header"] = (synth.bgzf_bytes(raw[:hdr_end - 100], block=65280, level=1), raw[:hdr_end - 100])
    # a block_size of 7 in record 1 000
    recs = _ftiny_records()
    at = hdr_end + sum(len(r) for r in recs[:1000])
    bad = raw[:at] + struct.pack("<I", 7) + raw[at + 4:]
    out["block_size_7"] = (synth.bgzf_bytes(bad, block=65280, level=1), at)
    blocks = BC.split_blocks(data)
    hurt = bytearray(data)
    hurt[blocks[9][0] + 18 + 40] ^= 0x04
    out["flipped_bit_block_9"] = (bytes(hurt), blocks[9][0])
    out["cram"] = (b"CRAM\x03\x00" + bytes(100), None)
    assert last_start < len(cut_raw)
    return out

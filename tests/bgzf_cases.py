"""BGZF inputs shared by tests/test_bgzf_cpu.py and tests/test_gpu_bgzf.py (a helper module, not a test file).

Everything is generated from seeds with vargeno_amd.synth.bgzf_bytes (Python's zlib, raw deflate); nothing compressed is
committed.  The expected text of a valid case is the text it was made from (checked here against gzip.decompress); what a
damaged block should do is what Python's zlib says about the same bytes."""
import functools
import gzip
import os
import struct
import zlib

import numpy as np

from conftest import GOLDEN
from vargeno_amd import synth

BLOCK_SIZES = (0, 1, 7, 311, 4096, 65280)


@functools.lru_cache(maxsize=None)
def ftiny_text():
    return gzip.open(os.path.join(GOLDEN, "ftiny.reads.fq.gz"), "rb").read()


@functools.lru_cache(maxsize=None)
def ftiny_variants():
    """F-tiny's reads.fq (1 043 070 bytes, 4 000 records) under every block shape: name -> BGZF bytes."""
    t = ftiny_text()
    v = {
        "stored": synth.bgzf_bytes(t, block=65000, level=0),
        "fixed": synth.bgzf_bytes(t, strategy=zlib.Z_FIXED),
        "level1": synth.bgzf_bytes(t, level=1),
        "level6": synth.bgzf_bytes(t, level=6),
        "level9": synth.bgzf_bytes(t, level=9),
        "huffman_only": synth.bgzf_bytes(t, strategy=zlib.Z_HUFFMAN_ONLY),
        "full_flush": synth.bgzf_bytes(t, flush_at=0.37),
        "block_sizes": synth.bgzf_bytes(t, block=BLOCK_SIZES, rng=np.random.default_rng(11)),
    }
    for name, data in v.items():
        assert gzip.decompress(data) == t, name
    return v


@functools.lru_cache(maxsize=None)
def valid_cases():
    """[(name, BGZF bytes, text)]"""
    t = ftiny_text()
    cases = [("ftiny_" + k, d, t) for k, d in ftiny_variants().items()]
    rng = np.random.default_rng(5)
    head = t[:150_000]
    # another subfield in front of BC
    cases.append(("extra_subfield", synth.bgzf_bytes(head, extra_before=b"XY" + struct.pack("<H", 3) + b"abc"), head))
    cases.append(("no_eof_marker", synth.bgzf_bytes(head, eof=False), head))
    r = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    far = r + r[:300]                                             # distance 32 768, after a stored fallback
    cases.append(("distance_32768", synth.bgzf_bytes(far, block=len(far), level=9), far))
    ones = b"I" * 65536                                           # ISIZE at its maximum, distance 1, length-258 chains
    cases.append(("isize_max", synth.bgzf_bytes(ones, block=65536), ones))
    p3 = b"ACG" * 7000 + b"T" + b"GT" * 3000 + b"ACGTA" * 900      # periods 3, 2, 5: copy distances below the lane count
    cases.append(("short_periods", synth.bgzf_bytes(p3), p3))
    noise = rng.integers(0, 256, 65280, dtype=np.uint8).tobytes()  # zlib stores it
    cases.append(("random_stored", synth.bgzf_bytes(noise), noise))
    cases.append(("empty_text", synth.bgzf_bytes(b""), b""))
    for name, data, text in cases[len(ftiny_variants()):]:
        assert gzip.decompress(data) == text, name
    return cases


def split_blocks(data):
    """[(offset, block bytes)] of a well-formed BGZF file (BC is the first subfield unless the header says otherwise)."""
    out, at = [], 0
    while at < len(data):
        xlen = struct.unpack_from("<H", data, at + 10)[0]
        x, bsize = at + 12, None
        while x < at + 12 + xlen:
            si, slen = data[x:x + 2], struct.unpack_from("<H", data, x + 2)[0]
            if si == b"BC":
                bsize = struct.unpack_from("<H", data, x + 4)[0]
            x += 4 + slen
        out.append((at, data[at:at + bsize + 1]))
        at += bsize + 1
    return out


def _reblock(block, payload=None, crc=None, isize=None):
    """A block (BC first, XLEN 6) with some of its parts replaced, BSIZE adjusted to the payload."""
    old_payload = block[18:-8]
    old_crc, old_isize = struct.unpack("<II", block[-8:])
    return synth.bgzf_block(old_payload if payload is None else payload, old_crc if crc is None else crc, old_isize if isize is None else isize)


def zlib_verdict(block):
    """What Python's zlib makes of a block's payload against its trailer: None if it is rejected (an error, trailing garbage,
    an unfinished stream, another length or CRC), else the text."""
    payload = block[18:-8]
    crc, isize = struct.unpack("<II", block[-8:])
    try:
        d = zlib.decompressobj(-15)
        text = d.decompress(payload)
        if not d.eof or len(text) != isize or zlib.crc32(text) != crc:
            return None
        return text
    except zlib.error:
        return None


def _oversubscribed_dynamic():
    """A dynamic-Huffman block whose code-length code has three codes of length 1."""
    bits, n = 0, 0

    def put(v, w):
        nonlocal bits, n
        bits |= v << n
        n += w

    put(1, 1); put(2, 2)                      # BFINAL, BTYPE = dynamic
    put(0, 5); put(0, 5); put(15, 4)          # HLIT 257, HDIST 1, HCLEN 19
    for i in range(19):
        put(1 if i < 3 else 0, 3)
    put(0, 16)
    return bits.to_bytes((n + 7) // 8, "little")


@functools.lru_cache(maxsize=None)
def damaged_cases():
    """{base: [(name, damaged block bytes, zlib's verdict)]} -- from one valid block each (stored, fixed, dynamic), a fixed seeded
    list of at most 32 mutations.  The verdict is None where zlib rejects the bytes (or their CRC / length differ), else the text."""
    t = ftiny_text()[:20_000]
    bases = {"stored": synth.bgzf_bytes(t, level=0, eof=False), "fixed": synth.bgzf_bytes(t, strategy=zlib.Z_FIXED, eof=False), "dynamic": synth.bgzf_bytes(t, level=6, eof=False)}
    out = {}
    for bi, (base, block) in enumerate(bases.items()):
        assert len(split_blocks(block)) == 1 and zlib_verdict(block) == t
        rng = np.random.default_rng(100 + bi)
        payload = block[18:-8]
        crc, isize = struct.unpack("<II", block[-8:])
        muts = []
        for k in range(12):                                        # payload bit flips: half of them in the first bytes, where the headers are
            at = int(rng.integers(0, 12 if k < 6 else len(payload)))
            bit = int(rng.integers(0, 8))
            p = bytearray(payload)
            p[at] ^= 1 << bit
            muts.append(("flip_%d_%d" % (at, bit), _reblock(block, payload=bytes(p))))
        muts.append(("truncated_by_1", _reblock(block, payload=payload[:-1])))
        muts.append(("truncated_by_half", _reblock(block, payload=payload[:len(payload) // 2])))
        muts.append(("isize_plus_1", _reblock(block, isize=isize + 1)))
        muts.append(("isize_minus_1", _reblock(block, isize=isize - 1)))
        muts.append(("isize_65536", _reblock(block, isize=65536)))
        muts.append(("crc_bit", _reblock(block, crc=crc ^ (1 << int(rng.integers(0, 32))))))
        if base == "stored":
            p = bytearray(payload)
            p[3] ^= 0x10                                           # NLEN of the first stored block
            muts.append(("nlen_wrong", _reblock(block, payload=bytes(p))))
        if base == "dynamic":
            muts.append(("oversubscribed_lengths", _reblock(block, payload=_oversubscribed_dynamic())))
        assert len(muts) <= 32
        out[base] = [(name, b, zlib_verdict(b)) for name, b in muts]
    return out


def bsize_past_the_data(block):
    """The block with BSIZE pointing 100 bytes past its end (as the last block of a buffer it is incomplete, never decoded)."""
    bsize = struct.unpack_from("<H", block, 16)[0]
    return block[:16] + struct.pack("<H", bsize + 100) + block[18:]

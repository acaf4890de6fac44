"""Texts shared by tests/test_deflate_cpu.py and tests/test_gpu_deflate.py (a helper module, not a test file).

Everything is generated from seeds or read from tests/golden; nothing compressed is committed.  What a BGZF file must inflate to is
the text it was made from, and who says so is Python's zlib (gzip.decompress, or -- for files of very many tiny blocks, where
gzip.decompress spends microseconds of Python per member -- zlib.decompress of every block's payload with its CRC32 and ISIZE
compared here) and the library's own host inflater, never the compressor under test."""
import functools
import glob
import gzip
import os
import struct
import zlib

import numpy as np

from bgzf_cases import BLOCK_SIZES, ftiny_text, split_blocks  # noqa: F401  (re-exported)
from conftest import GOLDEN

MAX_BLOCK = 65280
EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
HEADER12 = bytes.fromhex("1f8b08040000000000ff0600")


def golden_vcf_texts():
    """{file name: text} of every tests/golden/*.vcf.gz"""
    return {os.path.basename(f): gzip.open(f, "rb").read() for f in sorted(glob.glob(os.path.join(GOLDEN, "*.vcf.gz")))}


def _noise(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def far_repeat(distance, repeat=True):
    """One 65 280-byte block: 300 bytes of noise, newlines up to `distance`, then 300 bytes -- the block's first 300 again (a repeat
    at exactly that distance) or with repeat=False fresh noise --, then newlines.  The newlines between the two keep the match
    finder's memory of the first 300 bytes alive (a run looks the same everywhere), and the block shrinks: it is coded, not stored."""
    rng = np.random.default_rng(distance)
    r = _noise(rng, 300)
    mid = r if repeat else _noise(rng, 300)
    return r + b"\n" * (distance - 300) + mid + b"\n" * (MAX_BLOCK - distance - 300)


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, text)]"""
    rng = np.random.default_rng(2024)
    out = [("empty", b""), ("one_byte", b"V")]
    for b in (7, 311, 4096, MAX_BLOCK):                            # block - 1, block, block + 1 of every block length but 1 (whose neighbours are above)
        base = (b"##fileformat=VCFv4.2\n" + _noise(rng, 64)) * (b // 85 + 2)
        for n in (b - 1, b, b + 1):
            out.append(("len_%d" % n, base[:n]))
    out.append(("two_bytes", b"VC"))
    out.append(("run_131072", b"I" * 131072))                     # distance 1, length-258 chains, a run across a block cut
    out.append(("periods_2_3_5", b"GT" * 3000 + b"ACG" * 7000 + b"T" + b"ACGTA" * 900))      # copy distances below the lane count
    out.append(("distance_32768", far_repeat(32768)))             # the farthest copy the format has
    out.append(("distance_32769", far_repeat(32769)))             # one byte farther: must not be coded as a match
    acgt = bytes(b"ACGT"[i] for i in rng.integers(0, 4, 5000))
    out.append(("match_to_the_last_byte", acgt + acgt[1000:1200]))
    out.append(("runs_258_259", _noise(rng, 100) + b"x" * 258 + _noise(rng, 100) + b"y" * 259 + _noise(rng, 100)))
    out.append(("random_65280", _noise(rng, MAX_BLOCK)))
    out.append(("high_bytes", bytes(int(v) for v in rng.integers(0x80, 0x100, 3000)) * 9 + "Grüße, señor: 100 µg\n".encode() * 400))   # the 9-bit literals of the fixed code
    out += sorted(golden_vcf_texts().items())
    out.append(("ftiny_reads", ftiny_text()))
    return out


def names():
    return [c[0] for c in cases()]


def n_blocks(n, block):
    b = block or MAX_BLOCK
    return (n + b - 1) // b


def _check_stored_run(body, text, b):
    """The leading whole blocks of a file of very many blocks, when all of them are stored (blocks of a few bytes cannot shrink),
    without a Python step per block: the headers compared as one array; the payloads -- with BFINAL cleared and an empty final
    stored block behind them they are ONE raw deflate stream -- inflated by one zlib call; the trailers compared as one array.
    Returns (file bytes, text bytes) checked: (0, 0) when the file is not of that shape, and check_file's loop takes all of it."""
    size, k = 18 + 5 + b + 8, len(text) // b
    if k == 0 or k * size > len(body):
        return 0, 0
    rows = np.frombuffer(body, dtype=np.uint8)[:k * size].reshape(k, size)
    head = np.frombuffer(HEADER12 + b"BC\x02\x00" + struct.pack("<H", size - 1) + b"\x01", dtype=np.uint8)
    if not (rows[:, :19] == head).all():
        return 0, 0
    payloads = rows[:, 18:size - 8].copy()
    payloads[:, 0] = 0
    assert zlib.decompress(payloads.tobytes() + b"\x01\x00\x00\xff\xff", -15) == text[:k * b]
    trailers = rows[:, size - 8:].copy().view("<u4")
    crcs = np.fromiter((zlib.crc32(text[i:i + b]) for i in range(0, k * b, b)), dtype=np.uint32, count=k)
    assert (trailers[:, 0] == crcs).all() and (trailers[:, 1] == b).all()
    return k * size, k * b


def check_file(data, text, block, eof=True):
    """`data` is the BGZF file of `text` in blocks of `block`, by Python's zlib alone and block by block: bgzip's header (the 12
    fixed bytes, one BC subfield, BSIZE at most 65 536), a payload that zlib inflates to exactly the block's slice of the text, its
    CRC32 and ISIZE, nothing between the blocks; the end-of-file marker last iff `eof`.  Files of up to 20 000 blocks also go through
    gzip.decompress as a whole and through split_blocks."""
    b = block or MAX_BLOCK
    body = data[:-len(EOF_MARKER)] if eof else data
    if eof:
        assert data[-len(EOF_MARKER):] == EOF_MARKER
    elif text:
        assert data[-len(EOF_MARKER):] != EOF_MARKER
    at, t_at = 0, 0
    if n_blocks(len(text), b) > 20000:
        at, t_at = _check_stored_run(body, text, b)
    while at < len(body):                                          # one block per step
        assert body[at:at + 12] == HEADER12 and body[at + 12:at + 16] == b"BC\x02\x00", at
        total = struct.unpack_from("<H", body, at + 16)[0] + 1
        assert 26 < total <= 65536 and at + total <= len(body), at
        crc, isize = struct.unpack_from("<II", body, at + total - 8)
        want = text[t_at:t_at + b]
        assert isize == len(want) and 0 < isize <= b, at
        d = zlib.decompressobj(-15)
        got = d.decompress(body[at + 18:at + total - 8])
        assert d.eof and not d.unused_data and got == want and zlib.crc32(got) == crc, at
        at += total
        t_at += isize
    assert t_at == len(text)
    if n_blocks(len(text), b) <= 20000:
        assert gzip.decompress(data) == text
        blocks = split_blocks(data)
        assert len(blocks) == n_blocks(len(text), b) + (1 if eof else 0)
        assert b"".join(blk for _, blk in blocks) == data


def huffman_only_size(text):
    """Bytes of the BGZF file zlib's Z_HUFFMAN_ONLY makes of `text` in 65 280-byte blocks: raw deflate plus 26 bytes of header and
    trailer per block.  What a coder that finds no match can reach."""
    total = 0
    for at in range(0, len(text), MAX_BLOCK):
        c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_HUFFMAN_ONLY)
        total += len(c.compress(text[at:at + MAX_BLOCK]) + c.flush()) + 26
    return total

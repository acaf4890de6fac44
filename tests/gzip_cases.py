"""Plain gzip inputs shared by tests/test_gzip_cpu.py and tests/test_gpu_gzip.py (a helper module, not a test file).

Everything is generated from seeds with vargeno_amd.synth.gzip_bytes (Python's zlib, raw deflate); nothing compressed is committed.
The expected text of every valid case is what Python's gzip.decompress makes of the bytes; a damaged case is one Python rejects."""
import functools
import gzip
import os
import zlib

import numpy as np

from conftest import GOLDEN
from vargeno_amd import synth

CHUNKS = (1024, 8192, 32768)
HEADER = 10                                   # bytes of a member header without optional fields: where a file's first slot starts


@functools.lru_cache(maxsize=None)
def ftiny_text():
    return gzip.open(os.path.join(GOLDEN, "ftiny.reads.fq.gz"), "rb").read()


def _acgt(rng, n):
    return rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n).tobytes()


@functools.lru_cache(maxsize=None)
def decoy():
    """(bytes, text, file offset of the decoy).  Raw DEFLATE pieces joined by full flushes; the middle piece is a stored block whose
    payload is the bytes of a real, byte-aligned, non-final dynamic block, and its first payload byte is the first byte of a
    chunk's range at every chunk size of CHUNKS.  The finder must guess it, the confirm reject it, the repair fix it."""
    t = ftiny_text()
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    payload = co.compress(t[500_000:501_500]) + co.flush(zlib.Z_FULL_FLUSH)
    # BFINAL 0, BTYPE 2 at bit 0; and short enough that the stored block ends inside the decoy's own chunk at every chunk size:
    # the chain's exit lies before the next guess, so the chunk cannot be dropped, it has to be decoded again
    assert payload[0] & 7 == 4 and len(payload) < 1000
    data, text, where = synth.gzip_bytes(segments=[("deflate", t[:200_000]), ("pad", 32768, HEADER), ("stored", payload), ("deflate", t[200_000:400_000])])
    at = where[2] + 5
    assert (at - HEADER) % 32768 == 0
    return data, text, at


@functools.lru_cache(maxsize=None)
def far_references():
    """Distance-32 768 and length-258 period-1 references (a hand-made fixed block: zlib's deflate writes no distance beyond
    32 506) behind a dynamic block that a chunk can enter at: they reach in front of the chunk's entry."""
    rng = np.random.default_rng(23)
    a, b = _acgt(rng, 40_000), _acgt(rng, 3_000)
    ops = [(258, 32768), ord("Q"), (258, 1), (258, 32768), (100, 259), (3, 1), (17, 32767), (258, 3), (258, 32768)]
    segs = [("deflate", a), ("deflate", b), ("fixed", ops), ("deflate", a[:5000]), ("deflate", b), ("fixed", ops[::-1] + [ord("Z")])]
    data, text, _ = synth.gzip_bytes(segments=segs)
    return data, text


@functools.lru_cache(maxsize=None)
def valid_cases():
    """[(name, gzip bytes, text)]; the text is gzip.decompress's."""
    t = ftiny_text()
    cases = [
        ("level1", synth.gzip_bytes(t, level=1)),
        ("level6", synth.gzip_bytes(t, level=6)),
        ("level9", synth.gzip_bytes(t, level=9)),
        ("memlevel1", synth.gzip_bytes(t, mem_level=1)),
        ("memlevel9", synth.gzip_bytes(t, mem_level=9)),
        ("header_fields", synth.gzip_bytes(t[:300_000], name=b"reads.fq", extra=b"XY\x03\x00abc", comment=b"a comment", hcrc=True)),
        ("fixed", synth.gzip_bytes(t[:300_000], strategy=zlib.Z_FIXED)),
        ("stored", synth.gzip_bytes(t[:300_000], level=0)),
        ("sync_flush", synth.gzip_bytes(t[:300_000], flush=zlib.Z_SYNC_FLUSH)),
        ("full_flush", synth.gzip_bytes(t[:300_000], flush=zlib.Z_FULL_FLUSH)),
        ("three_members", synth.gzip_bytes(t[:200_000]) + synth.gzip_bytes(b"") + synth.gzip_bytes(t[200_000:300_000], level=1)),
        ("short_file", synth.gzip_bytes(t[:700])),
        ("empty_member", synth.gzip_bytes(b"")),
        ("ratio_254", synth.gzip_bytes(t[:260] * 20_000, level=9)),
        ("far_references", far_references()[0]),
        ("decoy", decoy()[0]),
    ]
    # a member that ends (trailer included) exactly on a chunk boundary of 1 024 bytes, counted from the slot's first byte: a stored
    # block of the right size behind the compressed part
    probe = synth.gzip_bytes(segments=[("deflate", t[:120_000])])[0]
    fill = (-(len(probe) - HEADER + 5)) % 1024
    m = synth.gzip_bytes(segments=[("deflate", t[:120_000]), ("stored", t[120_000:120_000 + fill])])[0]
    assert (len(m) - HEADER) % 1024 == 0
    cases.append(("ends_on_chunk_boundary", m + synth.gzip_bytes(t[120_000:150_000])))
    return [(name, data, gzip.decompress(data)) for name, data in cases]


ORDINARY = ("level1", "level6", "level9", "memlevel1", "memlevel9", "header_fields")


def python_rejects(data):
    try:
        gzip.decompress(data)
    except Exception:                                               # (zlib.error, EOFError, gzip.BadGzipFile)
        return True
    return False


@functools.lru_cache(maxsize=None)
def damaged_cases():
    """[(name, bytes)] -- every one rejected by Python's gzip module.  Seeded bit flips in the member header, the first block's
    header and code lengths, symbols further on, and the trailer; truncations at every kind of place; junk behind the last member."""
    t = ftiny_text()[:150_000]
    good = synth.gzip_bytes(t, level=6)
    two = good + synth.gzip_bytes(t[:20_000], level=1)
    rng = np.random.default_rng(77)
    out = []

    def flip(data, at, bit):
        b = bytearray(data)
        b[at] ^= 1 << bit
        return bytes(b)

    places = [("magic", 0, 2), ("method", 2, 3), ("flags_reserved", 3, 4)]
    places += [("block_header", HEADER, HEADER + 2), ("code_lengths", HEADER + 2, HEADER + 60), ("symbols", HEADER + 200, len(good) - 8),
               ("late_symbols", len(good) - 2000, len(good) - 8), ("crc", len(good) - 8, len(good) - 4), ("isize", len(good) - 4, len(good))]
    for name, lo, hi in places:
        for k in range(4):
            at, bit = int(rng.integers(lo, hi)), int(rng.integers(0, 8))
            if name == "flags_reserved":
                bit = 5 + k % 3
            out.append(("flip_%s_%d_%d" % (name, at, bit), flip(good, at, bit)))
    out.append(("flip_second_member_symbols", flip(two, len(good) + 400, 3)))
    out.append(("flip_second_member_crc", flip(two, len(two) - 6, 0)))
    for name, n in (("in_header", 5), ("after_header", HEADER), ("in_first_block_header", HEADER + 20), ("mid_stream", len(good) // 2),
                    ("before_trailer", len(good) - 8), ("in_trailer", len(good) - 3), ("second_member_header", len(good) + 4),
                    ("second_member_stream", len(good) + 1000)):
        out.append(("truncated_" + name, two[:n]))
    out.append(("junk_after_last_member", good + b"\x00\x01garbage that is no gzip header"))
    out.append(("junk_one_byte", good + b"\x1e"))
    return [(name, d) for name, d in out if python_rejects(d)]

"""Texts, histograms and independent judges shared by tests/test_deflate_dynamic_cpu.py and tests/test_gpu_deflate_dynamic.py (a
helper module, not a test file).  Everything is generated from seeds; nothing compressed is committed.  The judges are Python's
zlib, a reader of the dynamic header written here, and a Huffman tree built here -- never the compressor under test."""
import functools
import heapq
import zlib

import numpy as np

import deflate_cases as DC

MAX_BLOCK = DC.MAX_BLOCK
FILL = b"\n"
LENGTH_BASES = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]      # symbols 257..285
DIST_BASES = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]


def _marker(rng, n):
    """n bytes that hold no newline and begin with no byte another marker is likely to begin with"""
    return bytes(int(v) for v in rng.integers(0x21, 0x100, n))


@functools.lru_cache(maxsize=None)
def every_symbol_block():
    """One block in which every byte value, every length symbol the match finder can emit (258..285: it takes no match shorter
    than four bytes) and every distance symbol occurs: the largest header there is.
      - a permutation of the 256 byte values;
      - distance symbols 0..11: a pattern of period P in {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49} that begins P bytes before a
        multiple of 64, so that the position at the multiple finds its candidate -- entered by the group before -- exactly P back;
      - distance symbols 12..21, lengths 59..258: a marker of fresh bytes, newlines, and the marker again at the symbol's base;
      - distance symbols 22..29 and the lengths 4..51: eighteen short markers side by side, and far behind them their copies at
        distances that grow from copy to copy, so that a newline ends every copy where the source goes on with the next marker.
    Newlines fill the gaps: a run enters one hash value, so the markers' entries survive until their copies arrive."""
    rng = np.random.default_rng(20261020)
    t = bytearray(rng.permutation(256).astype(np.uint8).tobytes())
    for p in (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49):
        t += FILL * 8
        t += FILL * ((-(len(t) + p)) % 64)                            # the pattern begins p bytes before a multiple of 64
        period = bytes(0x30 + i for i in range(p))
        t += (period * (2 + 80 // p))[:p + 12 + p % 5]
    for d, ln in zip(DIST_BASES[12:22], LENGTH_BASES[19:]):
        m = _marker(rng, ln)
        t += FILL * 4 + m + FILL * (d - ln) + m
    short = LENGTH_BASES[1:19]
    src = len(t) + 4
    t += FILL * 4
    markers = [_marker(rng, ln) for ln in short]
    t += b"".join(markers)
    dists = DIST_BASES[22:] + [DIST_BASES[29] + 100 * k for k in range(1, 11)]
    at = src
    for m, d in zip(markers, dists):
        t += FILL * (at + d - len(t))
        t += m
        at += len(m)
    t += FILL * 50
    assert len(t) <= MAX_BLOCK
    return bytes(t)


@functools.lru_cache(maxsize=None)
def wide_token_block():
    """One block with a single match of length 240 at a distance of some 30 000 among many short near matches: its length and
    distance symbols occur once, so their codes are long, and both carry their most extra bits: a token of more than 32 bits, which
    straddles three words of the coder's window."""
    rng = np.random.default_rng(7)
    far = bytes(int(v) for v in rng.integers(0x80, 0x100, 240))       # bytes the rest never uses
    words = [b"0|0:", b"0|1:", b"1|1:", b"ACGT", b"\tPASS\t", b"GT:GQ", b"chr1\t", b"\t.\t"]
    def common(n):
        out = bytearray()
        while len(out) < n:
            out += words[int(rng.integers(0, len(words)))] + bytes([0x30 + int(rng.integers(0, 10))])
        return bytes(out[:n])
    return far + common(30000) + far + common(20000)


@functools.lru_cache(maxsize=None)
def new_cases():
    """[(name, text)]: the dynamic mode's own edge cases"""
    rng = np.random.default_rng(99)
    line = b"chr1\t1000\t.\tA\tG\t50\tPASS\t.\tGT:GQ\t0|1:45\n"
    return [("block_of_64", (line * 2)[:64]), ("block_of_65", (line * 2)[:65]),
            ("no_match_256", rng.permutation(256).astype(np.uint8).tobytes()),                    # 256 distinct bytes: literals alone
            ("one_byte_300", b"Q" * 300),                                                          # one literal and one distance in use
            ("every_symbol", every_symbol_block()),
            ("wide_token", wide_token_block())]


def zlib_level1_size(text):
    """Bytes of the BGZF file zlib level 1 (default strategy) makes of `text` in 65 280-byte blocks: raw deflate plus 26 bytes of
    header and trailer per block (the end-of-file marker is not counted: add it to compare whole files)."""
    total = 0
    for at in range(0, len(text), MAX_BLOCK):
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        total += len(c.compress(text[at:at + MAX_BLOCK]) + c.flush()) + 26
    return total


def block_payloads(data):
    """[(payload, ISIZE)] of the blocks of a BGZF file, the end-of-file marker included"""
    return [(blk[18:-8], int.from_bytes(blk[-4:], "little")) for _, blk in DC.split_blocks(data)]


def block_form(payload):
    """0 stored, 1 fixed, 2 dynamic"""
    return payload[0] >> 1 & 3


class _Bits:
    def __init__(self, data):
        self.v, self.at = int.from_bytes(data, "little"), 0

    def get(self, n):
        x = self.v >> self.at & ((1 << n) - 1)
        self.at += n
        return x


def _canonical_decoder(lens):
    """{(length, code as read MSB first): symbol}"""
    out, code = {}, 0
    for ln in range(1, 16):
        for s, l in enumerate(lens):
            if l == ln:
                out[(ln, code)] = s
                code += 1
        code <<= 1
    return out


def dynamic_header(payload):
    """The header of a BTYPE 2 payload read here: (literal/length code lengths, distance code lengths, HCLEN, bits of the header)."""
    b = _Bits(payload)
    assert b.get(3) == 5
    hlit, hdist, hclen = b.get(5) + 257, b.get(5) + 1, b.get(4) + 4
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    cl = [0] * 19
    for i in range(hclen):
        cl[order[i]] = b.get(3)
    dec, lens = _canonical_decoder(cl), []
    while len(lens) < hlit + hdist:
        code, n = 0, 0
        while (n, code) not in dec:
            code, n = code << 1 | b.get(1), n + 1
            assert n <= 7
        s = dec[(n, code)]
        if s < 16:
            lens.append(s)
        elif s == 16:
            lens += [lens[-1]] * (3 + b.get(2))
        else:
            lens += [0] * (3 + b.get(3) if s == 17 else 11 + b.get(7))
    assert len(lens) == hlit + hdist
    return lens[:hlit], lens[hlit:], hclen, b.at


# ---- histograms for the code-length builder, and an unlimited Huffman tree to judge it by ----
def fibonacci(n):
    out, a, b = [], 1, 1
    for _ in range(n):
        out.append(a)
        a, b = b, a + b
    return out


@functools.lru_cache(maxsize=None)
def histograms():
    """[(name, counts as a tuple)].  Fibonacci counts make the deepest Huffman tree there is (depth n - 1); the 47th Fibonacci number
    no longer fits 32 bits, so over 286 symbols the counts are the first 44 (their sum is below 2^31), scattered, and 1 elsewhere:
    depth 50 and more without a limit."""
    rng = np.random.default_rng(15)
    fib286 = [1] * 286
    for i, f in enumerate(fibonacci(44)):
        fib286[(i * 131) % 286] = f
    out = [("fibonacci_22", fibonacci(22)), ("fibonacci_286", fib286), ("all_equal_286", [7] * 286), ("all_equal_19", [3] * 19), ("all_equal_30", [1] * 30),
           ("one_symbol", [0] * 11 + [5] + [0] * 18), ("one_symbol_first", [9] + [0] * 29), ("no_symbol", [0] * 30), ("two_symbols", [0, 4] + [0] * 250 + [1] + [0] * 33),
           ("powers_of_two", [1] + [1 << k for k in range(21)])]
    for i in range(200):
        n = [19, 30, 286, 288, 64, 2, 3][i % 7]
        f = rng.integers(0, 1 << int(rng.integers(1, 21)), n) * (rng.random(n) < rng.uniform(0.2, 1.0))
        out.append(("random_%d" % i, [int(v) for v in f]))
    return [(name, tuple(f)) for name, f in out]


def huffman(freq):
    """(cost, depth) of an unlimited Huffman code for the non-zero counts of freq (two symbols at least, or (sum, 1))"""
    heap = [(f, 0) for f in freq if f]
    if len(heap) < 2:
        return sum(freq), 1
    heapq.heapify(heap)
    cost = 0
    while len(heap) > 1:
        (a, da), (b, db) = heapq.heappop(heap), heapq.heappop(heap)     # (of equal weights the shallower first: the least depth)
        cost += a + b
        heapq.heappush(heap, (a + b, max(da, db) + 1))
    return cost, heap[0][1]


def check_lengths(freq, lens, limit):
    """What every result of the builder must satisfy."""
    freq, lens = list(freq), [int(v) for v in lens]
    used = [s for s, f in enumerate(freq) if f]
    pad = [s for s, f in enumerate(freq) if not f][:max(0, 2 - len(used))]             # the lowest unused symbols join one or none
    for s, (f, l) in enumerate(zip(freq, lens)):
        assert (l != 0) == (f != 0 or s in pad), (s, f, l)
    assert max(lens) <= limit
    assert sum(1 << (15 - l) for l in lens if l) == 1 << 15                            # the Kraft sum is exactly 1
    if pad:
        assert all(lens[s] == 1 for s in used + pad)
        return
    cost, depth = huffman(freq)
    mine = sum(f * l for f, l in zip(freq, lens))
    assert mine >= cost
    if depth <= limit:
        assert mine == cost

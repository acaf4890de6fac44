"""The tabix index of a BGZF VCF, line by line in plain Python (the definition the library's scanners are held to), an independent
reader of .tbi bytes that answers region queries, and the texts the index tests share.  Nothing here calls the index code under test;
the reader inflates with api.bgzf_inflate and frames with api.bgzf_scan, which are older and tested elsewhere."""
import functools
import gzip
import os
import random
import struct

MAX_END = 1 << 29
PSEUDO_BIN = 37450
R_FEW, R_NAN, R_ZERO, R_REF, R_END = "fewer than four fields", "POS is not a number", "POS is 0", "REF is empty", "the end lies beyond 2^29"
R_UNSORTED, R_BLOCKS = "unsorted positions", "chromosome blocks not continuous"


class Refused(Exception):
    def __init__(self, rule, offset):
        super().__init__("%s at %d" % (rule, offset))
        self.rule, self.offset = rule, offset


def lines_of(text):
    """(offset of the line, offset behind it, the line without its newline) for every line; a last line without newline is a line."""
    at, n = 0, len(text)
    while at < n:
        e = text.find(b"\n", at)
        nxt = n if e < 0 else e + 1
        yield at, nxt, text[at:(n if e < 0 else e)]
        at = nxt


def parse_line(line):
    """None for a skipped line, (chrom, beg, end) for a data line, or the rule it breaks as a string."""
    if not line or line[:1] == b"#":
        return None
    f = line.split(b"\t")
    if len(f) < 4:
        return R_FEW
    if not f[1] or any(c not in b"0123456789" for c in f[1]):
        return R_NAN
    pos = int(f[1])
    if pos == 0:
        return R_ZERO
    if not f[3]:
        return R_REF
    if pos - 1 + len(f[3]) > MAX_END:
        return R_END
    return f[0], pos - 1, pos - 1 + len(f[3])


@functools.lru_cache(maxsize=8)
def data_lines(text):
    """[(tid, chrom, beg, end, start offset, end offset)] of a text that can be indexed; raises Refused at the first line that breaks a rule."""
    out, names, last_beg = [], [], {}
    for a, b, ln in lines_of(text):
        p = parse_line(ln)
        if p is None:
            continue
        if isinstance(p, str):
            raise Refused(p, a)
        chrom, beg, end = p
        if not names or names[-1] != chrom:
            if chrom in names:
                raise Refused(R_BLOCKS, a)
            names.append(chrom)
        elif beg < last_beg[chrom]:
            raise Refused(R_UNSORTED, a)
        last_beg[chrom] = beg
        out.append((len(names) - 1, chrom, beg, end, a, b))
    return out


def reg2bin(beg, end):
    end -= 1
    for shift, off in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return off + (beg >> shift)
    return 0


def reg2bins(beg, end):
    end -= 1
    bins = [0]
    for shift, off in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        bins.extend(range(off + (beg >> shift), off + (end >> shift) + 1))
    return bins


def build(text, block, cstart):
    """The raw .tbi bytes of `text` in blocks of `block` text bytes at file offsets cstart[0 .. blocks] (the last one: the marker's)."""
    block = block or 65280
    assert len(cstart) == (len(text) + block - 1) // block + 1, (len(cstart), len(text), block)

    def vo(u):
        return cstart[u // block] << 16 | u % block

    rows = data_lines(text)
    names = []
    for r in rows:
        if len(names) == r[0]:
            names.append(r[1])
    out = [b"TBI\1", struct.pack("<8i", len(names), 2, 1, 2, 0, 35, 0, sum(len(n) + 1 for n in names))] + [n + b"\0" for n in names]
    for tid in range(len(names)):
        mine = [r for r in rows if r[0] == tid]
        bins, prev_bin = {}, None
        for _, _, beg, end, a, b in mine:
            bn = reg2bin(beg, end)
            if bn == prev_bin:
                bins[bn][-1][1] = b
            else:
                bins.setdefault(bn, []).append([a, b])
            prev_bin = bn
        out.append(struct.pack("<i", len(bins) + 1))
        for bn in sorted(bins):
            out.append(struct.pack("<Ii", bn, len(bins[bn])))
            out.extend(struct.pack("<QQ", vo(a), vo(b)) for a, b in bins[bn])
        out.append(struct.pack("<IiQQQQ", PSEUDO_BIN, 2, vo(mine[0][4]), vo(mine[-1][5]), len(mine), 0))
        n_intv = ((max(r[3] for r in mine) - 1) >> 14) + 1
        ioff = [None] * n_intv
        for _, _, beg, end, a, _ in mine:
            for w in range(beg >> 14, ((end - 1) >> 14) + 1):
                if ioff[w] is None:
                    ioff[w] = a
        for w in range(n_intv - 2, -1, -1):
            if ioff[w] is None:
                ioff[w] = ioff[w + 1]
        out.append(struct.pack("<i", n_intv) + b"".join(struct.pack("<Q", vo(u)) for u in ioff))
    out.append(struct.pack("<Q", 0))
    return b"".join(out)


def expected(text, block=0, codes="fixed"):
    """(the BGZF file of the text, its raw index by the definition, or the Refused it raises)."""
    from vargeno_amd import api

    z = api.bgzf_deflate(text, block=block, codes=codes)
    cstart = [b[0] for b in api.bgzf_scan(z)[0]]
    try:
        return z, build(text, block, cstart)
    except Refused as e:
        return z, e


# ---- an independent reader -----------------------------------------------------------------------------------------------------
def parse_tbi(raw):
    assert raw[:4] == b"TBI\1"
    n_ref, fmt, c_seq, c_beg, c_end, meta, skip, l_nm = struct.unpack_from("<8i", raw, 4)
    assert (fmt, c_seq, c_beg, c_end, meta, skip) == (2, 1, 2, 0, 35, 0)
    at = 36
    names = raw[at:at + l_nm].split(b"\0")[:-1] if l_nm else []
    assert len(names) == n_ref
    at += l_nm
    refs = []
    for _ in range(n_ref):
        (n_bin,) = struct.unpack_from("<i", raw, at)
        at += 4
        bins = {}
        for _ in range(n_bin):
            bn, n_chunk = struct.unpack_from("<Ii", raw, at)
            at += 8
            bins[bn] = [struct.unpack_from("<QQ", raw, at + 16 * i) for i in range(n_chunk)]
            at += 16 * n_chunk
        (n_intv,) = struct.unpack_from("<i", raw, at)
        at += 4
        ioff = list(struct.unpack_from("<%dQ" % n_intv, raw, at))
        at += 8 * n_intv
        refs.append((bins, ioff))
    assert struct.unpack_from("<Q", raw, at) == (0,) and at + 8 == len(raw)
    return names, refs


class Reader:
    """Region queries on a BGZF VCF through its .tbi alone: bins, chunks, the linear index's minimum."""

    def __init__(self, bgzf, raw_tbi):
        from vargeno_amd import api

        self.names, self.refs = parse_tbi(raw_tbi)
        blocks = api.bgzf_scan(bgzf)[0]
        self.text = api.bgzf_inflate(bgzf, device=None)[0]
        self.text_at = {b[0]: b[1] for b in blocks}

    def _u(self, v):
        return self.text_at[v >> 16] + (v & 0xffff)

    def query(self, chrom, beg, end):
        """Start offsets (in the text) of the data lines of `chrom` that overlap [beg, end)."""
        if chrom not in self.names:
            return set()
        bins, ioff = self.refs[self.names.index(chrom)]
        min_off = ioff[min(beg >> 14, len(ioff) - 1)] if ioff else 0
        hits = set()
        for bn in reg2bins(beg, end):
            for vs, ve in bins.get(bn, ()):
                if ve <= min_off:
                    continue
                base = self._u(vs)
                for a, _, ln in lines_of(self.text[base:self._u(ve)]):
                    p = parse_line(ln)
                    if p is not None and p[0] == chrom and p[1] < end and p[2] > beg:
                        hits.add(base + a)
        return hits


def brute(text, chrom, beg, end):
    return {r[4] for r in data_lines(text) if r[1] == chrom and r[2] < end and r[3] > beg}


def queries(text, n, seed):
    rows = data_lines(text)
    rng = random.Random(seed)
    chroms = sorted({r[1] for r in rows})
    out = []
    for _ in range(n):
        r = rng.choice(rows)
        kind = rng.randrange(4)
        beg = max(0, r[2] - rng.choice((0, 1, 5, 1 << 14, 1 << 17)))
        end = min(MAX_END, {0: r[3], 1: beg + 1, 2: beg + rng.randrange(1, 1 << 20), 3: MAX_END}[kind])
        out.append((rng.choice(chroms) if kind == 3 else r[1], min(beg, end - 1), end))
    return out


# ---- texts ---------------------------------------------------------------------------------------------------------------------
HEADER = b"##fileformat=VCFv4.2\n##source=tbi_cases\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"


def synthetic(n_lines=9000, seed=20261020, long_refs=True, header_every=1500):
    """Three chromosomes, positions up to 2^29 that cluster round 2^14 and 2^26, REF of 1 to 20 000 bases, '#' lines mid-file."""
    rng = random.Random(seed)
    out = [HEADER]
    left = n_lines
    for ci, chrom in enumerate((b"chr1", b"chrUn_KI270742v1", b"7")):
        k = left if ci == 2 else n_lines // 3
        left -= k
        pos = []
        for _ in range(k):
            c = rng.random()
            centre = (1 << 14) if c < 0.3 else (1 << 26) if c < 0.6 else None
            pos.append(rng.randrange(1, MAX_END) if centre is None else max(1, centre + rng.randrange(-300, 300)))
        pos.sort()
        for i, p in enumerate(pos):
            ref_len = rng.randrange(1, 20001) if long_refs and rng.random() < 0.004 else rng.choice((1, 1, 1, 2, 3, 40))
            ref_len = min(ref_len, MAX_END - (p - 1))
            out.append(b"%s\t%d\trs%d\t%s\t%s\t.\tPASS\tAF=0.5\n" % (chrom, p, i, bytes(rng.choice(b"ACGT") for _ in range(ref_len)), rng.choice((b"A", b"C", b"G,T"))))
            if (i + 1) % header_every == 0:
                out.append(HEADER)
    return b"".join(out)


def small():
    return synthetic(n_lines=300, seed=7, long_refs=False, header_every=50)


def variants():
    """name -> text: the synthetic text and the edge cases of the definition."""
    s = small()
    v = {"synthetic": synthetic(), "small": s}
    v["no trailing newline"] = s[:-1]
    v["empty lines"] = s.replace(b"\nchr1\t", b"\n\nchr1\t", 40) + b"\n\n"
    long_chrom = b"c" * 300
    v["300-byte CHROM"] = HEADER + b"".join(b"%s\t%d\t.\tA\tC\n" % (long_chrom, p) for p in (5, 9, 16385)) + b"".join(b"%s\t%d\t.\tA\tC\n" % (long_chrom[:299] + b"d", p) for p in (1, 2))
    v["70 000-base REF"] = HEADER + b"x\t10\t.\tA\tC\n" + b"x\t100\t.\t" + b"ACGT" * 17500 + b"\t<DEL>\n" + b"x\t101\t.\tG\tC\nx\t70200\t.\tG\tC\n"
    v["end = 2^29"] = HEADER + b"x\t%d\t.\tACGT\tA\nx\t%d\t.\tA\tC\n" % (MAX_END - 3, MAX_END)
    v["headers only"] = HEADER
    v["empty"] = b""
    v["one line without newline"] = b"x\t5\t.\tA\tC"
    return v


def refused():
    """name -> text that cannot be indexed (hand-made lines behind a few good ones)."""
    good = HEADER + b"x\t5\t.\tA\tC\nx\t9\t.\tAC\tC\n"
    bad = {"POS 0": b"x\t0\t.\tA\tC\n", "POS 12x": b"x\t12x\t.\tA\tC\n", "POS 2^29 + 1": b"x\t%d\t.\tA\tC\n" % (MAX_END + 1), "three fields": b"x\t12\t.\n",
           "empty REF": b"x\t12\t.\t\tC\n", "empty POS": b"x\t\t.\tA\tC\n", "end one beyond": b"x\t%d\t.\tAC\tC\n" % MAX_END, "unsorted": b"x\t8\t.\tA\tC\n",
           "comes back": b"y\t1\t.\tA\tC\nx\t100\t.\tA\tC\n", "huge POS": b"x\t99999999999999999999999\t.\tA\tC\n"}
    return {k: good + v + b"x\t20\t.\tA\tC\n" for k, v in bad.items()}


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN_GOOD = ("fdense.out", "flowcomplex.out", "fsmall.out", "fstrands.out", "ftiny.out")
GOLDEN_REFUSED = ("fquirk.out", "frepeated.out", "ftiny.out.fmtcols")


def golden(name):
    with gzip.open(os.path.join(GOLDEN, name + ".vcf.gz"), "rb") as f:
        return f.read()


def cuts(n, how, seed=1):
    """Cut points of a streaming feed of n bytes: "whole", "bytes", "7", "random"."""
    if how == "whole" or n < 2:
        return []
    if how == "bytes":
        return list(range(1, n))
    if how == "7":
        return list(range(7, n, 7))
    rng = random.Random(seed)
    return sorted(set(rng.randrange(1, n) for _ in range(min(n - 1, 40))))

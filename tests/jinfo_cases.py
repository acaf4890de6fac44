"""The INFO mode of the joint VCF's data lines (NS / AN / AC / AF; vargeno_amd/csrc/vg_jtext.h) restated in plain Python: the
yardstick of the CPU and the GPU suite.  It takes the cell text from tests/jtext_cases.py and knows nothing of the code under test;
AF is a `decimal` division rounded ROUND_HALF_UP, not the integer expression of the header.  Its cases are those of jtext_cases
with real heads: eight fields with an INFO of ".", of nothing and of ordinary text, and heads of 0 to 6 tabs."""
import re
from decimal import ROUND_HALF_UP, Decimal

import numpy as np

import jtext_cases as JC

MISSING = "\t./.:."
INFO_DECL = [b'##INFO=<ID=NS,Number=1,Type=Integer,', b'##INFO=<ID=AN,Number=1,Type=Integer,', b'##INFO=<ID=AC,Number=A,Type=Integer,', b'##INFO=<ID=AF,Number=A,Type=Float,']
TAG_RE = re.compile(rb"(^|;)NS=(\d+);AN=(\d+);AC=(\d+);AF=([0-9.]+)$")


def af_text(ac, an):
    q = (Decimal(ac) / Decimal(an)).quantize(Decimal("0.000001"), rounding=ROUND_HALF_UP)
    t = format(q, "f")
    return t.rstrip("0").rstrip(".") if "." in t else t


def tag(ns, het, hom):
    an, ac = 2 * ns, het + 2 * hom
    return ("NS=%d;AN=%d;AC=%d;AF=%s" % (ns, an, ac, af_text(ac, an))).encode()


def splice(head, t):
    """The head with the tag in its INFO: eight fields (seven tabs) or the head as it is."""
    fields = head.split(b"\t")
    if len(fields) != 8:
        return head
    info = fields[7]
    fields[7] = t if info in (b".", b"") else info + b";" + t
    return b"\t".join(fields)


def shown(gt, sites, site_at, n):
    """Per sample the site of the run whose call the line shows (the last called one), or None."""
    out = []
    for g in gt:
        hit = [int(s) for s in sites[site_at:site_at + n] if g is not None and g[s]]
        out.append(hit[-1] if hit else None)
    return out


def counts_span(gt, records, sites):
    """[n_records, 3]: NS, het, hom over the shown calls; zeros for a record no sample has called."""
    out = np.zeros((len(records), 3), np.uint32)
    for i, (_, _, site_at, n) in enumerate(records):
        calls = [int(g[s]) for g, s in zip(gt, shown(gt, sites, site_at, n)) if s is not None]
        out[i] = (len(calls), calls.count(3), calls.count(2))
    return out


def format_span(gt, gq, heads, records, sites):
    out = []
    for (head_off, head_len, site_at, n), (ns, het, hom) in zip(records, counts_span(gt, records, sites)):
        if not ns:
            continue
        cells = [MISSING if s is None else "\t%s:%d" % (JC.GT_TEXT[int(g[s])], int(q[s])) for g, q, s in zip(gt, gq, shown(gt, sites, site_at, n))]
        out.append(splice(bytes(heads[head_off:head_off + head_len]), tag(int(ns), int(het), int(hom))) + b"\tGT:GQ" + "".join(cells).encode() + b"\n")
    return b"".join(out)


def expected(case, lo=0, hi=None):
    return format_span(case["gt"], case["gq"], case["heads"], case["records"][lo:hi], case["sites"])


def expected_counts(case, lo=0, hi=None):
    return counts_span(case["gt"], case["records"][lo:hi], case["sites"])


def head_of(i, rng, length=None):
    """Record i's head: by turns an INFO of ".", an ordinary one, an empty one, and -- every seventh -- a head of 0 .. 6 tabs.
    length: exactly so many bytes (the ID is padded)."""
    kind = i % 7
    if kind == 6:
        fields = ["c%d" % i, "%d" % (i + 1), "id", "A", "C", ".", "."][:(i // 7) % 7 + 1]              # 0 .. 6 tabs: no eighth field
    else:
        info = [".", "RS=%d;VC=SNV" % i, "", ".", "DP=%d" % int(rng.integers(0, 1000)), "X"][kind]
        fields = ["%d" % (1 + i % 22), "%d" % (100 + i), "rs%d" % i, "ACGT"[i % 4], "TGCA"[i % 4], ".", "PASS" if i % 2 else ".", info]
    if length is not None:
        fields[2 if len(fields) > 2 else 0] += "x" * (length - len("\t".join(fields)))
    head = "\t".join(fields).encode()
    assert length is None or len(head) == length
    return head


def with_heads(case, first=None, seed=0):
    """The case with real heads in place of the random bytes (junk between them, offsets not aligned).  first: record 0's head."""
    rng = np.random.default_rng(seed)
    heads, records = bytearray(b"\x01"), []
    for i, (_, hl, site_at, n) in enumerate(case["records"]):
        h = first if (i == 0 and first is not None) else head_of(i, rng, 70_000 if hl == 70_000 else None)
        heads += bytes(rng.integers(33, 127, size=int(rng.integers(0, 4)), dtype=np.uint8))
        records.append((len(heads), len(h), site_at, n))
        heads += h
    return dict(case, heads=bytes(heads), records=records)


def make_case(n_samples, n_records, seed, **kw):
    """jtext_cases.make_case -- site runs of 1 .. 5 sites, every call drawn on its own, unset samples, dropped records, a 70 000-byte
    head -- with the heads of head_of."""
    return with_heads(JC.make_case(n_samples, n_records, seed, **kw), seed=seed)


def strip_info(text):
    """The inverse over a whole VCF: the four declarations go, and every data line's INFO loses the tag (an INFO that was the tag
    alone becomes "."; the lists it is used on have no empty INFO).  Returns (the text without, [(line, NS, AN, AC, AF)])."""
    out, found = [], []
    for ln in text.split(b"\n"):
        if ln.startswith(b"##INFO=<ID=") and any(ln.startswith(d) for d in INFO_DECL):
            continue
        f = ln.split(b"\t")
        if ln[:1] != b"#" and len(f) > 8:
            m = TAG_RE.search(f[7])
            if m:
                found.append((ln, int(m.group(2)), int(m.group(3)), int(m.group(4)), m.group(5)))
                f[7] = f[7][:m.start()] or b"."
                ln = b"\t".join(f)
        out.append(ln)
    return b"\n".join(out), found


def cells_counts(line):
    """NS, AN, AC from a data line's own cells."""
    gts = [c.split(b":")[0] for c in line.rstrip(b"\r").split(b"\t")[9:]]
    ns = sum(g != b"./." for g in gts)
    return ns, 2 * ns, sum(g.count(b"1") for g in gts if g != b"./.")

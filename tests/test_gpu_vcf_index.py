"""The tabix index on the device: the scan kernels behind api.vcf_index(device=0) against the host scanner and the line-by-line
definition of tests/tbi_cases.py, the fused deflate call, and the joint text stream with an index attached.  Exact bytes throughout."""
import numpy as np
import pytest

import jtext_cases as JC
import tbi_cases as T
from vargeno_amd import api

pytestmark = pytest.mark.gpu


def _index(text, **kw):
    """The raw index, or (rule, offset) of the refusal."""
    try:
        return api.vcf_index(text, **kw)
    except api.VcfIndexRefused as e:
        return e.rule, e.offset


def _want(text, block=0):
    w = T.expected(text, block)[1]
    return (w.rule, w.offset) if isinstance(w, T.Refused) else w


@pytest.fixture(scope="module")
def texts():
    t = dict(T.variants())
    t.update(T.refused())
    for g in T.GOLDEN_GOOD + T.GOLDEN_REFUSED:
        t[g] = T.golden(g)
    return t


NAMES = sorted(list(T.variants()) + list(T.refused()) + list(T.GOLDEN_GOOD + T.GOLDEN_REFUSED))


@pytest.mark.parametrize("name", NAMES)
def test_device_scan_is_the_host_scan_and_the_definition(texts, name):
    """Every text of the CPU suite, refusals included (same rule, same offset): fed whole and at seeded random cuts."""
    text = texts[name]
    want = _want(text)
    assert _index(text) == want
    assert _index(text, device=0) == want
    assert _index(text, device=0, pieces=T.cuts(len(text), "random", seed=5)) == want
    if name in ("synthetic", "small", "fquirk.out"):
        assert _index(text, device=0, block=97) == _want(text, 97)


def _lines(n, pad=0):
    return b"".join(b"c\t%d\t.\tA%s\tC\n" % (i + 1, b"C" * pad) for i in range(n))


@pytest.mark.parametrize("at", [63, 64, 65])
def test_a_newline_at_the_edge_of_a_wave_step(at):
    """A first line whose '\\n' is byte 63, 64 or 65 of the piece, and the same with the piece cut there."""
    first = b"c\t1\t.\t"
    first += b"A" * (at - len(first)) + b"\n"
    text = first + _lines(300)[len(b"c\t1\t.\tA\tC\n"):]
    assert text[at:at + 1] == b"\n" and text.count(b"\n", 0, at) == 0
    want = _want(text)
    assert not isinstance(want, tuple)
    assert _index(text, device=0) == want
    assert _index(text, device=0, pieces=[at, at + 1, 1000, 1001]) == want


def test_a_line_longer_than_every_tile_among_short_ones():
    text = T.HEADER + _lines(50) + b"c\t60\t.\t" + b"ACGT" * 17500 + b"\tA\n" + b"c\t61\t.\tA\tC\n" * 3 + T.HEADER + b"d\t5\t.\tG\tC\n"
    assert _index(text, device=0) == _want(text)


def test_more_lines_than_one_scan_block_and_one_level_of_sums():
    """70 000 short lines: 18 scan blocks of 4 096 lines, and 300 tiles of newline counts; positions cross many 16 kb windows."""
    text = b"".join(b"c\t%d\t.\tA\tC\n" % (1 + 7 * i) for i in range(70000))
    want = _want(text)
    assert _index(text, device=0) == want
    assert _index(text, device=0, block=97, pieces=[len(text) // 3]) == _want(text, 97)


def test_pieces_of_one_byte():
    text = T.variants()["300-byte CHROM"]
    assert _index(text, device=0, pieces=T.cuts(len(text), "bytes")) == _want(text)


def test_no_device_number_is_an_error_not_a_fallback():
    with pytest.raises(api._lib.VgError):
        api.vcf_index(_lines(3), device=4096)


@pytest.fixture(scope="module")
def fused_text():
    """1.1 MiB, sorted, three chromosomes: at block 16 the deflate chunk is 65 536 blocks = 1 MiB, so a line straddles the chunks."""
    rows, at = [], 0
    for chrom in (b"chr1", b"chr2", b"chrX"):
        for i in range(14000):
            rows.append(b"%s\t%d\trs%d\t%s\tT\t.\t.\t.\n" % (chrom, 1 + 37 * i, i, b"ACG"[: 1 + i % 3]))
    text = T.HEADER + b"".join(rows)
    assert 1.05 * 2 ** 20 < len(text) < 1.3 * 2 ** 20 and text[2 ** 20 - 1:2 ** 20] != b"\n"
    return text


@pytest.mark.parametrize("codes", ["fixed", "dynamic"])
def test_the_fused_deflate_call(fused_text, codes):
    z, want = T.expected(fused_text, 16, codes)
    bgzf, tbi = api.bgzf_deflate(fused_text, device=0, block=16, codes=codes, index=True)
    assert bgzf == z
    assert tbi == want
    rd = T.Reader(bgzf, tbi)
    for chrom, beg, end in T.queries(fused_text, 40, seed=3):
        assert rd.query(chrom, beg, end) == T.brute(fused_text, chrom, beg, end), (chrom, beg, end)


def test_the_fused_call_reports_a_refusal():
    text = T.refused()["unsorted"]
    with pytest.raises(api.VcfIndexRefused) as e:
        api.bgzf_deflate(text, device=0, index=True)
    assert (e.value.rule, e.value.offset) == _want(text)


# ---- the joint text stream --------------------------------------------------------------------------------------------------------
def _joint_case(n_records=700, n_samples=3, seed=9):
    """A plan whose heads are the first eight fields of sorted VCF lines on two chromosomes; every seventh record has no call."""
    rng = np.random.default_rng(seed)
    heads, records = bytearray(), []
    for i in range(n_records):
        h = b"%s\t%d\trs%d\t%s\tG\t.\tPASS\tAF=0.1" % (b"chr1" if i < n_records // 2 else b"chr2", 100 + 53 * (i % (n_records // 2)), i, b"A" * (1 + i % 4))
        records.append((len(heads), len(h), i, 1))
        heads += h
    gt = [rng.choice(np.array([0, 1, 2, 3], np.uint8), size=n_records) for _ in range(n_samples)]
    for g in gt:
        g[::7] = 0
    gq = [rng.integers(0, 100, size=n_records).astype(np.int32) for _ in range(n_samples)]
    return dict(gt=gt, gq=gq, heads=bytes(heads), records=records, sites=np.arange(n_records, dtype=np.uint32), n_sites=n_records, n_samples=n_samples)


@pytest.mark.parametrize("block", [0, 97])
def test_the_joint_stream_with_an_index_attached(block):
    c = _joint_case()
    header = [b"##fileformat=VCFv4.2\n", b"##source=stream\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ta\tb\tc\n"]
    spans = [(0, 260), (260, 700)]
    whole = b"".join(header) + b"".join(JC.expected(c, lo, hi) for lo, hi in spans)
    assert 400 < JC.expected(c).count(b"\n") <= 600                                   # (some records produce no line)
    with api.JointText(c["n_sites"], c["n_samples"], max_records=700, max_head_bytes=len(c["heads"]), max_site_refs=700, bgzf=True) as jt:
        for s, (g, q) in enumerate(zip(c["gt"], c["gq"])):
            jt.set(s, g, q)
        jt.bgzf_begin(block=block)
        jt.bgzf_index()
        parts = [jt.bgzf_text(h) for h in header]                               # header text in pieces (at block 0: less than a block stays pending)
        parts += [jt.bgzf_lines(c["heads"], c["records"][lo:hi], c["sites"]) for lo, hi in spans]
        end, tbi = jt.bgzf_end()
    bgzf = b"".join(parts) + end
    z, want = T.expected(whole, block)
    assert bgzf == z
    assert api.bgzf_inflate(bgzf, device=None)[0] == whole
    assert tbi == want
    assert T.parse_tbi(tbi)[0] == [b"chr1", b"chr2"]

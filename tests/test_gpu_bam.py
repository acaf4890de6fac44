"""BAM records framed on the device (vg_bam_* kernels): the flat batch layout of vg_bam_frame_device against the layout computed from
the equivalent FASTQ text, and the stream (vg_fastq_stream_begin_bam) against the oracle, the text stream and a second sample
plane fed the text.  Inputs and the independent converter: tests/bam_cases.py."""
import os

import numpy as np
import pytest

import bam_cases as B
from oracle import oracle as O
from vargeno_amd import api
from vargeno_amd._lib import VgError
from vargeno_amd.api import GenoIndex

pytestmark = pytest.mark.gpu

EVENTS = ("reads", "reads_n", "reads_invalid", "passes", "chunks", "gate_open", "ctx", "walks", "incr")
CASES = {"ftiny": B.ftiny_bam, "corner": B.corner_bam}


def _check_frame(data, raw, aligned=False):
    text, reads, n_flag, n_empty = B.to_fastq(raw)
    want_off, want_bases, want_gate = B.expected_batch(reads)
    off, bases, gate, stats, bad = api.bam_frame(data)
    print("records %d, skipped %d + %d, repairs %d" % stats)
    assert bad is None
    assert np.array_equal(off, want_off)
    assert np.array_equal(bases, want_bases)
    assert np.array_equal(gate, want_gate)
    assert stats[:3] == (len(reads), n_flag, n_empty)
    if aligned:
        assert stats[3] == 0
    return stats


@pytest.mark.parametrize("style", B.STYLES)
@pytest.mark.parametrize("case", sorted(CASES))
def test_frame_equals_the_batch_of_the_equivalent_text(case, style):
    data, raw = CASES[case](style)
    _check_frame(data, raw, aligned=style == "aligned")


def test_a_wrong_speculation_is_repaired():
    """Aux arrays that hold three well-formed fake records right behind a window boundary: the window's guess is the fakes, its
    predecessor's exit says otherwise, and the repaired result is exact."""
    data, raw, hits = B.decoy_bam()
    stats = _check_frame(data, raw)
    assert stats[3] >= 1


def test_frame_reports_where_framing_stopped():
    dm = B.damaged()
    data, cut_raw = dm["cut_mid_record"]
    raw = B.ftiny_bam("spanning")[1]
    _, reads, _, _ = B.to_fastq(raw)
    last_start = B.boundary_before(raw, len(cut_raw))             # the record the file ends inside
    assert last_start < len(cut_raw)
    off, bases, gate, stats, bad = api.bam_frame(data)
    assert bad == last_start and len(gate) == sum(1 for r in reads if r[0] < last_start)
    data, at = dm["block_size_7"]
    off, bases, gate, stats, bad = api.bam_frame(data)
    assert bad is not None and bad <= at and len(gate) == 0       # one slot: the refused chunk is the whole file
    with pytest.raises(VgError) as e:
        api.bam_frame(dm["cram"][0])
    assert e.value.code == -2 and "CRAM" in str(e.value) and "samtools fastq" in str(e.value)


def _flat_arrays(reads):
    off, bases, _ = B.expected_batch(reads)
    quals = np.frombuffer("".join(q for _, _, q in reads).encode(), dtype=np.uint8)
    return bases, quals, off


def _want(prefix, raw):
    """What the equivalent reads of a BAM must count: by the oracle, and by a plain text stream of the equivalent text (with its
    event counts).  The two must agree before anything is held against them."""
    text, reads, _, _ = B.to_fastq(raw)
    bases, quals, off = _flat_arrays(reads)
    ox = O.OracleIndex.load(prefix)
    ox.process(bases, quals, off)
    so = ox.sites()
    with GenoIndex.open(prefix) as gx:
        n, used, last, refused = gx.fastq_stream([text])
        assert (n, used, refused) == (len(reads), len(text), False)
        counts, st = gx.counts(), gx.stats()
    assert np.array_equal(counts[0], so["ref_cnt"]) and np.array_equal(counts[1], so["alt_cnt"])
    return text, reads, (so["ref_cnt"], so["alt_cnt"]), counts, st


@pytest.fixture(scope="module")
def ftiny_want(ftiny_dir):
    return _want(os.path.join(ftiny_dir, "idx"), B.ftiny_bam("spanning")[1])


@pytest.fixture(scope="module")
def corner_want(ftiny_dir):
    return _want(os.path.join(ftiny_dir, "idx"), B.corner_bam("spanning")[1])


@pytest.mark.parametrize("style", ["spanning", "ragged"])
def test_stream_of_ftiny_cut_at_random_points(ftiny_dir, ftiny_want, style, monkeypatch):
    text, reads, (rco, aco), (rc0, ac0), st0 = ftiny_want
    data, raw = B.ftiny_bam(style)
    monkeypatch.setenv("VG_BGZF_SLOT_TEXT", "200000")             # many slots: records are carried from slot to slot on the device
    rng = np.random.default_rng(9)
    cuts = sorted(set([0, len(data)] + [int(v) for v in rng.integers(0, len(data), 40)]))
    with GenoIndex.open(os.path.join(ftiny_dir, "idx")) as gx:
        gx.reserve_samples(2)
        n, used, last, refused = gx.fastq_stream((data[a:b] for a, b in zip(cuts[:-1], cuts[1:])), bam=True)
        assert (n, used, last, refused) == (len(reads), len(raw), reads[-1][0], False)
        kept, n_flag, n_empty, repairs = gx.bam_stats()
        print("repairs", repairs)
        assert (kept, n_flag, n_empty) == (len(reads), 200, 0)
        st = gx.stats()
        gx.select(1)
        gx.fastq_stream([text])                                    # the second plane: the equivalent text
        rc, ac = gx.counts(sample=0)
        rc1, ac1 = gx.counts(sample=1)
        block, within = gx.bgzf_locate(last)
        assert api.bgzf_inflate(data[block:], device=None)[0][within:within + 36] == raw[last:last + 36]
    assert np.array_equal(rc, rco) and np.array_equal(ac, aco)     # the oracle's
    assert np.array_equal(rc, rc0) and np.array_equal(ac, ac0)     # the plain text stream's
    assert np.array_equal(rc, rc1) and np.array_equal(ac, ac1)
    for k in EVENTS:
        assert st[k] == st0[k], k


@pytest.mark.parametrize("style", ["spanning", "ragged"])
def test_stream_of_the_corner_set_one_byte_at_a_time(ftiny_dir, corner_want, style):
    text, reads, (rco, aco), (rc0, ac0), st0 = corner_want
    data, raw = B.corner_bam(style)
    assert raw == B.corner_bam("spanning")[1]                     # the styles differ in their blocks only
    n_flag, n_empty = B.to_fastq(raw)[2:]
    with GenoIndex.open(os.path.join(ftiny_dir, "idx")) as gx:
        gx.reserve_samples(2)
        n, used, last, refused = gx.fastq_stream((data[i:i + 1] for i in range(len(data))), bam=True)
        assert (n, used, last, refused) == (len(reads), len(raw), reads[-1][0], False)
        assert gx.bam_stats()[:3] == (len(reads), n_flag, n_empty)
        st = gx.stats()
        gx.select(1)
        gx.fastq_stream([text])                                    # the second plane: the equivalent text
        rc, ac = gx.counts(sample=0)
        rc1, ac1 = gx.counts(sample=1)
    assert np.array_equal(rc, rco) and np.array_equal(ac, aco)     # the oracle's
    assert np.array_equal(rc, rc0) and np.array_equal(ac, ac0)     # the plain text stream's
    assert np.array_equal(rc, rc1) and np.array_equal(ac, ac1)
    for k in EVENTS:
        assert st[k] == st0[k], k


def test_stream_errors_name_the_inflated_offset(ftiny_dir):
    dm = B.damaged()
    with GenoIndex.open(os.path.join(ftiny_dir, "idx")) as gx:
        data, cut_raw = dm["cut_mid_record"]
        last_start = B.boundary_before(B.ftiny_bam("spanning")[1], len(cut_raw))
        with pytest.raises(VgError) as e:
            gx.fastq_stream([data], bam=True)
        assert e.value.code == -2 and "inside a record" in str(e.value) and "offset %d" % last_start in str(e.value)
        data, cut_raw = dm["cut_mid_header"]
        with pytest.raises(VgError) as e:
            gx.fastq_stream([data], bam=True)
        assert e.value.code == -2 and "header" in str(e.value) and "offset %d" % len(cut_raw) in str(e.value)
        data, at = dm["flipped_bit_block_9"]
        with pytest.raises(VgError) as e:
            gx.fastq_stream([data], bam=True)
        assert e.value.code == -2 and "offset %d" % at in str(e.value)
        with pytest.raises(VgError) as e:                           # BGZF that is not BAM: the push says so
            gx.fastq_stream([B.BC.ftiny_variants()["level6"]], bam=True)
        assert e.value.code == -2 and "BAM" in str(e.value)
        # a block_size of 7 refuses its chunk: nothing of it is framed, the host converts from `consumed`
        data, at = dm["block_size_7"]
        gx.reset()
        n, used, last, refused = gx.fastq_stream([data], bam=True)
        assert refused and n == 0 and used <= at
        # the handle is usable
        data, raw = B.ftiny_bam("aligned")
        n, used, last, refused = gx.fastq_stream([data], bam=True)
        assert (n, used, refused) == (4000, len(raw), False)

"""BGZF inflated on the device (vg_bgzf_inflate_kernel): every inflated byte through vg_bgzf_inflate_device, the error path of a
hostile file, and the stream (vg_fastq_stream_begin_bgzf) against the text stream and the flat-batch path.  The inputs are those
of tests/test_bgzf_cpu.py (tests/bgzf_cases.py); expected text is what they were made from."""
import os

import numpy as np
import pytest

import bgzf_cases as BC
from vargeno_amd import api
from vargeno_amd._lib import VgError
from vargeno_amd.api import GenoIndex

pytestmark = pytest.mark.gpu

VALID = BC.valid_cases()
DAMAGED = BC.damaged_cases()
EVENTS = ("reads", "reads_n", "passes", "chunks", "gate_open", "ctx", "walks", "incr")


@pytest.mark.parametrize("case", range(len(VALID)), ids=[c[0] for c in VALID])
def test_device_inflate_is_byte_exact(case):
    _, data, text = VALID[case]
    got, consumed, bad = api.bgzf_inflate(data, device=0)
    assert bad is None and consumed == len(data)
    assert got == text


@pytest.mark.parametrize("base", sorted(DAMAGED))
def test_damaged_blocks_are_reported_not_decoded(base):
    """The error path of a hostile file: one launch per base block, with every damaged form of it between valid blocks.  The call
    returns normally; the block reported is the first that has to fail -- by Python's zlib, block by block (a form zlib accepts
    with the same CRC and length may decode; the decoder may refuse a form zlib tolerates, never the other way round), and it is
    the block the host build of the same source reports (tests/test_bgzf_cpu.py pins that build to zlib for every form alone).
    The text before it is exact, nothing is written behind text_cap, and a valid call on the same device afterwards is exact."""
    good = BC.split_blocks(VALID[3][1])[0][1]
    good_text = VALID[3][2][:65280]
    data, want, starts, must_fail = b"", [], [], None
    for name, block, verdict in DAMAGED[base]:
        data += good
        starts.append(len(data))
        if verdict is None and must_fail is None:
            must_fail = len(data)
        want.append((len(data), good_text, verdict))
        data += block
    assert must_fail is not None
    cap = sum(b[4] for b in api.bgzf_scan(data)[0])
    buf = np.full(cap + 4096, 0xA5, dtype=np.uint8)
    text, consumed, bad = api.bgzf_inflate(data, device=0, out=buf, text_cap=cap)
    assert (buf[cap:] == 0xA5).all()
    assert bad in starts and bad <= must_fail and consumed == bad
    assert text == b"".join(g + (v if at < bad else b"") for at, g, v in want if at <= bad)
    assert bad == api.bgzf_inflate(data, device=None)[2]
    got, consumed, bad = api.bgzf_inflate(VALID[3][1], device=0)
    assert bad is None and got == VALID[3][2]


def _cuts(n, rng, steps=(1, 2, 7, 311, 4096, 65_537, 300_000)):
    cuts = [0]
    while cuts[-1] < n:
        cuts.append(min(n, cuts[-1] + int(rng.choice(steps))))
        if len(cuts) > 400:                                       # keep the tiny steps to the head of the file
            cuts.append(n)
    return cuts


@pytest.fixture(scope="module")
def flat(ftiny_dir, ftiny_reads):
    """The flat-batch path's counters and event counts, and the text stream's last_record_start, computed once."""
    prefix = os.path.join(ftiny_dir, "idx")
    with GenoIndex.open(prefix) as gx:
        gx.submit(ftiny_reads.bases, ftiny_reads.quals, ftiny_reads.offsets)
        counts, st = gx.counts(), gx.stats()
    with GenoIndex.open(prefix) as gx:
        n, used, last, refused = gx.fastq_stream([BC.ftiny_text()])
    assert (n, used, refused) == (ftiny_reads.n, len(BC.ftiny_text()), False)
    return counts, st, last


@pytest.mark.parametrize("trial", [0, 1])
@pytest.mark.parametrize("variant", ["stored", "level6", "block_sizes"])
def test_bgzf_stream_equals_text_stream(ftiny_dir, flat, variant, trial, monkeypatch):
    (rc0, ac0), st0, last0 = flat
    text = BC.ftiny_text()
    data = BC.ftiny_variants()[variant]
    cuts = _cuts(len(data), np.random.default_rng(3 + trial))
    if trial == 1:
        monkeypatch.setenv("VG_BGZF_SLOT_TEXT", "200000")        # a push of more text than a slot takes is split at block boundaries
        cuts = [0, 17, len(data) - 5, len(data)]
    with GenoIndex.open(os.path.join(ftiny_dir, "idx")) as gx:
        n, used, last, refused = gx.fastq_stream((data[a:b] for a, b in zip(cuts[:-1], cuts[1:])), bgzf=True)
        assert (n, used, refused) == (4000, len(text), False)
        assert last == last0
        rc, ac = gx.counts()
        st = gx.stats()
    assert np.array_equal(rc, rc0) and np.array_equal(ac, ac0)
    for k in EVENTS:
        assert st[k] == st0[k], k


def test_a_damaged_block_in_the_second_push_ends_the_stream_there(ftiny_dir):
    text = BC.ftiny_text()
    data = BC.ftiny_variants()["level6"]
    blocks = BC.split_blocks(data)
    cut = blocks[6][0]                                            # first push: six whole blocks
    at = blocks[9][0]                                             # the damaged block, in the second push
    hurt = bytearray(data)
    hurt[at + 18 + 40] ^= 0x04                                    # a payload bit
    first_text = text[:6 * 65280]
    first_records = first_text.count(b"\n") // 4
    with GenoIndex.open(os.path.join(ftiny_dir, "idx")) as gx:
        with pytest.raises(VgError) as e:
            gx.fastq_stream([bytes(hurt[:cut]), bytes(hurt[cut:])], bgzf=True)
        assert e.value.code == -2 and "offset %d" % at in str(e.value), str(e.value)
        assert gx.stats()["reads"] == first_records               # nothing of the second push was framed
        # an incomplete block left at the end is an error too, naming where it starts
        gx.reset()
        with pytest.raises(VgError) as e:
            gx.fastq_stream([data[:at + 100]], bgzf=True)
        assert e.value.code == -2 and "offset %d" % at in str(e.value) and "incomplete" in str(e.value)
        # bytes that are no block header: the push itself says so
        gx.reset()
        with pytest.raises(VgError) as e:
            gx.fastq_stream([data[:at] + b"@r1\nACGT\n"], bgzf=True)
        assert e.value.code == -2 and "offset %d" % at in str(e.value)
        # the handle is usable: a text stream, then a BGZF stream
        before = gx.stats()["reads"]
        n, used, last, refused = gx.fastq_stream([text])           # (begins anew: the failed push had left its stream open)
        assert (n, used, refused) == (4000, len(text), False)
        n, used, last, refused = gx.fastq_stream([data], bgzf=True)
        assert (n, used, refused) == (4000, len(text), False)
        assert gx.stats()["reads"] == before + 8000


def test_locate_maps_text_offsets_to_blocks(ftiny_dir, flat):
    text = BC.ftiny_text()
    data = BC.ftiny_variants()["block_sizes"]
    rng = np.random.default_rng(21)
    with GenoIndex.open(os.path.join(ftiny_dir, "idx")) as gx:
        n, used, last, refused = gx.fastq_stream([data[:300_001], data[300_001:]], bgzf=True)
        assert last == flat[2]
        for off in [last, 0, len(text) - 1, len(text)] + [int(v) for v in rng.integers(0, len(text), 20)]:
            block, within = gx.bgzf_locate(off)
            got, _, bad = api.bgzf_inflate(data[block:], device=None)
            assert bad is None and got[within:] == text[off:], off
        with pytest.raises(VgError):
            gx.bgzf_locate(len(text) + 1)


def test_a_bgzf_stream_counts_into_the_sample_selected_at_its_begin(ftiny_dir, flat):
    (rc0, ac0), _, _ = flat
    data = BC.ftiny_variants()["level6"]
    with GenoIndex.open(os.path.join(ftiny_dir, "idx")) as gx:
        gx.reserve_samples(2)
        gx.select(1)
        gx.fastq_stream([data[:123_457], data[123_457:]], bgzf=True)
        rc1, ac1 = gx.counts(sample=1)
        rcz, acz = gx.counts(sample=0)
    assert np.array_equal(rc1, rc0) and np.array_equal(ac1, ac0)
    assert not rcz.any() and not acz.any()

"""The pack kernel of batch k+1 beside the wave kernel of batch k.  A large batch's pack kernel goes onto the ingest stream with
a grid of one workgroup per CU when the main stream is busy, and in front of its wave kernel on the main stream when it is not;
VG_PACK_OVERLAP=0 / 1 force either.  Batch k+1 is then packed -- and its slot's counters are reset -- while batch k's tiers read
their own slot: a counter that was not zero when its batch started, or a packed read that was not complete when the wave kernel
started, would show in the handle's sums (reads spilled to the deep tier, reads left for the lane machine, reads with a foreign
byte) and in the site counters.  Everything here goes through the C-ABI and is compared with the oracle.  The fixtures' batches
are small, so VG_PACK_SMALL_READS=0 sends them down the large batches' path, and VG_PACK_CORUN_WGS gives that path grids of one
and of three workgroups: every wave of the pack kernel then walks many tiles."""
import os
import subprocess

import numpy as np
import pytest

from conftest import BIN
from oracle import oracle as O
from vargeno_amd.api import GenoIndex, gate_words

pytestmark = pytest.mark.gpu

CMP_STATS = ["reads", "reads_n", "reads_invalid", "passes", "passes_ok", "chunks", "gate_open", "refbf_pos", "snpbf_pos",
             "large_block", "ref_query", "snp_query", "ref_probe", "snp_probe", "scan_ref", "scan_snp", "scan_oob",
             "aux_ref", "aux_snp", "site_test", "ctx", "walks", "incr", "ingest_bytes"]
# (VG_PACK_OVERLAP, VG_PACK_CORUN_WGS): as shipped (beside the wave kernel when the main stream is busy) with the grid of one
# workgroup per CU and with three workgroups in all; never beside it; always beside it, ONE workgroup
OVERLAP = [(None, None), (None, "3"), ("0", None), ("1", "1")]


def _set_overlap(monkeypatch, overlap):
    monkeypatch.setenv("VG_PACK_SMALL_READS", "0")
    for k, v in zip(("VG_PACK_OVERLAP", "VG_PACK_CORUN_WGS"), overlap):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)


def _gather(r, ids, extra=()):
    """The reads `ids` of `r`, then the byte strings `extra` (quality '#'), as one batch."""
    bs = [r.bases[int(r.offsets[i]):int(r.offsets[i + 1])] for i in ids] + [np.frombuffer(x, np.uint8) for x in extra]
    qs = [r.quals[int(r.offsets[i]):int(r.offsets[i + 1])] for i in ids] + [np.full(len(x), ord("#"), np.uint8) for x in extra]
    offs = np.concatenate([[0], np.cumsum([len(x) for x in bs])]).astype(np.uint64)
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0, np.uint8)
    return cat(bs), cat(qs), offs


@pytest.fixture(scope="module")
def manykeys(tmp_path_factory):
    from vargeno_amd import synth

    g, s, r = synth.f_manykeys()
    d = str(tmp_path_factory.mktemp("manykeys"))
    synth.write_fasta(os.path.join(d, "ref.fa"), g)
    synth.write_vcf(os.path.join(d, "snps.vcf"), g, s)
    subprocess.check_call([BIN, "index", "ref.fa", "snps.vcf", "idx"], cwd=d, env=dict(os.environ, VARGENO_NO_LITE="1"), stdout=subprocess.DEVNULL)
    return os.path.join(d, "idx"), r


@pytest.mark.parametrize("overlap", OVERLAP)
def test_more_batches_than_slots_with_counters_that_differ_from_batch_to_batch(manykeys, monkeypatch, overlap):
    """Eight batches through the handle's three slots (every slot is used two or three times).  The batches differ in what their counters end at: 0-14 of the fixture's 48 many-key reads (they spill
    to the deep tier and on to the lane machine) and 0-7 reads with a foreign byte each.  The sums over the eight batches in
    flight, over the same batches one at a time (a synchronisation after each) and of all their reads as ONE batch on a new
    handle -- whose counters nobody has used before -- are the same numbers, and the site counters are the oracle's."""
    _set_overlap(monkeypatch, overlap)
    prefix, r = manykeys
    many, plain = list(range(r.n - 48, r.n)), list(range(0, r.n - 48))
    n_many, n_bad = [0, 9, 1, 12, 0, 5, 14, 7], [3, 0, 5, 1, 0, 7, 2, 4]
    assert sum(n_many) == 48
    bad_read = b"ACGX" * 8 + b"ACGT" * 8
    batches, m0 = [], 0
    for i in range(8):
        ids = plain[i * len(plain) // 8:(i + 1) * len(plain) // 8] + many[m0:m0 + n_many[i]]
        m0 += n_many[i]
        batches.append(_gather(r, ids, [bad_read] * n_bad[i]))
    whole_b, whole_q = np.concatenate([b[0] for b in batches]), np.concatenate([b[1] for b in batches])
    whole_o = np.concatenate([[0], np.cumsum(np.concatenate([np.diff(b[2].astype(np.int64)) for b in batches]))]).astype(np.uint64)
    ox = O.OracleIndex.load(prefix)
    ox.process(whole_b, whole_q, whole_o)
    so, want = ox.sites(), ox.stats.as_dict()
    assert want["reads_invalid"] == sum(n_bad)
    keys = ("overflow_reads", "overflow_deep", "reads_invalid")
    with GenoIndex.open(prefix) as gx:
        gx.set_stats(False)
        gx.submit(whole_b, whole_q, whole_o)
        rc, ac = gx.counts()
        assert np.array_equal(rc, so["ref_cnt"]) and np.array_equal(ac, so["alt_cnt"])
        st = gx.stats()
        one = tuple(st[k] for k in keys)
    assert one[1] > 2 and one[0] >= one[1] and one[2] == sum(n_bad), one
    with GenoIndex.open(prefix) as gx:
        for stats in (False, True):
            gx.set_stats(stats)
            # one at a time
            singles = []
            for b in batches:
                gx.reset()
                gx.submit(*b)
                st = gx.stats()
                singles.append(tuple(st[k] for k in keys))
            print("per batch (spilled, left for the lane machine, invalid):", singles)
            assert [s_[2] for s_ in singles] == n_bad
            assert len(set(s_[0] for s_ in singles)) > 3 and len(set(s_[1] for s_ in singles)) > 2          # (they do differ)
            assert tuple(sum(s_[j] for s_ in singles) for j in range(3)) == one
            # all in flight, twice over
            gx.reset()
            for _ in range(2):
                for b in batches:
                    gx.submit(*b)
            st = gx.stats()
            assert tuple(st[k] for k in keys) == tuple(2 * x for x in one), stats
            gx.reset()
            for b in batches:
                gx.submit(*b)
            rc, ac = gx.counts()
            assert np.array_equal(rc, so["ref_cnt"]) and np.array_equal(ac, so["alt_cnt"]), stats
            st = gx.stats()
            assert tuple(st[k] for k in keys) == one, stats
            if stats:
                for k in CMP_STATS:
                    assert st[k] == want[k], k


@pytest.mark.parametrize("overlap", OVERLAP)
def test_edge_reads_in_device_batches_both_input_forms(ftiny_dir, ftiny_reads, monkeypatch, overlap):
    """Ragged and damaged reads, N runs, foreign bytes, reads of more than 160 bases (the pack kernel's direct path), 250 bp
    reads, one read, zero reads -- as device-resident batches cut so that most of them start at an odd byte of the text, seven of
    them in flight, as quality strings and as gate words: site counters, event counters and the count of invalid reads are the
    oracle's, with the pack kernel on either stream and with the small grids."""
    import torch

    _set_overlap(monkeypatch, overlap)
    prefix = os.path.join(ftiny_dir, "idx")
    r = ftiny_reads
    edge = [b"ACG", b"", b"ACGT", b"A" * 31, b"ACGTN" * 10, b"ACGT" * 8 + b"N", b"ACGX" * 8, b"acgt" * 16,
            b"ACGTACGTACGTACGTACGTACGTACGTACGN" + b"X" * 32, b"T" * 1021, b"N" * 40 + b"ACGT" * 30, b"ACGT" * 40 + b"-", b"ACGT" * 45 + b"X" * 32]
    ids = list(range(0, 1500))
    bases, quals, offs = _gather(r, ids[:700], edge)
    b2, q2, o2 = _gather(r, ids[700:], edge[::-1])
    bases, quals = np.concatenate([bases, b2]), np.concatenate([quals, q2])
    offs = np.concatenate([offs, offs[-1] + o2[1:]]).astype(np.uint64)
    n = len(offs) - 1
    lens = np.diff(offs.astype(np.int64))
    assert (lens > 160).any() and (lens == 250).any() and (lens == 0).any()
    ox = O.OracleIndex.load(prefix)
    ox.process(bases, quals, offs)
    so, want = ox.sites(), ox.stats.as_dict()
    assert want["reads_invalid"] >= 4 and want["reads_n"] >= 4
    cuts = [0, 1, 1, 2, 300, 701, 713, 1100, n]                  # (a batch of one read, a batch of none)
    assert sum(int(offs[c]) & 1 for c in cuts) >= 3
    dev = torch.device("cuda", 0)
    tb, tq = torch.from_numpy(bases).to(dev), torch.from_numpy(quals).to(dev)
    with GenoIndex.open(prefix) as gx:
        for stats in (True, False):
            for gated in (False, True):
                gx.reset()
                gx.set_stats(stats)
                keep = []
                for a, b in zip(cuts[:-1], cuts[1:]):
                    lo, hi = int(offs[a]), int(offs[b])
                    to = torch.from_numpy((offs[a:b + 1] - offs[a]).astype(np.int64)).to(dev)
                    if gated:
                        gw = gate_words(tq[lo:hi], to)
                        keep.append((to, gw))
                        gx.process_device_gated(tb[lo:hi], gw, to, b - a)
                    else:
                        keep.append(to)
                        gx.process_device(tb[lo:hi], tq[lo:hi], to, b - a)
                rc, ac = gx.counts()
                assert np.array_equal(rc, so["ref_cnt"]) and np.array_equal(ac, so["alt_cnt"]), (stats, gated)
                st = gx.stats()
                assert st["reads_invalid"] == want["reads_invalid"], (stats, gated)
                if stats:
                    for k in CMP_STATS:
                        if not (gated and k == "ingest_bytes"):
                            assert st[k] == want[k], (k, gated)
                del keep


@pytest.mark.parametrize("overlap", OVERLAP)
def test_both_kernels_are_timed_on_either_stream(ftiny_dir, ftiny_reads, monkeypatch, overlap):
    """The handle's event times with the pack kernel on either stream: five batches, positive intervals for both kernels."""
    _set_overlap(monkeypatch, overlap)
    r = ftiny_reads
    with GenoIndex.open(os.path.join(ftiny_dir, "idx")) as gx:
        gx.set_stats(False)
        for _ in range(5):
            gx.submit(r.bases, r.quals, r.offsets)
        gx.sync()
        tm = gx.timing()
        assert tm["batches"] == 5 and tm["ms_main"] > 0 and tm["ms_pack"] > 0 and tm["ms_total"] >= tm["ms_main"], tm

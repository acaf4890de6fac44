"""Held pairs (vg_wave.h, "HELD PAIRS"): a lane of the timed main tier whose pass still has gate-open pairs after the prune may wait,
its stage-A result intact, until the wave has VG_HOLD_PAIRS pairs for one run of stage B -- or until the launch runs out of reads.
The schedule must never show in the counters: every setting equals the oracle exactly, 0 (stage B every iteration) included.

A wave only meets a held lane again after a refill, so the cases run the main tier with one or two workgroups (VG_WAVE_WGS): the
13 000 reads of test_gpu_pair_prune's case -- a third with a substitution under an open gate; inverted repeats, chimeras, two- and
four-copy repeats that reach retries, ties and the deep tier -- then pass through 4 or 8 waves, dozens of refills each, with holds,
flushes on the threshold, flushes on the clamp (a threshold above the pair table's 32 rows) and the drain at the end of the launch.
The handle's held-pass counter says that lanes really waited (and that none did with the hold switched off)."""
import numpy as np
import pytest

import test_gpu_pair_prune as PP
import test_gpu_quiet_walk as QW
from oracle import oracle as O
from vargeno_amd.api import GenoIndex
from vargeno_amd.synth import Reads

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """Made once, read by every test, never changed."""
    return PP.build_case(str(tmp_path_factory.mktemp("hold")))


def _take(c, sel):
    o = c.reads.offsets.astype(np.int64)
    pick = np.concatenate([np.arange(o[i], o[i + 1]) for i in sel])
    return Reads(c.reads.bases[pick], c.reads.quals[pick], np.concatenate([[0], np.cumsum((o[1:] - o[:-1])[sel])]).astype(np.uint64))


def _held(prefix, reads, want):
    """The timed build on a handle of its own: counters equal to `want`; returns the passes its waves held."""
    with GenoIndex.open(prefix) as gx:
        gx.set_stats(False)
        gx.submit(reads.bases, reads.quals, reads.offsets)
        rc, ac = gx.counts()
        bad = np.nonzero((rc != want["ref_cnt"]) | (ac != want["alt_cnt"]))[0]
        assert len(bad) == 0, (want["pos"][bad[:10]], rc[bad[:10]], want["ref_cnt"][bad[:10]], ac[bad[:10]], want["alt_cnt"][bad[:10]])
        return gx.held_passes


# (VG_HOLD_PAIRS, VG_WAVE_WGS, further knobs); None: the variable is not set
COMBOS = [("0", None, ""), ("1", "1", ""), ("8", "2", ""), ("32", "2", ""), ("100000", "1", ""), (None, None, ""),
          ("8", "2", "VG_WORK_CHUNK=8"), ("8", "2", "VG_DX_BITS=18"), ("8", "2", "VG_NO_QUIET=1"), ("32", "2", "VG_NO_QUIET=1")]


@pytest.mark.parametrize("hold,wgs,more", COMBOS, ids=["%s-%s%s" % (h, w, "-" + m if m else "") for h, w, m in COMBOS])
def test_same_counters_under_every_schedule(case, monkeypatch, hold, wgs, more):
    """Off; a threshold of one pair (a flush per iteration that has one: nobody waits); 8 and 32; 100 000, clamped to the pair table's
    rows, so the run flushes on the clamp and on the drain; the default on the full grid; a pool of 8 reads, so refills fall between
    holds; the instantiation for a direct table of fewer than 2^32 buckets; no quiet bits, so no prune, at 8 and at 32.  Without the
    prune the lanes that ran stage A in one iteration of this case bring more than 8 or 16 pairs between them: the threshold is met
    at once and nobody waits (0 passes held at 8 and at 16 on an MI355X; 22 to 25 at 32, in the rare iteration poor in pairs, a
    number that depends on how the workgroups race for work).  So without the quiet bits this case checks the counters only; that
    lanes wait without the prune is test_no_quiet_sparse_gates_wait's, on reads chosen so that they must."""
    c = case
    monkeypatch.delenv("VG_HOLD_PAIRS", raising=False)
    monkeypatch.delenv("VG_WAVE_WGS", raising=False)
    if hold is not None:
        monkeypatch.setenv("VG_HOLD_PAIRS", hold)
    if wgs is not None:
        monkeypatch.setenv("VG_WAVE_WGS", wgs)
    if more:
        monkeypatch.setenv(*more.split("="))
    QW._run(c, c.reads)                                     # both builds against the oracle, counters and event counts
    held = _held(c.prefix, c.reads, c.so)
    print("VG_HOLD_PAIRS=%s VG_WAVE_WGS=%s %s: %d passes held, %d reads" % (hold, wgs, more, held, c.reads.n))
    if hold == "0":
        assert held == 0
    if hold is not None and int(hold) >= 8 and wgs is not None and int(wgs) <= 2 and "VG_NO_QUIET" not in more:
        assert held > 0
    if hold == "1":
        assert held == 0                                    # one pair is the threshold: whoever has a pair flushes


@pytest.fixture(scope="module")
def gate_open(case):
    """The case's reads with an open gate, in order."""
    return np.array([i for i, r in enumerate(case.plan) if r["gates"]])


@pytest.mark.parametrize("count", [1, 37, 64, 65, 255, 257])
def test_tiny_batches(case, gate_open, monkeypatch, count):
    """A wave that never fills, one that fills exactly, one read more than a wave, and a workgroup with one read less / more than
    its 256 lanes: the launch runs out at once, so every iteration flushes -- each against the oracle on the same reads."""
    c = case
    assert len(gate_open) >= 257
    sub = _take(c, gate_open[:count])
    ox = O.OracleIndex.load(c.prefix)
    ox.process(sub.bases, sub.quals, sub.offsets, nthreads=8)
    monkeypatch.setenv("VG_HOLD_PAIRS", "32")
    monkeypatch.setenv("VG_WAVE_WGS", "1")
    _held(c.prefix, sub, ox.sites())


def test_no_quiet_sparse_gates_wait(case, gate_open, monkeypatch):
    """No quiet bits, so no prune: every gate-open chunk of a pass with a key is a pair.  Seven reads in eight of the case have an
    open gate, which is why the case itself meets a threshold of 8 in every iteration.  Here the gates of all but every 32nd of them
    are shut (the gate's quality character made a high one): some 350 of 13 000 reads, one in 37, keep theirs, so the 64 lanes of
    an iteration bring two or three pairs between them, a threshold of 8 takes several iterations, and lanes must wait whatever the
    workgroups' race for work.  Counters equal the oracle's on the same reads."""
    c = case
    shut = np.ones(c.reads.n, bool)
    shut[gate_open[::32]] = False
    o = c.reads.offsets.astype(np.int64)
    quals = c.reads.quals.copy()
    per_base = np.repeat(shut, o[1:] - o[:-1])
    quals[per_base & (quals == ord("#"))] = ord("I")
    sub = Reads(c.reads.bases, quals, c.reads.offsets)
    ox = O.OracleIndex.load(c.prefix)
    ox.process(sub.bases, sub.quals, sub.offsets, nthreads=8)
    monkeypatch.setenv("VG_NO_QUIET", "1")
    monkeypatch.setenv("VG_HOLD_PAIRS", "8")
    monkeypatch.setenv("VG_WAVE_WGS", "2")
    held = _held(c.prefix, sub, ox.sites())
    print("VG_NO_QUIET=1, %d reads, %d of them with an open gate: %d passes held" % (c.reads.n, len(gate_open[::32]), held))
    assert held > 0


def test_long_reads_run_the_plain_kernel(case, monkeypatch):
    """A batch whose reads average five chunks or more goes to the kernel without the hold, whatever the threshold (enqueue_batch):
    3 000 reads of 250 bases, a third of them with a substitution under an open gate -- about one pair per three reads, so a
    threshold of 32 would make lanes wait -- equal the oracle, and no pass is held."""
    c = case
    rng = np.random.default_rng(77)
    hp, L, N = c.h[0], 250, 3000
    bases, quals = [], []
    for i, t in enumerate(rng.integers(0, len(hp) - L, N)):
        b = hp[t:t + L].copy()
        q = rng.integers(ord(":"), ord("I") + 1, size=L, dtype=np.uint8)
        if i % 3 == 0:
            ch = int(rng.integers(0, 7))
            b[32 * ch + 9] = PP._other(b[32 * ch + 9])
            q[ch] = ord("#")
        bases.append(b); quals.append(q)
    reads = Reads(np.concatenate(bases), np.concatenate(quals), (np.arange(N + 1) * L).astype(np.uint64))
    ox = O.OracleIndex.load(c.prefix)
    ox.process(reads.bases, reads.quals, reads.offsets, nthreads=8)
    monkeypatch.setenv("VG_HOLD_PAIRS", "32")
    monkeypatch.setenv("VG_WAVE_WGS", "2")
    assert _held(c.prefix, reads, ox.sites()) == 0


def test_sample_planes(case, monkeypatch):
    """Two samples on one index, two batches each in flight together, two workgroups and a threshold of 8: per-plane counters equal
    the oracle's on each sample alone, and lanes waited."""
    c = case
    monkeypatch.setenv("VG_HOLD_PAIRS", "8")
    monkeypatch.setenv("VG_WAVE_WGS", "2")
    idx = np.arange(c.reads.n)
    samples = [[_take(c, idx[idx % 4 == 0]), _take(c, idx[idx % 4 == 1])], [_take(c, idx[idx % 4 == 2]), _take(c, idx[idx % 4 == 3])]]
    want = []
    for bs in samples:
        ox = O.OracleIndex.load(c.prefix)
        for b in bs:
            ox.process(b.bases, b.quals, b.offsets, nthreads=8)
        so = ox.sites()
        want.append((so["ref_cnt"].copy(), so["alt_cnt"].copy()))
    assert not np.array_equal(want[0][0], want[1][0])
    with GenoIndex.open(c.prefix) as gx:
        gx.set_stats(False)
        gx.reserve_samples(2)
        for k in range(2):
            for s in range(2):
                gx.select(s)
                b = samples[s][k]
                gx.submit(b.bases, b.quals, b.offsets)
        for s in range(2):
            rc, ac = gx.counts(sample=s)
            assert np.array_equal(rc, want[s][0]) and np.array_equal(ac, want[s][1]), s
        assert gx.held_passes > 0

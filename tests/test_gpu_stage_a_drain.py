"""Stage A's drained candidates (vg_wave.h, "DRAINED CANDIDATES"; vg_acand.h): the look-up of a chunk only compares, and one loop per
pair of chunks inserts every lane's candidates -- reverse-strand pushes, reference hit, SNP hit, rows -- into the key table, a lane's
k-th candidate in trip k.  Nothing of that may show: the counters equal the oracle's exactly.

(1) The 13 000 reads of test_gpu_pair_prune's case (inverted repeats fill both key lists; two-copy repeats give PAIR entries,
    four-copy repeats rows; retries, ties, the deep tier) under the settings that change what the drain sees: one workgroup, the
    plain kernel, the direct table of 2^18 buckets (the other instantiation; full buckets, so `more` and the deep-bucket loop), no
    quiet bits, a pool of 8 reads; and batches of 1, 64, 65 and 257 reads.
(2) A small case of its own (60 kbp) with four features, each with sites that only its own reads reach:
      pal     a planted palindromic 32-mer: one entry is a forward and a reverse candidate at once;
      shared  reads with the alt allele over a 32-mer that the reference also holds elsewhere: reference and SNP candidate in one chunk;
      pair    a SNP inside a two-copy repeat: PAIR candidates and a SNP candidate in one read;
      rows    a SNP record listed three times (DevIndex::aux_dups: every row of this index takes the careful path through the
              drain), with its ordinary neighbour five bases on, and a four-copy repeat beside a site.
    test_small_case_features_reach_their_sites (CPU) says the GPU pass is not vacuous: by the oracle alone, every feature's sites
    have non-zero counters with the feature's reads and all-zero counters without them."""
import os
import subprocess

import numpy as np
import pytest

import test_gpu_pair_prune as PP
import test_gpu_quiet_walk as QW
from conftest import BIN
from oracle import oracle as O
from vargeno_amd import synth
from vargeno_amd.synth import ACGT, Reads

COMP, CODE = QW.COMP, QW.CODE
GL = 60_000
PAL, SHARED_Q, SHARED_COPY, REP2_A, REP2_B, TRIPLE, REP4 = 5_000, 8_000, 9_000, 12_000, 14_000, 20_000, 24_000


def _rc(b):
    return COMP[b[::-1]]


def _other(b, k=1):
    return ACGT[(CODE[b] + k) % 4]


class Case:
    pass


def _small_genome(rng):
    """The genome, the VCF's records (0-based position, ref, alt, times listed) and each feature's own sites."""
    g = synth.make_genome(rng, [GL], ["chr1"], repeats_per_mbp=0.0, microsat_per_mbp=0.0, n_gaps=False)
    s0 = g.seqs[0]
    s0[PAL + 16:PAL + 32] = _rc(s0[PAL:PAL + 16])                              # a 32-mer that is its own reverse complement
    assert np.array_equal(s0[PAL:PAL + 32], _rc(s0[PAL:PAL + 32]))
    recs = {}

    def site(p, times=1, k=1):
        recs[p] = (s0[p], _other(s0[p], k), times)
    site(PAL + 45)
    site(SHARED_Q)
    s0[SHARED_COPY:SHARED_COPY + 32] = s0[SHARED_Q - 10:SHARED_Q + 22]         # the alt allele's 32-mer, as reference sequence elsewhere
    s0[SHARED_COPY + 10] = recs[SHARED_Q][1]
    s0[REP2_B:REP2_B + 200] = s0[REP2_A:REP2_A + 200]
    site(REP2_A + 70)
    site(TRIPLE, times=3)
    site(TRIPLE + 5, k=2)
    for off in (500, 1_000, 2_000):
        s0[REP4 + off:REP4 + off + 150] = s0[REP4:REP4 + 150]
    site(REP4 + 1_000 + 155)
    for p in range(30_000, 58_000, 700):                                        # the background: a site every 700 bases
        site(p + int(rng.integers(0, 100)))
    feat_sites = dict(pal=[PAL + 45], shared=[SHARED_Q], pair=[REP2_A + 70], rows=[TRIPLE + 5, REP4 + 1_000 + 155])
    return g, recs, feat_sites


def _small_reads(rng, s0, recs):
    """(bases, quals, feature or None) per read; every read has four chunks (128 bases)."""
    out = []

    def add(feat, t, edits=(), rev=False, gates=()):
        w = s0[t:t + 128].copy()
        for p, b in edits:                                                      # genome position -> base
            w[p - t] = b
        q = np.full(128, ord("I"), np.uint8)
        for c in gates:
            q[c] = ord("#")
        out.append((_rc(w) if rev else w, q, feat))

    alt = lambda p: (p, recs[p][1])
    sub = lambda p: (p, _other(s0[p], 2))
    for rev in (False, True):
        # pal: the palindrome is chunk c, the site lies in chunk c + 1; every other chunk is broken by a substitution under a shut
        # gate, so the key is live only if the palindrome's entry gave chunk c its forward candidate
        for c in (0, 1, 2):
            t = PAL - 32 * c
            for allele in ((), (alt(PAL + 45),)):
                add("pal", t, tuple(sub(t + 32 * j + 9) for j in range(4) if j not in (c, c + 1)) + allele, rev)
                add("pal", t, allele, rev)
        # shared: chunk c is the alt allele's 32-mer, which the reference holds at SHARED_COPY: two candidates in one chunk
        for c in (0, 1, 2, 3):
            t = SHARED_Q - 10 - 32 * c
            add("shared", t, (alt(SHARED_Q),), rev)
            add("shared", t, (), rev)
            add("shared", t, (alt(SHARED_Q),) + tuple(sub(t + 32 * j + 9) for j in range(4) if j != c and j != (c + 1) % 4), rev)
        # pair: chunk 0 straddles the repeat's start (unique), the others lie inside it (PAIR entries); the site's chunk carries either allele
        for d in (0, 8, 20):
            for allele in ((), (alt(REP2_A + 70),)):
                add("pair", REP2_A - 20 + d, allele, rev)
                add("pair", REP2_A - 20 + d, allele + (sub(REP2_A - 20 + d + 5),), rev, gates=(3 if rev else 0,))
        add("pair", REP2_B - 20, (), rev)                                       # the other copy: the same PAIR entries, no site
        # rows: the record listed three times and its neighbour, either allele at both, the site in every chunk; the four-copy repeat
        for off in (3, 20, 45, 70, 100):
            for a0 in ((), (alt(TRIPLE),)):
                for a5 in ((), (alt(TRIPLE + 5),)):
                    add("rows", TRIPLE - off, a0 + a5, rev)
                    add("rows", TRIPLE - off, a0 + a5, rev, gates=(3 - off // 32 if rev else off // 32,))
        for c0 in (REP4, REP4 + 500, REP4 + 1_000, REP4 + 2_000):
            for d in (-40, 0, 22, 50):
                add("rows", c0 + d, (), rev)
    for _ in range(300):                                                        # the background: ordinary reads, both strands, either allele
        t = int(rng.integers(29_500, 58_500))
        ed = tuple(alt(p) for p in recs if t <= p < t + 128 and rng.random() < 0.5)
        gates = tuple(c for c in range(4) if rng.random() < 0.25)
        if gates and rng.random() < 0.5:
            ed += (sub(t + 32 * gates[0] + 5),) if (t + 32 * gates[0] + 5) not in recs else ()
        add(None, t, ed, bool(rng.integers(0, 2)), gates)
    return out


def _oracle(prefix, reads):
    ox = O.OracleIndex.load(prefix)
    ox.process(reads.bases, reads.quals, reads.offsets, nthreads=8)
    return ox.sites(), ox.stats.as_dict()


def _pack(rows):
    return Reads(np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows]), (128 * np.arange(len(rows) + 1)).astype(np.uint64))


def build_small_case(d, seed=4242):
    rng = np.random.default_rng(seed)
    c = Case()
    g, recs, c.feat_sites = _small_genome(rng)
    synth.write_fasta(os.path.join(d, "ref.fa"), g)
    with open(os.path.join(d, "snps.vcf"), "w") as f:
        f.write(synth.VCF_HEADER)
        for i, p in enumerate(sorted(recs)):
            ref, alt, times = recs[p]
            f.write(("1\t%d\trs%d\t%c\t%c\t.\t.\tRS=%d;CAF=0.6000,0.4000;COMMON=1\n" % (p + 1, i + 1, ref, alt, i + 1)) * times)
    subprocess.check_call([BIN, "index", "ref.fa", "snps.vcf", "idx"], cwd=d, env=dict(os.environ, VARGENO_NO_LITE="1"), stdout=subprocess.DEVNULL)
    c.prefix = os.path.join(d, "idx")
    c.rows = _small_reads(rng, g.seqs[0], recs)
    c.reads = _pack(c.rows)
    c.so, c.want = _oracle(c.prefix, c.reads)
    c.shift = int(c.so["pos"].astype(np.int64).min()) - min(recs)              # the pile-up's coordinate against the genome's
    return c


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    """Made once, read by every test, never changed."""
    return build_small_case(str(tmp_path_factory.mktemp("drain_small")))


def test_small_case_features_reach_their_sites(small):
    """CPU, the oracle alone: with all reads every feature's sites have a counter above zero; without the feature's own reads the
    same sites have none -- no other read reaches them, so the GPU parity below does rest on each feature."""
    c = small
    at = {int(p): i for i, p in enumerate(c.so["pos"].astype(np.int64))}
    for feat, sites in c.feat_sites.items():
        idx = [at[p + c.shift] for p in sites]
        with_f = c.so["ref_cnt"][idx].astype(np.int64) + c.so["alt_cnt"][idx]
        so, _ = _oracle(c.prefix, _pack([r for r in c.rows if r[2] != feat]))
        without = so["ref_cnt"][idx].astype(np.int64) + so["alt_cnt"][idx]
        print(feat, "sites", sites, "counters with its reads", with_f.tolist(), "without", without.tolist())
        assert (with_f > 0).all() and (without == 0).all(), (feat, with_f, without)
    # the alt allele is counted where only the SNP candidate can have counted it
    for feat in ("pal", "shared", "pair"):
        assert c.so["alt_cnt"][at[c.feat_sites[feat][0] + c.shift]] > 0, feat


@pytest.mark.gpu
@pytest.mark.parametrize("knob", ["", "VG_WAVE_WGS=1", "VG_HOLD_PAIRS=0", "VG_DX_BITS=18", "VG_NO_QUIET=1"])
def test_small_case_equals_the_oracle(small, monkeypatch, knob):
    """Both builds, counters and event counts; the index has a row that repeats a position, so its rows are expanded in the drain."""
    if knob:
        monkeypatch.setenv(*knob.split("="))
    views, _ = QW._run(small, small.reads)
    assert "dx" in views


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """test_gpu_pair_prune's case: made once, read by every test, never changed."""
    return PP.build_case(str(tmp_path_factory.mktemp("drain")))


@pytest.mark.gpu
@pytest.mark.parametrize("knob", ["", "VG_WAVE_WGS=1", "VG_HOLD_PAIRS=0", "VG_DX_BITS=18", "VG_NO_QUIET=1", "VG_WORK_CHUNK=8"])
def test_same_counters_under_every_setting(case, monkeypatch, knob):
    """The default with both builds (counters and event counts); the other settings change the timed build's schedule or tables only."""
    if knob:
        monkeypatch.setenv(*knob.split("="))
    views, _ = QW._run(case, case.reads, timed_only=bool(knob))
    assert "dx" in views


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 64, 65, 257])
def test_tiny_batches(case, count):
    """A wave that never fills, one that fills exactly, one read more, and one read more than a workgroup's 256 lanes: reads taken
    evenly from all over the case (every construct), each batch against the oracle on the same reads."""
    c = case
    sel = (np.arange(count) * (c.reads.n // 257)).astype(np.int64)
    o = c.reads.offsets.astype(np.int64)
    pick = np.concatenate([np.arange(o[i], o[i + 1]) for i in sel])
    sub = Reads(c.reads.bases[pick], c.reads.quals[pick], np.concatenate([[0], np.cumsum((o[1:] - o[:-1])[sel])]).astype(np.uint64))
    t = Case()
    t.prefix = c.prefix
    t.so, t.want = _oracle(c.prefix, sub)
    QW._run(t, sub)

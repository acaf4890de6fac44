"""The skipped pile-up walk of the timed build (vg_wave.h, stage C): a read of up to four chunks whose winning vote key is known, from
two bits in the records stage A fetches anyway (vg_quiet.h), to have no SNP site in its window does not fetch its rank blocks.  A
skipped walk and a walk that finds no site leave the same counters, so what can be checked is (1) exact parity with the oracle on
reads whose windows put a site just outside, just inside and on every seam, with every layout and tier, (2) that the bits were
really set -- the loader's counts against counts made here from the index files -- and (3) that a good part of the reads are ones
the rule lets skip, worked out here from where the reads start and where the sites are."""
import os
import subprocess

import numpy as np
import pytest

from conftest import BIN
from oracle import oracle as O
from vargeno_amd import index_io, synth
from vargeno_amd.api import GenoIndex
from vargeno_amd.synth import ACGT, Reads, SnpSet

pytestmark = pytest.mark.gpu

GLEN = 200_000
LENS = {64: 2, 96: 3, 101: 3, 128: 4, 150: 4}                 # read length -> chunks
POS_AMBIGUOUS = 0xFFFFFFFF
COMP = np.zeros(256, np.uint8)
for _a, _b in zip(b"ACGT", b"TGCA"):
    COMP[_a] = _b
CODE = np.zeros(256, np.uint8)
for _i, _a in enumerate(b"ACGT"):
    CODE[_a] = _i


def _genome_and_sites(rng):
    """200 kbp of random bases.  [2 000, 120 000): a SNP every 600-800 bases, so that most 128-base windows hold none.  Beyond:
    two-copy repeats of 200 bases (PAIR entries: one copy far from any site, the other -- the second or the first, in turn -- with a
    site 5 bases past its end and one 3 bases before its start) and four-copy repeats of 150 bases (auxiliary rows; a site beside the third copy only)."""
    g = synth.make_genome(rng, [GLEN], ["chr1"], repeats_per_mbp=0.0, microsat_per_mbp=0.0, n_gaps=False)
    s0 = g.seqs[0]
    sites = list(3_000 + 700 * np.arange(165) + rng.integers(-50, 51, size=165))
    pairs, multis = [], []
    for i in range(12):
        src = 122_000 + 3_000 * i
        s0[src + 1_500:src + 1_700] = s0[src:src + 200]
        near = src + 1_500 if i % 2 == 0 else src                          # the copy that has the sites beside it: the second / the first
        sites += [near - 3, near + 200 + 5]
        pairs.append((src, src + 1_500))
    for i in range(8):
        src = 160_000 + 4_000 * i
        for off in (500, 1_000, 2_000):
            s0[src + off:src + off + 150] = s0[src:src + 150]
        sites.append(src + 1_000 + 155)
        multis.append((src, src + 500, src + 1_000, src + 2_000))
    sites = np.unique(np.array(sites, dtype=np.int64))
    ref = s0[sites]
    alt = ACGT[(CODE[ref] + 1 + np.arange(len(sites)) % 3) % 4]
    s = SnpSet(np.zeros(len(sites), np.int32), sites + 1, ref, alt, np.full(len(sites), 0.6), np.full(len(sites), 0.4), (np.arange(len(sites)) % 3).astype(np.uint8))
    s._with_caf = True
    return g, s, sites, pairs, multis


def _make_reads(rng, g, s, plan):
    """plan: rows (window start t in the genome, read length, reverse strand, haplotype, substitution chunk or -1).  A read's window
    is the 32 n bases that its chunks cover: a forward read starts at t, a reverse one is the reverse complement of
    [t - (L - 32 n), t + 32 n).  A substitution sits at base 5 of a chunk of the read as given, whose quality character opens the gate."""
    h0, h1, _ = synth.haplotypes(g, s)
    bases, quals, lens = [], [], []
    for t, L, rev, hap, sub in plan:
        n = LENS[L]
        lo = t - (L - 32 * n) if rev else t
        b = (h1 if hap else h0)[lo:lo + L].copy()
        assert len(b) == L
        if rev:
            b = COMP[b[::-1]]
        q = rng.integers(ord(":"), ord("I") + 1, size=L, dtype=np.uint8)
        if sub >= 0:
            b[32 * sub + 5] = ACGT[(CODE[b[32 * sub + 5]] + 1) % 4]
            q[sub] = ord("#")
        bases.append(b); quals.append(q); lens.append(L)
    return Reads(np.concatenate(bases), np.concatenate(quals), np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64))


def _plan(rng, sites, pairs, multis):
    plan = []
    k = 0
    # (a) edge reads: a handful of the sparse sites at every interesting offset of the window, every length, both strands
    for P in sites[(sites > 10_000) & (sites < 100_000)][::12][:8]:
        for L, n in LENS.items():
            for off in (-1, 32 * n, 0, 32 * n - 1, 31, 32, 63, 64):
                for rev in (False, True):
                    sub = k % n if k % 3 == 0 else -1
                    plan.append((int(P) - off, L, rev, k % 2 == 1, sub))
                    k += 1
    n_edge = len(plan)
    # ordinary reads all over the sparse part, a third with a substitution in a gate-open chunk
    for _ in range(5_000):
        L = int(rng.choice(list(LENS)))
        n = LENS[L]
        plan.append((int(rng.integers(2_500, 119_000)), L, bool(rng.integers(0, 2)), bool(rng.integers(0, 2)), int(rng.integers(0, n)) if rng.random() < 1 / 3 else -1))
    # (c) reads aimed at every copy of the repeats, at several offsets into the copy
    for copies, rl in [(p, 200) for p in pairs] + [(m, 150) for m in multis]:
        for c0 in copies:
            for d in (-40, -8, 0, 20, rl - 128, rl - 100):
                for L in (101, 128, 150):
                    plan.append((c0 + d, L, k % 2 == 0, k % 4 >= 2, k % LENS[L] if k % 5 == 0 else -1))
                    k += 1
    return plan, n_edge


class Case:
    pass


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """Genome, index, reads and the oracle's counters: made once, read by every test, never changed."""
    rng = np.random.default_rng(606)
    c = Case()
    g, s, sites, pairs, multis = _genome_and_sites(rng)
    d = str(tmp_path_factory.mktemp("quiet"))
    synth.write_fasta(os.path.join(d, "ref.fa"), g)
    synth.write_vcf(os.path.join(d, "snps.vcf"), g, s)
    subprocess.check_call([BIN, "index", "ref.fa", "snps.vcf", "idx"], cwd=d, env=dict(os.environ, VARGENO_NO_LITE="1"), stdout=subprocess.DEVNULL)
    c.prefix = os.path.join(d, "idx")
    c.plan, c.n_edge = _plan(rng, sites, pairs, multis)
    c.reads = _make_reads(rng, g, s, c.plan)
    ox = O.OracleIndex.load(c.prefix)
    ox.process(c.reads.bases, c.reads.quals, c.reads.offsets, nthreads=8)
    c.so = ox.sites()
    c.want = ox.stats.as_dict()
    # the pile-up's coordinate against the genome's: one shift for every site
    sp = np.sort(c.so["pos"].astype(np.int64))
    assert len(sp) == len(sites)
    c.shift = int(sp[0] - sites[0])
    assert np.array_equal(sp, sites + c.shift)
    # what the loader must find, from the index files: single-position reference entries, their windows against the site list
    rd = index_io.read_ref_dict(c.prefix + ".ref.dict")
    sd = index_io.read_snp_dict(c.prefix + ".snp.dict")
    single = (rd["ref_amb"] == 0) & (rd["ref_pos"] != POS_AMBIGUOUS)
    named = [rd["ref_pos"][single], rd["ref_aux"][rd["ref_aux"] != 0], sd["snp_pos"][(sd["snp_amb"] == 0) & (sd["snp_pos"] != POS_AMBIGUOUS)], sd["snp_aux_pos"][sd["snp_aux_pos"] != 0]]
    c.pile_len = int(max(int(x.max()) for x in named if len(x))) + 64
    bits = np.zeros(c.pile_len + 1, np.int64)
    bits[sp] = 1
    cum = np.concatenate([[0], np.cumsum(bits)])
    c.clear = lambda a, b: cum[np.clip(b, 0, c.pile_len)] - cum[np.clip(a, 0, c.pile_len)] == 0       # no site in [a, b), element-wise
    kp = rd["ref_pos"][single].astype(np.int64)
    c.A = dict(zip(kp.tolist(), ((kp + 32 <= c.pile_len) & c.clear(kp - 96, kp + 32)).tolist()))
    c.B = dict(zip(kp.tolist(), ((kp + 128 <= c.pile_len) & c.clear(kp, kp + 128)).tolist()))
    c.n_entries = len(rd["ref_kmer"]) + len(sd["snp_kmer"])
    c.n_pair_or_row = int((rd["ref_amb"] != 0).sum())
    return c


def _skippable(c, rows):
    """Reads of `rows` that the rule lets skip, from where they start and where the sites are: a chunk c without a substitution whose
    32-mer is a single-position reference entry at kpos = t + 32 c proves the window quiet iff (c == 0 || A) && (c == n - 1 || B);
    a read counts when at least two of its chunks are exact (then its key wins the vote) and one of them is such a proof."""
    out = 0
    for t, L, rev, hap, sub in rows:
        n = LENS[L]
        bad = -1 if sub < 0 else (n - 1 - sub if rev else sub)                 # the substituted chunk, in the pile-up's orientation
        kpos = [t + c.shift + 32 * cc for cc in range(n)]
        if not c.clear(np.int64(kpos[0]), np.int64(kpos[0] + 32 * n)):
            continue                                                            # (a site in the window: an allele may break any chunk)
        exact = [cc for cc in range(n) if cc != bad and kpos[cc] in c.A]
        proof = [cc for cc in exact if (cc == 0 or c.A[kpos[cc]]) and (cc == n - 1 or c.B[kpos[cc]])]
        out += len(exact) >= 2 and len(proof) >= 1
    return out


def _run(c, reads, timed_only=False):
    """Both builds on one handle: counters equal to the oracle's."""
    with GenoIndex.open(c.prefix) as gx:
        info = (gx.views, gx.quiet_bits)
        for stats in ((False,) if timed_only else (True, False)):
            gx.reset()
            gx.set_stats(stats)
            gx.submit(reads.bases, reads.quals, reads.offsets)
            rc, ac = gx.counts()
            bad = np.nonzero((rc != c.so["ref_cnt"]) | (ac != c.so["alt_cnt"]))[0]
            assert len(bad) == 0, ("stats=%s" % stats, c.so["pos"][bad[:10]], rc[bad[:10]], c.so["ref_cnt"][bad[:10]], ac[bad[:10]], c.so["alt_cnt"][bad[:10]])
            if stats:
                st = gx.stats()
                for k in ("reads", "passes", "passes_ok", "chunks", "ctx", "walks", "incr"):
                    assert st[k] == c.want[k], k
    return info


def test_edge_reads_and_the_loaders_counts(case):
    """(a) and (c): sites at window offsets -1, 32 n, 0, 32 n - 1, 31 / 32, 63 / 64 for reads of 2, 3, 3, 4, 4 chunks on both strands,
    repeats with one copy beside a site; exact parity in both builds; the loader's counts of A, B and both equal the counts made
    from the index files (single-position reference entries only: no PAIR, no row, no SNP entry), all three non-zero; at least a
    third of the processed reads are ones the rule lets skip."""
    c = case
    assert c.so["ref_cnt"].sum() + c.so["alt_cnt"].sum() > 500 and c.n_pair_or_row > 1_000
    views, qb = _run(c, c.reads)
    assert "dx" in views and qb is not None
    nA, nB = sum(c.A.values()), sum(c.B.values())
    nAB = sum(1 for k, v in c.A.items() if v and c.B[k])
    assert 0 < nAB < min(nA, nB) and max(nA, nB) < len(c.A)
    assert qb == dict(a=nA, b=nB, both=nAB, entries=c.n_entries), (qb, nA, nB, nAB, c.n_entries)
    skip = _skippable(c, c.plan)
    assert 3 * skip >= c.want["passes_ok"], (skip, c.want["passes_ok"])
    assert 0 < _skippable(c, c.plan[:c.n_edge]) < c.n_edge               # the edge reads hold both kinds


@pytest.mark.parametrize("knob", ["VG_NO_QUIET=1", "VG_NO_DIRECT=1", "VG_NO_MX=1", "VG_DX_BITS=18", "VG_PACK_OVERLAP=0", "VG_FORCE_GENERIC=1+VG_SCRATCH_CAP=3+VG_SCRATCH_KCAP=2"])
def test_same_counters_under_every_knob(case, monkeypatch, knob):
    """(b): the bits left clear, the layouts that never see them, the direct table of fewer than 2^32 buckets (the other
    instantiation of the kernel), the pack kernel never beside the wave kernel, and the lane machine with a tiny first scratch."""
    c = case
    for kv in knob.split("+"):
        monkeypatch.setenv(*kv.split("="))
    views, qb = _run(c, c.reads)
    if knob == "VG_NO_QUIET=1":
        assert qb == dict(a=0, b=0, both=0, entries=c.n_entries)
    elif knob in ("VG_NO_DIRECT=1", "VG_NO_MX=1"):
        assert "dx" not in views and qb is None
    else:
        assert "dx" in views and qb["both"] > 0


def test_sample_planes_skip_in_one_batch_and_walk_in_the_other(case):
    """(d): two samples on one index; sample 0 gets the reads the rule lets skip first and the walking ones second, sample 1 the
    other way round, in alternating batches -- per-plane counters equal the oracle's on each sample alone."""
    c = case
    idx = np.arange(c.reads.n)
    quiet = np.array([_skippable(c, [row]) == 1 for row in c.plan])
    assert quiet.sum() > 500 and (~quiet).sum() > 500
    o = c.reads.offsets.astype(np.int64)

    def take(sel):
        pick = np.concatenate([np.arange(o[i], o[i + 1]) for i in sel])
        return Reads(c.reads.bases[pick], c.reads.quals[pick], np.concatenate([[0], np.cumsum((o[1:] - o[:-1])[sel])]).astype(np.uint64))
    half = idx % 2 == 0
    samples = [[take(idx[half & quiet]), take(idx[half & ~quiet])], [take(idx[~half & ~quiet]), take(idx[~half & quiet])]]
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
        for k in range(2):                                                      # batch k of both samples in flight together
            for s in range(2):
                gx.select(s)
                b = samples[s][k]
                gx.submit(b.bases, b.quals, b.offsets)
        for s in range(2):
            rc, ac = gx.counts(sample=s)
            assert np.array_equal(rc, want[s][0]) and np.array_equal(ac, want[s][1]), s

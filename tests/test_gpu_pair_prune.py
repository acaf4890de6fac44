"""The stage-B pair prune of the timed build (vg_wave.h, where `pend` is formed): for reads of up to four chunks a key's mask carries,
chunk by chunk, which of the read's 32-base windows are known to hold no SNP site (vg_quiet_chunks), and a gate-open (owner, chunk)
pair that can neither change the vote's outcome nor lie over a window that may hold a site is not expanded:
    R1  pass 1 and every key's chunks are all free              -> no pair of the pass;
    R2  one key with exact contexts of two different chunks     -> no pair of a free chunk.
A pruned pair and a pair that finds nothing leave the same counters, so what can be checked is exact parity with the oracle on reads
whose SUBSTITUTION sits in a gate-open chunk (stage B really finds the neighbour, and the counter of a site in that chunk's window
depends on it), with the nearest site just outside, just inside and on the seams of that chunk's window -- in every layout and tier --
and, from where the reads and the sites are, that the case is not vacuous: the rules prune at least 40 % of the gate-open pairs of
passes that have a key and leave at least 20 % of them, and the oracle's counters with the gates as given differ at 50 sites or more
from its counters with every quality character high (a kernel that pruned every pair would fail).

Constructs aimed at the rule's edges (each named in _plan): one exact chunk only (not pruned: the neighbours make the key live);
inverted repeats whose forward copy is quiet and whose reverse copy has a site (R1 is a rule of pass 1: applied in pass 0 it would
send the read to the other strand); chimeric reads with two tied keys of different free-chunk bits (the bits must not reach the
vote); diverged two-copy repeats and four-copy repeats where a neighbour makes or breaks a tie, on both strands; reads at both ends
of the pile-up, overhanging ones included."""
import os
import subprocess

import numpy as np
import pytest

import test_gpu_quiet_walk as QW
from conftest import BIN
from oracle import oracle as O
from vargeno_amd import index_io, synth
from vargeno_amd.api import GenoIndex
from vargeno_amd.synth import ACGT, Reads, SnpSet

pytestmark = pytest.mark.gpu

GLEN, LENS, COMP, CODE, POS_AMBIGUOUS = QW.GLEN, QW.LENS, QW.COMP, QW.CODE, QW.POS_AMBIGUOUS
N_SPARSE = 140                                                  # sites of the sparse part, one every 650-750 bases from 3 000 on
INV0, CHI0, REP2, REP4 = 102_000, 111_000, 122_000, 160_000     # where the constructs start (1 000 / 1 000 / 3 000 / 4 000 apart)


def _rc(b):
    return COMP[b[::-1]]


def _other(b, k=1):
    return ACGT[(CODE[b] + k) % 4]


def _genome_and_sites(rng):
    g = synth.make_genome(rng, [GLEN], ["chr1"], repeats_per_mbp=0.0, microsat_per_mbp=0.0, n_gaps=False)
    s0 = g.seqs[0]
    sites = list(3_000 + 700 * np.arange(N_SPARSE) + rng.integers(-50, 51, size=N_SPARSE))
    sites += [50, 140, GLEN - 61, GLEN - 150]                   # inside the first and the last 128 positions, and just beyond
    inv, chi, rep2, rep4 = [], [], [], []
    for i in range(8):
        # inverted repeat: [b, b + 128) is the reverse complement of [a, a + 128); no site within 400 bases of a, one in the LAST chunk's
        # window of the reverse copy as a read of three or four chunks sees it
        a = INV0 + 1_000 * i
        s0[a + 500:a + 628] = _rc(s0[a:a + 128])
        sites.append(a + 500 + 116)
        inv.append((a, a + 500))
        # chimera: chunks 0-1 of a read from a (sites 10 before a and 100 after it: neither chunk's entry has a bit), chunks 2-3 from
        # b + 64 (a site in chunk 3's window only: chunk 2's entry proves chunks 0-2 free)
        a = CHI0 + 1_000 * i
        sites += [a - 10, a + 100, a + 500 + 116]
        chi.append((a, a + 500))
    for i in range(12):
        # two copies of 200 bases that differ in ONE base (offset 40: chunk 1 of a read that starts with the copy), the even ones exact;
        # sites beside one copy only, as in test_gpu_quiet_walk.py
        src = REP2 + 3_000 * i
        s0[src + 1_500:src + 1_700] = s0[src:src + 200]
        if i % 2:
            s0[src + 1_540] = _other(s0[src + 1_540])
        near = src + 1_500 if i % 4 < 2 else src
        sites += [near - 3, near + 200 + 5]
        rep2.append((src, src + 1_500))
    for i in range(8):
        src = REP4 + 4_000 * i
        for off in (500, 1_000, 2_000):
            s0[src + off:src + off + 150] = s0[src:src + 150]
        if i % 2:
            s0[src + 2_040] = _other(s0[src + 2_040])           # the fourth copy diverges in one base
        sites.append(src + 1_000 + 155)
        rep4.append((src, src + 500, src + 1_000, src + 2_000))
    sites = np.unique(np.array(sites, dtype=np.int64))
    ref = s0[sites]
    alt = ACGT[(CODE[ref] + 1 + np.arange(len(sites)) % 3) % 4]
    s = SnpSet(np.zeros(len(sites), np.int32), sites + 1, ref, alt, np.full(len(sites), 0.6), np.full(len(sites), 0.4), (np.arange(len(sites)) % 3).astype(np.uint8))
    s._with_caf = True
    return g, s, sites, dict(inv=inv, chi=chi, rep2=rep2, rep4=rep4)


def _row(t, L, rev=False, hap=False, subs=(), gates=None, t2=None, junk=(), model=True):
    """One read: window start t in the genome (its chunks cover [t, t + 32 n): a forward read starts at t, a reverse one is the
    reverse complement of [t - (L - 32 n), t + 32 n)); subs: (chunk, offset in the chunk) in the PILE-UP's orientation; gates: chunks
    whose quality character opens the gate, in the orientation of the pass that aligns the read (quality strings are not reversed:
    character j belongs to chunk j of either pass) -- default: the substituted chunks; t2: chunks 2 .. come from t2 + 64 instead;
    junk: chunks replaced by random bases; model: the read lies where _pairs can tell what the rule does with it."""
    subs = tuple(subs)
    return dict(t=int(t), L=L, rev=bool(rev), hap=bool(hap), subs=subs, gates=tuple(sorted({c for c, _ in subs})) if gates is None else tuple(gates), t2=t2, junk=tuple(junk), model=model)


def _make_reads(rng, h, plan, all_high=False):
    bases, quals, lens = [], [], []
    for r in plan:
        L, t = r["L"], r["t"]
        n = LENS[L]
        hp = h[1] if r["hap"] else h[0]
        w = hp[t:t + 32 * n].copy() if t >= 0 else np.concatenate([np.full(-t, ord("A"), np.uint8), hp[0:t + 32 * n]])
        if len(w) < 32 * n:
            w = np.concatenate([w, np.full(32 * n - len(w), ord("A"), np.uint8)])
        if r["t2"] is not None:
            w[64:] = hp[r["t2"] + 64:r["t2"] + 32 * n]
        for c in r["junk"]:
            w[32 * c:32 * c + 32] = synth.random_bases(rng, 32)
        for c, o in r["subs"]:
            w[32 * c + o] = _other(w[32 * c + o])
        tail = L - 32 * n
        if r["rev"]:
            b = _rc(np.concatenate([hp[t - tail:t], w]))
        else:
            b = np.concatenate([w, hp[t + 32 * n:t + 32 * n + tail]])
        assert len(b) == L, r
        q = rng.integers(ord(":"), ord("I") + 1, size=L, dtype=np.uint8)
        if not all_high:
            for c in r["gates"]:
                q[c] = ord("#")
        bases.append(b); quals.append(q); lens.append(L)
    return Reads(np.concatenate(bases), np.concatenate(quals), np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64))


def _plan(rng, sites, cons):
    plan = []
    k = 0
    sparse = sites[(sites >= 2_900) & (sites < 3_000 + 700 * N_SPARSE)]
    # (a) edge reads: every second sparse site at offsets -1, 0, 31, 32 of the gate-open chunk's own window (the chunk that holds the
    # substitution), inside another chunk's window, and just outside either end of the read's window; every length, both strands
    for P in sparse[::2]:
        for L, n in LENS.items():
            for rev in (False, True):
                gc = k % n
                oc = (gc + 1 + k % (n - 1)) % n                                     # another chunk
                for where, t in (("-1", P + 1 - 32 * gc), ("0", P - 32 * gc), ("31", P - 31 - 32 * gc), ("32", P - 32 - 32 * gc), ("other", P - 13 - 32 * oc), ("left", P + 1), ("right", P - 32 * n)):
                    so = 5
                    if where in ("0", "31") and k % 2:                              # the substitution on the site's own base
                        so = int(where)
                    extra = (gc,) if k % 3 else (gc, oc)                            # sometimes a second gate-open chunk, without a substitution
                    plan.append(_row(t, L, rev, k % 4 >= 2, [(gc, so)], gates=extra))
                    k += 1
    # (b) ordinary reads all over the sparse part: a third with a substitution in a gate-open chunk, and any chunk's gate open one time in four
    for _ in range(6_000):
        L = int(rng.choice(list(LENS)))
        n = LENS[L]
        subs = [(int(rng.integers(0, n)), 5)] if rng.random() < 1 / 3 else []
        gates = sorted({c for c, _ in subs} | {c for c in range(n) if rng.random() < 1 / 4})
        plan.append(_row(int(rng.integers(2_500, 100_500)), L, bool(rng.integers(0, 2)), bool(rng.integers(0, 2)), subs, gates=gates))
    # (c) exactly one exact chunk: every other chunk has a substitution and an open gate -- the key is live only through stage B.
    # c1: the site in the exact chunk's own window (chunk 0 exact).  c2: chunk 1 exact, the site in chunk 0's window: chunk 1's entry
    # proves chunks 1 .. n - 1 free, and pruning them would leave the key dead and the site uncounted.
    for P in sparse[1::2][:40]:
        for L in (96, 101, 128, 150):
            n = LENS[L]
            for rev in (False, True):
                plan.append(_row(P - 9, L, rev, k % 2, [(c, 7) for c in range(1, n)]))
                plan.append(_row(P - 20, L, rev, k % 2, [(c, 7) for c in range(n) if c != 1]))
                k += 1
    # (d) inverted repeats: chunk 1 alone is exact, the forward copy is far from any site; then the same reads' reverse complements
    for a, b in cons["inv"]:
        for L in (96, 101, 128):
            n = LENS[L]
            for rev in (False, True):
                plan.append(_row(a, L, rev, False, [(c, 5) for c in range(n) if c != 1], model=False))
                plan.append(_row(a, L, rev, False, [(n - 1, 5)], model=False))
    # (e) chimeras: two keys with two exact chunks each -- a tie, whatever bits their masks carry; with and without open gates
    for a, b in cons["chi"]:
        for rev in (False, True):
            for gates in ((), (1,), (0, 3)):
                plan.append(_row(a, 128, rev, k % 2, [], gates=gates, t2=b, model=False))
                k += 1
    # (f) repeats: reads aimed at every copy, at several offsets into it; the gate of the chunk over the diverged base open, with and
    # without a substitution of its own (a neighbour makes the tie / breaks it), on both strands
    for copies, rl in [(p, 200) for p in cons["rep2"]] + [(m, 150) for m in cons["rep4"]]:
        for c0 in copies:
            for d in (-40, -8, 0, 20, rl - 128, rl - 100):
                for L in (101, 128, 150):
                    n = LENS[L]
                    gc = (40 - d) // 32 if 0 <= 40 - d < 32 * n else k % n           # the chunk over offset 40 of the copy
                    subs = [(gc, (45 - d) % 32)] if k % 3 == 0 else []
                    plan.append(_row(c0 + d, L, k % 2 == 0, k % 4 >= 2, subs, gates=(gc,) if k % 5 else (gc, (gc + 1) % n), model=False))
                    k += 1
    # (g) both ends of the pile-up: reads inside the first and the last 128 positions, and reads that overhang them -- their outer chunks
    # random bases, so that the key lies left of position 0 or the window ends past the last position
    for L in (64, 96, 128, 150):
        n = LENS[L]
        for d in (0, 1, 17, 40, 96, 127):
            for j, gc in enumerate(range(n)):
                plan.append(_row(d, L, False, j % 2, [(gc, 5)], model=False))
                plan.append(_row(GLEN - L - d, L, False, j % 2, [(gc, 5)], model=False))
                if d >= L - 32 * n:
                    plan.append(_row(d, L, True, j % 2, [(gc, 5)], model=False))
                plan.append(_row(GLEN - 32 * n - d, L, True, j % 2, [(gc, 5)], model=False))
        if L in (96, 128):
            for hang in (32, 64):
                plan.append(_row(-hang, L, False, False, [], gates=tuple(range(hang // 32)), junk=tuple(range(hang // 32)), model=False))
                plan.append(_row(GLEN - 32 * n + hang, L, True, False, [], gates=tuple(range(n - hang // 32, n)), junk=tuple(range(n - hang // 32, n)), model=False))
    return plan


def _pairs(c):
    """What the rule does with the gate-open pairs, from where the reads and the sites are.  A modelled read lies in the single-copy
    part: one pass has its key (the forward pass of a forward read; pass 1 of a reverse read, whose forward pass finds nothing), at
    key = window start.  A chunk without a substitution is exact: its 32-mer is the reference's (a single-position entry with bits A
    and B) or carries the donor's alt allele (an SNP-dictionary entry: no bits).  F = the union of vg_quiet_chunks over the reference
    entries.  Pruned: every pair under R1 (pass 1, F full), the pairs of F's chunks under R2 (two exact chunks).  Reads of the
    constructs are not modelled: all their gate-open chunks count, in both passes, into the total only (an upper bound).
    Returns (pruned, kept, total)."""
    pruned = kept = total = 0
    for r in c.plan:
        n = LENS[r["L"]]
        if not r["model"]:
            total += 2 * len(r["gates"])
            continue
        t = r["t"]
        w = (c.h[1] if r["hap"] else c.h[0])[t:t + 32 * n].copy()
        for cc, o in r["subs"]:
            w[32 * cc + o] = _other(w[32 * cc + o])
        exact, F = [], 0
        for cc in range(n):
            seg = slice(t + 32 * cc, t + 32 * cc + 32)
            mine = w[32 * cc:32 * cc + 32]
            if not np.all((mine == c.s0[seg]) | (mine == c.alt[seg])):
                continue                                                        # a substitution: no exact context (a neighbour at most)
            exact.append(cc)
            if np.array_equal(mine, c.s0[seg]):
                kp = t + c.shift + 32 * cc
                assert kp in c.A, r                                             # (single-copy: a single-position entry)
                if c.A[kp]:
                    F |= (2 << cc) - 1
                if c.B[kp]:
                    F |= ((1 << n) - 1) & ~((1 << cc) - 1)
        if not exact:
            continue                                                            # no key in either pass
        full = (1 << n) - 1
        for gc in r["gates"]:
            total += 1
            if (r["rev"] and F == full) or (len(exact) >= 2 and (F >> gc) & 1):
                pruned += 1
            else:
                kept += 1
    return pruned, kept, total


class Case:
    pass


def build_case(d, seed=909, with_oracle=True):
    """Genome, index, reads and the oracle's counters (with the gates as given, and with every quality character high)."""
    rng = np.random.default_rng(seed)
    c = Case()
    g, s, sites, cons = _genome_and_sites(rng)
    synth.write_fasta(os.path.join(d, "ref.fa"), g)
    synth.write_vcf(os.path.join(d, "snps.vcf"), g, s)
    subprocess.check_call([BIN, "index", "ref.fa", "snps.vcf", "idx"], cwd=d, env=dict(os.environ, VARGENO_NO_LITE="1"), stdout=subprocess.DEVNULL)
    c.prefix = os.path.join(d, "idx")
    c.s0 = g.seqs[0]
    c.h = synth.haplotypes(g, s)[:2]
    c.alt = c.s0.copy()
    c.alt[sites] = s.alt                                                        # the genome with every alt allele
    c.plan = _plan(rng, sites, cons)
    c.reads = _make_reads(np.random.default_rng(seed + 2), c.h, c.plan)
    high = _make_reads(np.random.default_rng(seed + 2), c.h, c.plan, all_high=True)
    assert np.array_equal(c.reads.bases, high.bases)
    ox = O.OracleIndex.load(c.prefix)
    ox.process(c.reads.bases, c.reads.quals, c.reads.offsets, nthreads=8)
    c.so = ox.sites()
    c.want = ox.stats.as_dict()
    oh = O.OracleIndex.load(c.prefix)
    oh.process(high.bases, high.quals, high.offsets, nthreads=8)
    sh = oh.sites()
    c.gate_sites = int(((sh["ref_cnt"] != c.so["ref_cnt"]) | (sh["alt_cnt"] != c.so["alt_cnt"])).sum())
    sp = np.sort(c.so["pos"].astype(np.int64))
    assert len(sp) == len(sites)
    c.shift = int(sp[0] - sites[0])
    assert np.array_equal(sp, sites + c.shift)
    rd = index_io.read_ref_dict(c.prefix + ".ref.dict")
    sd = index_io.read_snp_dict(c.prefix + ".snp.dict")
    single = (rd["ref_amb"] == 0) & (rd["ref_pos"] != POS_AMBIGUOUS)
    named = [rd["ref_pos"][single], rd["ref_aux"][rd["ref_aux"] != 0], sd["snp_pos"][(sd["snp_amb"] == 0) & (sd["snp_pos"] != POS_AMBIGUOUS)], sd["snp_aux_pos"][sd["snp_aux_pos"] != 0]]
    c.pile_len = int(max(int(x.max()) for x in named if len(x))) + 64
    bits = np.zeros(c.pile_len + 1, np.int64)
    bits[sp] = 1
    cum = np.concatenate([[0], np.cumsum(bits)])
    clear = lambda a, b: cum[np.clip(b, 0, c.pile_len)] - cum[np.clip(a, 0, c.pile_len)] == 0       # no site in [a, b), element-wise
    kp = rd["ref_pos"][single].astype(np.int64)
    c.A = dict(zip(kp.tolist(), ((kp + 32 <= c.pile_len) & clear(kp - 96, kp + 32)).tolist()))
    c.B = dict(zip(kp.tolist(), ((kp + 128 <= c.pile_len) & clear(kp, kp + 128)).tolist()))
    c.n_entries = len(rd["ref_kmer"]) + len(sd["snp_kmer"])
    return c


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """Made once, read by every test, never changed."""
    return build_case(str(tmp_path_factory.mktemp("prune")))


def test_parity_and_the_case_is_not_vacuous(case):
    """Both builds equal the oracle, counters and event counts (the counting build runs every pair: its events are priced).  The rules
    prune >= 40 % of the gate-open pairs of passes that have a key and leave >= 20 % in place (lower bounds: the constructs' reads count
    into the total only); the gates matter at >= 50 sites."""
    c = case
    pruned, kept, total = _pairs(c)
    print("gate-open pairs: pruned %d, kept %d, of at most %d; sites that depend on the gates: %d; reads %d" % (pruned, kept, total, c.gate_sites, c.reads.n))
    assert total > 3_000 and pruned >= 0.40 * total and kept >= 0.20 * total, (pruned, kept, total)
    assert c.gate_sites >= 50, c.gate_sites
    views, qb = QW._run(c, c.reads)
    assert "dx" in views and qb is not None and 0 < qb["both"] < min(qb["a"], qb["b"])


@pytest.mark.parametrize("knob", ["VG_NO_QUIET=1", "VG_NO_DIRECT=1", "VG_NO_MX=1", "VG_DX_BITS=18", "VG_PACK_OVERLAP=0", "VG_FORCE_GENERIC=1+VG_SCRATCH_CAP=3+VG_SCRATCH_KCAP=2"])
def test_same_counters_under_every_knob(case, monkeypatch, knob):
    """The bits left clear (the rule is off), the layouts that never see them, the direct table of fewer than 2^32 buckets (the other
    instantiation of the kernel), the pack kernel never beside the wave kernel, and the lane machine with a tiny first scratch."""
    c = case
    for kv in knob.split("+"):
        monkeypatch.setenv(*kv.split("="))
    views, qb = QW._run(c, c.reads)
    if knob == "VG_NO_QUIET=1":
        assert qb == dict(a=0, b=0, both=0, entries=c.n_entries)
    elif knob in ("VG_NO_DIRECT=1", "VG_NO_MX=1"):
        assert "dx" not in views and qb is None
    else:
        assert "dx" in views and qb["both"] > 0


def test_sample_planes(case):
    """Two samples on one index, two batches each in flight together: per-plane counters equal the oracle's on each sample alone."""
    c = case
    o = c.reads.offsets.astype(np.int64)
    idx = np.arange(c.reads.n)

    def take(sel):
        pick = np.concatenate([np.arange(o[i], o[i + 1]) for i in sel])
        return Reads(c.reads.bases[pick], c.reads.quals[pick], np.concatenate([[0], np.cumsum((o[1:] - o[:-1])[sel])]).astype(np.uint64))
    samples = [[take(idx[idx % 4 == 0]), take(idx[idx % 4 == 1])], [take(idx[idx % 4 == 2]), take(idx[idx % 4 == 3])]]
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

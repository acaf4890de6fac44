"""Sample planes: several samples genotyped against ONE resident index (vg_samples_reserve / vg_sample_select ...).  A batch
counts into the plane of the sample that was selected when it was handed over, through every tier and every input form; batches of
different samples are in flight together.  Bit-exact against the CPU oracle run on each sample's reads alone.

The samples are the three thirds of F-tiny's 4 000 reads.  On the oracle each third leaves 1 854-1 908 of the 2 928 sites non-zero
and any two thirds differ at 1 977-1 995 sites (checked below), so a batch counted into the wrong plane cannot pass."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import BIN
from oracle import oracle as O
from vargeno_amd._lib import VgError
from vargeno_amd.api import GenoIndex, HostPacker, ReadStore, all_reduce_devices, gate_words
from vargeno_amd.synth import Reads

pytestmark = pytest.mark.gpu

CMP_STATS = ["reads", "reads_n", "reads_invalid", "passes", "passes_ok", "chunks", "gate_open", "refbf_pos", "snpbf_pos",
             "large_block", "ref_query", "snp_query", "ref_probe", "snp_probe", "scan_ref", "scan_snp", "scan_oob",
             "aux_ref", "aux_snp", "site_test", "ctx", "walks", "incr", "ingest_bytes"]
THIRDS = [(0, 1333), (1333, 2666), (2666, 4000)]
NB = 5                                              # batches per sample


def _oracle(prefix, r):
    ox = O.OracleIndex.load(prefix)
    ox.process(r.bases, r.quals, r.offsets)
    so = ox.sites()
    return so["ref_cnt"].copy(), so["alt_cnt"].copy(), ox.stats.as_dict()


def _take(r, idx):
    """The reads idx of r, in that order, as a batch of their own."""
    o = r.offsets.astype(np.int64)
    lens = (o[1:] - o[:-1])[idx]
    pick = np.concatenate([np.arange(o[i], o[i + 1]) for i in idx]) if len(idx) else np.zeros(0, np.int64)
    return Reads(r.bases[pick], r.quals[pick], np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64))


def _fastq(r):
    o = r.offsets.astype(np.int64)
    out = []
    for i in range(r.n):
        out += [b"@r%d\n" % i, r.bases[o[i]:o[i + 1]].tobytes(), b"\n+\n", r.quals[o[i]:o[i + 1]].tobytes(), b"\n"]
    return b"".join(out)


def _batches(r, n=NB):
    cuts = [r.n * i // n for i in range(n + 1)]
    return [r.slice(a, b) for a, b in zip(cuts[:-1], cuts[1:])]


@pytest.fixture(scope="module")
def thirds(ftiny_dir, ftiny_reads):
    """The three samples, and the oracle on each of them alone: computed once, read by every test, never changed."""
    prefix = os.path.join(ftiny_dir, "idx")
    parts = [ftiny_reads.slice(a, b) for a, b in THIRDS]
    want = [_oracle(prefix, p) for p in parts]
    for rc, ac, _ in want:
        assert 1854 <= int(((rc != 0) | (ac != 0)).sum()) <= 1908
    for i in range(3):
        for j in range(i):
            assert 1977 <= int(((want[i][0] != want[j][0]) | (want[i][1] != want[j][1])).sum()) <= 1995
    total = {k: sum(w[2][k] for w in want) for k in CMP_STATS}
    return prefix, parts, want, total


def _same(gx, s, want, what=""):
    rc, ac = gx.counts(sample=s)
    assert np.array_equal(rc, want[s][0]) and np.array_equal(ac, want[s][1]), (what, "sample %d" % s, int((rc != want[s][0]).sum()), int((ac != want[s][1]).sum()))


FORMS = ["submit", "process_device", "process_device_gated", "submit_packed", "submit_store", "fastq_stream", "fastq_stream_host2"]


def _feed_interleaved(gx, parts, form):
    """Every sample's reads in NB batches, round robin over the samples, select in between, no synchronisation (the stream forms: one
    stream per sample, another sample selected between its pushes).  Returns what must stay alive until the next synchronisation."""
    keep = []
    if form.startswith("fastq_stream"):
        for s in (1, 2, 0):
            text = _fastq(parts[s])
            cuts = [len(text) * i // NB for i in range(NB + 1)]                 # cut anywhere

            def chunks():
                for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
                    if i:
                        gx.select((s + i) % 3)                                  # does not move the open stream
                    yield text[a:b]

            gx.select(s)
            n, used, _, refused = gx.fastq_stream(chunks(), host_threads=2 if form.endswith("host2") else None)
            assert (n, used, refused) == (parts[s].n, len(text), False)
        return keep
    import torch

    dev = torch.device("cuda", 0)
    pk = HostPacker(1)
    per = [_batches(p) for p in parts]
    for i in range(NB):
        for s in range(3):
            b = per[s][i]
            gx.select(s)
            if form == "submit":
                gx.submit(b.bases, b.quals, b.offsets)
            elif form in ("process_device", "process_device_gated"):
                tb, tq = torch.from_numpy(b.bases.copy()).to(dev), torch.from_numpy(b.quals.copy()).to(dev)
                to = torch.from_numpy(b.offsets.astype(np.int64)).to(dev)
                if form == "process_device":
                    torch.cuda.synchronize()
                    gx.process_device(tb, tq, to, b.n)
                    keep += [tb, tq, to]
                else:
                    gw = gate_words(tq, to)
                    torch.cuda.synchronize()
                    gx.process_device_gated(tb, gw, to, b.n)
                    keep += [tb, gw, to]
            else:
                pk.begin()
                k, m, o, bad = pk.push(_fastq(b))
                assert len(m) == b.n and bad == 0
                if form == "submit_packed":
                    gx.submit_packed(k, m, o)
                else:
                    st = ReadStore(0, 4 << 20)
                    st.push(k, m, o)
                    gx.submit_store(st)
                    keep.append(st)
    pk.close()
    return keep


def _interleaved(prefix, parts, want, total, form):
    with GenoIndex.open(prefix) as gx:
        gx.reserve_samples(3)
        assert gx.num_samples == 3
        for stats in (True, False):                     # the counting build, the timed build
            gx.reset()
            gx.set_stats(stats)
            keep = _feed_interleaved(gx, parts, form)
            for s in range(3):
                _same(gx, s, want, (form, stats))
            st = gx.stats()
            del keep
            assert st["reads_invalid"] == 0
            if stats:
                assert st["reads"] == 4000
                diff = {k: (st[k], total[k]) for k in CMP_STATS if st[k] != total[k]}
                print("interleaved %s: event counts that differ from the oracle's sum over the thirds: %s" % (form, diff or "none"))
                assert not diff, (form, diff)


@pytest.mark.parametrize("form", FORMS)
def test_interleaved_samples_count_into_their_own_planes(thirds, form):
    _interleaved(*thirds, form)


def test_a_handle_that_never_reserves_behaves_as_before(thirds, ftiny_reads):
    prefix, parts, want, _ = thirds
    r = ftiny_reads
    rc0, ac0, _ = _oracle(prefix, r)
    with GenoIndex.open(prefix) as gx:
        assert gx.num_samples == 1 and gx.selected == 0
        with pytest.raises(VgError) as e:
            gx.select(1)
        assert e.value.code == -1 and gx.selected == 0
        gx.submit(r.bases, r.quals, r.offsets)
        rc, ac = gx.counts()
        assert np.array_equal(rc, rc0) and np.array_equal(ac, ac0)
        gx.reserve_samples(2)                            # plane 0 keeps its counts, plane 1 starts at zero
        assert gx.num_samples == 2
        rc, ac = gx.counts(sample=0)
        assert np.array_equal(rc, rc0) and np.array_equal(ac, ac0)
        rc1, ac1 = gx.counts(sample=1)
        assert not rc1.any() and not ac1.any()
        with pytest.raises(VgError) as e:
            gx.reserve_samples(1)
        assert e.value.code == -1 and gx.num_samples == 2
        for bad in (0, 65536):
            with pytest.raises(VgError) as e:
                gx.reserve_samples(bad)
            assert e.value.code == -1
        gx.reserve_samples(2)                            # the size it has: nothing to do
        assert gx.num_samples == 2


def test_reset_of_one_sample_of_all_and_the_clamp(thirds):
    prefix, parts, want, _ = thirds
    with GenoIndex.open(prefix) as gx:
        gx.set_stats(False)
        gx.reserve_samples(3)
        for s in range(3):
            gx.select(s)
            gx.submit(parts[s].bases, parts[s].quals, parts[s].offsets)
        gx.reset_sample(1)
        rc, ac = gx.counts(sample=1)
        assert not rc.any() and not ac.any()
        _same(gx, 0, want)
        _same(gx, 2, want)
        gx.reset()
        for s in range(3):
            rc, ac = gx.counts(sample=s)
            assert not rc.any() and not ac.any(), s
        # 40 x coverage of sample 0 saturates where the oracle's 6-bit counters do; sample 1, given its third once, is untouched
        ox = O.OracleIndex.load(prefix)
        for i in range(40):
            gx.select(0)
            gx.submit(parts[0].bases, parts[0].quals, parts[0].offsets)
            ox.process(parts[0].bases, parts[0].quals, parts[0].offsets)
            if i == 20:
                gx.select(1)
                gx.submit(parts[1].bases, parts[1].quals, parts[1].offsets)
        so = ox.sites()
        rc, ac = gx.counts(sample=0)
        assert np.array_equal(rc, so["ref_cnt"]) and np.array_equal(ac, so["alt_cnt"])
        assert rc.max() == 63 and np.array_equal(rc == 63, so["ref_cnt"] == 63)
        _same(gx, 1, want)
        rc2, ac2 = gx.counts(sample=2)
        assert not rc2.any() and not ac2.any()


@pytest.fixture(scope="module")
def manykeys(tmp_path_factory):
    """synth.f_manykeys (48 reads that go all the way down to the lane machine) as two samples, its index built once, the oracle on
    each sample alone."""
    from vargeno_amd import synth

    g, s, r = synth.f_manykeys()
    d = str(tmp_path_factory.mktemp("manykeys"))
    synth.write_fasta(os.path.join(d, "ref.fa"), g)
    synth.write_vcf(os.path.join(d, "snps.vcf"), g, s)
    subprocess.check_call([BIN, "index", "ref.fa", "snps.vcf", "idx"], cwd=d, env=dict(os.environ, VARGENO_NO_LITE="1"), stdout=subprocess.DEVNULL)
    prefix = os.path.join(d, "idx")
    n_ord = r.n - 48                                     # (the 48 many-key reads are the fixture's last)
    many = np.arange(n_ord, r.n)
    idx = [np.concatenate([many[:20], np.arange(0, n_ord, 2)]), np.concatenate([many[20:], np.arange(1, n_ord, 2)])]
    samples = [_take(r, i) for i in idx]
    want = [_oracle(prefix, p) for p in samples]
    assert any((want[0][0] != want[1][0]) | (want[0][1] != want[1][1]))
    total = {k: want[0][2][k] + want[1][2][k] for k in CMP_STATS}
    yield prefix, samples, want, total
    shutil.rmtree(d, ignore_errors=True)                 # (an index carries 1.3 GB of bit-vector files whatever the genome)


@pytest.mark.parametrize("knob", [{}, {"VG_LATE_READS": "2"}, {"VG_NO_LATE_STORE": "1"}, {"VG_FORCE_GENERIC": "1"}], ids=lambda k: "+".join("%s=%s" % kv for kv in k.items()) or "default")
def test_the_tiers_below_the_wave_kernel_count_into_the_batch_s_plane(manykeys, monkeypatch, knob):
    """The deep tier's leftovers: the late store (reads of both samples in ONE lane-machine run, each tagged with its plane), the
    per-batch lane launch for what the store does not take, and the lane machine alone."""
    prefix, samples, want, total = manykeys
    for k, v in knob.items():
        monkeypatch.setenv(k, v)
    # three batches per sample: the many-key reads (20 / 28, each sample's first) in the first, the ordinary reads in two more
    cuts = [[0, 20, 20 + (samples[0].n - 20) // 2, samples[0].n], [0, 28, 28 + (samples[1].n - 28) // 2, samples[1].n]]
    with GenoIndex.open(prefix) as gx:
        gx.reserve_samples(2)
        for stats in (True, False):
            gx.reset()
            gx.set_stats(stats)
            for i in range(3):
                for s in range(2):
                    b = samples[s].slice(cuts[s][i], cuts[s][i + 1])
                    gx.select(s)
                    gx.submit(b.bases, b.quals, b.offsets)
                if i == 1:
                    gx.sync()                            # (one run of the store in the middle of the job)
            for s in range(2):
                _same(gx, s, want, (knob, stats))
            st = gx.stats()
            assert st["overflow_deep"] > 2, st["overflow_deep"]
            if stats:
                diff = {k: (st[k], total[k]) for k in CMP_STATS if st[k] != total[k]}
                assert not diff, (knob, diff)


@pytest.mark.parametrize("knob", ["VG_NO_MX", "VG_DX_BITS=16", "VG_PACK_OVERLAP", "VG_NO_INGEST_STREAM"])
def test_interleaved_samples_under_other_layouts(thirds, monkeypatch, knob):
    """The kernel of an index without the merged view, the instantiation for a small direct table, the pack kernel on the ingest
    stream, everything on the main stream."""
    monkeypatch.setenv(*(knob.split("=") if "=" in knob else (knob, "1")))
    _interleaved(*thirds, "submit")


def test_replicas_sum_one_sample_at_a_time(thirds):
    prefix, parts, want, _ = thirds
    with GenoIndex.open(prefix) as ga, GenoIndex.open(prefix) as gb:     # (two replicas that share the device: F-tiny's index is small)
        for gx in (ga, gb):
            gx.set_stats(False)
            gx.reserve_samples(2)
        for s in range(2):                               # each sample's reads split between the handles, the samples interleaved
            half = parts[s].n // 2 + 7 * s
            for gx, (lo, hi) in ((ga, (0, half)), (gb, (half, parts[s].n))):
                b = parts[s].slice(lo, hi)
                gx.select(s)
                gx.submit(b.bases, b.quals, b.offsets)
        ga.select(0)
        gb.select(1)
        with pytest.raises(VgError) as e:
            all_reduce_devices([ga, gb])
        assert e.value.code == -1
        for s in (0, 1):
            ga.select(s)
            gb.select(s)
            all_reduce_devices([ga, gb])
            for gx in (ga, gb):
                rc, ac = gx.counts()
                assert np.array_equal(rc, want[s][0]) and np.array_equal(ac, want[s][1]), s


def test_invalid_reads_are_counted_per_sample(thirds):
    prefix, parts, want, _ = thirds
    bad = Reads(parts[1].bases.copy(), parts[1].quals, parts[1].offsets)
    o = bad.offsets.astype(np.int64)
    i = next(k for k in range(bad.n) if o[k + 1] - o[k] >= 64 and not np.isin(bad.bases[o[k]:o[k + 1]], [ord("N"), ord("n")]).any())
    bad.bases[o[i] + 5] = ord("X")
    with GenoIndex.open(prefix) as gx:
        gx.set_stats(False)
        gx.reserve_samples(2)
        for b0, b1 in zip(_batches(parts[0], 2), _batches(bad, 2)):
            gx.select(0)
            gx.submit(b0.bases, b0.quals, b0.offsets)
            gx.select(1)
            gx.submit(b1.bases, b1.quals, b1.offsets)
        assert gx.invalid_reads(1) == 1 and gx.invalid_reads(0) == 0
        assert gx.stats()["reads_invalid"] == 1
        _same(gx, 0, want)
        # the packed route finds such a read on the host: the same count, the same sample
        gx.reset()
        pk = HostPacker(1)
        pk.begin()
        k, m, off, n_bad = pk.push(_fastq(bad))
        pk.close()
        assert n_bad == 1
        gx.select(1)
        gx.submit_packed(k, m, off)
        assert gx.invalid_reads(1) == 1 and gx.invalid_reads(0) == 0 and gx.stats()["reads_invalid"] == 1
        gx.reset_sample(1)
        assert gx.invalid_reads(1) == 0
        with pytest.raises(VgError) as e:
            gx.invalid_reads(2)
        assert e.value.code == -1


def test_every_plane_is_counted_in_the_device_bytes(thirds):
    """A plane is one block of 24 bytes per site + 16 (8 per site of exact sums, 16 per site + 16 of base-indexed counters), taken as
    it is: nothing is rounded, the handle's tables have their full width from the start."""
    prefix = thirds[0]
    with GenoIndex.open(prefix) as gx:
        n, b1 = gx.num_sites, gx.device_bytes
        gx.reserve_samples(2)
        assert gx.device_bytes - b1 == 24 * n + 16
        gx.reserve_samples(7)
        assert gx.device_bytes - b1 == 6 * (24 * n + 16)
        gx.reserve_samples(7)
        assert gx.device_bytes - b1 == 6 * (24 * n + 16)

"""Deep sums and high plane numbers.  Three things behind every `cohort` / `joint` run that the rest of the suite cannot see:

* the host branch of vg_sample_calls_fetch (escaped sites: vg_clamp_counters on the selected plane, the two clamped columns fetched,
  resolve_calls with libm) -- F-tiny's own frequencies never reach it (tests/test_deep_planes_cpu.py holds that), seeded frequency
  bytes do, at some 300 sites a call;
* exact sums far above the 6-bit cap -- 64, 255 / 256, 65 535 / 65 536, 2^31 (where a signed compare flips), 2^32 - 1 -- through a
  plane, into counts() and calls(), and uint8 counters above 63 into vg_call_device;
* plane numbers above 255: the late store's 16-bit tag, a fold over 300 dirty planes, the device's plane table filled piece by
  piece as the handle grows, the re-upload of the dirty list when its members change and its length does not.

Expected values: oracle.oracle and numpy (tests/deep_plane_cases.py).  Sums are written through counts_tensor(): select, copy the
int32 view in, torch.cuda.synchronize() before the next library call (torch and the handle use different streams)."""
import os

import numpy as np
import pytest

import deep_plane_cases as DP
from oracle import oracle as O
from test_gpu_samples import manykeys  # noqa: F401  (the fixture: synth.f_manykeys as two samples, its index, the oracle on each)
from vargeno_amd.api import GenoIndex, call_device

pytestmark = pytest.mark.gpu

NP = DP.N_PLANES


def _write(gx, s, sums):
    """The plane s takes `sums` (uint32[2 n]) as its exact sums; the selection is put back."""
    import torch

    before = gx.selected
    gx.select(s)
    t = gx.counts_tensor()
    assert t.dtype == torch.int32 and t.numel() == len(sums)
    t.copy_(torch.from_numpy(np.ascontiguousarray(sums, np.uint32).view(np.int32)))
    torch.cuda.synchronize()
    gx.select(before)


def _raw(gx, s):
    """The exact sums of plane s, uint32[2 n]; the selection is put back."""
    before = gx.selected
    gx.select(s)
    out = gx.counts_tensor().cpu().numpy().view(np.uint32).copy()
    gx.select(before)
    return out


def _eq_counts(gx, s, want, what=""):
    rc, ac = gx.counts(sample=s)
    assert np.array_equal(rc, want[0]) and np.array_equal(ac, want[1]), (what, "plane %d" % s, int((rc != want[0]).sum()), int((ac != want[1]).sum()))


def _eq_calls(got, want, what=""):
    assert got[0].dtype == np.uint8 and got[1].dtype == np.int32
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (what, int((got[0] != want[0]).sum()), int((got[1] != want[1]).sum()))


# ---- B. deep sums through a plane ---------------------------------------------------------------------------------------------
class Seeded:
    pass


@pytest.fixture(scope="module")
def seeded(ftiny_dir):
    """The index with seeded frequencies: its arrays, the oracle on them, the two arrays of sums and the oracle's calls on each --
    computed once, read by every test, never changed."""
    z = Seeded()
    z.prefix = os.path.join(ftiny_dir, "idx")
    z.arrays = DP.freq_arrays(z.prefix)
    z.ox = O.OracleIndex.from_arrays(z.arrays)
    z.sites = z.ox.sites()
    z.n = len(z.sites["pos"])
    z.rf, z.af = z.sites["ref_freq"], z.sites["alt_freq"]
    z.sums, z.want = {}, {}
    for seed in (DP.SUMS_SEED, DP.OTHER_SEED):
        z.sums[seed] = DP.deep_sums(z.n, seed)
        gt, gq, conf = DP.oracle_calls(*DP.clamp(z.sums[seed]), z.rf, z.af)
        _, forced, near = DP.conditions(gt, conf, 1e-5)
        assert forced >= 100
        z.want[seed] = (gt, gq, forced, near)
    return z


@pytest.fixture(scope="module")
def deep_gx(seeded):
    """ONE handle on the seeded index with 300 planes for the tests of part B: each of them writes the planes it reads."""
    with GenoIndex.create(seeded.arrays) as gx:
        sg = gx.sites()
        for k in ("pos", "ref_base", "alt_base", "ref_freq", "alt_freq"):                   # (the last-writer-wins rule of the frequencies)
            assert np.array_equal(sg[k], seeded.sites[k]), k
        gx.reserve_samples(NP)
        assert gx.num_samples == NP and gx.num_sites == seeded.n
        yield gx


@pytest.mark.parametrize("s", [0, NP - 1])
def test_counts_of_deep_sums_are_clamped(seeded, deep_gx, s):
    gx = deep_gx
    sums = seeded.sums[DP.SUMS_SEED]
    gx.select(5)
    _write(gx, s, sums)
    _eq_counts(gx, s, DP.clamp(sums))
    assert gx.selected == 5
    assert np.array_equal(_raw(gx, s), sums)                                               # ... and the sums themselves are left as they were


@pytest.mark.parametrize("s", [0, NP - 1])
def test_calls_on_deep_sums(seeded, deep_gx, s):
    gx = deep_gx
    gt, gq, forced, near = seeded.want[DP.SUMS_SEED]
    _write(gx, 0, seeded.sums[DP.OTHER_SEED])                                              # (plane 0 is the handle's first counter array)
    _write(gx, s, seeded.sums[DP.SUMS_SEED])
    gx.select(1)
    got = gx.calls(sample=s)
    _eq_calls(got, (gt, gq), "plane %d" % s)
    assert int((got[1] == DP.INT_MIN).sum()) == forced                                     # the reference's INT_MIN, from the host branch
    print("plane %d: last_escaped %d, forced by the oracle's confidence %d, within 1e-5 of an integer %d" % (s, gx.last_escaped, forced, near))
    assert forced <= gx.last_escaped <= forced + near
    assert gx.selected == 1


def test_calls_of_another_plane_leave_the_selection_alone(seeded, deep_gx):
    """Plane 7 is selected and holds other sums, plane 0 holds nothing: both launches of the host branch must take plane 299."""
    gx = deep_gx
    a, b = seeded.want[DP.SUMS_SEED], seeded.want[DP.OTHER_SEED]
    gx.reset_sample(0)
    _write(gx, 7, seeded.sums[DP.OTHER_SEED])
    _write(gx, NP - 1, seeded.sums[DP.SUMS_SEED])
    gx.select(7)
    _eq_calls(gx.calls(sample=NP - 1), a[:2], "plane 299 while 7 is selected")
    assert a[2] <= gx.last_escaped <= a[2] + a[3]
    assert gx.selected == 7
    _eq_calls(gx.calls(), b[:2], "plane 7, the selected one")
    assert b[2] <= gx.last_escaped <= b[2] + b[3]
    _eq_counts(gx, 7, DP.clamp(seeded.sums[DP.OTHER_SEED]))
    _eq_counts(gx, NP - 1, DP.clamp(seeded.sums[DP.SUMS_SEED]))


def test_a_second_call_returns_the_same_and_takes_no_memory(seeded, deep_gx):
    gx = deep_gx
    gt, gq, forced, near = seeded.want[DP.SUMS_SEED]
    _write(gx, 130, seeded.sums[DP.SUMS_SEED])
    gx.select(130)
    first = gx.calls()
    esc, held = gx.last_escaped, gx.device_bytes
    second = gx.calls()
    _eq_calls(first, (gt, gq))
    _eq_calls(second, (gt, gq))
    assert gx.last_escaped == esc and gx.device_bytes == held
    assert np.array_equal(_raw(gx, 130), seeded.sums[DP.SUMS_SEED])


def test_a_fold_on_top_of_deep_sums(seeded, deep_gx, ftiny_reads):
    """60 everywhere in plane 256, then a third of F-tiny's reads: the fold adds to the exact sums, the clamp and the caller see
    60 + count."""
    gx = deep_gx
    r = ftiny_reads.slice(0, 1333)
    oc = np.stack(DP.oracle_counts(seeded.ox, r), axis=1).reshape(-1).astype(np.uint32)    # interleaved as a plane is
    assert int((oc != 0).sum()) > 1500 and oc.max() < DP.CAP
    base = np.full(2 * seeded.n, 60, np.uint32)
    want = DP.clamp(base + oc)
    assert int((want[0] == DP.CAP).sum()) > 100 and int((want[1] == DP.CAP).sum()) > 50    # (sites reach the cap, most do not)
    gt, gq, conf = DP.oracle_calls(*want, seeded.rf, seeded.af)
    _, forced, near = DP.conditions(gt, conf, 1e-5)
    try:
        for stats in (False, True):                     # the timed build (base-indexed counters, folded into the sums), the counting build
            gx.set_stats(stats)
            _write(gx, 256, base)
            _write(gx, 255, base)
            gx.select(256)
            gx.submit(r.bases, r.quals, r.offsets)
            gx.select(0)
            _eq_counts(gx, 256, want, stats)
            _eq_calls(gx.calls(sample=256), (gt, gq), stats)
            assert forced <= gx.last_escaped <= forced + near
            raw = _raw(gx, 256)
            assert np.array_equal(raw[oc < DP.CAP], (base + oc)[oc < DP.CAP]), stats
            assert np.array_equal(_raw(gx, 255), base), stats                              # the neighbour took nothing
    finally:
        gx.set_stats(True)


def test_call_device_clamps_u8_counters_above_the_cap():
    rc, ac, rf, af = DP.u8_case()
    gt, gq, conf = DP.oracle_calls(np.minimum(rc, DP.CAP), np.minimum(ac, DP.CAP), rf, af)
    _, forced, near = DP.conditions(gt, conf, 1e-5)
    g_gt, g_gq, esc = call_device(rc, ac, rf, af)
    _eq_calls((g_gt, g_gq), (gt, gq))
    print("n_escaped:", esc, "forced by the oracle's confidence:", forced, "within 1e-5 of an integer:", near)
    assert forced >= 100 and forced <= esc <= forced + near


# ---- C. high plane numbers ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dealt(ftiny_dir, ftiny_reads):
    """F-tiny's reads dealt round robin to 300 planes, and the oracle on every plane's reads alone (one loaded index, reset in
    between)."""
    prefix = os.path.join(ftiny_dir, "idx")
    ox = O.OracleIndex.load(prefix)
    per = DP.round_robin(ftiny_reads)
    want = [DP.oracle_counts(ox, p) for p in per]
    assert all(w[0].any() or w[1].any() for w in want)
    return prefix, ox, per, want


def test_300_dirty_planes_in_one_fold(dealt, ftiny_reads):
    prefix, _, per, want = dealt
    r = ftiny_reads
    with GenoIndex.open(prefix) as one:
        one.submit(r.bases, r.quals, r.offsets)
        all_raw = _raw(one, 0)
    assert all_raw.max() < DP.CAP
    with GenoIndex.open(prefix) as gx:
        gx.reserve_samples(NP)
        for stats in (False, True):                     # the timed build, whose base-indexed counters the fold adds up; the counting build
            gx.reset()
            gx.set_stats(stats)
            for s in range(NP):                                                            # no synchronisation until every plane is dirty
                gx.select(s)
                gx.submit(per[s].bases, per[s].quals, per[s].offsets)
            total = np.zeros(2 * gx.num_sites, np.uint64)
            for s in range(NP):
                _eq_counts(gx, s, want[s], stats)
                total += _raw(gx, s)
            assert np.array_equal(total, all_raw.astype(np.uint64)), stats
            if stats:
                assert gx.stats()["reads"] == r.n


def test_a_handle_that_grows_between_batches(dealt):
    """1 -> 3 -> 257 -> 300 planes between batches that are already counted: the device's table of planes is filled piece by piece."""
    prefix, _, per, want = dealt
    fed = {}
    with GenoIndex.open(prefix) as gx:
        n, b1 = gx.num_sites, gx.device_bytes
        zero = np.zeros(n, np.uint8)
        gx.set_stats(False)                                                                # the timed build: every batch is folded

        def feed(s, k):                                                                    # plane s takes the reads dealt to plane k
            gx.select(s)
            gx.submit(per[k].bases, per[k].quals, per[k].offsets)
            fed[s] = want[k]

        def check(size):
            assert gx.num_samples == size and gx.device_bytes - b1 == (size - 1) * (24 * n + 16)
            for s in range(size):
                _eq_counts(gx, s, fed.get(s, (zero, zero)), "at %d planes" % size)

        feed(0, 100)
        for size, planes in ((3, (2,)), (257, (1, 255, 256)), (NP, (NP - 1, 257, 3))):
            gx.reserve_samples(size)
            check(size)                                                                    # earlier planes keep their counts, new ones start at zero
            for s in planes:
                feed(s, (11 + 7 * s) % NP)
        check(NP)
        for s in range(NP):
            if s not in fed:
                assert not _raw(gx, s).any(), s


def test_dirty_sets_of_one_length_with_other_members(dealt):
    """{3}, {4}, {3, 4}, {4}, {3}: the list of dirty planes goes up again when its members change, not only when its length does."""
    prefix, ox, per, _ = dealt
    rounds = [(3,), (4,), (3, 4), (4,), (3,)]
    got = {3: [], 4: []}
    with GenoIndex.open(prefix) as gx:
        gx.reserve_samples(6)
        gx.set_stats(False)                                                                # the timed build: the counting build folds nothing
        zero = np.zeros(gx.num_sites, np.uint8)
        k = 0
        for planes in rounds:
            for s in planes:
                gx.select(s)
                gx.submit(per[k].bases, per[k].quals, per[k].offsets)
                got[s].append(k)
                k += 1
            gx.sync()
            for s in (3, 4):
                if got[s]:
                    reads = DP.take_many([per[i] for i in got[s]])
                    _eq_counts(gx, s, DP.oracle_counts(ox, reads), "after %r" % (planes,))
                else:
                    _eq_counts(gx, s, (zero, zero), "after %r" % (planes,))
            for s in (0, 2, 5):
                _eq_counts(gx, s, (zero, zero), "after %r" % (planes,))


@pytest.mark.parametrize("pa,pb,knob", [(256, 1, {}), (256, 1, {"VG_LATE_READS": "2"}), (256, 1, {"VG_NO_LATE_STORE": "1"}), (NP - 1, 257, {}), (1, 256, {})],
                         ids=lambda v: ("+".join("%s=%s" % kv for kv in v.items()) or "default") if isinstance(v, dict) else str(v))
def test_the_late_store_above_plane_255(manykeys, monkeypatch, pa, pb, knob):  # noqa: F811
    """The many-key reads go through the late store with a plane number that does not fit a byte: they must land in their sample's
    plane -- an 8-bit tag would put those of plane 256 into plane 0 -- and nowhere else.  Of the reads that reach the store only
    sample B's move counters (two sites), so the placement with B on 256 is the one that sees such a tag at plane 256 itself."""
    prefix, samples, want, total = manykeys
    for k, v in knob.items():
        monkeypatch.setenv(k, v)
    cuts = [[0, 20, 20 + (samples[0].n - 20) // 2, samples[0].n], [0, 28, 28 + (samples[1].n - 28) // 2, samples[1].n]]
    plane = (pa, pb)
    with GenoIndex.open(prefix) as gx:
        gx.reserve_samples(NP)
        for stats in (True, False):
            gx.reset()
            gx.set_stats(stats)
            for i in range(3):
                for s in range(2):
                    b = samples[s].slice(cuts[s][i], cuts[s][i + 1])
                    gx.select(plane[s])
                    gx.submit(b.bases, b.quals, b.offsets)
                if i == 1:
                    gx.sync()                                                              # (one run of the store in the middle of the job)
            for s in range(2):
                _eq_counts(gx, plane[s], want[s][:2], (knob, stats))
            assert gx.stats()["overflow_deep"] > 2
            for s in range(NP):
                if s not in plane:
                    assert not _raw(gx, s).any(), (knob, stats, "plane %d took counts" % s)


def test_reset_of_a_high_plane(dealt):
    prefix, _, per, want = dealt
    with GenoIndex.open(prefix) as gx:
        gx.reserve_samples(NP)
        gx.set_stats(False)
        for s, k in ((NP - 1, 0), (NP - 2, 1), (43, 2), (0, 3)):                           # (299 & 255 == 43)
            gx.select(s)
            gx.submit(per[k].bases, per[k].quals, per[k].offsets)
        _eq_counts(gx, NP - 1, want[0])
        gx.reset_sample(NP - 1)
        assert not _raw(gx, NP - 1).any()
        rc, ac = gx.counts(sample=NP - 1)
        assert not rc.any() and not ac.any()
        for s, k in ((NP - 2, 1), (43, 2), (0, 3)):
            _eq_counts(gx, s, want[k])

"""The inputs of test_gpu_deep_planes.py do what that file needs them to do -- stated with the oracle alone, on any machine.  If a
seed of tests/deep_plane_cases.py misses a condition here, the seed changes, not the condition."""
import os

import numpy as np
import pytest

import deep_plane_cases as DP
from oracle import oracle as O


@pytest.fixture(scope="module")
def seeded(ftiny_dir):
    prefix = os.path.join(ftiny_dir, "idx")
    own = O.OracleIndex.load(prefix).sites()
    so = O.OracleIndex.from_arrays(DP.freq_arrays(prefix)).sites()
    return prefix, own, so


def test_seeded_frequencies_keep_the_sites_and_spread_over_the_byte(seeded):
    _, own, so = seeded
    for k in ("pos", "ref_base", "alt_base"):
        assert np.array_equal(so[k], own[k]), k
    assert len(so["pos"]) == 2928
    assert len(np.unique(so["ref_freq"])) > 200 and len(np.unique(so["alt_freq"])) > 200
    assert not np.array_equal(so["ref_freq"], own["ref_freq"])


@pytest.mark.parametrize("seed", [DP.SUMS_SEED, DP.OTHER_SEED])
def test_deep_sums_force_the_host_branch_at_many_sites(seeded, seed):
    _, _, so = seeded
    n = len(so["pos"])
    sums = DP.deep_sums(n, seed)
    assert sums.dtype == np.uint32 and sums.shape == (2 * n,)
    assert set(np.unique(sums[sums > DP.CAP]).tolist()) == set(DP.DEEP[DP.DEEP > DP.CAP].tolist())        # every deep value occurs
    rc, ac = DP.clamp(sums)
    gt, gq, conf = DP.oracle_calls(rc, ac, so["ref_freq"], so["alt_freq"])
    called, forced, near = DP.conditions(gt, conf, 1e-5)
    deep = int(((sums[0::2] > DP.CAP) | (sums[1::2] > DP.CAP)).sum())
    print("seed %d: %d sites, %d called, %d forced, %d within 1e-5, %d deep" % (seed, n, called, forced, near, deep))
    assert 2 * called >= n
    assert forced >= 100
    assert near <= 5
    assert 3 * deep >= 2 * n
    assert np.array_equal(gq[(gt != 0) & ~((conf > 0) & (conf < 1))], np.full(forced, DP.INT_MIN))          # the reference's INT_MIN


def test_the_two_arrays_of_sums_differ_in_their_calls(seeded):
    """Plane 7 of the selection test holds the other array: a call taken from the wrong plane cannot pass."""
    _, _, so = seeded
    n = len(so["pos"])
    a = DP.oracle_calls(*DP.clamp(DP.deep_sums(n, DP.SUMS_SEED)), so["ref_freq"], so["alt_freq"])
    b = DP.oracle_calls(*DP.clamp(DP.deep_sums(n, DP.OTHER_SEED)), so["ref_freq"], so["alt_freq"])
    assert int((a[0] != b[0]).sum()) > n // 4 and int((a[1] != b[1]).sum()) > n // 4


def test_flat_u8_counters_above_the_cap(seeded):
    rc, ac, rf, af = DP.u8_case()
    assert len(rc) == 4050 and rc.dtype == np.uint8 and rc.max() == 255
    gt, gq, conf = DP.oracle_calls(np.minimum(rc, DP.CAP), np.minimum(ac, DP.CAP), rf, af)
    called, forced, near = DP.conditions(gt, conf, 1e-5)
    print("u8 case: %d entries, %d called, %d forced, %d within 1e-5" % (len(rc), called, forced, near))
    assert 2 * called >= len(rc) and forced >= 100 and near <= 5


def test_ftiny_alone_never_leaves_the_device(seeded, ftiny_reads):
    """The premise: with F-tiny's own frequencies (p and 1 - p) and its own counts the device settles every site, so no test that
    uses them reaches the host branch of vg_sample_calls_fetch.  A later change of the fixture that alters this shows here."""
    prefix, own, _ = seeded
    ox = O.OracleIndex.load(prefix)
    rc, ac = DP.oracle_counts(ox, ftiny_reads)
    assert int(max(rc.max(), ac.max())) < DP.CAP
    gt, gq, conf = DP.oracle_calls(rc, ac, own["ref_freq"], own["alt_freq"])
    called, forced, near = DP.conditions(gt, conf, 1e-6)
    print("F-tiny: %d sites, %d called, %d forced, %d within 1e-6, largest counter %d" % (len(rc), called, forced, near, max(rc.max(), ac.max())))
    assert called > 2000 and forced == 0 and near == 0


def test_round_robin_leaves_no_plane_empty(seeded, ftiny_reads):
    prefix, _, _ = seeded
    ox = O.OracleIndex.load(prefix)
    per = DP.round_robin(ftiny_reads)
    assert len(per) == DP.N_PLANES and sum(p.n for p in per) == ftiny_reads.n
    seen = set()
    for p in per:
        rc, ac = DP.oracle_counts(ox, p)
        assert rc.any() or ac.any()
        seen.add(rc.tobytes() + ac.tobytes())
    assert len(seen) == DP.N_PLANES                               # no two planes alike: a batch in the wrong plane shows

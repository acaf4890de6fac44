"""The cohort prior on the device (vg_cprior_*, api.CohortPrior) against the header's host loop (api.cohort_prior_host, itself pinned
to the numpy restatement by test_cprior_cpu.py): q bit-identical, gt and gq equal -- over the CPU suite's shapes, a shape past one
round of the grid, a guard that leaves about half the entries to the host, and the handle's edges."""
import numpy as np
import pytest

import cprior_cases as CC
from vargeno_amd import _lib, api

pytestmark = pytest.mark.gpu


def _device(c, iters=8, pseudo=2.0, guard=0, n_samples=None):
    ref, alt, rf, af = c
    n_samples = ref.shape[0] if n_samples is None else n_samples
    with api.CohortPrior(ref.shape[1], n_samples) as cp:
        for s in range(ref.shape[0]):
            cp.set(s, ref[s], alt[s])
        q = cp.run(rf, af, iters=iters, pseudo=pseudo, guard=guard)
        gt, gq = np.empty((n_samples, ref.shape[1]), np.uint8), np.empty((n_samples, ref.shape[1]), np.int32)
        for s in range(n_samples):
            gt[s], gq[s] = cp.calls(s)
        return gt, gq, q, cp.n_escaped


def _same(got, want):
    assert np.array_equal(CC.bits(got[2]), CC.bits(want[2]))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("n_samples", CC.SAMPLES)
@pytest.mark.parametrize("n_sites", CC.SITES)
def test_the_kernel_computes_what_the_host_loop_computes(n_sites, n_samples):
    c = CC.shaped(n_sites, n_samples)
    for iters, pseudo in ((8, 2.0), (1, 0.0), (64, 2.0), (64, 0.0)):
        _same(_device(c, iters, pseudo), api.cohort_prior_host(*c, iters=iters, pseudo=pseudo, threads=3))


def test_every_counter_pair_and_the_seeded_cohort():
    for c in (CC.all_pairs(), CC.cohort(4096, 24, seed=20261021)):
        got = _device(c)
        _same(got, api.cohort_prior_host(*c, threads=3))
        _same(got, CC.expected(*c))
        assert got[3] < 100                                                    # the default guard leaves next to nothing to the host


def test_more_sites_than_one_round_of_the_grid():
    n = api.CPRIOR_BLOCK * api.CPRIOR_MAX_GRID + 300
    c = CC.cohort(n, 2, seed=11)
    _same(_device(c), api.cohort_prior_host(*c, threads=16))


def test_a_wide_guard_leaves_half_the_entries_to_the_host_and_the_values_stay():
    c = CC.cohort(4096, 24, seed=3)
    want = api.cohort_prior_host(*c, threads=3)
    got = _device(c, guard=0.25)
    _same(got, want)
    called = int((want[0] != 0).sum())
    assert 0.3 * called < got[3] < 0.7 * called


def test_a_sample_set_twice_and_a_sample_never_set():
    c = CC.cohort(257, 3, seed=9)
    ref, alt, rf, af = c
    with api.CohortPrior(257, 4) as cp:
        cp.set(0, alt[0], ref[0])                                              # replaced below
        cp.set(2, ref[2], alt[2])
        cp.set(0, ref[0], alt[0])
        cp.set(3, ref[1], alt[1])                                              # sample 1 is never set
        q = cp.run(rf, af)
        cols = [cp.calls(s) for s in range(4)]
        zero = np.zeros(257, np.uint8)
        want = api.cohort_prior_host(np.array([ref[0], zero, ref[2], ref[1]]), np.array([alt[0], zero, alt[2], alt[1]]), rf, af)
        assert np.array_equal(CC.bits(q), CC.bits(want[2]))
        for s in range(4):
            assert np.array_equal(cols[s][0], want[0][s]) and np.array_equal(cols[s][1], want[1][s])
        assert not cols[1][0].any() and not cols[1][1].any()
        # a sample set after the run: the calls are of other counters, and the handle says so until the next run
        cp.set(1, ref[1], alt[1])
        with pytest.raises(_lib.VgError) as e:
            cp.calls(0)
        assert _lib.VG_ERRORS.get(e.value.code) == "VG_EINVAL"
        cp.run(rf, af)
        assert np.array_equal(cp.calls(1)[0], cp.calls(3)[0])


def test_calls_before_a_run_and_arguments_out_of_range_are_einval():
    c = CC.cohort(65, 2, seed=4)
    with api.CohortPrior(65, 2) as cp:
        cp.set(0, c[0][0], c[1][0])
        for bad in (lambda: cp.calls(0), lambda: cp.set(2, c[0][0], c[1][0]), lambda: cp.run(c[2], c[3], iters=0), lambda: cp.run(c[2], c[3], iters=65),
                    lambda: cp.run(c[2], c[3], pseudo=-1.0), lambda: cp.run(c[2], c[3], pseudo=float("inf")), lambda: cp.run(c[2], c[3], guard=0.5)):
            with pytest.raises(_lib.VgError) as e:
                bad()
            assert _lib.VG_ERRORS.get(e.value.code) == "VG_EINVAL"
        cp.run(c[2], c[3])
        with pytest.raises(_lib.VgError):
            cp.calls(2)
        assert cp.calls(0)[0].any()


def test_device_bytes_are_the_sizes_the_header_states():
    for n_sites, n_samples in ((1000, 3), (257, 24), (1, 1)):
        with api.CohortPrior(n_sites, n_samples) as cp:
            assert cp.device_bytes == 4 * n_samples * n_sites + 12 * n_sites + api.CPRIOR_FIXED_BYTES
    with api.CohortPrior(0, 5) as cp:                                          # an empty buffer counts 8 bytes: six of them
        assert cp.device_bytes == 6 * 8 + api.CPRIOR_FIXED_BYTES
        assert cp.run(np.zeros(0, np.uint8), np.zeros(0, np.uint8)).shape == (0,) and cp.calls(4)[0].shape == (0,)

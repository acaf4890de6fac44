"""The genotype matrix on the device (vg_gmatrix_*: the pack kernel and the pair kernel) against the numpy oracle of
tests/pairs_cases.py and against vg_pairs_host: exact, at every edge of the tiling -- sample counts around the tile, site counts
around the 64-site word, site blocks of one and two words and the default, a launch whose default block length itself splits the
sites -- plus replacement of a sample, samples never set, and the error codes."""
import ctypes as C

import numpy as np
import pytest

import pairs_cases as PC
from vargeno_amd import api
from vargeno_amd._lib import VgError

pytestmark = pytest.mark.gpu

T = api.PAIR_TILE
SITES = (0, 1, 63, 64, 65, 64 * 7 + 1)
_cases = {}


def case(n_samples, n_sites, min_gq):
    """Input, oracle and host table of one shape: computed once, shared by the block lengths, never modified."""
    key = (n_samples, n_sites, min_gq)
    if key not in _cases:
        gt, gq = PC.make_case(n_samples, n_sites, min_gq, seed=77 * n_samples + n_sites)
        want = PC.oracle(gt, gq, min_gq)
        assert np.array_equal(api.pairs_host(gt, gq, min_gq=min_gq, threads=2), want)
        for a in (gt, gq, want):
            a.setflags(write=False)
        _cases[key] = (gt, gq, want)
    return _cases[key]


def fill(gm, gt, gq, min_gq):
    for s in range(gt.shape[0]):
        gm.set(s, gt[s], gq[s], min_gq=min_gq)


@pytest.mark.parametrize("n_samples", [1, 2, T - 1, T, T + 1, 2 * T + 1])
def test_pairs_equal_the_oracle_and_the_host_loop(n_samples):
    min_gq = 20
    for n_sites in SITES:
        gt, gq, want = case(n_samples, n_sites, min_gq)
        with api.GenotypeMatrix(n_sites, n_samples) as gm:
            assert gm.device_bytes >= n_samples * 3 * ((n_sites + 63) // 64) * 8 + n_samples * n_samples * 40
            fill(gm, gt, gq, min_gq)
            for wpb in (1, 2, 0):                     # 449 sites at 1: eight blocks, the last one holds one bit
                got = gm.pairs(words_per_block=wpb)
                assert got.dtype == np.uint64 and got.shape == (n_samples, n_samples, 5)
                assert np.array_equal(got, want), (n_sites, wpb)
            PC.check_identities(got)
            PC.check_adversaries(got, gt, gq, min_gq)


def test_the_default_block_length_splits_a_longer_matrix():
    """One word and one bit more than PAIR_WORDS_DEFAULT words, at T + 1 samples: two site blocks per tile without being asked."""
    n_sites = (api.PAIR_WORDS_DEFAULT + 1) * 64 + 1
    gt, gq, want = case(T + 1, n_sites, 0)
    with api.GenotypeMatrix(n_sites, T + 1) as gm:
        fill(gm, gt, gq, 0)
        got = gm.pairs()
        assert np.array_equal(got, want)
        assert np.array_equal(gm.pairs(words_per_block=api.PAIR_WORDS_DEFAULT + 2), want)      # ... and as one block
    PC.check_identities(got)
    assert want[0, 0, 0] > 20000


def test_set_replaces_a_sample_and_a_sample_never_set_is_all_missing():
    n_samples, n_sites, min_gq = 5, 449, 0
    gt, gq, _ = case(n_samples, n_sites, min_gq)
    gt, gq = gt.copy(), gq.copy()
    with api.GenotypeMatrix(n_sites, n_samples) as gm:
        for s in (0, 2, 3):                           # 1 and 4 are never set
            gm.set(s, gt[s], gq[s])
        seen = gt.copy()
        seen[[1, 4]] = 0
        first = gm.pairs(words_per_block=2)
        assert np.array_equal(first, PC.oracle(seen, gq, min_gq))
        assert not first[4].any() and not first[:, 4].any() and first[0, 0, 0] > 100
        other_gt, other_gq = PC.make_case(1, n_sites, min_gq, seed=4242)
        gm.set(2, other_gt[0], other_gq[0])
        seen[2], gq[2] = other_gt[0], other_gq[0]
        second = gm.pairs(words_per_block=2)
        assert np.array_equal(second, PC.oracle(seen, gq, min_gq))
        assert not np.array_equal(second[2], first[2])
        gm.set(2, other_gt[0], other_gq[0], min_gq=41)                          # the threshold belongs to the set
        assert np.array_equal(gm.pairs()[2, 2], PC.oracle(other_gt, other_gq, 41)[0, 0])


def test_error_codes():
    L = api.lib()
    h = C.c_void_p()
    assert L.vg_gmatrix_create(0, 100, 0, C.byref(h)) == -1 and not h.value and L.vg_last_error()
    assert L.vg_gmatrix_create(0, 100, api.PAIR_MAX_SAMPLES + 1, C.byref(h)) == -5 and not h.value and L.vg_last_error()
    assert L.vg_gmatrix_create(0, 2 ** 32, 2, C.byref(h)) == -1 and not h.value
    with pytest.raises(VgError) as e:
        api.GenotypeMatrix(10, 0)
    assert e.value.code == -1
    gt, gq, want = case(3, 65, 20)
    with api.GenotypeMatrix(65, 3) as gm:
        fill(gm, gt, gq, 20)
        with pytest.raises(VgError) as e:
            gm.set(3, gt[0], gq[0])
        assert e.value.code == -1 and b"out of range" in L.vg_last_error()
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        assert L.vg_gmatrix_set(gm._h, 0, None, p(gq[0]), 0) == -1 and b"null" in L.vg_last_error()
        assert L.vg_gmatrix_set(gm._h, 0, p(gt[0]), None, 0) == -1
        assert L.vg_gmatrix_pairs(gm._h, 0, None) == -1 and b"null" in L.vg_last_error()
        assert np.array_equal(gm.pairs(), want)                                # still usable, nothing changed
    assert L.vg_gmatrix_device_bytes(None) == 0
    L.vg_gmatrix_destroy(None)

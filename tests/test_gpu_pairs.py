"""The genotype matrix on the device (vg_gmatrix_*: the pack kernel and the pair kernel) against the numpy oracle of
tests/pairs_cases.py and against vg_pairs_host: exact, at every edge of the tiling -- sample counts around the tile, site counts
around the 64-site word, site blocks of one and two words and the default, a launch whose default block length itself splits the
sites -- plus replacement of a sample, samples never set, and the error codes.  Then the launch paths beyond those shapes: a matrix
longer than the pack kernel's grid and than a grid's second dimension, a block length above the cap, six rows of tiles, two hundred
site blocks adding into one tile, gt values above 3, thresholds at the ends of int32, a table that follows from counting residues
by hand, planes of full words, permutations of sites and samples, and two matrices in use at once."""
import ctypes as C
import re

import numpy as np
import pytest

import pairs_cases as PC
from vargeno_amd import api
from vargeno_amd._lib import VgError

pytestmark = pytest.mark.gpu

T = api.PAIR_TILE
SITES = (0, 1, 63, 64, 65, 64 * 7 + 1)
_cases = {}


def frozen(gt, gq, min_gq):
    """(gt, gq, oracle), read-only, after the host loop has agreed with the oracle."""
    want = PC.oracle(gt, gq, min_gq)
    assert np.array_equal(api.pairs_host(gt, gq, min_gq=min_gq, threads=2), want)
    for a in (gt, gq, want):
        a.setflags(write=False)
    return gt, gq, want


def case(n_samples, n_sites, min_gq, wild_gt=False):
    """Input, oracle and host table of one shape: computed once, shared by the block lengths, never modified."""
    key = (n_samples, n_sites, min_gq, wild_gt)
    if key not in _cases:
        _cases[key] = frozen(*PC.make_case(n_samples, n_sites, min_gq, seed=77 * n_samples + n_sites, wild_gt=wild_gt), min_gq)
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


def test_a_matrix_longer_than_the_pack_grid_and_than_65535_blocks(monkeypatch, capfd):
    """65 537 words: the pack kernel's 16 384 waves go round their loop four times and a fifth for one word; one word per block
    would be more blocks than a grid's second dimension has, so the block length is derived again -- (65537 + 65534) / 65535 = 2
    words, 32 769 blocks --, and a block length above the cap of 2^24 words is cut to it: one block."""
    n_sites = 65537 * 64 - 5
    gt, gq, want = case(3, n_sites, 20)
    assert want[0, 0, 0] > 10 ** 6
    monkeypatch.setenv("VG_VERBOSE", "1")
    with api.GenotypeMatrix(n_sites, 3) as gm:
        fill(gm, gt, gq, 20)
        capfd.readouterr()
        for wpb in (1, 0, 2 ** 40):
            assert np.array_equal(gm.pairs(words_per_block=wpb), want), wpb
    said = re.findall(r"vg_gmatrix_pairs: 3 samples, 65537 site words in (\d+) blocks of (\d+):", capfd.readouterr().err)
    assert said == [("32769", "2"), ("65", "1024"), ("1", str(2 ** 24))]


@pytest.mark.parametrize("n_samples", [4 * T + 3, 5 * T + 3])
def test_fifteen_tiles(n_samples):
    """Five rows of tiles (15 tiles) and six (21): the walk from blockIdx.x to (ti, tj) past its third row, one sample short of a
    full last tile."""
    gt, gq, want = case(n_samples, 130, 20)
    with api.GenotypeMatrix(130, n_samples) as gm:
        fill(gm, gt, gq, 20)
        for wpb in (1, 0):
            got = gm.pairs(words_per_block=wpb)
            assert np.array_equal(got, want), wpb
    PC.check_identities(got)
    PC.check_adversaries(got, gt, gq, 20)
    assert want[n_samples - 1, 0, 0] > 0 and want[4 * T + 2, 2 * T + 5, 0] > 0    # the far corner and a tile of the third row count


def test_two_hundred_blocks_add_into_one_tile():
    """201 words: at one word per block 201 workgroups add into each counter; 2, 7 and 9 leave a shorter last block (1, 5 and 3
    words), 3 divides evenly; 7 and 9 lie either side of the kernel's run of 8 words."""
    n_sites = 200 * 64 + 1
    gt, gq, want = case(T + 1, n_sites, 20)
    with api.GenotypeMatrix(n_sites, T + 1) as gm:
        fill(gm, gt, gq, 20)
        for wpb in (1, 2, 3, 7, 9):
            got = gm.pairs(words_per_block=wpb)
            assert np.array_equal(got, want), wpb
    PC.check_identities(got)
    PC.check_adversaries(got, gt, gq, 20)


def test_wild_gt_values_are_not_counted():
    """gt of 4, 5, 7, 128 .. 131 and 255 is no call, whatever its low bits: the packer tests the value, not gt & 3."""
    gt, gq, want = case(T + 1, 449, 20, wild_gt=True)
    _, _, plain = case(T + 1, 449, 20)
    wild = np.isin(gt, PC.WILD_GT)
    assert wild.any(axis=1).all() and ((gt[wild] & 3 != 0) & (gq[wild] >= 20)).any()
    with api.GenotypeMatrix(449, T + 1) as gm:
        fill(gm, gt, gq, 20)
        got = gm.pairs(words_per_block=1)
        assert np.array_equal(got, want)
        assert np.array_equal(gm.pairs(), want)
    assert got[0, 0, 0] < plain[0, 0, 0]
    PC.check_identities(got)
    PC.check_adversaries(got, gt, gq, 20)


def test_thresholds_at_the_ends_of_int32():
    """min_gq = INT_MIN counts every called entry, those with gq = INT_MIN too; min_gq = INT_MAX only those at INT_MAX; and two
    samples set at different thresholds keep each its own."""
    int_max = 2147483647
    gt, gq, _ = case(5, 130, 0)
    called = (gt != 0)
    assert (called & (gq == PC.INT_MIN)).any(axis=1)[[0, 4]].all() and (called & (gq == int_max)).any(axis=1)[[0, 4]].all()
    with api.GenotypeMatrix(130, 5) as gm:
        for min_gq in (PC.INT_MIN, int_max):
            fill(gm, gt, gq, min_gq)
            got = gm.pairs(words_per_block=1)
            assert np.array_equal(got, PC.oracle(gt, gq, min_gq)) and np.array_equal(got, api.pairs_host(gt, gq, min_gq=min_gq))
            counted = called if min_gq == PC.INT_MIN else called & (gq == int_max)
            assert got[np.arange(5), np.arange(5), 0].tolist() == counted.sum(axis=1).tolist() and got[0, 0, 0] > 0
        gm.set(0, gt[0], gq[0], min_gq=PC.INT_MIN)              # 2 is a copy of 0, still at INT_MAX; 4 as well
        seen = np.where(gq == int_max, gt, 0).astype(np.uint8)
        seen[0] = gt[0]
        got = gm.pairs()
        assert np.array_equal(got, PC.oracle(seen, gq, PC.INT_MIN))
        assert got[0, 0, 0] == called[0].sum() > got[0, 2, 0] == got[2, 2, 0] > 0


@pytest.mark.parametrize("n_samples,n_sites", [(37, 577), (T + 1, 64 * 9)])
def test_the_residue_case_equals_its_closed_form(n_samples, n_sites):
    """gt[i][s] = (s + i) % 4: the table counted by hand from the sites' residues (pairs_cases.residue_table), no oracle between."""
    gt, gq = PC.residue_case(n_samples, n_sites)
    want = PC.residue_table(n_samples, n_sites)
    with api.GenotypeMatrix(n_sites, n_samples) as gm:
        fill(gm, gt, gq, 0)
        for wpb in (1, 0):
            assert np.array_equal(gm.pairs(words_per_block=wpb), want), wpb
    assert np.array_equal(want, PC.oracle(gt, gq, 0))


@pytest.mark.parametrize("n_sites", [64, 65, 512, 513])
def test_saturated_planes(n_sites):
    """Samples all of one class, gq at the threshold: words with all 64 bits set, counters that are n_sites, n_sites - 1,
    n_sites - 2 or nothing."""
    gt, gq, want = frozen(*PC.saturated_case(n_sites, min_gq=20), 20)
    with api.GenotypeMatrix(n_sites, 6) as gm:
        fill(gm, gt, gq, 20)
        for wpb in (1, 0):
            got = gm.pairs(words_per_block=wpb)
            assert np.array_equal(got, want), wpb
            PC.check_saturated(got, n_sites)
        fill(gm, gt, gq, 21)                                    # one above every gq: nothing is counted
        assert not gm.pairs().any()
    PC.check_identities(got)


def test_site_and_sample_permutations():
    """Device table against device table: the order of the sites does not matter, and samples in the order p give table[p][:, p]."""
    n_samples, n_sites = T + 1, 449
    gt, gq, want = case(n_samples, n_sites, 20)
    rng = np.random.default_rng(606)
    sites, p = rng.permutation(n_sites), rng.permutation(n_samples)
    assert (sites // 64 != np.arange(n_sites) // 64).sum() > n_sites // 2 and p[T] != T
    with api.GenotypeMatrix(n_sites, n_samples) as gm:
        fill(gm, gt, gq, 20)
        first = gm.pairs(words_per_block=2)
        fill(gm, gt[:, sites], gq[:, sites], 20)
        assert np.array_equal(gm.pairs(words_per_block=2), first)
        fill(gm, gt[p], gq[p], 20)
        assert np.array_equal(gm.pairs(words_per_block=2), first[p][:, p])
    assert np.array_equal(first, want)


def test_two_matrices_side_by_side():
    """Two handles of different shapes, filled sample by sample in turn and asked in turn: each has its own stream, staging
    buffers and table, and a sample replaced in one leaves the other as it was."""
    a_gt, a_gq, a_want = case(3, 65, 20)
    b_gt, b_gq, b_want = case(T + 1, 449, 20)
    with api.GenotypeMatrix(65, 3) as a, api.GenotypeMatrix(449, T + 1) as b:
        for s in range(T + 1):
            if s < 3:
                a.set(s, a_gt[s], a_gq[s], min_gq=20)
            b.set(s, b_gt[s], b_gq[s], min_gq=20)
        assert np.array_equal(a.pairs(), a_want)
        assert np.array_equal(b.pairs(words_per_block=1), b_want)
        assert np.array_equal(a.pairs(words_per_block=1), a_want)
        other_gt, other_gq = PC.make_case(1, 449, 20, seed=4243)
        b.set(T, other_gt[0], other_gq[0], min_gq=20)
        assert np.array_equal(a.pairs(), a_want)
        seen_gt, seen_gq = b_gt.copy(), b_gq.copy()
        seen_gt[T], seen_gq[T] = other_gt[0], other_gq[0]
        b_second = b.pairs()
        assert np.array_equal(b_second, PC.oracle(seen_gt, seen_gq, 20)) and not np.array_equal(b_second[T], b_want[T])
        a.set(0, a_gt[1], a_gq[1], min_gq=20)                   # a's sample 0 becomes the all-missing one
        a_second = a.pairs()
        assert not a_second[0].any() and not a_second[:, 0].any() and np.array_equal(a_second[2, 2], a_want[2, 2])
        assert np.array_equal(b.pairs(words_per_block=2), b_second)


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

"""The genotype caller on the device (vg_call_kernel behind vg_call_device / vg_sample_calls_fetch): GT and GQ must be exactly the
reference's.  Everything up to the confidence is the host caller's own arithmetic (csrc/vg_caller.h); the logarithm is not, so the
kernel settles a site only when its -10 ln(confidence) is farther than a guard from an integer and leaves the rest -- counted in
n_escaped -- to the host.  The checks: the values over the reference's own table and over a seeded sample of the whole domain, and
the escape count, which must be what the reference's values force and no more (a kernel that escaped more would be hiding its
arithmetic behind the host)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from oracle import oracle as O
from vargeno_amd.api import CALL_BLOCK, CALL_MAX_GRID, GenoIndex, call_device

pytestmark = pytest.mark.gpu

INT_MIN = -2147483648
THIRDS = [(0, 1333), (1333, 2666), (2666, 4000)]


@pytest.fixture(scope="module")
def table():
    """tests/golden/caller_table.npz: the reference's own choose_best_genotype for every count pair and 16 frequency pairs."""
    z = np.load(os.path.join(GOLDEN, "caller_table.npz"))
    t = {k: z[k] for k in z.files}
    t["want_gq"] = np.where(t["genotype"] != 0, t["gq"], 0).astype(np.int32)        # (gq is 0 where nothing is called)
    # what the reference alone forces off the device: called entries whose confidence is not inside (0, 1)
    t["forced"] = (t["genotype"] != 0) & ~((t["conf"] > 0) & (t["conf"] < 1))
    assert len(t["genotype"]) == 65536 and int((t["genotype"] == 0).sum()) == 32
    assert int(t["forced"].sum()) == 3326 and np.array_equal(t["forced"], (t["genotype"] != 0) & (t["gq"] == INT_MIN))
    return t


def _run(t, n, guard=0.0):
    """The first n entries of the table, repeated from its start when n is longer."""
    idx = np.arange(n) % len(t["genotype"])
    gt, gq, esc = call_device(t["ref_cnt"][idx], t["alt_cnt"][idx], t["ref_freq"][idx], t["alt_freq"][idx], guard=guard)
    return idx, gt, gq, esc


def test_the_reference_table_with_the_default_guard(table):
    idx, gt, gq, esc = _run(table, 65536)
    assert gt.dtype == np.uint8 and gq.dtype == np.int32
    assert np.array_equal(gt, table["genotype"]), int((gt != table["genotype"]).sum())
    assert np.array_equal(gq, table["want_gq"]), int((gq != table["want_gq"]).sum())
    # the 62 178 called entries with a confidence inside (0, 1) lie at least 1.56e-5 from an integer: nothing else may escape
    y = -10 * np.log(table["conf"][(table["genotype"] != 0) & ~table["forced"]])
    assert len(y) == 62178 and np.abs(y - np.round(y)).min() > 1.5e-5
    assert esc == 3326


def test_the_reference_table_with_a_wide_guard_takes_the_near_integer_branch(table):
    idx, gt, gq, esc = _run(table, 65536, guard=1e-3)
    assert np.array_equal(gt, table["genotype"]) and np.array_equal(gq, table["want_gq"])
    print("n_escaped with guard 1e-3:", esc)
    assert 3326 < esc <= 3326 + 64


def test_a_seeded_sample_of_the_whole_domain_against_the_oracle():
    rng = np.random.default_rng(20261018)
    n = 200_000
    rc, ac = rng.integers(0, 64, n), rng.integers(0, 64, n)
    rf, af = rng.integers(0, 256, n), rng.integers(0, 256, n)
    want = [O.call(rc[i], ac[i], rf[i], af[i]) for i in range(n)]
    w_gt = np.array([w[0] for w in want], dtype=np.uint8)
    conf = np.array([w[1] for w in want])
    w_gq = np.where(w_gt != 0, np.array([w[2] for w in want], dtype=np.int64), 0).astype(np.int32)
    gt, gq, esc = call_device(rc, ac, rf, af)
    assert np.array_equal(gt, w_gt), int((gt != w_gt).sum())
    assert np.array_equal(gq, w_gq), int((gq != w_gq).sum())
    inside = (conf > 0) & (conf < 1)
    forced = int(((w_gt != 0) & ~inside).sum())
    y = -10 * np.log(conf[(w_gt != 0) & inside])
    near = int((np.abs(y - np.round(y)) < 1e-5).sum())
    print("n_escaped:", esc, "forced by the oracle's confidence:", forced, "within 1e-5 of an integer:", near)
    assert forced > 30_000
    assert forced <= esc <= forced + near


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 65536 + 1, CALL_BLOCK * CALL_MAX_GRID + 257])
def test_shapes(table, n):
    """Prefixes of the table around the wave and the block size, the table plus one entry, and an array longer than the capped
    grid has lanes (CALL_BLOCK x CALL_MAX_GRID), so that the grid-stride loop wraps."""
    idx, gt, gq, esc = _run(table, n)
    assert len(gt) == n and len(gq) == n
    assert np.array_equal(gt, table["genotype"][idx]) and np.array_equal(gq, table["want_gq"][idx])
    assert esc == int(table["forced"][idx].sum())


def _oracle_calls(prefix, r):
    ox = O.OracleIndex.load(prefix)
    ox.process(r.bases, r.quals, r.offsets)
    so = ox.sites()
    want = [O.call(so["ref_cnt"][i], so["alt_cnt"][i], so["ref_freq"][i], so["alt_freq"][i]) for i in range(len(so["pos"]))]
    gt = np.array([w[0] for w in want], dtype=np.uint8)
    return gt, np.where(gt != 0, np.array([w[2] for w in want], dtype=np.int64), 0).astype(np.int32)


def test_calls_of_an_index_equal_the_oracle_on_its_own_counts(ftiny_dir, ftiny_reads):
    prefix = os.path.join(ftiny_dir, "idx")
    w_gt, w_gq = _oracle_calls(prefix, ftiny_reads)
    assert int((w_gt != 0).sum()) > 2000
    with GenoIndex.open(prefix, device=0) as gx:
        n = gx.num_sites
        before = gx.device_bytes
        gx.submit(ftiny_reads.bases, ftiny_reads.quals, ftiny_reads.offsets)
        gt, gq = gx.calls()
        assert np.array_equal(gt, w_gt) and np.array_equal(gq, w_gq), (int((gt != w_gt).sum()), int((gq != w_gq).sum()))
        # the caller's buffers: 4 bytes per site, the factor tables (638 doubles) and the escape count, each part rounded up to
        # 256 bytes at the most (five parts), taken at the first call and not again
        grown = gx.device_bytes - before
        assert 4 * n <= grown <= 4 * n + 638 * 8 + 8 + 5 * 256, grown
        gt2, gq2 = gx.calls()
        assert gx.device_bytes - before == grown
        assert np.array_equal(gt2, w_gt) and np.array_equal(gq2, w_gq)
        # the counters are still what they were
        rc, ac = gx.counts()
        assert int(rc.sum()) + int(ac.sum()) > 0


def test_calls_of_three_planes_fed_batch_by_batch(ftiny_dir, ftiny_reads):
    prefix = os.path.join(ftiny_dir, "idx")
    parts = [ftiny_reads.slice(a, b) for a, b in THIRDS]
    want = [_oracle_calls(prefix, p) for p in parts]
    assert not np.array_equal(want[0][0], want[1][0]) and not np.array_equal(want[1][0], want[2][0])
    nb = 5
    with GenoIndex.open(prefix, device=0) as gx:
        gx.reserve_samples(3)
        per = [[p.slice(p.n * i // nb, p.n * (i + 1) // nb) for i in range(nb)] for p in parts]
        for i in range(nb):
            for s in range(3):
                gx.select(s)
                gx.submit(per[s][i].bases, per[s][i].quals, per[s][i].offsets)
        gx.select(1)
        for s in (2, 0, 1):
            gt, gq = gx.calls(sample=s)
            assert gx.selected == 1                                   # calls(sample=k) does not disturb the selection
            assert np.array_equal(gt, want[s][0]) and np.array_equal(gq, want[s][1]), s
        gt, gq = gx.calls()                                           # the selected sample
        assert np.array_equal(gt, want[1][0]) and np.array_equal(gq, want[1][1])

"""Helper of the pair-table tests (test_pairs_cpu.py, test_gpu_pairs.py, test_gpu_joint_pairs_cli.py): the numpy oracle -- integer
matrix products of the 0/1 class matrices --, the adversarial inputs, the identities every table obeys, and the table's text."""
import numpy as np

INT_MIN = -2147483648
WILD_GT = (4, 5, 7, 128, 129, 130, 131, 255)              # no classes; 129, 130 and 131 have the low bits of 1, 2 and 3


def oracle(gt, gq, min_gq=0):
    """uint64[N, N, 5] = (n, ibs0, ibs2, hethet, het_i) from gt uint8[N, S], gq int32[N, S]: a call counts iff gt != 0 and gq >= min_gq."""
    gt, gq = np.asarray(gt), np.asarray(gq).astype(np.int64)
    ok = (gt != 0) & (gq >= min_gq)
    R, A, H = [((gt == v) & ok).astype(np.int64) for v in (1, 2, 3)]
    Cn = R + H + A
    out = np.stack([Cn @ Cn.T, R @ A.T + A @ R.T, R @ R.T + H @ H.T + A @ A.T, H @ H.T, H @ Cn.T], axis=-1)
    return out.astype(np.uint64)


def make_case(n_samples, n_sites, min_gq, seed, wild_gt=False):
    """Seeded gt over {0, 1, 2, 3} with 0-40 % missing per sample and gq straddling min_gq (min_gq - 1, min_gq and INT_MIN among
    them); where there is room: sample 1 all-missing, sample 2 a copy of sample 0, sample 3 the hom-swap (R <-> A) of sample 0.
    wild_gt: about 5 % of every sample's entries -- those of the all-missing sample too -- become values of WILD_GT, gq left as
    drawn (many pass the threshold); they come from a generator of their own, so every other entry is what the same seed gives
    without them, and samples 2 and 3 are derived after the replacement."""
    rng = np.random.default_rng(seed)
    wild = np.random.default_rng([seed, 0x57494c44])
    gt = np.zeros((n_samples, n_sites), np.uint8)
    gq = np.zeros((n_samples, n_sites), np.int32)
    for s in range(n_samples):
        g = rng.integers(1, 4, size=n_sites).astype(np.uint8)
        g[rng.random(n_sites) < rng.uniform(0.0, 0.4)] = 0
        gt[s] = g
        gq[s] = rng.choice(np.array([min_gq - 1, min_gq, min_gq + 1, min_gq + 40, min_gq - 30, INT_MIN, 2147483647], np.int64), size=n_sites,
                           p=[0.08, 0.2, 0.2, 0.4, 0.04, 0.04, 0.04]).astype(np.int32)
    if n_samples > 1:
        gt[1] = 0
    if wild_gt:
        for s in range(n_samples):
            at = wild.random(n_sites) < 0.05
            gt[s][at] = wild.choice(np.array(WILD_GT, np.uint8), size=int(at.sum()))
    if n_samples > 2:
        gt[2], gq[2] = gt[0], gq[0]
    if n_samples > 3:
        gt[3], gq[3] = np.where(gt[0] == 1, 2, np.where(gt[0] == 2, 1, gt[0])).astype(np.uint8), gq[0]
    return gt, gq


def residue_case(n_samples, n_sites):
    """gt[i][s] = (s + i) % 4 and gq = 0, for min_gq = 0: every class of every sample pair at a known share of the sites."""
    gt = ((np.arange(n_sites)[None, :] + np.arange(n_samples)[:, None]) % 4).astype(np.uint8)
    return gt, np.zeros((n_samples, n_sites), np.int32)


def residue_table(n_samples, n_sites):
    """The table of residue_case(n_samples, n_sites) at min_gq = 0 without the oracle: plain integers from the number of sites of
    each residue mod 4.  Classes: 0 missing, 1 R, 2 A, 3 H.  At a site of residue r sample i has class u = (r + i) % 4 and, with
    d = (j - i) % 4, sample j has class (u + d) % 4."""
    sites = [len(range(r, n_sites, 4)) for r in range(4)]
    table = [[[0] * 5 for _ in range(n_samples)] for _ in range(n_samples)]
    for i in range(n_samples):
        for j in range(n_samples):
            d = (j - i) % 4
            for r in range(4):
                u = (r + i) % 4
                v = (u + d) % 4
                if u == 0 or v == 0:
                    continue
                t = table[i][j]
                t[0] += sites[r]                                                 # n: both called
                if (u, v) in ((1, 2), (2, 1)):
                    t[1] += sites[r]                                             # ibs0: opposite homozygotes
                if u == v:
                    t[2] += sites[r]                                             # ibs2: the same genotype
                if u == 3 and v == 3:
                    t[3] += sites[r]                                             # hethet
                if u == 3:
                    t[4] += sites[r]                                             # het_i: i het where j is called
    return np.array(table, dtype=np.uint64).reshape(n_samples, n_samples, 5)


def saturated_case(n_sites, min_gq=20):
    """Six samples whose planes are full words: all R, all A, all H, all missing, all R but the last site missing, all H but site
    0 missing; every gq exactly at min_gq."""
    gt = np.zeros((6, n_sites), np.uint8)
    gt[0], gt[1], gt[2], gt[4], gt[5] = 1, 2, 3, 1, 3
    gt[4, n_sites - 1:] = 0
    gt[5, :1] = 0
    return gt, np.full((6, n_sites), min_gq, np.int32)


def check_saturated(c, n_sites):
    """The table of saturated_case as functions of S = n_sites (rows (n, ibs0, ibs2, hethet, het_i))."""
    S, S1, S2 = n_sites, max(n_sites - 1, 0), max(n_sites - 2, 0)
    row = lambda i, j: [int(v) for v in c[i, j]]
    assert row(0, 0) == [S, 0, S, 0, 0] and row(1, 1) == [S, 0, S, 0, 0] and row(2, 2) == [S, 0, S, S, S]
    assert row(0, 1) == [S, S, 0, 0, 0] and row(1, 0) == [S, S, 0, 0, 0]             # R against A: every site opposite
    assert row(0, 2) == [S, 0, 0, 0, 0] and row(2, 0) == [S, 0, 0, 0, S]             # hom against het: het_i on the het's side only
    assert row(1, 2) == [S, 0, 0, 0, 0] and row(2, 1) == [S, 0, 0, 0, S]
    assert not c[3].any() and not c[:, 3].any()
    assert row(4, 4) == [S1, 0, S1, 0, 0] and row(5, 5) == [S1, 0, S1, S1, S1]
    assert row(0, 4) == [S1, 0, S1, 0, 0] and row(1, 4) == [S1, S1, 0, 0, 0] and row(2, 4) == [S1, 0, 0, 0, S1]
    assert row(0, 5) == [S1, 0, 0, 0, 0] and row(5, 0) == [S1, 0, 0, 0, S1] and row(2, 5) == [S1, 0, S1, S1, S1]
    assert row(4, 5) == [S2, 0, 0, 0, 0] and row(5, 4) == [S2, 0, 0, 0, S2]          # sites 1 .. S - 2 are shared


def check_identities(c):
    """What holds for every table, whatever the input."""
    n = c.shape[0]
    for k in range(4):
        assert np.array_equal(c[:, :, k], c[:, :, k].T), k
    assert (c[:, :, 4] <= c[:, :, 0]).all()
    assert (c[:, :, 1] + c[:, :, 2] <= c[:, :, 0]).all()
    d = c[np.arange(n), np.arange(n)]
    assert np.array_equal(d[:, 2], d[:, 0]) and not d[:, 1].any() and np.array_equal(d[:, 3], d[:, 4])


def check_adversaries(c, gt, gq, min_gq):
    """The planted samples of make_case."""
    n = c.shape[0]
    if n > 1:
        assert not c[1].any() and not c[:, 1].any()                              # all-missing
    if n > 2:
        assert c[0, 2, 2] == c[0, 2, 0] == c[0, 0, 0] and c[0, 2, 1] == 0        # identical: ibs2 == n, ibs0 == 0
    if n > 3:
        ok = (gt[0] != 0) & (gq[0].astype(np.int64) >= min_gq)
        assert c[0, 3, 1] == int((ok & ((gt[0] == 1) | (gt[0] == 2))).sum())     # hom-swap: ibs0 = the shared hom sites


def _ratio(num, den):
    return "nan" if den == 0 else "%.6f" % (num / den)


def table_text(names, n_sites, min_gq, c):
    """The pair table as the command line writes it, from the integers of `c`."""
    out = ["##sites=%d" % n_sites, "##min_gq=%d" % min_gq]
    out += ["##sample=%s\tcalled=%d\thet=%d" % (nm, c[i, i, 0], c[i, i, 3]) for i, nm in enumerate(names)]
    out.append("#sample_a\tsample_b\tn\tibs0\tibs2\thethet\thet_a\thet_b\tconcordance\trelatedness")
    for i in range(len(names)):
        for j in range(i + 1, len(names)):
            n, ibs0, ibs2, hh, ha, hb = [int(v) for v in (c[i, j, 0], c[i, j, 1], c[i, j, 2], c[i, j, 3], c[i, j, 4], c[j, i, 4])]
            out.append("\t".join([names[i], names[j]] + [str(v) for v in (n, ibs0, ibs2, hh, ha, hb)] + [_ratio(ibs2, n), _ratio(hh - 2 * ibs0, min(ha, hb))]))
    return "\n".join(out) + "\n"

"""Helper of the pair-table tests (test_pairs_cpu.py, test_gpu_pairs.py, test_gpu_joint_pairs_cli.py): the numpy oracle -- integer
matrix products of the 0/1 class matrices --, the adversarial inputs, the identities every table obeys, and the table's text."""
import numpy as np

INT_MIN = -2147483648


def oracle(gt, gq, min_gq=0):
    """uint64[N, N, 5] = (n, ibs0, ibs2, hethet, het_i) from gt uint8[N, S], gq int32[N, S]: a call counts iff gt != 0 and gq >= min_gq."""
    gt, gq = np.asarray(gt), np.asarray(gq).astype(np.int64)
    ok = (gt != 0) & (gq >= min_gq)
    R, A, H = [((gt == v) & ok).astype(np.int64) for v in (1, 2, 3)]
    Cn = R + H + A
    out = np.stack([Cn @ Cn.T, R @ A.T + A @ R.T, R @ R.T + H @ H.T + A @ A.T, H @ H.T, H @ Cn.T], axis=-1)
    return out.astype(np.uint64)


def make_case(n_samples, n_sites, min_gq, seed):
    """Seeded gt over {0, 1, 2, 3} with 0-40 % missing per sample and gq straddling min_gq (min_gq - 1, min_gq and INT_MIN among
    them); where there is room: sample 1 all-missing, sample 2 a copy of sample 0, sample 3 the hom-swap (R <-> A) of sample 0."""
    rng = np.random.default_rng(seed)
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
    if n_samples > 2:
        gt[2], gq[2] = gt[0], gq[0]
    if n_samples > 3:
        gt[3], gq[3] = np.where(gt[0] == 1, 2, np.where(gt[0] == 2, 1, gt[0])).astype(np.uint8), gq[0]
    return gt, gq


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

"""The cohort prior (csrc/vg_cprior.h) restated in numpy, independently of the header: the factor tables by math.pow / math.exp /
math.lgamma as vg_caller_tables_fill makes them, a Python loop over the samples with vector operations over the sites -- every
operation one IEEE f64 add, subtract, multiply, divide or compare, in the order the rule writes them -- and the GQ by math.log per
element, which is libm's.  So the comparisons against the library are exact: q as bit patterns, gt and gq equal.  Also the caller
of one sample (vg_call_site) restated the same way, and a seeded cohort generator."""
import math

import numpy as np

CAP = 63
ERR, MEAN_DEPTH = 0.01, 7.1
KEEP = np.array([math.pow(1.0 - ERR, k) for k in range(CAP + 1)])
FLIP = np.array([math.pow(ERR, k) for k in range(CAP + 1)])
HALF = np.array([math.pow(0.5, k) for k in range(2 * CAP + 1)])
DEPTH = np.array([(math.exp(-MEAN_DEPTH) * math.pow(MEAN_DEPTH, k)) / math.exp(math.lgamma(k + 1.0)) for k in range(2 * CAP + 1)])
FREQ = np.array([k / 255.0 for k in range(256)])
Q_MIN, Q_MAX = 1e-6, 1 - 1e-6
NONE, HOM_REF, HOM_ALT, HET = 0, 1, 2, 3


def _clamp(x):
    return np.minimum(np.maximum(x, Q_MIN), Q_MAX)


def _gq(conf):
    return np.array([int(-10 * math.log(c)) for c in conf], np.int32)


def _pick(w0, w1, w2):
    """best exactly as vg_call_site chooses it: the strict maximum, hom-ref tested before het, otherwise hom-alt"""
    ref = (w0 > w1) & (w0 > w2)
    het = ~ref & (w1 > w0) & (w1 > w2)
    gt = np.where(ref, HOM_REF, np.where(het, HET, HOM_ALT)).astype(np.uint8)
    top = np.where(ref, w0, np.where(het, w1, w2))
    return gt, top


def expected(ref_cnt, alt_cnt, ref_freq, alt_freq, iters=8, pseudo=2.0):
    """ref_cnt, alt_cnt: [n_samples, n_sites]; ref_freq, alt_freq: [n_sites].  Returns (gt, gq, q)."""
    r = np.minimum(np.asarray(ref_cnt, np.int64), CAP)
    a = np.minimum(np.asarray(alt_cnt, np.int64), CAP)
    n_samples, n_sites = r.shape
    inf = ((r | a) != 0) & ~((r == CAP) & (a == CAP))
    l0, l1, l2 = KEEP[r] * FLIP[a], HALF[r + a], FLIP[r] * KEEP[a]
    pr, pa = FREQ[np.asarray(ref_freq, np.int64)], FREQ[np.asarray(alt_freq, np.int64)]
    t = pr + pa
    with np.errstate(invalid="ignore", divide="ignore"):
        qd = np.where(t > 0, pa / t, 0.5)
    m = inf.sum(axis=0)
    q = _clamp(qd)
    some = m > 0
    for _ in range(iters):
        u = 1 - q
        g0, g1, g2 = u * u, (q * u) + (q * u), q * q
        e = np.zeros(n_sites)
        for s in range(n_samples):
            w0, w1, w2 = g0 * l0[s], g1 * l1[s], g2 * l2[s]
            total = (w0 + w1) + w2
            e = np.where(inf[s], e + (w1 + (w2 + w2)) / total, e)
        with np.errstate(invalid="ignore", divide="ignore"):
            q = np.where(some, _clamp((e + pseudo * qd) / ((2 * m).astype(np.float64) + pseudo)), q)
    u = 1 - q
    g0, g1, g2 = u * u, (q * u) + (q * u), q * q
    gt, gq = np.zeros((n_samples, n_sites), np.uint8), np.zeros((n_samples, n_sites), np.int32)
    for s in range(n_samples):
        w0, w1, w2 = g0 * l0[s], g1 * l1[s], g2 * l2[s]
        total = (w0 + w1) + w2
        best, top = _pick(w0, w1, w2)
        conf = (top / total) * DEPTH[r[s] + a[s]]
        k = np.flatnonzero(inf[s])
        gt[s, k] = best[k]
        gq[s, k] = _gq(conf[k])
    return gt, gq, q


def single_sample_calls(ref_cnt, alt_cnt, ref_freq, alt_freq):
    """vg_call_site + vg_genotype_quality over flat arrays: what every sample gets when it is called alone."""
    r = np.minimum(np.asarray(ref_cnt, np.int64), CAP)
    a = np.minimum(np.asarray(alt_cnt, np.int64), CAP)
    inf = ((r | a) != 0) & ~((r == CAP) & (a == CAP))
    pr, pa = FREQ[np.asarray(ref_freq, np.int64)], FREQ[np.asarray(alt_freq, np.int64)]
    rr, aa = pr * pr, pa * pa
    w0, w1, w2 = rr * (KEEP[r] * FLIP[a]), (1.0 - rr - aa) * HALF[r + a], aa * (FLIP[r] * KEEP[a])
    total = w0 + w1 + w2
    best, top = _pick(w0, w1, w2)
    with np.errstate(invalid="ignore", divide="ignore"):
        conf = (top / total) * DEPTH[r + a]
    gt, gq = np.zeros(len(r), np.uint8), np.zeros(len(r), np.int32)
    k = np.flatnonzero(inf & (conf > 0) & (conf < 1))                         # (outside (0, 1) the reference's GQ is an accident; no such site is compared)
    gt[inf] = best[inf]
    gq[k] = _gq(conf[k])
    return gt, gq


def cohort(n_sites, n_samples, seed, mean_depth=7.1):
    """A seeded cohort: a true alt frequency per site, Hardy-Weinberg genotypes, Poisson depth, 1 % errors; dictionary frequencies
    unrelated to the truth; a sprinkling of empty, saturated and over-the-cap counters.  Returns (ref_cnt, alt_cnt, ref_freq, alt_freq)."""
    rng = np.random.default_rng(seed)
    q = rng.beta(0.5, 0.5, n_sites)
    g = (rng.random((n_samples, n_sites)) < q).astype(np.int64) + (rng.random((n_samples, n_sites)) < q)
    depth = rng.poisson(mean_depth, (n_samples, n_sites))
    p_alt = np.where(g == 0, 0.01, np.where(g == 1, 0.5, 0.99))
    alt = rng.binomial(depth, p_alt)
    ref = depth - alt
    odd = rng.random((n_samples, n_sites))
    ref = np.where(odd < 0.02, 0, np.where(odd < 0.03, 63, np.where(odd < 0.04, 200, ref)))
    alt = np.where(odd < 0.02, 0, np.where(odd < 0.03, 63, np.where(odd < 0.035, 255, alt)))
    ref_freq = rng.integers(0, 256, n_sites).astype(np.uint8)
    alt_freq = rng.integers(0, 256, n_sites).astype(np.uint8)
    return ref.astype(np.uint8), alt.astype(np.uint8), ref_freq, alt_freq


def all_pairs():
    """One sample, 4 096 sites: every (r, a) of 0 .. 63 x 0 .. 63, under frequency pairs that include 0/0, 255/255 and 255/0."""
    k = np.arange(4096)
    ref, alt = (k >> 6).astype(np.uint8)[None, :], (k & 63).astype(np.uint8)[None, :]
    pairs = [(0, 0), (255, 255), (255, 0), (0, 255), (230, 25), (128, 128), (1, 1), (200, 60)]
    rf = np.array([pairs[i % len(pairs)][0] for i in k // 7], np.uint8)
    af = np.array([pairs[i % len(pairs)][1] for i in k // 7], np.uint8)
    return ref, alt, rf, af


SITES, SAMPLES = (0, 1, 63, 64, 65, 257), (1, 2, 3, 24)
FREQ_EDGES = ((0, 0), (255, 255), (255, 0))


def shaped(n_sites, n_samples):
    """The cohort of a shape, with the frequency edges planted, a site with no informative sample and one with only saturated ones."""
    ref, alt, rf, af = cohort(n_sites, n_samples, seed=7919 * n_sites + n_samples)
    for i, (x, y) in enumerate(FREQ_EDGES):
        if i < n_sites:
            rf[i], af[i] = x, y
    if n_sites > 4:
        ref[:, 3], alt[:, 3] = 0, 0
        ref[:, 4], alt[:, 4] = 63, 63
    return ref, alt, rf, af


def bits(q):
    return np.ascontiguousarray(q, np.float64).view(np.uint64)

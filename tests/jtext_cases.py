"""Seeded cases of the joint VCF's data lines (vargeno_amd/csrc/vg_jtext.h), shared by the CPU and the GPU suite, and the yardstick
both compare with: a formatter of the cell rule in plain Python (`format_span`), which knows nothing of the code under test."""
import numpy as np

INT_MIN = -2 ** 31
GQ_EDGES = [0, 9, 10, 99, 100, 999, 1000, 9999, 10000, 16382, 16383, 16384, 2 ** 31 - 1, -1, INT_MIN]
GT_TEXT = {1: "0/0", 2: "1/1", 3: "0/1"}


def format_span(gt, gq, heads, records, sites):
    """The text of a span by the rule: gt / gq are per-sample columns (None: a sample never set), records are
    (head_off, head_len, site_at, n_sites)."""
    out = []
    for head_off, head_len, site_at, n in records:
        cells = []
        for g, q in zip(gt, gq):
            hit = [int(s) for s in sites[site_at:site_at + n] if g is not None and g[s]]
            cells.append("\t%s:%d" % (GT_TEXT[int(g[hit[-1]])], int(q[hit[-1]])) if hit else "\t./.:.")
        if any(c != "\t./.:." for c in cells):
            out.append(bytes(heads[head_off:head_off + head_len]) + b"\tGT:GQ" + "".join(cells).encode() + b"\n")
    return b"".join(out)


def make_case(n_samples, n_records, seed, unset=(), drop=(), long_head=False, edges=True):
    """n_records records over site runs of 1 .. 5 sites (indices not consecutive, the runs disjoint), heads of 1, 3, 4, 5 and 20 .. 60
    bytes (long_head: record 0's has 70 000) at offsets that are not dword-aligned, calls with gq drawn from GQ_EDGES (edges) and
    from 0 .. 99; the samples in `unset` are None; the records in `drop` have no call in any sample.  Samples differ in which site
    of a run is their last called one: every call is drawn on its own."""
    rng = np.random.default_rng(seed)
    run_len = rng.integers(1, 6, size=n_records)
    n_sites = int(run_len.sum()) + 37
    pool = rng.permutation(n_sites)
    sites, records, heads, at = [], [], bytearray(b"\x01"), 0
    small = [1, 3, 4, 5]
    for i in range(n_records):
        run = np.sort(pool[at:at + run_len[i]])
        at += int(run_len[i])
        hl = 70_000 if (long_head and i == 0) else small[i % 4] if i % 3 else int(rng.integers(20, 61))
        heads += bytes(rng.integers(33, 127, size=int(rng.integers(0, 4)), dtype=np.uint8))          # junk between the heads
        records.append((len(heads), hl, len(sites), len(run)))
        heads += bytes(rng.integers(33, 127, size=hl, dtype=np.uint8))
        sites.extend(int(s) for s in run)
    gt = [rng.choice(np.array([0, 0, 1, 2, 3], np.uint8), size=n_sites) for _ in range(n_samples)]
    gq = []
    for _ in range(n_samples):
        q = rng.integers(0, 100, size=n_sites).astype(np.int64)
        if edges:
            pick = rng.random(n_sites) < 0.5
            q[pick] = rng.choice(np.array(GQ_EDGES, np.int64), size=int(pick.sum()))
        gq.append(q.astype(np.int32))
    for i in drop:
        _, _, site_at, n = records[i]
        for g in gt:
            g[sites[site_at:site_at + n]] = 0
    for s in unset:
        gt[s] = None
        gq[s] = None
    return dict(gt=gt, gq=gq, heads=bytes(heads), records=records, sites=np.array(sites, np.uint32), n_sites=n_sites, n_samples=n_samples)


def expected(case, lo=0, hi=None):
    return format_span(case["gt"], case["gq"], case["heads"], case["records"][lo:hi], case["sites"])


# the shapes of the two suites: (samples, records, unset samples, dropped records, a 70 000-byte head)
def shapes():
    out = []
    for n_samples in (1, 2, 63, 64, 65, 130):
        for n_records in (0, 1, 64, 65, 1000):
            if n_records == 1000 and n_samples not in (1, 65, 130):
                continue                                                # (the long spans at the smallest, a two-group and the largest width)
            drop = ()
            if n_records == 64:
                drop = (0, 63)
            if n_records == 65:
                drop = (64,)                                            # (record 0 has the long head)
            if n_records == 1000:
                drop = (0, 999) + tuple(range(300, 500))
            out.append((n_samples, n_records, (n_samples - 1,) if n_samples in (2, 65) else (), drop, n_records == 65))
    return out

"""Helper of the deep-sum and high-plane tests (test_deep_planes_cpu.py, test_gpu_deep_planes.py): the inputs -- an F-tiny index
whose allele frequencies are seeded bytes, exact sums far above the 6-bit cap -- and what the oracle makes of them.  Every expected
value comes from oracle.oracle (OracleIndex, O.call) and numpy; nothing here touches the library under test.

Why other frequencies: every fixture's frequencies come from synth.make_snps, p and 1 - p, and on F-tiny with its own counts no
called site has a confidence outside (0, 1) or a -10 ln c near an integer -- the device caller settles every site and the branch
of vg_sample_calls_fetch that fetches the clamped counters and recomputes on the host never runs (conditions() states it, the CPU
file asserts it).  Independent bytes for both frequencies give 1 - rr - aa < 0 at a good part of the sites: a negative confidence,
the reference's INT_MIN in the GQ column, and a site the device must hand to the host."""
import numpy as np

from oracle import oracle as O

INT_MIN = -2147483648
CAP = 63
# sums around the cap, the byte, the half word, the sign bit and the top of a u32
DEEP = np.array([0, 1, 62, 63, 64, 127, 128, 255, 256, 65535, 65536, 2**31 - 1, 2**31, 2**32 - 1], np.uint32)
DEEP_U8 = np.array([0, 1, 62, 63, 64, 127, 128, 254, 255], np.uint8)
FREQ_SEED = 20261020                       # the seeds the CPU file holds the conditions for
SUMS_SEED = 20261021
OTHER_SEED = 20261022                      # a second array of sums, for the plane that stays selected
U8_SEED = 20261023
N_PLANES = 300


def freq_arrays(prefix, seed=FREQ_SEED):
    """index_io.read_index(prefix) with snp_rf / snp_af replaced by seeded bytes, 0..255, drawn independently for every dictionary
    entry (entries of one site disagree: OracleIndex.from_arrays(a).sites() applies the reference's last-writer-wins rule)."""
    from vargeno_amd import index_io

    a = index_io.read_index(prefix)
    rng = np.random.default_rng(seed)
    n = len(a["snp_kmer"])
    a["snp_rf"] = rng.integers(0, 256, n).astype(np.uint8)
    a["snp_af"] = rng.integers(0, 256, n).astype(np.uint8)
    return a


def deep_sums(n_sites, seed=SUMS_SEED):
    """uint32[2 * n_sites] laid out as a plane's exact sums (ref, alt interleaved): a third of the sites (deep, shallow 0..63), a
    third (shallow, deep), a third (deep, deep) -- a pair saturated on both sides is not called, so (deep, deep) alone would leave
    most sites without a call."""
    rng = np.random.default_rng(seed)
    deep = rng.choice(DEEP, size=(n_sites, 2))
    shallow = rng.integers(0, CAP + 1, size=(n_sites, 2)).astype(np.uint32)
    kind = rng.permutation(n_sites) % 3
    out = deep.copy()
    out[kind == 0, 1] = shallow[kind == 0, 1]
    out[kind == 1, 0] = shallow[kind == 1, 0]
    return np.ascontiguousarray(out.reshape(-1), dtype=np.uint32)


def u8_case(seed=U8_SEED, n_freq=50):
    """Flat arrays for vg_call_device: every pair of DEEP_U8 counters (81) crossed with n_freq seeded frequency pairs."""
    rng = np.random.default_rng(seed)
    rc, ac = [x.reshape(-1) for x in np.meshgrid(DEEP_U8, DEEP_U8, indexing="ij")]
    rf, af = rng.integers(0, 256, n_freq).astype(np.uint8), rng.integers(0, 256, n_freq).astype(np.uint8)
    return np.tile(rc, n_freq), np.tile(ac, n_freq), np.repeat(rf, len(rc)), np.repeat(af, len(rc))


def clamp(sums):
    """(ref, alt) uint8 columns: min(sum, 63)."""
    c = np.minimum(np.asarray(sums, np.uint32), CAP).astype(np.uint8)
    return c[0::2].copy(), c[1::2].copy()


def oracle_calls(rc, ac, rf, af):
    """O.call over arrays -> gt uint8, gq int32 (0 where nothing is called, the reference's INT_MIN where its logarithm had a
    negative argument), confidence float64."""
    want = [O.call(rc[i], ac[i], rf[i], af[i]) for i in range(len(rc))]
    gt = np.array([w[0] for w in want], dtype=np.uint8)
    conf = np.array([w[1] for w in want], dtype=np.float64)
    gq = np.where(gt != 0, np.array([w[2] for w in want], dtype=np.int64), 0).astype(np.int32)
    return gt, gq, conf


def conditions(gt, conf, eps):
    """(called, forced, near): called sites, those among them whose confidence is not inside (0, 1) -- the device cannot settle
    them --, and those inside whose -10 ln c lies within eps of an integer -- the device may hand them over."""
    called = gt != 0
    inside = (conf > 0) & (conf < 1)
    y = -10 * np.log(conf[called & inside])
    return int(called.sum()), int((called & ~inside).sum()), int((np.abs(y - np.round(y)) < eps).sum())


def take(r, idx):
    """The reads idx of r, in that order, as a batch of their own."""
    from vargeno_amd.synth import Reads

    o = r.offsets.astype(np.int64)
    idx = np.asarray(idx, np.int64)
    lens = (o[1:] - o[:-1])[idx]
    pick = np.concatenate([np.arange(o[i], o[i + 1]) for i in idx]) if len(idx) else np.zeros(0, np.int64)
    return Reads(r.bases[pick], r.quals[pick], np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64))


def take_many(batches):
    """Several batches as one, in that order."""
    from vargeno_amd.synth import Reads

    lens = np.concatenate([np.diff(b.offsets.astype(np.int64)) for b in batches])
    return Reads(np.concatenate([b.bases for b in batches]), np.concatenate([b.quals for b in batches]),
                 np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64))


def oracle_counts(ox, r):
    """One loaded OracleIndex, reset, run on r alone -> (ref_cnt, alt_cnt) uint8 copies."""
    ox.reset()
    ox.process(r.bases, r.quals, r.offsets)
    so = ox.sites()
    return so["ref_cnt"].copy(), so["alt_cnt"].copy()


def round_robin(r, n_planes=N_PLANES):
    """Read i goes to plane i % n_planes: the planes' batches, in plane order."""
    return [take(r, np.arange(s, r.n, n_planes)) for s in range(n_planes)]

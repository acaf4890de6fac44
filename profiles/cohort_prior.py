"""The cohort prior's first measurement: the prior kernel (vg_cprior_run) against the header's host loop (vg_cprior_host).

    python profiles/cohort_prior.py [--sites 10000000] [--samples 64] [--threads 16] [--iters 8] [--out profiles/cohort_prior.txt]

The cohort is synthetic: a block of 2^20 sites (a true alt frequency per site, Hardy-Weinberg genotypes, Poisson(7.1) depth, 1 %
errors, dictionary frequencies unrelated to the truth) repeated up to --sites.  Reported: the uploads of the counters (vg_cprior_set
per sample), the kernel's own time (the library's VG_VERBOSE line, taken from stderr), the whole vg_cprior_run call, the read-back
of the calls (vg_cprior_calls per sample), and the host loop on --threads threads; then q is compared as bit patterns and the calls
of every sample for equality.  There is no threshold: it is a record, taken against the host loop."""
import argparse
import os
import re
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def cohort(n_sites, n_samples, seed=1):
    rng = np.random.default_rng(seed)
    block = min(n_sites, 1 << 20)
    q = rng.beta(0.5, 0.5, block)
    g = (rng.random((n_samples, block)) < q).astype(np.int8) + (rng.random((n_samples, block)) < q)
    depth = rng.poisson(7.1, (n_samples, block))
    alt = rng.binomial(depth, np.where(g == 0, 0.01, np.where(g == 1, 0.5, 0.99)))
    ref = np.minimum(depth - alt, 63).astype(np.uint8)
    alt = np.minimum(alt, 63).astype(np.uint8)
    reps = -(-n_sites // block)
    tile = lambda a: np.ascontiguousarray(np.tile(a, (1, reps))[:, :n_sites])
    rf, af = rng.integers(0, 256, n_sites).astype(np.uint8), rng.integers(0, 256, n_sites).astype(np.uint8)
    return tile(ref), tile(alt), rf, af


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=10_000_000)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.environ["VG_VERBOSE"] = "1"
    from vargeno_amd import api

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("cohort prior: %d sites x %d samples, %d iterations, pseudo %g" % (a.sites, a.samples, a.iters, api.CPRIOR_PSEUDO))
    t0 = time.time()
    ref, alt, rf, af = cohort(a.sites, a.samples)
    say("synthetic cohort made in %.1f s; informative entries: %.1f %%" % (time.time() - t0, 100.0 * float(((ref | alt) != 0).mean())))

    with api.CohortPrior(a.sites, a.samples, device=a.device) as cp:
        say("device bytes: %d" % cp.device_bytes)
        t0 = time.time()
        for s in range(a.samples):
            cp.set(s, ref[s], alt[s])
        say("vg_cprior_set x %d: %.3f s" % (a.samples, time.time() - t0))
        kernel_ms = []
        for rep in range(3):
            with tempfile.TemporaryFile() as tmp:                                # the library's VG_VERBOSE line carries the kernel's own time
                sys.stderr.flush()
                keep = os.dup(2)
                os.dup2(tmp.fileno(), 2)
                try:
                    t0 = time.time()
                    q = cp.run(rf, af, iters=a.iters)
                    wall = time.time() - t0
                finally:
                    os.dup2(keep, 2)
                    os.close(keep)
                tmp.seek(0)
                m = re.search(r"kernel ([0-9.]+) ms", tmp.read().decode(errors="replace"))
            kernel_ms.append(float(m.group(1)) if m else float("nan"))
            say("vg_cprior_run %d: kernel %.3f ms, whole call %.3f s, %d entries left to the host" % (rep, kernel_ms[-1], wall, cp.n_escaped))
        t0 = time.time()
        cols = [cp.calls(s) for s in range(a.samples)]
        say("vg_cprior_calls x %d: %.3f s" % (a.samples, time.time() - t0))
    best = min(kernel_ms)
    say("kernel, best of 3: %.3f ms = %.3e sample-sites/s" % (best, a.sites * a.samples / (best * 1e-3)))

    t0 = time.time()
    gt, gq, qh = api.cohort_prior_host(ref, alt, rf, af, iters=a.iters, threads=a.threads)
    host = time.time() - t0
    say("vg_cprior_host on %d threads: %.3f s = %.3e sample-sites/s; kernel / host loop: %.1f x" % (a.threads, host, a.sites * a.samples / host, host / (best * 1e-3)))
    same_q = bool(np.array_equal(q.view(np.uint64), qh.view(np.uint64)))
    same_calls = all(np.array_equal(cols[s][0], gt[s]) and np.array_equal(cols[s][1], gq[s]) for s in range(a.samples))
    say("q bit-identical: %s; calls equal: %s" % (same_q, same_calls))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if same_q and same_calls else 1


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""The pair kernel at cohort scale: a recipe, not part of bench.py.

    python3 profiles/pairs_bench.py [--sites 10000000] [--out profiles/pairs.txt]

Fills a genotype matrix from a seed at --sites sites for N in {8, 64, 1024} samples and times vg_gmatrix_pairs: the median of five
calls after one warm-up, the time being the library's own (HIP events around the memset and the two kernels, printed under
VG_VERBOSE).  vg_pairs_host is timed on 16 threads at N = 64 only; its pair-word rate is what the other sizes are compared with.
A pair-word is one 64-site word of one unordered pair, diagonal included: N (N + 1) / 2 x ceil(sites / 64) per table.
The kernel's VALU instructions per pair-word are read from the library's gfx950 code (the body of the word loop, 16 pairs per lane
and pass); with a wave64 VALU instruction issuing in 2 cycles on each of the 4 SIMDs of the 256 CUs that gives the issue-rate bound
at the device's peak clock of 2.4 GHz.  The shader clock level the device reports after the timed calls is printed beside it and is
no part of the bound: the first run showed 2 402, 217 and 158 MHz there -- by the time it is read the device has idled down."""
import argparse
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LLVM = "/opt/rocm/lib/llvm/bin"
CUS, SIMDS, CYCLES_PER_VALU, LANES, PAIRS_PER_LANE = 256, 4, 2, 64, 16
PEAK_HZ = 2.4e9


def valu_per_pair_word(lib_path):
    """VALU instructions in the pair kernel's innermost loop (the backward branch whose body holds the LDS reads) over 16 pairs."""
    with tempfile.TemporaryDirectory() as t:
        fb, co = os.path.join(t, "fb.bin"), os.path.join(t, "co.o")
        subprocess.check_call([LLVM + "/llvm-objcopy", "--dump-section", ".hip_fatbin=" + fb, lib_path, os.path.join(t, "discard.so")])
        subprocess.check_call([LLVM + "/clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fb, "--output=" + co, "--unbundle"])
        text = subprocess.check_output([LLVM + "/llvm-objdump", "-d", co], text=True)
    body = text[text.index("vg_pairs_kernel"):]
    body = body[:body.index("\n\n") if "\n\n" in body else len(body)]
    ins = []                                                # (address, mnemonic, text)
    for ln in body.splitlines():
        m = re.match(r"\s+(\S+)\s.*//\s*([0-9A-Fa-f]+):", ln + " ")
        if m:
            ins.append((int(m.group(2), 16), m.group(1), ln))
    base = ins[0][0]
    best = None
    for k, (addr, op, ln) in enumerate(ins):
        m = re.search(r"\+0x([0-9a-f]+)>", ln)
        if op.startswith("s_cbranch") and m and base + int(m.group(1), 16) < addr:
            loop = [i for i in ins if base + int(m.group(1), 16) <= i[0] <= addr]
            if any(i[1].startswith("ds_read") for i in loop) and (best is None or len(loop) < len(best)):
                best = loop
    if best is None:
        raise RuntimeError("no word loop found in vg_pairs_kernel")
    valu = sum(1 for i in best if i[1].startswith("v_"))
    return valu / PAIRS_PER_LANE, valu, len(best)


def device_clock_hz():
    """The shader clock the device reports now (its current DPM level, which after a short kernel is an idle one), or None."""
    import glob

    for f in sorted(glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk")):
        try:
            for ln in open(f):
                if "*" in ln:
                    return float(re.search(r"(\d+)\s*Mhz", ln, re.I).group(1)) * 1e6
        except Exception:
            pass
    return None


class stderr_to:
    """File descriptor 2 into a file for the length of the block: the library prints its timing there."""

    def __init__(self, path):
        self.path = path

    def __enter__(self):
        sys.stderr.flush()
        self.saved = os.dup(2)
        self.fd = os.open(self.path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
        os.dup2(self.fd, 2)

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.fd)
        os.close(self.saved)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=10_000_000)
    ap.add_argument("--samples", type=int, nargs="*", default=[8, 64, 1024])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairs.txt"))
    a = ap.parse_args()
    os.environ["VG_VERBOSE"] = "1"
    from vargeno_amd import _lib, api

    if _lib.lib().vg_device_count() < 1:
        sys.exit("pairs_bench: no HIP device: nothing is measured without one")
    per_pw, valu, loop_len = valu_per_pair_word(_lib.LIB_PATH)
    words = (a.sites + 63) // 64
    rng = np.random.default_rng(2024)
    base_gt = rng.integers(1, 4, size=a.sites).astype(np.uint8)
    base_gt[rng.random(a.sites) < 0.1] = 0
    base_gq = rng.integers(0, 99, size=a.sites).astype(np.int32)
    lines = ["pair kernel, %d sites (%d words), seed 2024; pair-words = N (N + 1) / 2 x words" % (a.sites, words),
             "word loop of vg_pairs_kernel: %d VALU of %d instructions per pass over 16 pairs = %.2f VALU per pair-word" % (valu, loop_len, per_pw)]
    log = os.path.join(tempfile.gettempdir(), "pairs_bench_stderr.txt")
    rates = {}
    for n in a.samples:
        with api.GenotypeMatrix(a.sites, n) as gm:
            for s in range(n):                                       # sample s: the base sample rotated, a tenth of it redrawn
                gt = np.roll(base_gt, 9973 * s)
                gt[s % 10::10] = base_gt[s % 10::10][::-1]
                gm.set(s, gt, np.roll(base_gq, 7919 * s), min_gq=10)
            ms = []
            for it in range(6):
                with stderr_to(log):
                    gm.pairs()
                m = re.search(r"kernels ([0-9.]+) ms", open(log).read())
                if it:
                    ms.append(float(m.group(1)))
            clock = device_clock_hz()
            med = float(np.median(ms))
            pw = n * (n + 1) / 2 * words
            rates[n] = pw / (med * 1e-3)
            bound = CUS * SIMDS * LANES / CYCLES_PER_VALU * PEAK_HZ / per_pw
            lines.append("N = %4d: kernels %.3f ms (median of 5: %s), %.3e pair-words/s; issue-rate bound at the peak %.0f MHz %.3e: %.1f %% of it (clock level read afterwards: %s); matrix %.2f GB"
                         % (n, med, " ".join("%.3f" % v for v in ms), rates[n], PEAK_HZ / 1e6, bound, 100 * rates[n] / bound, "%.0f MHz" % (clock / 1e6) if clock else "none reported", gm.device_bytes / 1e9))
    # the host loop: N = 64 only, 16 threads
    n = 64
    gt = np.stack([np.roll(base_gt, 9973 * s) for s in range(n)])
    gq = np.stack([np.roll(base_gq, 7919 * s) for s in range(n)])
    t0 = time.perf_counter()
    api.pairs_host(gt, gq, min_gq=10, threads=16)
    dt = time.perf_counter() - t0
    host = n * (n + 1) / 2 * words / dt
    lines.append("vg_pairs_host, N = 64, 16 threads: %.3f s (pack and count), %.3e pair-words/s" % (dt, host))
    for k in a.samples:
        lines.append("N = %4d: device / host pair-word rate = %.0f x (host: %.1f s at its N = 64 rate)" % (k, rates[k] / host, k * (k + 1) / 2 * words / host))
    if 8 in rates and 1024 in rates and rates[8] < 0.1 * rates[1024]:
        lines.append("N = 8 runs at %.1f %% of N = 1024's pair-word rate: under a tenth -- the site split does not fill the device at that size" % (100 * rates[8] / rates[1024]))
    open(a.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()

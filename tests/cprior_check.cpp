// cprior_check.cpp -- the host loop of csrc/vg_cprior.h under AddressSanitizer + UBSan (tests/test_cprior_cpu.py compiles and runs
// it): every array is a heap array of exactly its size, and the result is compared with a naive loop that writes the rule out per
// site with plain arrays of likelihoods, counts the informative samples first and never stops early.  Shapes: n_sites in
// {0, 1, 63, 64, 65, 257} x n_samples in {1, 2, 3, 24}, counters up to 255 (clamped by the loop), every frequency byte, iters in
// {1, 8, 64}, pseudo in {0, 2}, one and three threads, with and without q_out.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "vg_cprior.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n)
{
	rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
	return (uint32_t)((rng_state >> 20) % n);
}

static double naive_clamp(double x) { return fmin(fmax(x, 1e-6), 1 - 1e-6); }

static void naive(const vg_caller_tables &t, const uint8_t *ref_cnt, const uint8_t *alt_cnt, size_t n_sites, size_t n_samples, const uint8_t *rf, const uint8_t *af, int iters, double pseudo,
                  uint8_t *gt, int32_t *gq, double *q_out)
{
	std::vector<double> l0(n_samples), l1(n_samples), l2(n_samples), dp(n_samples);
	std::vector<char> inf(n_samples);
	for (size_t site = 0; site < n_sites; site++) {
		unsigned m = 0;
		for (size_t s = 0; s < n_samples; s++) {
			unsigned r = ref_cnt[s * n_sites + site], a = alt_cnt[s * n_sites + site];
			if (r > 63) r = 63;
			if (a > 63) a = 63;
			inf[s] = (r | a) != 0 && !(r == 63 && a == 63);
			m += inf[s] ? 1 : 0;
			l0[s] = t.keep[r] * t.flip[a]; l1[s] = t.half[r + a]; l2[s] = t.flip[r] * t.keep[a]; dp[s] = t.depth[r + a];
		}
		const double pr = t.freq[rf[site]], pa = t.freq[af[site]], sum_f = pr + pa, qd = sum_f > 0 ? pa / sum_f : 0.5;
		double q = naive_clamp(qd);
		for (int it = 0; m > 0 && it < iters; it++) {
			const double u = 1 - q, g0 = u * u, g1 = (q * u) + (q * u), g2 = q * q;
			double e = 0;
			for (size_t s = 0; s < n_samples; s++) {
				if (!inf[s]) continue;
				const double w0 = g0 * l0[s], w1 = g1 * l1[s], w2 = g2 * l2[s], sum = (w0 + w1) + w2;
				e = e + (w1 + (w2 + w2)) / sum;
			}
			q = naive_clamp((e + pseudo * qd) / ((double)(2 * m) + pseudo));
		}
		q_out[site] = q;
		const double u = 1 - q, g0 = u * u, g1 = (q * u) + (q * u), g2 = q * q;
		for (size_t s = 0; s < n_samples; s++) {
			uint8_t g = 0;
			int32_t quality = 0;
			if (inf[s]) {
				const double w0 = g0 * l0[s], w1 = g1 * l1[s], w2 = g2 * l2[s], sum = (w0 + w1) + w2;
				double top = w2;
				g = VGC_HOM_ALT;
				if (w0 > w1 && w0 > w2) { g = VGC_HOM_REF; top = w0; }
				else if (w1 > w0 && w1 > w2) { g = VGC_HET; top = w1; }
				quality = (int)(-10 * log((top / sum) * dp[s]));
			}
			gt[s * n_sites + site] = g;
			gq[s * n_sites + site] = quality;
		}
	}
}

template <class T>
static std::unique_ptr<T[]> exact(size_t n) { return std::unique_ptr<T[]>(new T[n]); }       // (new T[0] is a valid, unreadable pointer)

int main()
{
	vg_caller_tables t;
	vg_caller_tables_fill(t);
	const size_t SITES[] = {0, 1, 63, 64, 65, 257}, SAMPLES[] = {1, 2, 3, 24};
	const int ITERS[] = {1, 8, 64};
	const double PSEUDO[] = {0.0, 2.0};
	unsigned long cases = 0, differ_from_single = 0, called = 0;
	for (size_t n_sites : SITES)
		for (size_t n_samples : SAMPLES) {
			auto r = exact<uint8_t>(n_sites * n_samples), a = exact<uint8_t>(n_sites * n_samples), rf = exact<uint8_t>(n_sites), af = exact<uint8_t>(n_sites);
			for (size_t k = 0; k < n_sites * n_samples; k++) {
				const uint32_t kind = rnd(16);
				r[k] = kind == 0 ? 0 : kind == 1 ? 63 : kind == 2 ? 255 : (uint8_t)rnd(kind < 10 ? 12 : 64);
				a[k] = kind == 0 ? 0 : kind == 1 ? 63 : kind == 2 ? 200 : (uint8_t)rnd(kind < 10 ? 12 : 64);
			}
			for (size_t k = 0; k < n_sites; k++) { rf[k] = (uint8_t)rnd(256); af[k] = (uint8_t)rnd(256); }
			if (n_sites > 2) { rf[0] = af[0] = 0; rf[1] = af[1] = 255; rf[2] = 255; af[2] = 0; }
			if (n_sites > 4) for (size_t s = 0; s < n_samples; s++) { r[s * n_sites + 3] = a[s * n_sites + 3] = 0; r[s * n_sites + 4] = a[s * n_sites + 4] = 63; }
			for (int iters : ITERS)
				for (double pseudo : PSEUDO) {
					auto want_gt = exact<uint8_t>(n_sites * n_samples); auto want_gq = exact<int32_t>(n_sites * n_samples); auto want_q = exact<double>(n_sites);
					naive(t, r.get(), a.get(), n_sites, n_samples, rf.get(), af.get(), iters, pseudo, want_gt.get(), want_gq.get(), want_q.get());
					for (int threads : {1, 3})
						for (int with_q : {1, 0}) {
							auto gt = exact<uint8_t>(n_sites * n_samples); auto gq = exact<int32_t>(n_sites * n_samples); auto q = exact<double>(with_q ? n_sites : 0);
							vg_cprior_host_run(r.get(), a.get(), n_sites, (uint32_t)n_samples, rf.get(), af.get(), iters, pseudo, threads, gt.get(), gq.get(), with_q ? q.get() : nullptr);
							if (memcmp(gt.get(), want_gt.get(), n_sites * n_samples) || memcmp(gq.get(), want_gq.get(), n_sites * n_samples * sizeof(int32_t)) ||
							    (with_q && memcmp(q.get(), want_q.get(), n_sites * sizeof(double)))) {
								printf("MISMATCH n_sites %zu n_samples %zu iters %d pseudo %g threads %d\n", n_sites, n_samples, iters, pseudo, threads);
								return 1;
							}
							cases++;
						}
					if (iters == 8 && pseudo == 2.0)
						for (size_t k = 0; k < n_sites * n_samples; k++) {
							const vg_site_call c = vg_call_site(t, r[k], a[k], rf[k % n_sites], af[k % n_sites]);
							called += c.gt != VGC_NONE;
							differ_from_single += c.gt != want_gt[k];
						}
				}
		}
	if (differ_from_single == 0) { printf("the cohort's calls are the single-sample caller's\n"); return 1; }
	printf("ok: %lu cases, %lu of %lu calls differ from the single-sample caller's\n", cases, differ_from_single, called);
	return 0;
}

// vg_cprior.h -- the cohort prior: the samples of a joint run re-called with an allele frequency estimated from the cohort itself,
// once, for the host loop and the device kernel.  No reference counterpart (the reference calls one sample per process, with the
// Hardy-Weinberg prior of the two frequencies the dictionary stores; vg_caller.h).
//
// Per site the inputs are the dictionary's ref_freq and alt_freq (n/255) and, for every sample s in index order, its counters
// (r, a) clamped at 63.  A sample is INFORMATIVE at the site iff (r | a) != 0 && !(r == 63 && a == 63): vg_call_site's own "not
// called" rule.  With the per-count factors of vg_caller_tables (keep, flip, half, depth, freq):
//
//   L0 = keep[r] * flip[a];   L1 = half[r + a];   L2 = flip[r] * keep[a]                  the three likelihoods of a sample
//   pr = freq[ref_freq]; pa = freq[alt_freq]; t = pr + pa;   qd = t > 0 ? pa / t : 0.5     the dictionary's alt frequency
//   clamp(x) = min(max(x, 1e-6), 1 - 1e-6)
//   m = informative samples of the site;   q = clamp(qd)
//   if m > 0, `iters` times (EM over the genotype posteriors):
//       u = 1 - q;  g0 = u * u;  g1 = (q * u) + (q * u);  g2 = q * q                       Hardy-Weinberg at q
//       e = 0;  for s = 0 .. N-1, informative only:
//           w0 = g0 * L0;  w1 = g1 * L1;  w2 = g2 * L2;  sum = (w0 + w1) + w2
//           e = e + (w1 + (w2 + w2)) / sum                                                  expected alt alleles of s
//       q = clamp((e + pseudo * qd) / ((double)(2 * m) + pseudo))
//   the call of an informative sample, with the last q: w0, w1, w2, sum as above; the strict maximum wins, hom-ref tested before
//       het, anything else (ties included) is hom-alt -- as vg_call_site chooses; confidence = (top / sum) * depth[r + a];
//       gq = (int)(-10 ln(confidence))
//   a sample that is not informative: gt 0, gq 0
//
// `pseudo` is the weight of the dictionary's frequency in alleles (2.0, one diploid pseudo-sample, by default: a cohort of three
// does not overrule the SNP list); finite and >= 0.  `iters` is 1 .. 64 (8 by default).  sum is positive over the whole domain: the
// het term alone is at least 2e-6 * 2^-126.  The confidence keeps the reference's Poisson depth factor, so a GQ threshold means
// what it means in a per-sample file.  A site may stop early when an iteration returns the bit pattern of the q it started from:
// every later iteration would return it again.
//
// Host and device give the same bits by vg_caller.h's three rules: the factors come from the table the HOST filled (uploaded, never
// recomputed on the device); the arithmetic is f64 add, subtract, multiply, divide and compare, in exactly the order written above,
// under `fp contract(off)`; the logarithm is not shared -- the kernel settles a call only when vg_gq_settled holds for its own log
// and leaves VG_CALL_ESCAPE otherwise, and the host recomputes those entries from (r, a) and the site's final q with libm.
//
// Words: a sample's counters at a site are one uint16, r | a << 8; its call is one uint16, gt << 14 | gq (vg_caller.h).
#pragma once
#include <stdint.h>
#include <string.h>

#include <thread>
#include <vector>

#include "vg_caller.h"

#if defined(__HIPCC__)
#define VG_CPRIOR_HD __host__ __device__
#else
#define VG_CPRIOR_HD
#endif

#ifndef VG_CPRIOR_ITERS                  // (include/vargeno_hip.h states the same three for its callers)
#define VG_CPRIOR_ITERS     8
#define VG_CPRIOR_PSEUDO    2.0
#define VG_CPRIOR_ITERS_MAX 64
#endif
#define VG_CPRIOR_Q_MIN 1e-6

// The factors the rule takes per sample.  They are the first four members of vg_caller_tables, in its order: a kernel stages
// sizeof(vg_cprior_factors) bytes of the uploaded table (3 056; the 256 frequencies are read once per site, from the table itself).
struct vg_cprior_factors {
	double keep[VGC_CAP + 1];
	double flip[VGC_CAP + 1];
	double half[2 * VGC_CAP + 1];
	double depth[2 * VGC_CAP + 1];
};
static_assert(sizeof(vg_cprior_factors) == (2 * (VGC_CAP + 1) + 2 * (2 * VGC_CAP + 1)) * sizeof(double), "vg_cprior_factors has no padding");
static_assert(sizeof(vg_cprior_factors) + 256 * sizeof(double) == sizeof(vg_caller_tables), "vg_cprior_factors is the head of vg_caller_tables");

VG_CPRIOR_HD inline uint16_t vg_cprior_word(unsigned ref_cnt, unsigned alt_cnt)
{
	if (ref_cnt > VGC_CAP) ref_cnt = VGC_CAP;
	if (alt_cnt > VGC_CAP) alt_cnt = VGC_CAP;
	return (uint16_t)(ref_cnt | alt_cnt << 8);
}
VG_CPRIOR_HD inline bool vg_cprior_informative(unsigned word)
{
	const unsigned r = word & 0xFF, a = word >> 8;
	return (r | a) != 0 && !(r == VGC_CAP && a == VGC_CAP);
}
VG_CPRIOR_HD inline double vg_cprior_clamp(double x)
{
	const double lo = VG_CPRIOR_Q_MIN, hi = 1.0 - VG_CPRIOR_Q_MIN;
	x = x < lo ? lo : x;
	return x > hi ? hi : x;
}
// the dictionary's alt frequency from the two freq[] entries of the site
VG_CPRIOR_HD inline double vg_cprior_qd(double pr, double pa)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	const double t = pr + pa;
	return t > 0 ? pa / t : 0.5;
}

// Hardy-Weinberg at q, and a sample's three weights under it
struct vg_cprior_hw { double g0, g1, g2; };
VG_CPRIOR_HD inline vg_cprior_hw vg_cprior_hw_at(double q)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	const double u = 1.0 - q;
	vg_cprior_hw g;
	g.g0 = u * u;
	g.g1 = (q * u) + (q * u);
	g.g2 = q * q;
	return g;
}
struct vg_cprior_weights { double w0, w1, w2, sum; };
template <class F>
VG_CPRIOR_HD inline vg_cprior_weights vg_cprior_weigh(const F &f, const vg_cprior_hw &g, unsigned word)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	const unsigned r = word & 0xFF, a = word >> 8;
	const double l0 = f.keep[r] * f.flip[a], l1 = f.half[r + a], l2 = f.flip[r] * f.keep[a];
	vg_cprior_weights w;
	w.w0 = g.g0 * l0;
	w.w1 = g.g1 * l1;
	w.w2 = g.g2 * l2;
	w.sum = (w.w0 + w.w1) + w.w2;
	return w;
}

// The site's final q.  word(s) hands out sample s's counter word; f: the factors (vg_caller_tables or vg_cprior_factors).  The
// informative samples are counted in the first pass over them, so the samples are read `iterations run` times, not once more.
template <class F, class W>
VG_CPRIOR_HD inline double vg_cprior_site_q(const F &f, W word, uint32_t n_samples, double qd, int iters, double pseudo)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	double q = vg_cprior_clamp(qd);
	for (int it = 0; it < iters; it++) {
		const vg_cprior_hw g = vg_cprior_hw_at(q);
		double e = 0;
		uint32_t m = 0;
		for (uint32_t s = 0; s < n_samples; s++) {
			const unsigned c = word(s);
			if (!vg_cprior_informative(c)) continue;
			const vg_cprior_weights w = vg_cprior_weigh(f, g, c);
			e = e + (w.w1 + (w.w2 + w.w2)) / w.sum;
			m++;
		}
		if (m == 0) break;                                       // no informative sample: q stays clamp(qd)
		const double next = vg_cprior_clamp((e + pseudo * qd) / ((double)(2 * m) + pseudo));
		uint64_t was, is;
		memcpy(&was, &q, 8); memcpy(&is, &next, 8);
		q = next;
		if (was == is) break;                                    // a fixed point: every later iteration returns it again
	}
	return q;
}

// the call of one sample under the site's final Hardy-Weinberg weights (gt VGC_NONE, confidence 0 for a sample that is not informative)
template <class F>
VG_CPRIOR_HD inline vg_site_call vg_cprior_call(const F &f, const vg_cprior_hw &g, unsigned word)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	vg_site_call out{VGC_NONE, 0.0};
	if (!vg_cprior_informative(word)) return out;
	const vg_cprior_weights w = vg_cprior_weigh(f, g, word);
	int best = 2;
	if (w.w0 > w.w1 && w.w0 > w.w2) best = 0;
	else if (w.w1 > w.w0 && w.w1 > w.w2) best = 1;
	out.gt = best == 0 ? VGC_HOM_REF : best == 1 ? VGC_HET : VGC_HOM_ALT;
	const double top = best == 0 ? w.w0 : best == 1 ? w.w1 : w.w2;
	out.confidence = (top / w.sum) * f.depth[(word & 0xFF) + (word >> 8)];
	return out;
}

// ---- the host loop (plain host functions; a device compiler only parses them) ----
// Sites [lo, hi): ref_cnt, alt_cnt are [n_samples][n_sites] (clamped here), gt, gq likewise, q_out (may be NULL) per site.
inline void vg_cprior_host_range(const vg_caller_tables &t, const uint8_t *ref_cnt, const uint8_t *alt_cnt, uint64_t n_sites, uint32_t n_samples, const uint8_t *ref_freq, const uint8_t *alt_freq,
                                 int iters, double pseudo, uint64_t lo, uint64_t hi, uint8_t *gt, int32_t *gq, double *q_out)
{
	for (uint64_t site = lo; site < hi; site++) {
		auto word = [&](uint32_t s) -> unsigned { return vg_cprior_word(ref_cnt[(uint64_t)s * n_sites + site], alt_cnt[(uint64_t)s * n_sites + site]); };
		const double q = vg_cprior_site_q(t, word, n_samples, vg_cprior_qd(t.freq[ref_freq[site]], t.freq[alt_freq[site]]), iters, pseudo);
		if (q_out) q_out[site] = q;
		const vg_cprior_hw g = vg_cprior_hw_at(q);
		for (uint32_t s = 0; s < n_samples; s++) {
			const vg_site_call c = vg_cprior_call(t, g, word(s));
			gt[(uint64_t)s * n_sites + site] = c.gt;
			gq[(uint64_t)s * n_sites + site] = c.gt == VGC_NONE ? 0 : vg_genotype_quality(c.confidence);
		}
	}
}

// The whole matrix on `threads` host threads (< 1: one), each a contiguous range of sites.  Throws what std::thread throws.
inline void vg_cprior_host_run(const uint8_t *ref_cnt, const uint8_t *alt_cnt, uint64_t n_sites, uint32_t n_samples, const uint8_t *ref_freq, const uint8_t *alt_freq, int iters, double pseudo, int threads,
                               uint8_t *gt, int32_t *gq, double *q_out)
{
	vg_caller_tables t;
	vg_caller_tables_fill(t);
	const uint64_t T = threads < 1 ? 1 : (uint64_t)threads > n_sites ? (n_sites ? n_sites : 1) : (uint64_t)threads;
	auto work = [&](uint64_t k) { vg_cprior_host_range(t, ref_cnt, alt_cnt, n_sites, n_samples, ref_freq, alt_freq, iters, pseudo, n_sites * k / T, n_sites * (k + 1) / T, gt, gq, q_out); };
	std::vector<std::thread> th;
	for (uint64_t k = 1; k < T; k++) th.emplace_back(work, k);
	work(0);
	for (auto &x : th) x.join();
}

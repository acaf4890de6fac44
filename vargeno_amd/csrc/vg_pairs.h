// vg_pairs.h -- pairwise sample comparison over the cohort's genotype matrix, once, for the host loop and the device kernels.
//
// Input per sample: the final calls of vg_sample_calls_fetch, gt (0 not called, 1 hom-ref, 2 hom-alt, 3 het) and gq per site.
//   * a call is COUNTED iff gt != 0 && gq >= min_gq (so the reference's accidental gq of -2147483648 is never counted for
//     min_gq >= 0); a counted call is of class R (gt 1), A (gt 2) or H (gt 3); C = R | H | A;
//   * per sample three bit planes R, H, A of ceil(n_sites / 64) 64-bit words: site s is bit s & 63 of word s >> 6, the bits at and
//     beyond n_sites are zero;
//   * per pair (i, j) five counters, sums over the words: n = |Ci & Cj|, ibs0 = |Ri&Aj | Ai&Rj| (opposite
//     homozygotes), ibs2 = |Ri&Rj | Hi&Hj | Ai&Aj| (same genotype), hethet = |Hi & Hj|, het_i = |Hi & Cj| (i het where j is counted).
//     n, ibs0, ibs2 and hethet are symmetric in (i, j); het_i is not: [j][i] holds het_j.
// Everything is an integer sum, so the result does not depend on the order or the split of the work.
#pragma once
#include <stdint.h>

#include <thread>
#include <vector>

#if defined(__HIPCC__)
#define VG_PAIRS_HD __host__ __device__
#else
#define VG_PAIRS_HD
#endif

enum { VGP_N = 0, VGP_IBS0 = 1, VGP_IBS2 = 2, VGP_HETHET = 3, VGP_HET_I = 4, VGP_COUNTERS = 5 };    // the order of counts[i][j][..]
enum { VGP_R = 0, VGP_H = 1, VGP_A = 2, VGP_PLANES = 3 };

// class plane of a call: VGP_R / VGP_H / VGP_A, or -1 for a call that is not counted
VG_PAIRS_HD inline int vg_pair_class(uint8_t gt, int32_t gq, int32_t min_gq)
{
	if (gt == 0 || gt > 3 || gq < min_gq) return -1;
	return gt == 1 ? VGP_R : gt == 2 ? VGP_A : VGP_H;
}

// The per-word pair function.  The planes of a sample are DISJOINT (a call has one class), so with M = R | A (the homozygous
// calls) five popcounts per word carry all five counters of (i, j) and het_j of (j, i) -- 11 logic operations and popcounts per
// 32 bits where the definitions taken one by one need 18:
//   hh = |Hi & Hj|   x = |Hi & Mj|   y = |Mi & Hj|   mm = |Mi & Mj|   opp = |Mi & Mj & (Ri ^ Rj)|   (inside Mi & Mj, R differs = opposite)
//   n = mm + x + y + hh   ibs0 = opp   ibs2 = hh + mm - opp   hethet = hh   het_i = hh + x   het_j = hh + y
// vg_pair_word_add adds one word's terms to t[] (A: u32 in a kernel's registers, u64 on the host); vg_pair_counters turns sums of
// terms into the counters.
enum { VGT_HH = 0, VGT_X = 1, VGT_Y = 2, VGT_MM = 3, VGT_OPP = 4, VGP_TERMS = 5 };
template <class A>
VG_PAIRS_HD inline void vg_pair_popc_add(A &acc, uint64_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
	acc = (A)__builtin_popcount((uint32_t)x) + acc;                     // (each half a v_bcnt_u32_b32 that adds into the counter itself)
	acc = (A)__builtin_popcount((uint32_t)(x >> 32)) + acc;
#else
	acc += (A)__builtin_popcountll(x);
#endif
}
template <class A>
VG_PAIRS_HD inline void vg_pair_word_add(A t[VGP_TERMS], uint64_t ri, uint64_t hi, uint64_t ai, uint64_t rj, uint64_t hj, uint64_t aj)
{
	const uint64_t mi = ri | ai, mj = rj | aj, mm = mi & mj;
	vg_pair_popc_add(t[VGT_HH], hi & hj);
	vg_pair_popc_add(t[VGT_X], hi & mj);
	vg_pair_popc_add(t[VGT_Y], mi & hj);
	vg_pair_popc_add(t[VGT_MM], mm);
	vg_pair_popc_add(t[VGT_OPP], mm & (ri ^ rj));
}
// ij[VGP_COUNTERS]: the counters of (i, j); the return value is het_j, counter VGP_HET_I of (j, i)
template <class A>
VG_PAIRS_HD inline uint64_t vg_pair_counters(const A t[VGP_TERMS], uint64_t ij[VGP_COUNTERS])
{
	const uint64_t hh = t[VGT_HH], x = t[VGT_X], y = t[VGT_Y], mm = t[VGT_MM], opp = t[VGT_OPP];
	ij[VGP_N] = mm + x + y + hh;
	ij[VGP_IBS0] = opp;
	ij[VGP_IBS2] = hh + mm - opp;
	ij[VGP_HETHET] = hh;
	ij[VGP_HET_I] = hh + x;
	return hh + y;
}

// ---- the host loop (plain host functions; a device compiler only parses them) ----
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
#define VG_PAIRS_POPCNT __attribute__((target("popcnt")))      // the host tools are built for x86-64-v2, the library's host half is not
#else
#define VG_PAIRS_POPCNT
#endif

// one sample's columns -> its planes: out[VGP_R / VGP_H / VGP_A][n_words]
inline void vg_pairs_pack_host(const uint8_t *gt, const int32_t *gq, uint64_t n_sites, int32_t min_gq, uint64_t *r, uint64_t *h, uint64_t *a)
{
	const uint64_t n_words = (n_sites + 63) / 64;
	uint64_t *const plane[VGP_PLANES] = {r, h, a};
	for (uint64_t w = 0; w < n_words; w++) {
		uint64_t word[VGP_PLANES] = {0, 0, 0};
		const uint64_t end = n_sites - w * 64 < 64 ? n_sites - w * 64 : 64;
		for (uint64_t b = 0; b < end; b++) {
			const int c = vg_pair_class(gt[w * 64 + b], gq[w * 64 + b], min_gq);
			if (c >= 0) word[c] |= 1ull << b;
		}
		for (int p = 0; p < VGP_PLANES; p++) plane[p][w] = word[p];
	}
}

// rows first, first + step, ... of the table from planes[sample][VGP_PLANES][n_words]: counts[i][j] and counts[j][i] for j >= i
VG_PAIRS_POPCNT inline void vg_pairs_count_rows(const uint64_t *planes, uint64_t n_words, uint32_t n_samples, uint32_t first, uint32_t step, uint64_t *counts)
{
	for (uint32_t i = first; i < n_samples; i += step) {
		const uint64_t *ri = planes + ((uint64_t)i * VGP_PLANES + VGP_R) * n_words, *hi = ri + n_words, *ai = hi + n_words;
		for (uint32_t j = i; j < n_samples; j++) {
			const uint64_t *rj = planes + ((uint64_t)j * VGP_PLANES + VGP_R) * n_words, *hj = rj + n_words, *aj = hj + n_words;
			uint64_t t[VGP_TERMS] = {0, 0, 0, 0, 0}, sum[VGP_COUNTERS];
			for (uint64_t w = 0; w < n_words; w++) vg_pair_word_add(t, ri[w], hi[w], ai[w], rj[w], hj[w], aj[w]);
			const uint64_t het_j = vg_pair_counters(t, sum);
			uint64_t *ij = counts + ((uint64_t)i * n_samples + j) * VGP_COUNTERS, *ji = counts + ((uint64_t)j * n_samples + i) * VGP_COUNTERS;
			for (int k = 0; k < VGP_COUNTERS; k++) ji[k] = sum[k];
			ji[VGP_HET_I] = het_j;
			for (int k = 0; k < VGP_COUNTERS; k++) ij[k] = sum[k];           // (after [j][i]: on the diagonal the two are one entry)
		}
	}
}

// gt, gq: [n_samples][n_sites]; counts: [n_samples][n_samples][VGP_COUNTERS].  Packs and counts on `threads` host threads (samples,
// then rows, dealt round robin).  Throws what std::vector and std::thread throw.
inline void vg_pairs_host_run(const uint8_t *gt, const int32_t *gq, uint64_t n_sites, uint32_t n_samples, int32_t min_gq, int threads, uint64_t *counts)
{
	const uint64_t n_words = (n_sites + 63) / 64;
	std::vector<uint64_t> planes((size_t)((uint64_t)n_samples * VGP_PLANES * n_words));
	const uint32_t T = (uint32_t)(threads < 1 ? 1 : (uint32_t)threads > n_samples ? n_samples : (uint32_t)threads);
	auto work = [&](uint32_t t, int phase) {
		if (phase == 0) {
			for (uint32_t s = t; s < n_samples; s += T) {
				uint64_t *r = planes.data() + (uint64_t)s * VGP_PLANES * n_words;
				vg_pairs_pack_host(gt + (uint64_t)s * n_sites, gq + (uint64_t)s * n_sites, n_sites, min_gq, r, r + n_words, r + 2 * n_words);
			}
		} else vg_pairs_count_rows(planes.data(), n_words, n_samples, t, T, counts);
	};
	for (int phase = 0; phase < 2; phase++) {
		std::vector<std::thread> th;
		for (uint32_t t = 1; t < T; t++) th.emplace_back(work, t, phase);
		work(0, phase);
		for (auto &x : th) x.join();
	}
}

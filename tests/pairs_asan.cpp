// tests/pairs_asan.cpp -- TEST ONLY: AddressSanitizer + UBSan harness for the host half of vargeno_amd/csrc/vg_pairs.h: the pack and the
// pair count over exact-size heap arrays (any overread trips the sanitizer) against a naive per-site loop written here -- for gt drawn
// from 0 .. 3, for gt with values above 3 mixed in (they are no classes: no plane may hold them) and for saturated samples (every
// site of one class, gq at the threshold); compiled and run by tests/test_pairs_cpu.py (sanitizers run on the CPU build, in a
// program of their own).
#include <limits.h>
#include <stdio.h>
#include <random>
#include <vector>
#include "vg_pairs.h"

enum { PLAIN = 0, WILD = 1, SATURATED = 2, MODES = 3 };

static int run(int mode, uint64_t S, uint32_t N, int32_t min_gq, int threads, std::mt19937_64 &rng)
{
	const int32_t gqs[] = {-1, 0, 1, 19, 20, 21, 99, INT_MIN, INT_MAX};
	const uint8_t wild[] = {4, 5, 7, 128, 129, 130, 131, 255};
	std::vector<uint8_t> gt((size_t)(N * S));
	std::vector<int32_t> gq((size_t)(N * S));
	for (auto &g : gt) g = (uint8_t)(rng() % 4);
	for (auto &q : gq) q = gqs[rng() % 9];
	if (mode == WILD)
		for (auto &g : gt) if (rng() % 4 == 0) g = wild[rng() % 8];
	if (mode == SATURATED)                                            // sample i: class (i + 1) % 4 at every site -- R, A, H, missing, R
		for (uint32_t i = 0; i < N; i++)
			for (uint64_t s = 0; s < S; s++) { gt[i * S + s] = (uint8_t)((i + 1) % 4); gq[i * S + s] = min_gq; }
	std::vector<uint64_t> got((size_t)N * N * VGP_COUNTERS, ~0ull), want((size_t)N * N * VGP_COUNTERS, 0);
	vg_pairs_host_run(gt.data(), gq.data(), S, N, min_gq, threads, got.data());
	for (uint32_t i = 0; i < N; i++)
		for (uint32_t j = 0; j < N; j++)
			for (uint64_t s = 0; s < S; s++) {
				const uint8_t a = gt[i * S + s], b = gt[j * S + s];
				const bool ca = a >= 1 && a <= 3 && gq[i * S + s] >= min_gq, cb = b >= 1 && b <= 3 && gq[j * S + s] >= min_gq;
				uint64_t *w = &want[((size_t)i * N + j) * VGP_COUNTERS];
				if (ca && cb) {
					w[VGP_N]++;
					if ((a == 1 && b == 2) || (a == 2 && b == 1)) w[VGP_IBS0]++;
					if (a == b) w[VGP_IBS2]++;
					if (a == 3 && b == 3) w[VGP_HETHET]++;
					if (a == 3) w[VGP_HET_I]++;
				}
			}
	if (got != want) { printf("mismatch at mode=%d S=%lu N=%u min_gq=%d threads=%d\n", mode, (unsigned long)S, N, min_gq, threads); return 1; }
	if (mode == SATURATED && N >= 5) {                                // R against A: all opposite; H against R: het_i on H's side; R against R
		const uint64_t *ra = &got[(0 * N + 1) * VGP_COUNTERS], *hr = &got[(2 * N + 0) * VGP_COUNTERS], *rr = &got[(0 * N + 4) * VGP_COUNTERS];
		const bool ok = ra[VGP_N] == S && ra[VGP_IBS0] == S && ra[VGP_IBS2] == 0 && hr[VGP_N] == S && hr[VGP_HET_I] == S && hr[VGP_HETHET] == 0 && rr[VGP_IBS2] == S &&
		                got[(2 * N + 2) * VGP_COUNTERS + VGP_HETHET] == S && got[(3 * N + 3) * VGP_COUNTERS + VGP_N] == 0;
		if (!ok) { printf("saturated counters are not S at S=%lu\n", (unsigned long)S); return 1; }
	}
	const uint64_t n_words = (S + 63) / 64;
	std::vector<uint64_t> r((size_t)n_words), h((size_t)n_words), a((size_t)n_words);
	for (uint32_t i = 0; i < N; i++) {
		const uint8_t *g = gt.data() + i * S;
		const int32_t *q = gq.data() + i * S;
		vg_pairs_pack_host(g, q, S, min_gq, r.data(), h.data(), a.data());
		// the tail bits of the last word are zero
		if (S % 64 && ((r[n_words - 1] | h[n_words - 1] | a[n_words - 1]) >> (S % 64))) { printf("tail bits set at S=%lu\n", (unsigned long)S); return 1; }
		// a plane holds the sites of its own gt value at or above the threshold and nothing else: no value above 3
		for (uint64_t s = 0; s < S; s++) {
			const bool counted = q[s] >= min_gq;
			const uint64_t bit = 1ull << (s % 64);
			if (!!(r[s / 64] & bit) != (counted && g[s] == 1) || !!(a[s / 64] & bit) != (counted && g[s] == 2) || !!(h[s / 64] & bit) != (counted && g[s] == 3)) {
				printf("a wrong plane bit for gt %u at mode=%d S=%lu\n", g[s], mode, (unsigned long)S);
				return 1;
			}
		}
	}
	return 0;
}

int main()
{
	std::mt19937_64 rng(11);
	for (int mode = 0; mode < MODES; mode++)
		for (uint64_t S : {0ull, 1ull, 63ull, 64ull, 65ull, 129ull})
			for (uint32_t N : {1u, 2u, 5u})
				for (int32_t min_gq : {0, 20})
					for (int threads : {1, 3})
						if (run(mode, S, N, min_gq, threads, rng)) return 1;
	printf("ok\n");
	return 0;
}

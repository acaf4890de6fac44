// tests/pairs_asan.cpp -- TEST ONLY: AddressSanitizer + UBSan harness for the host half of vargeno_amd/csrc/vg_pairs.h: the pack and the
// pair count over exact-size heap arrays (any overread trips the sanitizer) against a naive per-site loop written here; compiled and
// run by tests/test_pairs_cpu.py (sanitizers run on the CPU build, in a program of their own).
#include <limits.h>
#include <stdio.h>
#include <random>
#include <vector>
#include "vg_pairs.h"

int main()
{
	std::mt19937_64 rng(11);
	const int32_t gqs[] = {-1, 0, 1, 19, 20, 21, 99, INT_MIN, INT_MAX};
	for (uint64_t S : {0ull, 1ull, 63ull, 64ull, 65ull, 129ull})
		for (uint32_t N : {1u, 2u, 5u})
			for (int32_t min_gq : {0, 20})
				for (int threads : {1, 3}) {
					std::vector<uint8_t> gt((size_t)(N * S));
					std::vector<int32_t> gq((size_t)(N * S));
					for (auto &g : gt) g = (uint8_t)(rng() % 4);
					for (auto &q : gq) q = gqs[rng() % 9];
					std::vector<uint64_t> got((size_t)N * N * VGP_COUNTERS, ~0ull), want((size_t)N * N * VGP_COUNTERS, 0);
					vg_pairs_host_run(gt.data(), gq.data(), S, N, min_gq, threads, got.data());
					for (uint32_t i = 0; i < N; i++)
						for (uint32_t j = 0; j < N; j++)
							for (uint64_t s = 0; s < S; s++) {
								const uint8_t a = gt[i * S + s], b = gt[j * S + s];
								const bool ca = a != 0 && gq[i * S + s] >= min_gq, cb = b != 0 && gq[j * S + s] >= min_gq;
								uint64_t *w = &want[((size_t)i * N + j) * VGP_COUNTERS];
								if (ca && cb) {
									w[VGP_N]++;
									if ((a == 1 && b == 2) || (a == 2 && b == 1)) w[VGP_IBS0]++;
									if (a == b) w[VGP_IBS2]++;
									if (a == 3 && b == 3) w[VGP_HETHET]++;
									if (a == 3) w[VGP_HET_I]++;
								}
							}
					if (got != want) { printf("mismatch at S=%lu N=%u min_gq=%d threads=%d\n", (unsigned long)S, N, min_gq, threads); return 1; }
					// the tail bits of the last word are zero
					const uint64_t n_words = (S + 63) / 64;
					std::vector<uint64_t> r((size_t)n_words), h((size_t)n_words), a((size_t)n_words);
					vg_pairs_pack_host(gt.data(), gq.data(), S, min_gq, r.data(), h.data(), a.data());
					if (S % 64 && ((r[n_words - 1] | h[n_words - 1] | a[n_words - 1]) >> (S % 64))) { printf("tail bits set at S=%lu\n", (unsigned long)S); return 1; }
				}
	printf("ok\n");
	return 0;
}

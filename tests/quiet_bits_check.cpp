// tests/quiet_bits_check.cpp -- TEST ONLY: AddressSanitizer + UBSan harness for vargeno_amd/csrc/vg_quiet.h, the function that gives a
// single-position reference entry of the merged view its two quiet bits, and the rule that turns them into "this read's window holds
// no SNP site".  Rank blocks in exact-size heap arrays (a read past the last block trips the sanitizer; the rank words hold all ones,
// so a function that looked at them would see sites everywhere), against a scan position by position written here, for EVERY k-mer
// position from 0 to well past the pile-up's end.  Compiled and run by tests/test_quiet_bits_cpu.py (sanitizers run on the CPU
// build, in a program of their own).
#include <stdio.h>
#include <random>
#include <vector>
#include "vg_quiet.h"

static long checked = 0;

// one pile-up: sites[p] for p < pile_len
static int check(const std::vector<uint8_t> &sites, const char *what)
{
	const uint64_t plen = sites.size(), nblk = plen / 64 + 1;                 // the loader's block count
	std::vector<unsigned long long> w((size_t)(2 * nblk));
	for (uint64_t b = 0; b < nblk; b++) { w[2 * b] = 0; w[2 * b + 1] = ~0ull; }
	for (uint64_t p = 0; p < plen; p++) if (sites[p]) w[2 * (p >> 6)] |= 1ull << (p & 63);
	auto clear = [&](int64_t a, int64_t b) {                                 // no site in [a, b); positions below 0 hold none
		for (int64_t p = a < 0 ? 0 : a; p < b; p++) if (sites[(size_t)p]) return false;
		return true;
	};
	for (uint64_t kpos = 0; kpos < plen + 200; kpos++) {
		const int64_t k = (int64_t)kpos;
		const bool wantA = kpos + 32 <= plen && clear(k - 96, k + 32), wantB = kpos + 128 <= plen && clear(k, k + 128);
		const uint32_t got = vg_quiet_bits(w.data(), plen, (uint32_t)kpos);
		if (got != ((wantA ? VG_QUIET_A : 0u) | (wantB ? VG_QUIET_B : 0u))) {
			printf("FAIL %s: pile_len %llu kpos %llu: got %u, want A %d B %d\n", what, (unsigned long long)plen, (unsigned long long)kpos, got, (int)wantA, (int)wantB);
			return 1;
		}
		// the rule: whenever it says quiet, the read's whole window is free of sites and inside the pile-up
		for (uint32_t n = 1; n <= 5; n++)
			for (uint32_t c = 0; c < n; c++) {
				if (kpos < 32ull * c) continue;
				const bool q = vg_quiet_key(got, c, n);
				if (q && (n < 2 || n > 4)) { printf("FAIL %s: rule fired for n = %u\n", what, n); return 1; }
				const int64_t t = k - 32 * (int64_t)c;
				if (q && !((uint64_t)t + 32ull * n <= plen && clear(t, t + 32 * (int64_t)n))) {
					printf("FAIL %s: pile_len %llu kpos %llu c %u n %u: quiet, but the window holds a site or leaves the pile-up\n", what, (unsigned long long)plen, (unsigned long long)kpos, c, n);
					return 1;
				}
				checked++;
			}
	}
	return 0;
}

int main()
{
	// the rule's truth table: (c == 0 || A) && (c == n - 1 || B), for 2 <= n <= 4 only
	for (uint32_t bits = 0; bits < 4; bits++)
		for (uint32_t n = 0; n <= 6; n++)
			for (uint32_t c = 0; c < 6; c++) {
				const uint32_t f = (bits & 1u ? VG_QUIET_A : 0u) | (bits & 2u ? VG_QUIET_B : 0u);
				const bool want = n >= 2 && n <= 4 && c < n && (c == 0 || (bits & 1u)) && (c == n - 1 || (bits & 2u));
				if (vg_quiet_key(f, c, n) != want || vg_quiet_key(f | 0x3Fu | 0xFFFFFF00u, c, n) != want) { printf("FAIL rule table: bits %u c %u n %u\n", bits, c, n); return 1; }
			}
	std::mt19937_64 rng(20240607);
	const uint64_t lens[] = {0, 1, 31, 32, 63, 64, 65, 127, 128, 129, 191, 192, 193, 300, 320, 383, 384, 385, 449};
	for (uint64_t plen : lens) {
		std::vector<uint8_t> s((size_t)plen, 0);
		if (check(s, "empty")) return 1;
		std::fill(s.begin(), s.end(), 1);
		if (check(s, "every bit set")) return 1;
		// one site at every position in turn: for every k-mer position that is the site at kpos - 97, - 96, - 1, 0, 31, 32, 127, 128 and at
		// every other offset, on both sides of every 64-bit block boundary
		for (uint64_t p = 0; p < plen; p++) {
			std::fill(s.begin(), s.end(), 0);
			s[(size_t)p] = 1;
			if (check(s, "one site")) return 1;
		}
		// two sites a given distance apart (a quiet stretch between them of every length around the windows' 128 and 224 positions)
		for (uint64_t gap : {1ull, 33ull, 64ull, 127ull, 128ull, 129ull, 223ull, 224ull, 225ull})
			for (uint64_t p = 0; p + gap < plen; p += 7) {
				std::fill(s.begin(), s.end(), 0);
				s[(size_t)p] = 1; s[(size_t)(p + gap)] = 1;
				if (check(s, "two sites")) return 1;
			}
		for (int rep = 0; rep < 20; rep++) {
			const uint64_t every = 1 + rng() % 200;
			for (auto &x : s) x = rng() % every == 0;
			if (check(s, "random")) return 1;
		}
	}
	printf("ok %ld\n", checked);
	return 0;
}

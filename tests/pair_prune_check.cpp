// tests/pair_prune_check.cpp -- TEST ONLY: AddressSanitizer + UBSan harness for vg_quiet_chunks (vargeno_amd/csrc/vg_quiet.h), the
// function that turns the two quiet bits of the entry behind an exact context into "these chunks' windows hold no SNP site", which
// the wave kernel ORs over a key's exact contexts and reads where it prunes stage-B pairs.  Rank blocks in exact-size heap arrays as in
// quiet_bits_check.cpp, against a scan position by position written here, for EVERY k-mer position from 0 to well past the pile-up's
// end and every (chunk, chunks of the read).  Compiled and run by tests/test_pair_prune_cpu.py.
#include <stdio.h>
#include <random>
#include <vector>
#include "vg_quiet.h"

static long checked = 0, set_bits = 0, unions = 0;

// one pile-up: sites[p] for p < pile_len
static int check(const std::vector<uint8_t> &sites, const char *what)
{
	const uint64_t plen = sites.size(), nblk = plen / 64 + 1;                 // the loader's block count
	std::vector<unsigned long long> w((size_t)(2 * nblk));
	for (uint64_t b = 0; b < nblk; b++) { w[2 * b] = 0; w[2 * b + 1] = ~0ull; }
	for (uint64_t p = 0; p < plen; p++) if (sites[p]) w[2 * (p >> 6)] |= 1ull << (p & 63);
	auto clear = [&](int64_t a, int64_t b) {                                 // no site in [a, b); positions outside the pile-up hold none
		for (int64_t p = a < 0 ? 0 : a; p < b && p < (int64_t)plen; p++) if (sites[(size_t)p]) return false;
		return true;
	};
	std::vector<uint32_t> bits((size_t)(plen + 200));
	for (uint64_t kpos = 0; kpos < plen + 200; kpos++) bits[(size_t)kpos] = vg_quiet_bits(w.data(), plen, (uint32_t)kpos);
	for (uint32_t n = 1; n <= 5; n++)
		for (uint64_t key = 0; key < plen + 72; key++) {
			// the key's exact contexts: chunk c at k-mer position key + 32 c; F of each alone, and the union the kernel keeps per key
			uint32_t U = 0;
			for (uint32_t c = 0; c < n; c++) {
				const uint32_t b = bits[(size_t)(key + 32 * c)];
				const uint32_t F = vg_quiet_chunks(b, c, n);
				if ((n < 2 || n > 4) && F) { printf("FAIL %s: bits for n = %u\n", what, n); return 1; }
				if (F >> n) { printf("FAIL %s: n %u c %u: a bit beyond the read's chunks (%u)\n", what, n, c, F); return 1; }
				if (vg_quiet_chunks(b | 0x3Fu | 0xFFFFFF00u, c, n) != F) { printf("FAIL %s: other bits of the flags word read\n", what); return 1; }
				// A gives 0 .. c, B gives c .. n - 1, nothing else
				const uint32_t wantF = n < 2 || n > 4 ? 0u : ((b & VG_QUIET_A) ? (2u << c) - 1u : 0u) | ((b & VG_QUIET_B) ? ((1u << n) - 1u) & ~((1u << c) - 1u) : 0u);
				if (F != wantF) { printf("FAIL %s: n %u c %u bits %u: got %u, want %u\n", what, n, c, b, F, wantF); return 1; }
				if (vg_quiet_key(b, c, n) != (n >= 2 && n <= 4 && F == (1u << n) - 1u)) { printf("FAIL %s: vg_quiet_key != covers all: n %u c %u bits %u\n", what, n, c, b); return 1; }
				for (uint32_t j = 0; j < n; j++) if ((F >> j) & 1u) {
					set_bits++;
					const int64_t a = (int64_t)key + 32 * (int64_t)j;
					if ((uint64_t)a + 32 > plen || !clear(a, a + 32)) {                  // (a set bit's window also lies inside the pile-up)
						printf("FAIL %s: pile_len %llu key %llu n %u: chunk %u called free by the context of chunk %u, but its window holds a site\n", what, (unsigned long long)plen, (unsigned long long)key, n, j, c);
						return 1;
					}
				}
				U |= F;
				checked++;
			}
			if (U == (1u << n) - 1u && n >= 2 && n <= 4) {
				unions++;
				if (!clear((int64_t)key, (int64_t)key + 32 * (int64_t)n)) { printf("FAIL %s: union covers a window with a site\n", what); return 1; }
			}
		}
	// chunks of a key that starts left of the pile-up (key < 0: k-mer position kpos of chunk c < 32 c)
	for (uint32_t n = 2; n <= 4; n++)
		for (uint32_t c = 1; c < n; c++)
			for (uint64_t kpos = 0; kpos < 32ull * c && kpos < plen + 200; kpos++) {
				const uint32_t F = vg_quiet_chunks(bits[(size_t)kpos], c, n);
				for (uint32_t j = 0; j < n; j++) if ((F >> j) & 1u) {
					const int64_t a = (int64_t)kpos - 32 * (int64_t)c + 32 * (int64_t)j;
					if (!clear(a, a + 32)) { printf("FAIL %s: key below 0: kpos %llu c %u n %u chunk %u\n", what, (unsigned long long)kpos, c, n, j); return 1; }
				}
				checked++;
			}
	return 0;
}

int main()
{
	// the function's table, arguments out of range included
	for (uint32_t ab = 0; ab < 4; ab++)
		for (uint32_t n = 0; n <= 6; n++)
			for (uint32_t c = 0; c < 7; c++) {
				const uint32_t f = (ab & 1u ? VG_QUIET_A : 0u) | (ab & 2u ? VG_QUIET_B : 0u);
				uint32_t want = 0;
				if (n >= 2 && n <= 4 && c < n) for (uint32_t j = 0; j < n; j++) if (((ab & 1u) && j <= c) || ((ab & 2u) && j >= c)) want |= 1u << j;
				if (vg_quiet_chunks(f, c, n) != want) { printf("FAIL table: bits %u c %u n %u: got %u, want %u\n", ab, c, n, vg_quiet_chunks(f, c, n), want); return 1; }
				if (vg_quiet_key(f, c, n) != (n >= 2 && n <= 4 && c < n && want == (1u << n) - 1u)) { printf("FAIL table: vg_quiet_key, bits %u c %u n %u\n", ab, c, n); return 1; }
			}
	std::mt19937_64 rng(20240911);
	const uint64_t lens[] = {0, 1, 31, 32, 63, 64, 65, 127, 128, 129, 191, 192, 193, 300, 320, 383, 384, 385, 449};
	for (uint64_t plen : lens) {
		std::vector<uint8_t> s((size_t)plen, 0);
		if (check(s, "empty")) return 1;
		std::fill(s.begin(), s.end(), 1);
		if (check(s, "every bit set")) return 1;
		// one site at every position in turn: for every key that is the site at offsets -1, 0, 31, 32 of every chunk's window
		for (uint64_t p = 0; p < plen; p += (plen > 200 ? 3 : 1)) {
			std::fill(s.begin(), s.end(), 0);
			s[(size_t)p] = 1;
			if (check(s, "one site")) return 1;
		}
		for (uint64_t gap : {1ull, 32ull, 33ull, 64ull, 96ull, 127ull, 128ull, 129ull, 223ull, 224ull, 225ull})
			for (uint64_t p = 0; p + gap < plen; p += 13) {
				std::fill(s.begin(), s.end(), 0);
				s[(size_t)p] = 1; s[(size_t)(p + gap)] = 1;
				if (check(s, "two sites")) return 1;
			}
		for (int rep = 0; rep < 12; rep++) {
			const uint64_t every = 1 + rng() % 200;
			for (auto &x : s) x = rng() % every == 0;
			if (check(s, "random")) return 1;
		}
	}
	if (set_bits < 100000 || unions < 10000) { printf("FAIL vacuous: %ld bits, %ld unions\n", set_bits, unions); return 1; }
	printf("ok %ld %ld %ld\n", checked, set_bits, unions);
	return 0;
}

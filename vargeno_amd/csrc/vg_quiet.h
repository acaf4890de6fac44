// vg_quiet.h -- the two "quiet" bits of a single-position reference entry of the merged view, once, for the loader's kernel and a
// host test.
//
// The pile-up walk of a processed read of n <= 4 chunks touches the site bits of [target, target + 32 n) only, and an exact
// context of chunk c at k-mer position kpos has target = kpos - 32 c (vg_wave.h, stage C).  Per entry the loader records
//   A: no site bit of srank in [kpos - 96, kpos + 32)      (what a read reaches to the LEFT of the k-mer, and the k-mer itself)
//   B: no site bit of srank in [kpos, kpos + 128)          (the k-mer itself and what a read reaches to its RIGHT)
// so that (c == 0 || A) && (c == n - 1 || B) proves the whole window free of sites (vg_quiet_key) and the walk, which would fire
// no atomic, is not made.  Positions below 0 hold no site; a window that reaches past pile_len gets a clear bit.  A clear bit
// always means "walk as before".
// srank as the loader lays it out: 16 bytes per 64 positions, the first 8 the site bits (position p = bit p & 63 of block p >> 6).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VG_QUIET_HD __host__ __device__
#else
#define VG_QUIET_HD
#endif

// where the bits travel: the same two bits of the flags word of an mx entry and of a dx record's inline first entry
enum : uint32_t { VG_QUIET_A = 1u << 6, VG_QUIET_B = 1u << 7, VG_QUIET_MASK = VG_QUIET_A | VG_QUIET_B };

// any site bit in [a, b)?  0 <= a < b <= pile_len; words[2 * blk] = the site bits of block blk
VG_QUIET_HD inline bool vg_range_has_site(const unsigned long long *words, uint64_t a, uint64_t b)
{
	const uint64_t b0 = a >> 6, b1 = (b - 1) >> 6;
	for (uint64_t blk = b0; blk <= b1; blk++) {
		unsigned long long m = ~0ull;
		if (blk == b0) m &= ~0ull << (a & 63u);
		if (blk == b1) m &= ~0ull >> (63u - ((b - 1) & 63u));
		if (words[2 * blk] & m) return true;
	}
	return false;
}

// VG_QUIET_A | VG_QUIET_B of a k-mer position
VG_QUIET_HD inline uint32_t vg_quiet_bits(const unsigned long long *words, uint64_t pile_len, uint32_t kpos)
{
	const uint64_t p = kpos;
	uint32_t f = 0;
	if (p + 32 <= pile_len && !vg_range_has_site(words, p >= 96 ? p - 96 : 0, p + 32)) f |= VG_QUIET_A;
	if (p + 128 <= pile_len && !vg_range_has_site(words, p, p + 128)) f |= VG_QUIET_B;
	return f;
}

// Is the window [kpos - 32 c, kpos - 32 c + 32 n) of a read of n chunks (2 <= n <= 4) known to be free of sites from the bits
// of the entry that gave chunk c its exact context?
VG_QUIET_HD inline bool vg_quiet_key(uint32_t bits, uint32_t c, uint32_t n)
{
	return n >= 2u && n <= 4u && c < n && (c == 0u || (bits & VG_QUIET_A)) && (c == n - 1u || (bits & VG_QUIET_B));
}

// The same proof chunk by chunk: bit j of the result = the window [key + 32 j, key + 32 j + 32) of chunk j of that read, key = kpos - 32 c,
// is known to be free of sites.  A covers [kpos - 96, kpos + 32), which holds the windows of chunks 0 .. c (c <= 3); B covers
// [kpos, kpos + 128), which holds those of chunks c .. n - 1.  Neither bit, or a read of another length: 0.  Masks of several exact
// contexts of one key may be ORed; vg_quiet_key(bits, c, n) is vg_quiet_chunks(bits, c, n) == (1 << n) - 1.
VG_QUIET_HD inline uint32_t vg_quiet_chunks(uint32_t bits, uint32_t c, uint32_t n)
{
	if (n < 2u || n > 4u || c >= n) return 0u;
	const uint32_t upto_c = (2u << c) - 1u, all = (1u << n) - 1u;
	return ((bits & VG_QUIET_A) ? upto_c : 0u) | ((bits & VG_QUIET_B) ? all & ~(upto_c >> 1) : 0u);
}

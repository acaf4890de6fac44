// vg_acand.h -- stage A's exact candidates of one chunk (vg_wave.h, the direct-table look-up), once, for the kernel and a host test.
//
// The bucket of a chunk's canonical key holds at most four entries with that key: reference or SNP dictionary x the two strands
// (a palindrome is its own reverse complement: one entry per dictionary, of both strands at once).  An entry of the chunk's own
// strand is a hit of THIS pass; an entry of the other strand is a hit of the other pass, for the mirrored chunk, and in pass 0 --
// while the block of reverse-strand keys is still usable -- it is kept for pass 1 unless it has several positions.
// The compare-only part of stage A calls vg_acand_note for every matching entry, in bucket order, and touches no key table; what
// the chunk then asks of the key table is the ordered list of at most six candidates that vg_acand_meta describes:
//     slot 0, 1   reverse-strand pushes, in the order met (position; only single-position entries; their own quiet bits)
//     slot 2      this pass's reference hit: a push (with the entry's quiet bits), or -- ambiguous and not a PAIR -- its auxiliary row
//     slot 3      the second position of a reference PAIR
//     slot 4      this pass's SNP hit: a push (never quiet), or its auxiliary row
//     slot 5      the second position of a SNP PAIR
// A lane drains its list slot by slot in this order, so every read's key table is built chunk by chunk, reverse-strand pushes
// before forward pushes, exactly as when each site of the look-up searched the table itself.
// An entry of the other strand with several positions (flag 2) ends the block's use: candidates met before it stay in the list,
// none is taken after it, and `usable` comes out false (the caller then gives the block up after the drain, and hands `usable` to the next chunk's vg_acand_begin before it).  A third
// reverse-strand candidate -- no index has one -- is answered the same way: without the block pass 1 is looked up the plain way.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VG_ACAND_HD __host__ __device__ __forceinline__
#else
#define VG_ACAND_HD inline
#endif

// an entry's flags as the look-up has them: 1 hit, 2 ambiguous, 4 PAIR, 64 / 128 the entry's quiet bits (vg_quiet.h)
enum : uint32_t { VG_AC_HIT = 1u, VG_AC_AMB = 2u, VG_AC_PAIR = 4u, VG_AC_QUIET_SHIFT = 6u };
enum : uint32_t { VG_AC_POS_AMBIGUOUS = 0xFFFFFFFFu };                     // (POS_AMBIGUOUS of vg_device.h)
enum : uint32_t { VG_AC_SLOTS = 6u };
// vg_acand_meta: bits 0-5 slot s holds a candidate; 6 / 7 slot 2 / slot 4 is an auxiliary row; 8 + 2 s (s = 0, 1, 2) the two quiet
// bits of slot s
enum : uint32_t { VG_AC_ROW_REF = 1u << 6, VG_AC_ROW_SNP = 1u << 7, VG_AC_QBITS = 8u };

struct VgAChunk {
	uint32_t v[VG_AC_SLOTS];     // the slots' values: positions, or the index of the row (indexed by constants only)
	uint32_t rf, sf;             // flags of this pass's reference / SNP hit (0: none)
	uint32_t rv;                 // bits 0-1 reverse-strand candidates taken, 2-3 / 4-5 the quiet bits of the first / second
	bool usable;                 // the block of reverse-strand keys may still take candidates
};

// the two quiet bits a push of an entry with flags f carries: those of a single-position entry only
VG_ACAND_HD uint32_t vg_acand_quiet2(uint32_t f) { return (f & (VG_AC_AMB | VG_AC_PAIR)) == 0u ? (f >> VG_AC_QUIET_SHIFT) & 3u : 0u; }

// rc_usable: the block [rc_top, capacity) has not been given up (it is, from the start, in every pass but 0)
VG_ACAND_HD void vg_acand_begin(VgAChunk &s, uint32_t pass, bool rc_usable)
{
	s.v[0] = s.v[1] = s.v[2] = s.v[3] = s.v[4] = s.v[5] = 0u;
	s.rf = s.sf = s.rv = 0u;
	s.usable = pass == 0u && rc_usable;
}

// an entry with the chunk's key.  ks / pal: strand bit and palindrome flag of the chunk's k-mer; es: the entry's strand bit;
// p1, p2: its position (or row index) and the second position of a PAIR; f: its flags
VG_ACAND_HD void vg_acand_note(VgAChunk &s, uint32_t ks, bool pal, bool is_snp, uint32_t es, uint32_t p1, uint32_t p2, uint32_t f)
{
	if (pal || es == ks) { if (is_snp) { s.v[4] = p1; s.v[5] = p2; s.sf = f; } else { s.v[2] = p1; s.v[3] = p2; s.rf = f; } }
	if ((pal || es != ks) && s.usable) {
		if (f & VG_AC_AMB) s.usable = false;
		else if (p1 != VG_AC_POS_AMBIGUOUS) {
			const uint32_t k = s.rv & 3u;
			if (k >= 2u) s.usable = false;
			else {
				if (k == 0u) s.v[0] = p1; else s.v[1] = p1;
				s.rv = (s.rv + 1u) | (vg_acand_quiet2(f) << (2u + 2u * k));
			}
		}
	}
}

VG_ACAND_HD uint32_t vg_acand_meta(const VgAChunk &s)
{
	const uint32_t k = s.rv & 3u;
	uint32_t m = (k >= 1u ? 1u : 0u) | (k >= 2u ? 2u : 0u) | (((s.rv >> 2) & 15u) << VG_AC_QBITS);
	const bool r_ok = (s.rf & VG_AC_HIT) && ((s.rf & VG_AC_PAIR) || s.v[2] != VG_AC_POS_AMBIGUOUS);
	const bool s_ok = (s.sf & VG_AC_HIT) && ((s.sf & VG_AC_PAIR) || s.v[4] != VG_AC_POS_AMBIGUOUS);
	if (r_ok) {
		m |= 1u << 2;
		if ((s.rf & (VG_AC_AMB | VG_AC_PAIR)) == VG_AC_AMB) m |= VG_AC_ROW_REF;      // ambiguous and not a PAIR: the row
		else { m |= vg_acand_quiet2(s.rf) << (VG_AC_QBITS + 4u); if (s.rf & VG_AC_PAIR) m |= 1u << 3; }
	}
	if (s_ok) {
		m |= 1u << 4;
		if ((s.sf & (VG_AC_AMB | VG_AC_PAIR)) == VG_AC_AMB) m |= VG_AC_ROW_SNP;
		else if (s.sf & VG_AC_PAIR) m |= 1u << 5;
	}
	return m;
}

// what slot s (a set bit of the meta word's low six) is
VG_ACAND_HD bool vg_acand_is_reverse(uint32_t s) { return s < 2u; }
VG_ACAND_HD bool vg_acand_is_row(uint32_t meta, uint32_t s) { return (s == 2u && (meta & VG_AC_ROW_REF)) || (s == 4u && (meta & VG_AC_ROW_SNP)); }
VG_ACAND_HD uint32_t vg_acand_quiet_of(uint32_t meta, uint32_t s) { return s < 3u ? ((meta >> (VG_AC_QBITS + 2u * s)) & 3u) << VG_AC_QUIET_SHIFT : 0u; }   // as VG_QUIET_A | VG_QUIET_B

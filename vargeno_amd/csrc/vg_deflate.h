// Raw DEFLATE (RFC 1951) written for BGZF: ONE compressor core for the host and for the device, the inverse of vg_inflate.h.  Under
// hipcc every function here is __host__ __device__; under g++ they are ordinary functions.  No zlib.
//
// THE CONTRACT.  The payload of a block is a function of its text and its length alone: the same bytes from the host policy and from
// the wave policy, whatever the launch shape, the number of host threads, or the way a caller cuts a text into calls at block
// boundaries.  The match finder is therefore stated over 64 VIRTUAL lanes, not over the lanes that exist:
//   - positions are taken in groups of 64; lane l of group g owns position p = 64 g + l;
//   - a position with four bytes behind it hashes them (VG_DEF_HASH_BITS bits); its candidate is the table's entry AS IT STOOD
//     BEFORE THE GROUP; then the group's positions are entered, and the greatest position with a given hash wins (a max);
//   - the match at p is measured against the candidate byte by byte: at most 258 bytes, never past the block's end, and none at
//     all at a distance above 32 768 (a 65 280-byte block is longer than the window) or shorter than VG_DEF_MIN_MATCH;
//   - a greedy scan over the group, left to right, emits the match of every position no earlier match covers, a literal where
//     there is none; `next free position` carries into the next group;
//   - every emitted position forms its code (fixed Huffman codes, BTYPE 1: at most 31 bits), an exclusive prefix sum of the bit
//     lengths gives its bit offset, and the bits are ORed into a staging window whose whole words leave for the output.
// A block whose fixed-coded form would not be smaller than its text is stored instead (the caller writes 01 LEN NLEN and the text):
// no payload exceeds the text by more than 5 bytes.
//
// The core is written once, in SPMD form, over an IO policy:
//   LANES                 cooperating lanes (host: 1; device: one wave of 64); a lane works for 64 / LANES virtual lanes
//   lane()  sync()  u(x)  as in vg_inflate.h
//   ballot(m)             OR over the lanes of m, where every lane passes the bits of its own virtual lanes
//   scan(v, off)          off[k] = sum of v over the virtual lanes below this one; returns the sum over all 64
//   max32(p, v)  or32(p, v)    *p = max(*p, v), *p |= v on a word of the shared tables, atomically among the lanes
// DefHostIO below is the host's policy; the wave policy lives next to the kernel (vargeno_hip.hip).
//
// TERMINATION.  Every loop of the compressor consumes text: a group of 64 positions, one candidate byte, or at least one position of
// the group's scan per iteration; each loop carries a comment that says which.  A block costs at most n / 64 + 1 groups.
#pragma once
#include "vg_inflate.h"

constexpr uint32_t VG_BGZF_TEXT_BLOCK = 65280;           // text bytes per block as htslib cuts them; the most a caller may ask for
constexpr uint32_t VG_BGZF_HEADER = 18, VG_BGZF_TRAILER = 8, VG_BGZF_EOF_BYTES = 28;
constexpr uint32_t VG_DEF_HASH_BITS = 12, VG_DEF_MIN_MATCH = 4, VG_DEF_MAX_MATCH = 258, VG_DEF_WINDOW = 32768;
constexpr uint32_t VG_DEF_STAGE = 66;                    // words of the staging window: a group adds at most 64 x 31 bits to at most 31 carried ones
// bytes the core may write behind out32[0]: it gives up as soon as n bytes have left, a group adds at most 63 words, the end two
constexpr uint32_t VG_DEF_SLACK = 320;

struct VgDefShared {
	uint32_t hash[1u << VG_DEF_HASH_BITS];               // position + 1 of the last group's winner, 0: none yet (host: heap; device: LDS)
	uint32_t stage[VG_DEF_STAGE];
	uint16_t mlen[64];                                   // the group's match lengths, for the scan
};

VG_HD uint32_t vg_def_hash(const uint8_t *p)
{
	const uint32_t w = p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
	return (w * 2654435761u) >> (32 - VG_DEF_HASH_BITS);
}
VG_HD uint32_t vg_def_log2(uint32_t x) { return 31u - (uint32_t)__builtin_clz(x); }     // x > 0
// the low `len` bits of code, reversed (len <= 16): Huffman codes enter the stream from their most significant bit
VG_HD uint32_t vg_def_bitrev(uint32_t code, uint32_t len)
{
	uint32_t x = code;
	x = (x & 0x5555u) << 1 | (x >> 1 & 0x5555u);
	x = (x & 0x3333u) << 2 | (x >> 2 & 0x3333u);
	x = (x & 0x0f0fu) << 4 | (x >> 4 & 0x0f0fu);
	x = (x & 0x00ffu) << 8 | (x >> 8 & 0x00ffu);
	return x >> (16u - len);
}
// the match at p against the candidate at c < p: its length, at most 258 and never past n; 0 when it is shorter than VG_DEF_MIN_MATCH
VG_HD uint32_t vg_def_measure(const uint8_t *t, uint32_t n, uint32_t p, uint32_t c)
{
	const uint8_t *a = t + c, *b = t + p;
	const uint32_t most = n - p < VG_DEF_MAX_MATCH ? n - p : VG_DEF_MAX_MATCH;
	uint32_t m = 0;
	while (m < most && a[m] == b[m]) m++;                             // consumes one candidate byte per iteration, at most 258
	return m >= VG_DEF_MIN_MATCH ? m : 0;
}

// The code of a literal, LSB first as the stream takes it; *nbits its length (8 or 9).  RFC 1951 3.2.6.
VG_HD uint32_t vg_def_literal(uint32_t c, uint32_t *nbits)
{
	if (c < 144) { *nbits = 8; return vg_def_bitrev(0x30u + c, 8); }
	*nbits = 9;
	return vg_def_bitrev(0x190u + (c - 144u), 9);
}
// The code of a match: length code, its extra bits, distance code, its extra bits; at most 8 + 5 + 5 + 13 = 31 bits.
VG_HD uint32_t vg_def_match(uint32_t len, uint32_t dist, uint32_t *nbits)
{
	// length 3..258 -> symbol 257..285: no extra bits up to 10, then four symbols per extra bit; 258 has a symbol of its own
	const uint32_t x = len - 3u;
	uint32_t sym, le = 0, lx = 0;
	if (len == 258) sym = 285;
	else if (x < 8) sym = 257 + x;
	else { le = vg_def_log2(x) - 2u; sym = 261u + 4u * le + ((x >> le) & 3u); lx = x & ((1u << le) - 1u); }
	uint32_t code, n;
	if (sym < 280) { code = vg_def_bitrev(sym - 256u, 7); n = 7; }
	else { code = vg_def_bitrev(0xc0u + (sym - 280u), 8); n = 8; }
	code |= lx << n; n += le;
	// distance 1..32768 -> symbol 0..29: no extra bits up to 4, then two symbols per extra bit; five-bit codes
	const uint32_t d = dist - 1u;
	uint32_t ds = d, de = 0, dx = 0;
	if (d >= 4) { const uint32_t hb = vg_def_log2(d); de = hb - 1u; ds = 2u * hb + ((d >> de) & 1u); dx = d & ((1u << de) - 1u); }
	code |= vg_def_bitrev(ds, 5) << n; n += 5;
	code |= dx << n; n += de;
	*nbits = n;
	return code;
}

VG_HD uint64_t vg_def_bits_from_to(uint32_t a, uint32_t b)                  // bits [a, b), a < 64, b <= 64
{
	return (b >= 64 ? ~0ull : (1ull << b) - 1ull) & ~((1ull << a) - 1ull);
}

// text t[0, n), 1 <= n <= 65280 -> its fixed-coded DEFLATE stream in out32 (room for n + VG_DEF_SLACK bytes, 4-byte aligned).
// Returns the stream's bytes, fewer than n; 0: the stream would not be smaller than the text, which is to be stored.
template <class IO>
VG_HD uint32_t vg_deflate_block(IO &io, VgDefShared &sh, const uint8_t *t, uint32_t n, uint32_t *out32)
{
	constexpr uint32_t NL = IO::LANES, PER = 64 / IO::LANES;
	const uint32_t L = io.lane();
	// (a block of one group never reads the table: every candidate is taken before the group's own positions are entered)
	if (n > 64) for (uint32_t i = L; i < (1u << VG_DEF_HASH_BITS); i += NL) sh.hash[i] = 0;
	for (uint32_t i = L; i < VG_DEF_STAGE; i += NL) sh.stage[i] = i == 0 ? 3u : 0u;      // BFINAL 1, BTYPE 01
	io.sync();
	uint32_t bit = 3;                                                 // bits of the stream so far
	uint32_t wbase = 0;                                               // words that have left for out32; stage[0] is word wbase
	uint32_t next_free = 0;                                           // the first position no emitted match covers
	for (uint32_t base = 0; base < n; base += 64) {                   // one group per iteration: consumes 64 positions of the text
		const uint32_t cnt = n - base < 64 ? n - base : 64;
		uint32_t mlen[PER], cand[PER], hsh[PER];                      // cand: the candidate's position + 1, 0: none that could be used
		for (uint32_t k = 0; k < PER; k++) {
			const uint32_t l = L + k * NL, p = base + l;
			mlen[k] = 0; cand[k] = 0; hsh[k] = ~0u;
			if (l >= cnt || p + 4 > n) continue;
			hsh[k] = vg_def_hash(t + p);
			if (base == 0 || p < next_free) continue;                 // (a position an earlier group's match covers is never emitted)
			const uint32_t c1 = sh.hash[hsh[k]];
			if (c1 != 0 && p - (c1 - 1u) <= VG_DEF_WINDOW) cand[k] = c1;
		}
		io.sync();                                                    // every candidate has been read: the group's positions may go in
		for (uint32_t k = 0; k < PER; k++)
			if (hsh[k] != ~0u && base + 64 < n) io.max32(&sh.hash[hsh[k]], base + L + k * NL + 1u);
		// The greedy scan, the same in every lane: emit = the group's positions that no match covers, mlen their match lengths.  The
		// scan reads the length of an emitted position only, so one lane that works for all 64 measures just those, as it goes;
		// several lanes measure every position at once and scan the result.  The output is the same.
		uint64_t emit = 0;
		uint32_t q = next_free > base ? next_free - base : 0;
		if constexpr (NL == 1) {
			while (q < cnt) {                                         // every iteration consumes at least one position of the group
				mlen[q] = cand[q] ? vg_def_measure(t, n, base + q, cand[q] - 1u) : 0;
				emit |= 1ull << q;
				q += mlen[q] ? mlen[q] : 1u;
			}
		} else {
			uint64_t mine = 0;
			for (uint32_t k = 0; k < PER; k++) {
				const uint32_t l = L + k * NL;
				if (cand[k]) mlen[k] = vg_def_measure(t, n, base + l, cand[k] - 1u);
				if (mlen[k]) mine |= 1ull << l;
				sh.mlen[l] = (uint16_t)mlen[k];
			}
			const uint64_t has = io.ballot(mine);
			io.sync();
			while (q < cnt) {                                         // every iteration consumes at least one position of the group
				const uint64_t m = has >> q;
				if (m == 0) { emit |= vg_def_bits_from_to(q, cnt); q = cnt; break; }
				const uint32_t z = (uint32_t)__builtin_ctzll(m);
				if (z) emit |= vg_def_bits_from_to(q, q + z);
				q += z;
				emit |= 1ull << q;
				q += io.u(sh.mlen[q]);
			}
		}
		next_free = base + q;
		uint32_t code[PER], nb[PER], off[PER];
		for (uint32_t k = 0; k < PER; k++) {
			const uint32_t l = L + k * NL;
			code[k] = 0; nb[k] = 0;
			if (!(emit >> l & 1ull)) continue;
			code[k] = mlen[k] ? vg_def_match(mlen[k], base + l - (cand[k] - 1u), &nb[k]) : vg_def_literal(t[base + l], &nb[k]);
		}
		const uint32_t total = io.scan(nb, off);
		const uint32_t rel = bit - wbase * 32u;                       // < 32: the bits carried in stage[0]
		for (uint32_t k = 0; k < PER; k++) {
			if (!nb[k]) continue;
			const uint32_t at = rel + off[k], w = at >> 5, s = at & 31u;
			io.or32(&sh.stage[w], code[k] << s);
			if (s + nb[k] > 32) io.or32(&sh.stage[w + 1], code[k] >> (32u - s));
		}
		bit += total;
		io.sync();
		const uint32_t full = (bit >> 5) - wbase;                     // whole words of the window: at most 63
		for (uint32_t w = L; w < full; w += NL) out32[wbase + w] = sh.stage[w];
		const uint32_t carry = io.u(sh.stage[full]);
		io.sync();
		for (uint32_t w = L; w <= full; w += NL) sh.stage[w] = w == 0 ? carry : 0u;
		io.sync();
		wbase += full;
		if (wbase * 4u >= n) return 0;                                // as long as the text already: store it
	}
	bit += 7;                                                         // end of block: seven zero bits
	const uint32_t bytes = (bit + 7u) >> 3;
	if (bytes >= n) return 0;
	const uint32_t words = ((bytes + 3u) >> 2) - wbase;               // at most 2
	for (uint32_t w = L; w < words; w += NL) out32[wbase + w] = sh.stage[w];
	io.sync();
	return bytes;
}

// ---- BGZF framing ----------------------------------------------------------------------------------------------------------------
// the 18 header bytes of a block whose payload has `payload` bytes, as bgzip writes them: MTIME 0, XFL 0, OS ff, BC = BSIZE - 1
VG_HD uint8_t vg_bgzf_header_byte(uint32_t i, uint32_t payload)
{
	const uint32_t bsize1 = VG_BGZF_HEADER + payload + VG_BGZF_TRAILER - 1u;
	switch (i) {
	case 0: return 0x1f; case 1: return 0x8b; case 2: return 0x08; case 3: return 0x04;
	case 9: return 0xff; case 10: return 0x06; case 12: return 'B'; case 13: return 'C'; case 14: return 0x02;
	case 16: return (uint8_t)bsize1; case 17: return (uint8_t)(bsize1 >> 8);
	}
	return 0;
}
// the five bytes in front of a stored block's text: BFINAL 1, BTYPE 00, LEN, NLEN
VG_HD uint8_t vg_def_stored_byte(uint32_t i, uint32_t n)
{
	return i == 0 ? 1 : i == 1 ? (uint8_t)n : i == 2 ? (uint8_t)(n >> 8) : i == 3 ? (uint8_t)~n : (uint8_t)(~n >> 8);
}
VG_HD uint64_t vg_bgzf_blocks_of(uint64_t nbytes, uint32_t block) { return (nbytes + block - 1) / block; }
// the worst case of nbytes of text in blocks of `block`: every block stored, headers, trailers and the end-of-file marker
VG_HD uint64_t vg_bgzf_bound(uint64_t nbytes, uint32_t block)
{
	return nbytes + vg_bgzf_blocks_of(nbytes, block) * (5u + VG_BGZF_HEADER + VG_BGZF_TRAILER) + VG_BGZF_EOF_BYTES;
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
// htslib's empty block, which ends a BGZF file
inline const uint8_t *vg_bgzf_eof_marker()
{
	static const uint8_t m[VG_BGZF_EOF_BYTES] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 'B', 'C', 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};
	return m;
}

// the host's policy: one lane that works for all 64
struct DefHostIO {
	static constexpr uint32_t LANES = 1;
	static uint32_t lane() { return 0; }
	static void sync() {}
	static uint32_t u(uint32_t x) { return x; }
	static uint64_t ballot(uint64_t m) { return m; }
	static uint32_t scan(const uint32_t *v, uint32_t *off) { uint32_t s = 0; for (uint32_t k = 0; k < 64; k++) { off[k] = s; s += v[k]; } return s; }
	static void max32(uint32_t *p, uint32_t v) { if (v > *p) *p = v; }
	static void or32(uint32_t *p, uint32_t v) { *p |= v; }
};

// One block on the host: text[0, n), 1 <= n <= 65280 -> a whole BGZF block at dst (room for n + 5 + 26 bytes); returns its bytes.
// sh and slot (n + VG_DEF_SLACK bytes, as words) are the caller's scratch.
inline uint32_t vg_bgzf_deflate_block_host(const uint8_t *text, uint32_t n, uint8_t *dst, VgDefShared &sh, uint32_t *slot)
{
	DefHostIO io;
	const uint32_t coded = vg_deflate_block(io, sh, text, n, slot);
	const uint32_t payload = coded ? coded : n + 5u;
	for (uint32_t i = 0; i < VG_BGZF_HEADER; i++) dst[i] = vg_bgzf_header_byte(i, payload);
	uint8_t *p = dst + VG_BGZF_HEADER;
	if (coded) memcpy(p, slot, coded);
	else { for (uint32_t i = 0; i < 5; i++) p[i] = vg_def_stored_byte(i, n); memcpy(p + 5, text, n); }
	const uint32_t crc = vg_crc32(vg_crc_tab_host(), 0, text, n);
	uint8_t *tr = p + payload;
	for (uint32_t i = 0; i < 4; i++) { tr[i] = (uint8_t)(crc >> (8 * i)); tr[4 + i] = (uint8_t)(n >> (8 * i)); }
	return VG_BGZF_HEADER + payload + VG_BGZF_TRAILER;
}

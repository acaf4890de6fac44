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
// no payload exceeds the text by more than 5 bytes.  The second coding mode (vg_deflate_block_dyn, further down) runs the same finder,
// keeps its tokens, and codes them with Huffman codes built for the block (BTYPE 2) where that is the smallest form.
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
// the group's scan per iteration; each loop carries a comment that says which.  A block costs at most n / 64 + 1 groups.  The loops
// of the dynamic path's plan and second pass consume tokens, symbols, code lengths or nodes of the tree, and say so the same way.
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
// length 3..258 -> symbol 257..285: no extra bits up to 10, then four symbols per extra bit; 258 has a symbol of its own.
// *le the number of extra bits, *lx their value
VG_HD uint32_t vg_def_len_sym(uint32_t len, uint32_t *le, uint32_t *lx)
{
	const uint32_t x = len - 3u;
	*le = 0; *lx = 0;
	if (len == 258) return 285;
	if (x < 8) return 257 + x;
	const uint32_t e = vg_def_log2(x) - 2u;
	*le = e; *lx = x & ((1u << e) - 1u);
	return 261u + 4u * e + ((x >> e) & 3u);
}
// distance 1..32768 -> symbol 0..29: no extra bits up to 4, then two symbols per extra bit
VG_HD uint32_t vg_def_dist_sym(uint32_t dist, uint32_t *de, uint32_t *dx)
{
	const uint32_t d = dist - 1u;
	*de = 0; *dx = 0;
	if (d < 4) return d;
	const uint32_t hb = vg_def_log2(d), e = hb - 1u;
	*de = e; *dx = d & ((1u << e) - 1u);
	return 2u * hb + ((d >> e) & 1u);
}
// The code of a match: length code, its extra bits, distance code, its extra bits; at most 8 + 5 + 5 + 13 = 31 bits.
VG_HD uint32_t vg_def_match(uint32_t len, uint32_t dist, uint32_t *nbits)
{
	uint32_t le, lx, de, dx;
	const uint32_t sym = vg_def_len_sym(len, &le, &lx);
	uint32_t code, n;
	if (sym < 280) { code = vg_def_bitrev(sym - 256u, 7); n = 7; }
	else { code = vg_def_bitrev(0xc0u + (sym - 280u), 8); n = 8; }
	code |= lx << n; n += le;
	const uint32_t ds = vg_def_dist_sym(dist, &de, &dx);                  // five-bit codes
	code |= vg_def_bitrev(ds, 5) << n; n += 5;
	code |= dx << n; n += de;
	*nbits = n;
	return code;
}

VG_HD uint64_t vg_def_bits_from_to(uint32_t a, uint32_t b)                  // bits [a, b), a < 64, b <= 64
{
	return (b >= 64 ? ~0ull : (1ull << b) - 1ull) & ~((1ull << a) - 1ull);
}

// One group of the match finder, the statements both coding paths run: positions [base, base + 64) of t[0, n).  Returns the emit
// mask (bit l: position base + l is emitted); for an emitted virtual lane, mlen is its match length (0: a literal) and cand its
// candidate's position + 1 (0: none that could be used).  *next_free, the first position no emitted match covers, is carried.
template <class IO>
VG_HD uint64_t vg_def_group(IO &io, VgDefShared &sh, const uint8_t *t, uint32_t n, uint32_t base, uint32_t *next_free, uint32_t *mlen, uint32_t *cand)
{
	constexpr uint32_t NL = IO::LANES, PER = 64 / IO::LANES;
	const uint32_t L = io.lane();
	const uint32_t cnt = n - base < 64 ? n - base : 64;
	uint32_t hsh[PER];
	for (uint32_t k = 0; k < PER; k++) {
		const uint32_t l = L + k * NL, p = base + l;
		mlen[k] = 0; cand[k] = 0; hsh[k] = ~0u;
		if (l >= cnt || p + 4 > n) continue;
		hsh[k] = vg_def_hash(t + p);
		if (base == 0 || p < *next_free) continue;                 // (a position an earlier group's match covers is never emitted)
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
	uint32_t q = *next_free > base ? *next_free - base : 0;
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
	*next_free = base + q;
	return emit;
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
		uint32_t mlen[PER], cand[PER];
		const uint64_t emit = vg_def_group(io, sh, t, n, base, &next_free, mlen, cand);
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

// ---- dynamic Huffman codes (BTYPE 2), the second coding mode ---------------------------------------------------------------------
// The same finder, the same tokens; two passes.  Pass 1 runs the finder over the whole block, stores every emitted position as a
// token (io.tokens(): at most n words, global memory on the device) and counts its symbols.  From the two histograms come the code
// lengths (vg_def_code_lengths), the run-length coded header and the exact size of the three forms a block can take: stored, fixed
// codes, dynamic codes.  The smallest is taken -- on a tie stored, then fixed -- before a bit is emitted, so there is no give-up on
// the way, and a block that takes the fixed form carries the bytes vg_deflate_block writes for it (the same tokens, the same codes,
// and as there a coded form has to be shorter than the text itself).  Pass 2 reads the tokens back 64 at a time and codes them from
// the tables, through a window wide enough for 64 codes of 48 bits.  Two more primitives of the policy:
//   add32(p, v)           *p += v on a counter of the shared tables, atomically among the lanes
//   tokens()              the block's token buffer
constexpr uint32_t VG_DEF_LL = 286, VG_DEF_DS = 30, VG_DEF_CL = 19;  // the alphabets: literal/length, distance, code length
constexpr uint32_t VG_DEF_LL_TAB = 288, VG_DEF_DS_TAB = 32;          // ... as the fixed code counts them (RFC 1951 3.2.6)
// words of the dynamic path's window: a group adds at most 64 x 48 bits (15 + 5 + 15 + 13 a match) to at most 31 carried ones,
// 3 103 bits or 97 words; one more, so that the word after the last whole one always exists
constexpr uint32_t VG_DEF_STAGE_DYN = 98;
// Slack of the dynamic path: the form's size is known before a bit is emitted and a coded form has fewer bytes than the text, so
// what leaves for out32 are the whole words of at most n - 1 bytes: at most n + 2 bytes, well within VG_DEF_SLACK.

struct VgDefLenScratch {                                 // the scratch of vg_def_code_lengths
	uint32_t key[VG_DEF_LL_TAB];                         // the used symbols' counts in sorted order, then the tree in place
	uint16_t used[VG_DEF_LL_TAB];                        // the used symbols in symbol order
	uint16_t sorted[VG_DEF_LL_TAB];                      // ... by (count, symbol)
	uint32_t num[16];                                    // codes per length
};
struct VgDefDynTables {                                  // what pass 2 needs; live only once the finder's table is dead
	uint32_t stage[VG_DEF_STAGE_DYN];
	uint16_t ll_code[VG_DEF_LL_TAB], d_code[VG_DEF_DS_TAB], cl_code[VG_DEF_CL + 1];      // LSB first, as the stream takes them
	uint8_t ll_len[VG_DEF_LL_TAB], d_len[VG_DEF_DS_TAB], cl_len[VG_DEF_CL + 1];
	uint32_t cl_freq[VG_DEF_CL + 1];
	uint16_t rle[VG_DEF_LL + VG_DEF_DS];                 // the header's code-length symbols: symbol | value of its extra bits << 8
	uint32_t n_rle, hlit, hdist, hclen;
	uint32_t form, bits;                                 // 0 stored, 1 fixed, 2 dynamic; the coded stream's bits
	VgDefLenScratch sc;
};
struct VgDefDynShared {
	union { VgDefShared d; VgDefDynTables t; };          // pass 1 | the plan and pass 2
	uint32_t ll_freq[VG_DEF_LL_TAB], d_freq[VG_DEF_DS_TAB];      // written by pass 1, read by the plan
};
static_assert(sizeof(VgDefDynTables) <= sizeof(VgDefShared), "the tables overlay pass 1's state");

VG_HD uint32_t vg_def_len_extra(uint32_t sym) { return sym < 265 || sym == 285 ? 0 : (sym - 261u) >> 2; }      // sym >= 257
VG_HD uint32_t vg_def_dist_extra(uint32_t sym) { return sym < 4 ? 0 : (sym >> 1) - 1u; }
VG_HD uint32_t vg_def_fixed_len(uint32_t sym) { return sym < 144 ? 8 : sym < 256 ? 9 : sym < 280 ? 7 : 8; }
VG_HD uint32_t vg_def_cl_extra(uint32_t sym) { return sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0; }
// the order in which the header lists the code-length code's own lengths (RFC 1951 3.2.7)
VG_HD uint32_t vg_def_cl_order(uint32_t i)
{
	constexpr uint8_t order[VG_DEF_CL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
	return order[i];
}

// Code lengths of a Huffman code for the counts freq[0, n_sym), none above `limit`: 2 <= n_sym <= 288, n_sym <= 2^limit,
// limit <= 15, the counts' sum below 2^32.  Integers only, ties broken by symbol number: a function of freq alone.  A symbol with
// count 0 gets length 0 -- but when fewer than two symbols are in use the lowest unused ones join them at count 0 and come out at
// length 1, so that no decoder sees an empty or a one-code set.  The Kraft sum of the result is exactly 1.
// All lanes call it; len_out and sc are shared; the sort is spread over the lanes, the tree (at most 287 merges) is lane 0's.
template <class IO>
VG_HD void vg_def_code_lengths(IO &io, const uint32_t *freq, uint32_t n_sym, uint32_t limit, uint8_t *len_out, VgDefLenScratch &sc)
{
	constexpr uint32_t NL = IO::LANES, PER = 64 / IO::LANES;
	const uint32_t L = io.lane();
	uint32_t m = 0;                                                   // symbols in use
	for (uint32_t c = 0; c < n_sym; c += 64) {                        // consumes 64 symbols: those in use, in symbol order
		uint32_t v[PER], off[PER];
		for (uint32_t k = 0; k < PER; k++) {
			const uint32_t s = c + L + k * NL;
			v[k] = s < n_sym && freq[s] != 0;
			if (s < n_sym) len_out[s] = 0;
		}
		const uint32_t total = io.scan(v, off);
		for (uint32_t k = 0; k < PER; k++) if (v[k]) sc.used[m + off[k]] = (uint16_t)(c + L + k * NL);
		m += total;
	}
	io.sync();
	if (m < 2) {
		if (L == 0) {
			uint32_t k = m;
			for (uint32_t s = 0; k < 2; s++) if (freq[s] == 0) sc.used[k++] = (uint16_t)s;      // consumes one symbol, at most two
		}
		m = 2;
		io.sync();
	}
	for (uint32_t i = L; i < m; i += NL) {                            // consumes one symbol in use per lane: its rank by (count, symbol)
		const uint32_t s = sc.used[i], f = freq[s];
		uint32_t r = 0;
		for (uint32_t j = 0; j < m; j++) {                            // consumes one symbol in use
			const uint32_t sj = sc.used[j], fj = freq[sj];
			r += (fj < f || (fj == f && sj < s)) ? 1u : 0u;
		}
		sc.sorted[r] = (uint16_t)s;
		sc.key[r] = f;
	}
	io.sync();
	if (L == 0) {
		// Moffat and Katajainen's in-place minimum-redundancy code over the sorted counts: key[i] becomes the depth of the i-th
		// least frequent symbol.  Of a leaf and an internal node of equal weight the leaf is taken first.
		uint32_t *A = sc.key;
		A[0] += A[1];
		uint32_t root = 0, leaf = 2;
		for (uint32_t next = 1; next + 1 < m; next++) {               // one merge per iteration, at most 286
			if (leaf >= m || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = next; } else A[next] = A[leaf++];
			if (leaf >= m || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = next; } else A[next] += A[leaf++];
		}
		A[m - 2] = 0;
		for (int32_t next = (int32_t)m - 3; next >= 0; next--) A[next] = A[A[next]] + 1u;      // consumes one internal node: its depth
		int32_t avbl = 1, used = 0, rt = (int32_t)m - 2, nx = (int32_t)m - 1;
		uint32_t dpth = 0;
		while (avbl > 0) {                                            // consumes one level of the tree, at most 287
			while (rt >= 0 && A[rt] == dpth) { used++; rt--; }        // consumes one internal node
			while (avbl > used) { A[nx--] = dpth; avbl--; }           // consumes one leaf
			avbl = 2 * used; dpth++; used = 0;
		}
		// The limit, as miniz and libdeflate enforce it: every deeper code is lifted to `limit`, which over-subscribes the code by
		// `over` units of 2^-limit; each round below takes one code away from `limit`, pairs it with the deepest shallower code
		// (which moves one level down), and so lowers `over` by exactly one.  WHY IT ENDS AND NEVER STARTS EMPTY-HANDED: a lifted
		// code adds less than one unit, so over < the lifted codes <= num[limit]; a round lowers both by at most one, hence
		// num[limit] > over >= 1 whenever a round starts; and a shallower code exists, or more than 2^limit >= n_sym codes would
		// all sit at `limit`.  At most 287 rounds.
		for (uint32_t i = 0; i < 16; i++) sc.num[i] = 0;
		for (uint32_t i = 0; i < m; i++) sc.num[A[i] < limit ? A[i] : limit]++;                 // consumes one symbol in use
		uint32_t total = 0;
		for (uint32_t i = 1; i <= limit; i++) total += sc.num[i] << (limit - i);              // consumes one length: the Kraft sum in units of 2^-limit
		while (total > (1u << limit)) {                               // lowers the over-subscription by one unit
			sc.num[limit]--;
			for (uint32_t i = limit - 1; i > 0; i--)                  // consumes one length
				if (sc.num[i]) { sc.num[i]--; sc.num[i + 1] += 2; break; }
			total--;
		}
		uint32_t j = m;                                               // the shortest codes to the most frequent symbols
		for (uint32_t i = 1; i <= limit; i++)                         // consumes one length
			for (uint32_t c = sc.num[i]; c > 0; c--) len_out[sc.sorted[--j]] = (uint8_t)i;      // consumes one symbol in use
	}
	io.sync();
}

// canonical codes of the lengths len[0, n), bit-reversed (lane 0's; num and key of the scratch are its counters)
VG_HD void vg_def_canonical(const uint8_t *len, uint32_t n, uint16_t *code, VgDefLenScratch &sc)
{
	for (uint32_t b = 0; b < 16; b++) sc.num[b] = 0;
	for (uint32_t s = 0; s < n; s++) sc.num[len[s]]++;                // consumes one symbol
	sc.num[0] = 0;
	uint32_t c = 0;
	for (uint32_t b = 1; b < 16; b++) { c = (c + sc.num[b - 1]) << 1; sc.key[b] = c; }      // consumes one length: its first code
	for (uint32_t s = 0; s < n; s++) if (len[s]) code[s] = (uint16_t)vg_def_bitrev(sc.key[len[s]]++, len[s]);      // consumes one symbol
}

// The plan of a block of n text bytes whose histograms pass 1 has left in sh: code lengths, header, the three forms' sizes, the
// choice, and the chosen form's code tables.  Returns the form (the same in every lane).
template <class IO>
VG_HD uint32_t vg_def_dyn_plan(IO &io, VgDefDynShared &sh, uint32_t n)
{
	VgDefDynTables &T = sh.t;
	const uint32_t L = io.lane();
	vg_def_code_lengths(io, sh.ll_freq, VG_DEF_LL, 15, T.ll_len, T.sc);
	vg_def_code_lengths(io, sh.d_freq, VG_DEF_DS, 15, T.d_len, T.sc);
	if (L == 0) {
		// HLIT and HDIST without their trailing zero lengths; the lengths of both, as one sequence, in runs: 16 repeats the length
		// before it 3 to 6 times, 17 and 18 stand for 3 to 10 and 11 to 138 zeros
		uint32_t hlit = VG_DEF_LL, hdist = VG_DEF_DS, nr = 0;
		while (hlit > 257 && T.ll_len[hlit - 1] == 0) hlit--;         // consumes one length
		while (hdist > 1 && T.d_len[hdist - 1] == 0) hdist--;         // consumes one length
		for (uint32_t s = 0; s <= VG_DEF_CL; s++) T.cl_freq[s] = 0;
		const uint32_t all = hlit + hdist;
		auto len_at = [&](uint32_t i) -> uint32_t { return i < hlit ? T.ll_len[i] : T.d_len[i - hlit]; };
		auto put = [&](uint32_t x) { T.rle[nr++] = (uint16_t)x; T.cl_freq[x & 31u]++; };
		for (uint32_t i = 0; i < all;) {                              // consumes one run of equal lengths
			const uint32_t v = len_at(i);
			uint32_t run = 1;
			while (i + run < all && len_at(i + run) == v) run++;      // consumes one length
			i += run;
			if (v == 0) {
				while (run >= 11) { const uint32_t c = run < 138 ? run : 138; put(18u | (c - 11u) << 8); run -= c; }      // consumes 11 to 138 zeros
				if (run >= 3) { put(17u | (run - 3u) << 8); run = 0; }
			} else {
				put(v); run--;
				while (run >= 3) { const uint32_t c = run < 6 ? run : 6; put(16u | (c - 3u) << 8); run -= c; }            // consumes 3 to 6 repeats
			}
			while (run) { put(v); run--; }                            // consumes one length
		}
		T.n_rle = nr; T.hlit = hlit; T.hdist = hdist;
	}
	io.sync();
	vg_def_code_lengths(io, T.cl_freq, VG_DEF_CL, 7, T.cl_len, T.sc);
	if (L == 0) {
		uint32_t hclen = VG_DEF_CL;
		while (hclen > 4 && T.cl_len[vg_def_cl_order(hclen - 1)] == 0) hclen--;      // consumes one length
		T.hclen = hclen;
		// the exact bits of the two coded forms: a fixed code's cost is a function of the symbol
		uint32_t dyn = 3 + 5 + 5 + 4 + 3 * hclen, fix = 3;
		for (uint32_t s = 0; s < VG_DEF_CL; s++) dyn += T.cl_freq[s] * (T.cl_len[s] + vg_def_cl_extra(s));      // consumes one symbol
		for (uint32_t s = 0; s < VG_DEF_LL; s++) {                    // consumes one symbol
			const uint32_t f = sh.ll_freq[s], x = s < 257 ? 0 : vg_def_len_extra(s);
			dyn += f * (T.ll_len[s] + x); fix += f * (vg_def_fixed_len(s) + x);
		}
		for (uint32_t s = 0; s < VG_DEF_DS; s++) {                    // consumes one symbol
			const uint32_t f = sh.d_freq[s], x = vg_def_dist_extra(s);
			dyn += f * (T.d_len[s] + x); fix += f * (5u + x);
		}
		uint32_t form = dyn < fix ? 2u : 1u;
		const uint32_t bits = dyn < fix ? dyn : fix;
		if (((bits + 7u) >> 3) >= n) form = 0;                        // as in vg_deflate_block: not shorter than the text, store it
		T.form = form; T.bits = bits;
		if (form == 1) {
			for (uint32_t s = 0; s < VG_DEF_LL_TAB; s++) T.ll_len[s] = (uint8_t)vg_def_fixed_len(s);      // consumes one symbol; so does the next
			for (uint32_t s = 0; s < VG_DEF_DS_TAB; s++) T.d_len[s] = 5;
			vg_def_canonical(T.ll_len, VG_DEF_LL_TAB, T.ll_code, T.sc);
			vg_def_canonical(T.d_len, VG_DEF_DS_TAB, T.d_code, T.sc);
		} else if (form == 2) {
			vg_def_canonical(T.ll_len, VG_DEF_LL, T.ll_code, T.sc);
			vg_def_canonical(T.d_len, VG_DEF_DS, T.d_code, T.sc);
			vg_def_canonical(T.cl_len, VG_DEF_CL, T.cl_code, T.sc);
		}
	}
	io.sync();
	return io.u(T.form);
}

// One group of up to 64 codes appended to the stream: code[k] in nb[k] bits, at most 48 (0: none), LSB first.  The bit offsets are
// the wave scan; a code can straddle three words of the window; the window's whole words leave for out32.
template <class IO>
VG_HD void vg_def_put_group(IO &io, uint32_t *stage, const uint64_t *code, const uint32_t *nb, uint32_t *bit, uint32_t *wbase, uint32_t *out32)
{
	constexpr uint32_t NL = IO::LANES, PER = 64 / IO::LANES;
	const uint32_t L = io.lane();
	uint32_t off[PER];
	const uint32_t total = io.scan(nb, off);
	const uint32_t rel = *bit - *wbase * 32u;                         // < 32: the bits carried in stage[0]
	for (uint32_t k = 0; k < PER; k++) {
		if (!nb[k]) continue;
		const uint32_t at = rel + off[k], w = at >> 5, s = at & 31u;
		io.or32(&stage[w], (uint32_t)(code[k] << s));
		if (s + nb[k] > 32) io.or32(&stage[w + 1], (uint32_t)(code[k] >> (32u - s)));
		if (s + nb[k] > 64) io.or32(&stage[w + 2], (uint32_t)(code[k] >> (64u - s)));
	}
	*bit += total;
	io.sync();
	const uint32_t full = (*bit >> 5) - *wbase;                       // whole words of the window: at most 96
	for (uint32_t w = L; w < full; w += NL) out32[*wbase + w] = stage[w];
	const uint32_t carry = io.u(stage[full]);
	io.sync();
	for (uint32_t w = L; w <= full; w += NL) stage[w] = w == 0 ? carry : 0u;
	io.sync();
	*wbase += full;
}

// text t[0, n), 1 <= n <= 65280 -> its DEFLATE stream in the smallest of the three forms, in out32 (room as for vg_deflate_block).
// Returns the stream's bytes, fewer than n; 0: the block is to be stored.
template <class IO>
VG_HD uint32_t vg_deflate_block_dyn(IO &io, VgDefDynShared &sh, const uint8_t *t, uint32_t n, uint32_t *out32)
{
	constexpr uint32_t NL = IO::LANES, PER = 64 / IO::LANES;
	const uint32_t L = io.lane();
	uint32_t *tok = io.tokens();
	// ---- pass 1: tokens and histograms
	if (n > 64) for (uint32_t i = L; i < (1u << VG_DEF_HASH_BITS); i += NL) sh.d.hash[i] = 0;
	for (uint32_t i = L; i < VG_DEF_LL_TAB; i += NL) sh.ll_freq[i] = i == 256 ? 1u : 0u;      // the end-of-block symbol, once
	for (uint32_t i = L; i < VG_DEF_DS_TAB; i += NL) sh.d_freq[i] = 0;
	io.sync();
	uint32_t ntok = 0, next_free = 0;
	for (uint32_t base = 0; base < n; base += 64) {                   // one group per iteration: consumes 64 positions of the text
		uint32_t mlen[PER], cand[PER];
		const uint64_t emit = vg_def_group(io, sh.d, t, n, base, &next_free, mlen, cand);
		for (uint32_t k = 0; k < PER; k++) {
			const uint32_t l = L + k * NL;
			if (!(emit >> l & 1ull)) continue;
			uint32_t tk = t[base + l];                                // a literal: its byte; a match: length << 16 | distance
			if (mlen[k]) {
				const uint32_t dist = base + l - (cand[k] - 1u);
				uint32_t e, x;
				tk = mlen[k] << 16 | dist;
				io.add32(&sh.ll_freq[vg_def_len_sym(mlen[k], &e, &x)], 1u);
				io.add32(&sh.d_freq[vg_def_dist_sym(dist, &e, &x)], 1u);
			} else io.add32(&sh.ll_freq[tk], 1u);
			tok[ntok + (uint32_t)__builtin_popcountll(emit & ((1ull << l) - 1ull))] = tk;
		}
		ntok += (uint32_t)__builtin_popcountll(emit);
	}
	io.sync();
	// ---- the plan
	const uint32_t form = vg_def_dyn_plan(io, sh, n);
	if (form == 0) return 0;
	// ---- pass 2: the header and the tokens through the window
	VgDefDynTables &T = sh.t;
	for (uint32_t i = L; i < VG_DEF_STAGE_DYN; i += NL) T.stage[i] = (i == 0 && form == 1) ? 3u : 0u;      // fixed: BFINAL 1, BTYPE 01
	io.sync();
	uint32_t bit = form == 1 ? 3u : 0u, wbase = 0;
	uint64_t code[PER];
	uint32_t nb[PER];
	if (form == 2) {
		const uint32_t hlit = io.u(T.hlit), hdist = io.u(T.hdist), hclen = io.u(T.hclen), n_rle = io.u(T.n_rle);
		for (uint32_t k = 0; k < PER; k++) {                          // BFINAL 1, BTYPE 10, HLIT, HDIST, HCLEN; the code-length code's lengths
			const uint32_t l = L + k * NL;
			code[k] = 0; nb[k] = 0;
			if (l == 0) { code[k] = 5u | (hlit - 257u) << 3 | (hdist - 1u) << 8 | (hclen - 4u) << 13; nb[k] = 17; }
			else if (l <= hclen) { code[k] = T.cl_len[vg_def_cl_order(l - 1u)]; nb[k] = 3; }
		}
		vg_def_put_group(io, T.stage, code, nb, &bit, &wbase, out32);
		for (uint32_t r0 = 0; r0 < n_rle; r0 += 64) {                 // consumes 64 code-length symbols
			for (uint32_t k = 0; k < PER; k++) {
				const uint32_t i = r0 + L + k * NL;
				code[k] = 0; nb[k] = 0;
				if (i >= n_rle) continue;
				const uint32_t x = T.rle[i], s = x & 31u;
				nb[k] = T.cl_len[s];
				code[k] = T.cl_code[s] | (x >> 8) << nb[k];
				nb[k] += vg_def_cl_extra(s);
			}
			vg_def_put_group(io, T.stage, code, nb, &bit, &wbase, out32);
		}
	}
	for (uint32_t g0 = 0; g0 <= ntok; g0 += 64) {                     // consumes 64 tokens; the end-of-block symbol is the last
		for (uint32_t k = 0; k < PER; k++) {
			const uint32_t i = g0 + L + k * NL;
			code[k] = 0; nb[k] = 0;
			if (i > ntok) continue;
			const uint32_t tk = i < ntok ? tok[i] : 256u, len = tk >> 16;
			if (!len) { code[k] = T.ll_code[tk]; nb[k] = T.ll_len[tk]; continue; }
			uint32_t le, lx, de, dx;
			const uint32_t ls = vg_def_len_sym(len, &le, &lx), ds = vg_def_dist_sym(tk & 0xffffu, &de, &dx);
			uint32_t b = T.ll_len[ls];
			uint64_t c = T.ll_code[ls];
			c |= (uint64_t)lx << b; b += le;
			c |= (uint64_t)T.d_code[ds] << b; b += T.d_len[ds];
			c |= (uint64_t)dx << b; b += de;
			code[k] = c; nb[k] = b;
		}
		vg_def_put_group(io, T.stage, code, nb, &bit, &wbase, out32);
	}
	const uint32_t bytes = (bit + 7u) >> 3;                           // (bit is T.bits: the plan counted what pass 2 emits)
	const uint32_t words = ((bytes + 3u) >> 2) - wbase;               // at most 1
	for (uint32_t w = L; w < words; w += NL) out32[wbase + w] = T.stage[w];
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
	static void add32(uint32_t *p, uint32_t v) { *p += v; }
};
// ... with the dynamic path's token buffer: n words of the caller's
struct DefHostDynIO : DefHostIO {
	uint32_t *tok;
	uint32_t *tokens() const { return tok; }
};

// the block around a payload that is in slot (coded bytes of it) or, coded 0, the stored text
inline uint32_t vg_bgzf_block_around_host(const uint8_t *text, uint32_t n, uint8_t *dst, const uint32_t *slot, uint32_t coded)
{
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

// One block on the host: text[0, n), 1 <= n <= 65280 -> a whole BGZF block at dst (room for n + 5 + 26 bytes); returns its bytes.
// sh and slot (n + VG_DEF_SLACK bytes, as words) are the caller's scratch.
inline uint32_t vg_bgzf_deflate_block_host(const uint8_t *text, uint32_t n, uint8_t *dst, VgDefShared &sh, uint32_t *slot)
{
	DefHostIO io;
	return vg_bgzf_block_around_host(text, n, dst, slot, vg_deflate_block(io, sh, text, n, slot));
}
// ... in the dynamic mode; tok: n words more of the caller's scratch
inline uint32_t vg_bgzf_deflate_block_host_dyn(const uint8_t *text, uint32_t n, uint8_t *dst, VgDefDynShared &sh, uint32_t *slot, uint32_t *tok)
{
	DefHostDynIO io;
	io.tok = tok;
	return vg_bgzf_block_around_host(text, n, dst, slot, vg_deflate_block_dyn(io, sh, text, n, slot));
}

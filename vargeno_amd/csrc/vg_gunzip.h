// Plain gzip (RFC 1952 members around one RFC 1951 stream, no block table): the member header and trailer, a finder of block starts,
// a stream decoder over 16-bit symbols, and the window resolve -- ONE core for the host and for the device, beside vg_inflate.h and
// built from its parts (vg_inf_dynamic_header, vg_inf_build, vg_inf_decode, the IO policy, the CRC helpers).  Under hipcc every
// function here is __host__ __device__; under g++ they are ordinary functions.  No zlib.
//
// A DEFLATE stream can be cut wherever a block starts, but nothing says where that is, and a block's back-references reach into the
// 32 KiB in front of it.  So a slot of compressed bytes is cut into fixed chunks and decoded in stages:
//   find      per chunk, the first bit offset in its range that passes the candidate test (a non-final dynamic-Huffman block) -- a GUESS
//   decode    per chunk with a guess, from the guess to the first block boundary at or beyond the next existing guess, into 16-bit
//             symbols: below 256 a byte, from 0x8000 "byte v - 0x8000 of the 32 KiB in front of my entry" (a placeholder)
//   confirm   a chunk is right iff its guess is its predecessor's exit
//   repair    serially, each mismatched chunk decoded again from its predecessor's now-final exit (at most VG_GZ_MAX_REPAIRS)
//   resolve   symbols -> bytes at their final place; a placeholder reads the text in front of its chunk
// Chunk 0 starts at an exact boundary (the member's first block, or the exit of the slot before).  By induction over the chunks the
// chain of entries is the sequential decoder's chain of block boundaries whatever was guessed, and by induction over the text every
// placeholder reads a byte that is final: the result equals vg_gunzip_sequential's.  The same functions run the stages on the host
// (VgGzHostStages: one lane, one stage after the other) and in the kernels of vargeno_hip.hip (one wave per chunk).
//
// TERMINATION.  Every loop of the decoder consumes at least one input bit or writes at least one output unit per iteration; the
// input is the slot's [in, in + len) and the output the [0, cap) it was given, and both ends are checked inside the loop.  Each loop
// carries a comment that says which of the two it is.  A decode speculated on garbage therefore costs at most len * 8 + cap
// iterations.  The finder tests each bit offset of a chunk's range once; a full test is one header parse (bounded as in vg_inflate.h).
#pragma once
#include "vg_inflate.h"

#include <algorithm>

enum {
	VG_GZ_ECAP = 11,          // the output capacity is used up (the ratio bound of a slot, or the caller's buffer)
	VG_GZ_EHEADER = 12,       // not a gzip member header
	VG_GZ_EBLOCK = 13,        // a slot holds no whole DEFLATE block
	VG_GZ_EREPAIRS = 14       // more mismatched chunks in a slot than VG_GZ_MAX_REPAIRS
};
VG_HD const char *vg_gunzip_strerror(int rc)
{
	switch (rc) {
	case VG_GZ_ECAP: return "output larger than the ratio bound allows";
	case VG_GZ_EHEADER: return "not a gzip member header";
	case VG_GZ_EBLOCK: return "deflate block larger than a slot";
	case VG_GZ_EREPAIRS: return "more mismatched chunks than the repair bound";
	}
	return vg_inflate_strerror(rc);
}

constexpr uint32_t VG_GZ_WINDOW = 32768;
constexpr uint32_t VG_GZ_MAX_REPAIRS = 64;           // serial work per slot, bounded as in vg_bam.h -- not a tuned number
constexpr uint64_t VG_GZ_NONE = ~0ull;
constexpr uint64_t VG_GZ_CHUNK_DEFAULT = 16384;      // provisional, from the library-call sweep of profiles/gzip_inflate.txt: every block start of zlib's 16-17 KB blocks is caught
constexpr uint64_t VG_GZ_SLOT_DEFAULT = 16ull << 20;
constexpr uint64_t VG_GZ_RATIO_DEFAULT = 8;          // DESIGN.md §4 "The plain-gzip kernels": FASTQ compresses 3.5-5 : 1; the staging is 2 * ratio bytes per compressed byte
constexpr uint64_t VG_GZ_SLOT_MAX = 64ull << 20;     // bit offsets inside a slot stay below 2^31
constexpr uint64_t VG_GZ_SYMBOLS_MAX = 1ull << 31;   // ... and so do its symbol offsets (slot bytes * ratio)

struct VgGzStats { uint64_t members, chunks, guessed, confirmed, repaired, tested, slots_refused, resume_bit; };
struct VgGzOpts { uint64_t chunk_bytes, slot_bytes, max_ratio, slot_max; };      // slot_max: how far a slot may grow to hold one whole block

// one chunk of a slot (bit offsets are relative to the slot's first byte)
struct VgGzChunkRec {
	uint64_t guess;           // the finder's guess (chunk 0: the exact entry), VG_GZ_NONE
	uint64_t entry;           // where its symbols were decoded from: the guess, or after a repair the predecessor's exit
	uint64_t exit_bit;        // the last block boundary the decode reached
	uint64_t err_bit;         // where the decode stopped when rc != 0
	uint32_t out_len;         // symbols up to exit_bit
	int32_t rc;               // VG_INF_* / VG_GZ_*: why the decode stopped short of its stop (0: it did not)
	uint32_t ended;           // the member ended at exit_bit
	uint32_t state;           // 0 no guess, 1 on the chain, 2 dropped
};
enum { VG_GZ_ST_NONE = 0, VG_GZ_ST_VALID = 1, VG_GZ_ST_DROPPED = 2 };
// what the host reads back after the chain of a slot is final
struct VgGzSlotRec {
	uint64_t exit_bit, err_bit;
	int32_t rc; uint32_t ended;
	uint32_t guessed, confirmed, repaired, tested;
};

// ---- the member header (RFC 1952) -----------------------------------------------------------------------------------------------
// The header at p, of which `avail` bytes are there.  0: *hdr_len bytes of header, the DEFLATE stream follows; 1: more bytes are
// needed; VG_GZ_EHEADER.  FEXTRA, FNAME, FCOMMENT are skipped, FHCRC (the low half of the header's CRC32) is checked.
inline int vg_gz_header(const uint8_t *p, uint64_t avail, uint64_t *hdr_len)
{
	static const uint8_t magic[3] = {0x1f, 0x8b, 0x08};
	for (uint64_t i = 0; i < 3 && i < avail; i++) if (p[i] != magic[i]) return VG_GZ_EHEADER;
	if (avail < 10) return 1;
	const uint32_t flg = p[3];
	if (flg & 0xe0u) return VG_GZ_EHEADER;
	uint64_t at = 10;
	if (flg & 4u) {
		if (avail < at + 2) return 1;
		at += 2 + (p[at] | (uint64_t)p[at + 1] << 8);
		if (avail < at) return 1;
	}
	for (uint32_t f = 8; f <= 16; f <<= 1) {
		if (!(flg & f)) continue;
		while (at < avail && p[at]) at++;                                // a zero-terminated string: one byte per step
		if (at >= avail) return 1;
		at++;
	}
	if (flg & 2u) {
		if (avail < at + 2) return 1;
		const uint32_t want = p[at] | (uint32_t)p[at + 1] << 8;
		if ((vg_crc32(vg_crc_tab_host(), 0, p, at) & 0xffffu) != want) return VG_GZ_EHEADER;
		at += 2;
	}
	*hdr_len = at;
	return 0;
}

// ---- the candidate test ---------------------------------------------------------------------------------------------------------
// Stage 1, registers only: can bit offset `bit` of in[0, n) be the start of a non-final dynamic-Huffman block?  BFINAL 0, BTYPE 2,
// HLIT <= 29, HDIST <= 29, the whole header inside the input, and the code-length code's Kraft sum exactly 1.
VG_HD bool vg_gz_prefilter(const uint8_t *in, uint64_t n, uint64_t bit)
{
	const uint64_t at = bit >> 3;
	uint32_t w = 0;
	for (uint32_t k = 0; k < 3; k++) w |= (uint32_t)(at + k < n ? in[at + k] : 0) << (8 * k);
	w >>= bit & 7u;                                                       // 17 bits of header
	if ((w & 7u) != 4u) return false;
	if (((w >> 3) & 31u) > 29u || ((w >> 8) & 31u) > 29u) return false;
	const uint32_t hclen = ((w >> 13) & 15u) + 4u;
	const uint64_t b2 = bit + 17, at2 = b2 >> 3;
	if (b2 + 3u * hclen > n * 8) return false;
	uint64_t v = 0;
	for (uint32_t k = 0; k < 8; k++) v |= (uint64_t)(at2 + k < n ? in[at2 + k] : 0) << (8 * k);
	v >>= b2 & 7u;                                                        // 57 bits: 19 lengths of 3 bits
	uint32_t kraft = 0;
	for (uint32_t i = 0; i < hclen; i++) { const uint32_t l = (uint32_t)(v >> (3 * i)) & 7u; if (l) kraft += 128u >> l; }
	return kraft == 128u;
}

// Stage 2, by the cooperating lanes, the reader behind the block's three header bits: the header parses, both code tables build,
// and there is an end-of-block code.
template <class IO>
VG_HD bool vg_gz_full_test(IO &io, VgInfTables &t)
{
	uint32_t n_lit = 0, n_dist = 0;
	if (vg_inf_dynamic_header(io, t, &n_lit, &n_dist)) return false;
	if (io.u(t.lens[256]) == 0) return false;
	if (vg_inf_build(io, t.lens, n_lit, t.lit_fast, VG_INF_LIT_FAST, t.lit_cnt, t.lit_sym, false)) return false;
	return vg_inf_build(io, t.lens + n_lit, n_dist, t.dist_fast, VG_INF_DIST_FAST, t.dist_cnt, t.dist_sym, true) == VG_INF_OK;
}

// The guess of chunk c (c >= 1) of in[0, n): the first accepted bit offset of [c * chunk_bytes * 8, (c + 1) * chunk_bytes * 8), or
// VG_GZ_NONE.  lanes() offsets are prefiltered per round; the survivors take the full test in ascending order.
template <class IO>
VG_HD uint64_t vg_gz_find_chunk(IO &io, VgInfTables &t, const uint8_t *in, uint64_t n, uint64_t c, uint64_t chunk_bytes, uint32_t *tested)
{
	const uint64_t lo = c * chunk_bytes * 8, end = (c + 1) * chunk_bytes * 8, hi = end < n * 8 ? end : n * 8;
	for (uint64_t base = lo; base < hi; base += io.lanes()) {             // every bit offset of the range once
		const uint64_t b = base + io.lane();
		uint64_t mask = io.ballot(b < hi && vg_gz_prefilter(in, n, b));
		while (mask) {                                                    // at most lanes() survivors
			const uint32_t k = (uint32_t)__builtin_ctzll(mask);
			mask &= mask - 1;
			io.seek_bit(base + k + 3);
			(*tested)++;
			if (vg_gz_full_test(io, t)) return base + k;
		}
	}
	return VG_GZ_NONE;
}

// ---- the stream decoder -----------------------------------------------------------------------------------------------------------
// Block after block from where the reader stands, output units [0, cap) through the IO (bytes or symbols: the IO knows).  It stops
// at the first block boundary at or beyond stop_bit or at the member's end (0), when the input runs out (VG_INF_EINPUT), when the
// capacity is used up (VG_GZ_ECAP), or at bad data.  *x_bit / *x_out / *x_ended: the latest block boundary, the output there, and
// whether the member ended there -- what lies behind it is an incomplete block's and does not count.  See TERMINATION at the top.
template <class IO>
VG_HD int vg_gz_stream(IO &io, VgInfTables &t, uint64_t stop_bit, typename IO::opos cap, uint64_t *x_bit, typename IO::opos *x_out, uint32_t *x_ended)
{
	typedef typename IO::opos opos;
	opos o = 0;                                                       // units written; o <= cap throughout
	*x_bit = io.bitpos(); *x_out = 0; *x_ended = 0;
	for (;;) {                                                        // one DEFLATE block per iteration: consumes at least its 3 header bits
		if (io.bitpos() >= stop_bit) return VG_INF_OK;
		io.need();
		const uint32_t hdr = io.bits(3);
		if (io.overrun()) return VG_INF_EINPUT;
		const uint32_t type = hdr >> 1;
		if (type == 3) return VG_INF_EBTYPE;
		if (type == 0) {
			io.align_byte();
			io.need();
			const uint32_t len = io.bits(16), nlen = io.bits(16);
			if (io.overrun()) return VG_INF_EINPUT;
			if ((len ^ 0xffffu) != nlen) return VG_INF_ESTORED;
			if (len > cap - o) return VG_GZ_ECAP;
			if (!io.stored_copy(o, len)) return VG_INF_EINPUT;
			o += len;
		} else {
			uint32_t n_lit = 288, n_dist = 32;
			if (type == 1) {
				// fixed codes (RFC 1951 3.2.6); all 32 five-bit distance codes, so that the set is complete -- 30 and 31 are refused when met
				for (uint32_t i = io.lane(); i < 320; i += io.lanes()) t.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
				io.sync();
			} else {
				const int rc = vg_inf_dynamic_header(io, t, &n_lit, &n_dist);
				if (rc) return rc;
				if (io.u(t.lens[256]) == 0) return VG_INF_ESYMBOL;   // no end-of-block code
			}
			int rc = vg_inf_build(io, t.lens, n_lit, t.lit_fast, VG_INF_LIT_FAST, t.lit_cnt, t.lit_sym, false);
			if (rc) return rc;
			rc = vg_inf_build(io, t.lens + n_lit, n_dist, t.dist_fast, VG_INF_DIST_FAST, t.dist_cnt, t.dist_sym, true);
			if (rc) return rc;
			for (;;) {                                                // every iteration consumes at least one input bit (a literal/length code)
				io.need();
				int s = vg_inf_decode(io, t.lit_fast, VG_INF_LIT_FAST, t.lit_cnt, t.lit_sym);
				if (s < 0) return VG_INF_ESYMBOL;
				if (io.overrun()) return VG_INF_EINPUT;
				if (s < 256) {
					if (o >= cap) return VG_GZ_ECAP;
					io.put(o++, (uint8_t)s);
					continue;
				}
				if (s == 256) break;
				s -= 257;
				if (s >= 29) return VG_INF_ESYMBOL;
				// length 3..258: codes 257-264 no extra bits, then four codes per extra bit; 285 is 258
				const uint32_t lext = s < 8 || s == 28 ? 0u : ((uint32_t)s >> 2) - 1u;
				const uint32_t len = (s < 8 ? 3u + (uint32_t)s : s == 28 ? 258u : 3u + ((4u + ((uint32_t)s & 3u)) << lext)) + io.bits(lext);
				io.need();
				const int d = vg_inf_decode(io, t.dist_fast, VG_INF_DIST_FAST, t.dist_cnt, t.dist_sym);
				if (d < 0 || d >= 30) return VG_INF_ESYMBOL;
				// distance 1..32768: codes 0-3 no extra bits, then two codes per extra bit
				const uint32_t dext = d < 4 ? 0u : ((uint32_t)d >> 1) - 1u;
				const uint32_t dist = (d < 4 ? 1u + (uint32_t)d : 1u + ((2u + ((uint32_t)d & 1u)) << dext)) + io.bits(dext);
				if (io.overrun()) return VG_INF_EINPUT;
				if (len > cap - o) return VG_GZ_ECAP;
				if (!io.copy(o, dist, len)) return VG_INF_EDIST;      // (a symbol IO takes every distance: the resolve checks it)
				o += len;
			}
		}
		*x_bit = io.bitpos(); *x_out = o;
		if (hdr & 1u) { *x_ended = 1; return VG_INF_OK; }
	}
}

// chunk c's symbols: from `entry` to the first block boundary at or beyond `stop`, the IO's output already set; the record is
// the same in every lane (the caller's lane 0 stores it)
template <class IO>
VG_HD void vg_gz_decode_chunk(IO &io, VgInfTables &t, uint64_t entry, uint64_t stop, uint64_t cap, VgGzChunkRec *r)
{
	typename IO::opos out = 0;
	io.seek_bit(entry);
	r->entry = entry;
	r->rc = vg_gz_stream(io, t, stop, (typename IO::opos)cap, &r->exit_bit, &out, &r->ended);
	r->err_bit = io.bitpos();
	r->out_len = (uint32_t)out;
	r->state = VG_GZ_ST_VALID;
}

// the next chunk after c that has a guess, or n_chunks (the gaps of all chunks together are n_chunks steps)
VG_HD uint32_t vg_gz_next_guess(const VgGzChunkRec *ck, uint32_t n_chunks, uint32_t c)
{
	uint32_t j = c + 1;
	while (j < n_chunks && ck[j].guess == VG_GZ_NONE) j++;
	return j;
}

// confirm: chunk c (c >= 1, with a guess) is right iff its guess is the exit of the chunk with a guess before it, which got there
VG_HD bool vg_gz_confirm_one(const VgGzChunkRec *ck, uint32_t c)
{
	uint32_t p = c - 1;
	while (ck[p].guess == VG_GZ_NONE) p--;                               // (chunk 0 always has one)
	return ck[p].rc == VG_INF_OK && !ck[p].ended && ck[p].exit_bit == ck[c].guess;
}

// Repair and summary, one wave / one lane.  all_ok: confirm found no mismatch, and the chain is the chunks as decoded.  Otherwise the
// chunks are walked in order from chunk 0, whose entry is exact: a chunk whose guess is the chain's exit stays as decoded; one that
// the chain has already passed is dropped; any other is decoded again from the chain's exit into its own staging area
// (stag + c * area symbols, up to the next chunk with a guess).  More than VG_GZ_MAX_REPAIRS of those refuse the slot.
template <class IO>
VG_HD void vg_gz_repair_chain(IO &io, VgInfTables &t, VgGzChunkRec *ck, uint32_t n_chunks, uint64_t n_bits, uint64_t area, uint16_t *stag, bool all_ok, VgGzSlotRec *sr)
{
	VgGzChunkRec cur = ck[0];                                             // the chain's last chunk: the same in every lane
	cur.exit_bit = io.u64(cur.exit_bit); cur.rc = (int32_t)io.u((uint32_t)cur.rc); cur.ended = io.u(cur.ended);
	uint32_t repairs = 0, confirmed = 0, guessed = 1;
	int32_t refused = 0;
	if (all_ok) {                                                         // nothing to walk: the lanes count the guesses and find the last
		uint32_t cnt = 0, last = 0;
		for (uint32_t c = io.lane(); c < n_chunks; c += io.lanes()) if (ck[c].guess != VG_GZ_NONE) { cnt++; last = c; }
		guessed = io.reduce_add(cnt); confirmed = guessed - 1;
		cur = ck[io.reduce_max(last)];
	}
	for (uint32_t c = 1; c < n_chunks && !all_ok; c++) {                  // serial over the chunks; at most VG_GZ_MAX_REPAIRS decodes among them
		const uint64_t g = io.u64(ck[c].guess);
		if (g == VG_GZ_NONE) continue;
		guessed++;
		if (refused) continue;
		bool drop = cur.ended || cur.rc != VG_INF_OK;
		if (!drop && g == cur.exit_bit) {
			cur = ck[c];
			cur.exit_bit = io.u64(cur.exit_bit); cur.rc = (int32_t)io.u((uint32_t)cur.rc); cur.ended = io.u(cur.ended);
			confirmed++;
			continue;
		}
		uint32_t nx = n_chunks;
		uint64_t stop = n_bits;
		if (!drop) {
			nx = io.u(vg_gz_next_guess(ck, n_chunks, c));
			if (nx < n_chunks) stop = io.u64(ck[nx].guess);
			drop = cur.exit_bit >= stop;                                  // the chain is already past this chunk's whole range
		}
		if (drop) {
			if (io.lane() == 0) { ck[c].state = VG_GZ_ST_DROPPED; ck[c].out_len = 0; }
			continue;
		}
		if (repairs == VG_GZ_MAX_REPAIRS) { refused = VG_GZ_EREPAIRS; continue; }
		repairs++;
		io.set_out(stag + (uint64_t)c * area);
		VgGzChunkRec r = ck[c];
		vg_gz_decode_chunk(io, t, cur.exit_bit, stop, (uint64_t)(nx - c) * area, &r);
		if (io.lane() == 0) ck[c] = r;
		cur = r;
	}
	if (io.lane() == 0) {
		sr->exit_bit = cur.exit_bit; sr->err_bit = cur.err_bit; sr->rc = refused ? refused : cur.rc; sr->ended = cur.ended;
		sr->guessed = guessed; sr->confirmed = confirmed; sr->repaired = repairs;
	}
}

// ---- the window resolve -----------------------------------------------------------------------------------------------------------
// One symbol of a chunk whose text starts at text[chunk_off] -> its byte.  A placeholder k is text[chunk_off - 32768 + k]; `before`
// bytes of the member lie in front of text[0] (at most 32768 matter).  false: the reference reaches before the member.
VG_HD bool vg_gz_resolve_sym(uint16_t s, const uint8_t *text, int64_t chunk_off, int64_t before, uint8_t *out)
{
	if (s < 0x8000u) { *out = (uint8_t)s; return true; }
	const int64_t p = chunk_off - (int64_t)VG_GZ_WINDOW + (int64_t)(s - 0x8000u);
	if (p < -before) return false;
	*out = text[p];
	return true;
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
// the host's reader: plain memory, one lane, any bit offset of in[0, len)
struct VgGzHostReader : VgHostLanes {
	const uint8_t *in = nullptr; uint64_t len = 0, pos = 0;
	uint64_t bitbuf = 0; uint32_t bitcnt = 0;
	int64_t bits_left = 0;                                            // input bits not yet consumed; negative: the decoder ran past the end
	uint64_t needs = 0;                                               // calls of need(): at least one, at most two per iteration of a decoder loop
	static uint32_t u(uint32_t x) { return x; }
	static uint64_t u64(uint64_t x) { return x; }
	static uint64_t ballot(bool p) { return p ? 1u : 0u; }
	static uint32_t reduce_add(uint32_t x) { return x; }              // over the lanes
	static uint32_t reduce_max(uint32_t x) { return x; }
	void seek_bit(uint64_t bit)
	{
		pos = bit >> 3; bitbuf = 0; bitcnt = 0;
		bits_left = (int64_t)(len * 8) - (int64_t)(pos * 8);
		need();
		drop((uint32_t)(bit & 7u));
	}
	uint64_t bitpos() const { return (uint64_t)((int64_t)(len * 8) - bits_left); }
	void need() { needs++; while (bitcnt <= 56) { bitbuf |= (uint64_t)(pos < len ? in[pos] : 0) << bitcnt; pos++; bitcnt += 8; } }   // (8 steps at most)
	uint32_t peek() const { return (uint32_t)bitbuf; }
	void drop(uint32_t n) { bitbuf >>= n; bitcnt -= n; bits_left -= n; }
	uint32_t bits(uint32_t n) { const uint32_t v = (uint32_t)bitbuf & ((1u << n) - 1u); drop(n); return v; }
	void align_byte() { drop(bitcnt & 7u); }
	bool overrun() const { return bits_left < 0; }
	// a stored block's bytes: the reader is byte-aligned and not past the end (the caller checked)
	const uint8_t *stored_take(uint64_t n)
	{
		const uint64_t at = len - (uint64_t)(bits_left >> 3);
		if (n > len - at) return nullptr;
		pos = at + n; bitbuf = 0; bitcnt = 0; bits_left -= (int64_t)n * 8;
		return in + at;
	}
};
// output as bytes, the window known throughout: the member's own text, `before` bytes of it in front of out[0]
struct VgGzHostBytes : VgGzHostReader {
	typedef uint64_t opos;
	uint8_t *out = nullptr;
	uint64_t before = 0;                                              // bytes of the member's text in front of out[0] (a window carried over)
	void put(opos o, uint8_t b) { out[o] = b; }
	bool copy(opos o, uint32_t dist, uint32_t n)
	{
		if (dist > o + before) return false;
		for (uint32_t j = 0; j < n; j++) out[o + j] = out[o + j - dist];      // n output bytes
		return true;
	}
	bool stored_copy(opos o, uint32_t n)
	{
		const uint8_t *s = stored_take(n);
		if (!s) return false;
		if (n) memcpy(out + o, s, n);
		return true;
	}
};
// output as symbols, the window in front of the entry unknown
struct VgGzHostSyms : VgGzHostReader {
	typedef uint32_t opos;
	uint16_t *out = nullptr;
	void set_out(uint16_t *p) { out = p; }
	void put(opos o, uint8_t b) { out[o] = b; }
	bool copy(opos o, uint32_t dist, uint32_t n)
	{
		for (uint32_t j = 0; j < n; j++) {                                     // n output symbols
			const int64_t s = (int64_t)o + j - (int64_t)dist;
			out[o + j] = s >= 0 ? out[s] : (uint16_t)(0x8000u + (uint32_t)((int64_t)VG_GZ_WINDOW + s));
		}
		return true;
	}
	bool stored_copy(opos o, uint32_t n)
	{
		const uint8_t *s = stored_take(n);
		if (!s) return false;
		for (uint32_t j = 0; j < n; j++) out[o + j] = s[j];
		return true;
	}
};

struct VgGzResult { int rc = 0; uint64_t text_len = 0, consumed = 0, bad_offset = UINT64_MAX; VgGzStats st = {}; uint64_t steps = 0; };

inline uint32_t vg_gz_le32(const uint8_t *p) { return p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// The reference decoder: gz[0, n) member after member, sequentially, one lane, the window known throughout.  r->rc 0: every member
// decoded and its CRC32 and ISIZE verified; otherwise r->bad_offset names the compressed offset, and text_len / consumed stand at
// the end of the last good member.
inline void vg_gunzip_sequential(const uint8_t *gz, uint64_t n, uint8_t *text, uint64_t text_cap, VgGzResult *r)
{
	VgInfTables t;
	uint64_t pos = 0, len = 0;
	while (pos < n) {                                                         // one member per iteration: at least 18 bytes
		uint64_t hl = 0;
		const int hrc = vg_gz_header(gz + pos, n - pos, &hl);
		if (hrc) { r->rc = hrc == 1 ? VG_INF_EINPUT : hrc; r->bad_offset = hrc == 1 ? n : pos; return; }
		VgGzHostBytes io;
		io.in = gz; io.len = n; io.out = text + len;
		io.seek_bit((pos + hl) * 8);
		uint64_t x_bit = 0, x_out = 0; uint32_t ended = 0;
		const int rc = vg_gz_stream(io, t, UINT64_MAX, text_cap - len, &x_bit, &x_out, &ended);
		r->steps += io.needs;
		if (rc) { r->rc = rc; r->bad_offset = io.bitpos() / 8 < n ? io.bitpos() / 8 : n; return; }
		const uint64_t tb = (x_bit + 7) >> 3;
		if (tb + 8 > n) { r->rc = VG_INF_EINPUT; r->bad_offset = n; return; }
		if (vg_crc32(vg_crc_tab_host(), 0, text + len, x_out) != vg_gz_le32(gz + tb)) { r->rc = VG_INF_ECRC; r->bad_offset = tb; return; }
		if ((uint32_t)x_out != vg_gz_le32(gz + tb + 4)) { r->rc = VG_INF_ESIZE; r->bad_offset = tb + 4; return; }
		len += x_out; pos = tb + 8;
		r->st.members++; r->text_len = len; r->consumed = pos;
	}
}

// ---- the chunked route: what the host decides between the stages of a slot --------------------------------------------------------
// A backend runs the stages of one slot (host: VgGzHostStages below; device: the kernels of vargeno_hip.hip):
//   int chain(in_off, in_len, entry_bit, last, VgGzSlotRec *rec, uint64_t *text_len)   find, decode, confirm, repair, output offsets
//   int resolve(text_off, before, text_len, uint32_t *crc, uint64_t *bad_bit)          symbols -> text[text_off, +text_len) and its CRC32;
//                                                                                       *bad_bit: entry of a chunk that reaches before the member
// Both return a backend failure (not a verdict on the data) or 0.  The slot is gz[in_off, in_off + in_len), entered at entry_bit (< 8).
// (a slot is never longer than the input: nbytes bounds it, and with it the staging)
inline VgGzOpts vg_gz_opts_checked(VgGzOpts op, uint64_t nbytes)
{
	if (!op.chunk_bytes) op.chunk_bytes = VG_GZ_CHUNK_DEFAULT;
	if (!op.slot_bytes) op.slot_bytes = VG_GZ_SLOT_DEFAULT;
	if (!op.max_ratio) op.max_ratio = VG_GZ_RATIO_DEFAULT;
	if (op.chunk_bytes < 64) op.chunk_bytes = 64;
	if (op.slot_bytes > VG_GZ_SLOT_MAX) op.slot_bytes = VG_GZ_SLOT_MAX;
	if (op.slot_bytes > nbytes) op.slot_bytes = nbytes;
	if (op.slot_bytes < op.chunk_bytes) op.slot_bytes = op.chunk_bytes;
	if (op.max_ratio * op.slot_bytes > VG_GZ_SYMBOLS_MAX) op.max_ratio = VG_GZ_SYMBOLS_MAX / op.slot_bytes;
	if (!op.slot_max || op.slot_max > VG_GZ_SLOT_MAX) op.slot_max = VG_GZ_SLOT_MAX;
	if (op.slot_max < op.slot_bytes) op.slot_max = op.slot_bytes;
	if (op.max_ratio * op.slot_max > VG_GZ_SYMBOLS_MAX) op.slot_max = std::max<uint64_t>(op.slot_bytes, VG_GZ_SYMBOLS_MAX / op.max_ratio);
	return op;
}

template <class B>
inline int vg_gunzip_chunked(B &be, const uint8_t *gz, uint64_t n, uint64_t text_cap, const VgGzOpts &op, VgGzResult *r)
{
	uint64_t pos = 0, text = 0;
	while (pos < n) {                                                         // one member per iteration: at least 18 bytes
		uint64_t hl = 0;
		const int hrc = vg_gz_header(gz + pos, n - pos, &hl);
		if (hrc) { r->rc = hrc == 1 ? VG_INF_EINPUT : hrc; r->bad_offset = hrc == 1 ? n : pos; return 0; }
		const uint64_t member_text = text;
		uint64_t bit = (pos + hl) * 8;
		uint32_t crc = 0;
		uint64_t slot_len = op.slot_bytes;
		for (;;) {                                                            // one slot per iteration: at least one block further, or the slot twice as long
			if ((bit >> 3) >= n) { r->rc = VG_INF_EINPUT; r->bad_offset = n; r->text_len = member_text; r->consumed = pos; return 0; }
			const uint64_t at = bit >> 3, in_len = n - at < slot_len ? n - at : slot_len;
			const bool last = at + in_len == n;
			VgGzSlotRec rec = {};
			uint64_t slot_text = 0;
			int brc = be.chain(at, in_len, (uint32_t)(bit & 7u), &rec, &slot_text);
			if (brc) return brc;
			r->st.chunks += (in_len + op.chunk_bytes - 1) / op.chunk_bytes;
			r->st.guessed += rec.guessed; r->st.confirmed += rec.confirmed; r->st.repaired += rec.repaired; r->st.tested += rec.tested;
			int rc = rec.rc;
			uint64_t bad = at + rec.err_bit / 8;
			if (rc == VG_INF_EINPUT && !last) {                               // the slot's tail block is incomplete: the next slot starts at its boundary
				rc = 0;
				if (rec.exit_bit == (bit & 7u)) {                             // ... not one whole block: the same entry again with more bytes behind it
					if (slot_len * 2 <= op.slot_max) { slot_len *= 2; continue; }
					rc = VG_GZ_EBLOCK;
				}
				bad = at;
			}
			slot_len = op.slot_bytes;
			if (rc == VG_GZ_ECAP || rc == VG_GZ_EREPAIRS) {                   // refused: nothing of the slot counts
				r->st.slots_refused++; r->st.resume_bit = bit;
				r->text_len = text; r->consumed = at;
				return 0;
			}
			// bad data inside a member: nothing of the member counts (its text was not verified)
			if (rc) { r->rc = rc; r->bad_offset = bad < n ? bad : n; r->text_len = member_text; r->consumed = pos; return 0; }
			if (slot_text > text_cap - text) { r->rc = VG_GZ_ECAP; r->bad_offset = at; r->text_len = member_text; r->consumed = pos; return 0; }
			const uint64_t before = text - member_text < VG_GZ_WINDOW ? text - member_text : VG_GZ_WINDOW;
			uint32_t slot_crc = 0;
			uint64_t bad_bit = VG_GZ_NONE;
			brc = be.resolve(text, before, slot_text, &slot_crc, &bad_bit);
			if (brc) return brc;
			if (bad_bit != VG_GZ_NONE) { r->rc = VG_INF_EDIST; r->bad_offset = at + bad_bit / 8; r->text_len = member_text; r->consumed = pos; return 0; }
			crc = vg_crc_mul(crc, vg_crc_x8n((uint32_t)slot_text)) ^ slot_crc;
			text += slot_text;
			bit = at * 8 + rec.exit_bit;
			r->text_len = text; r->consumed = bit >> 3; r->st.resume_bit = bit;
			if (rec.ended) break;
		}
		const uint64_t tb = (bit + 7) >> 3;
		r->text_len = member_text; r->consumed = pos;
		if (tb + 8 > n) { r->rc = VG_INF_EINPUT; r->bad_offset = n; return 0; }
		if (crc != vg_gz_le32(gz + tb)) { r->rc = VG_INF_ECRC; r->bad_offset = tb; return 0; }
		if ((uint32_t)(text - member_text) != vg_gz_le32(gz + tb + 4)) { r->rc = VG_INF_ESIZE; r->bad_offset = tb + 4; return 0; }
		pos = tb + 8;
		r->st.members++; r->text_len = text; r->consumed = pos; r->st.resume_bit = pos * 8;
	}
	return 0;
}

// The stages on the host, one after the other, one lane: what the kernels do, with no device.  `steps` counts the iterations of
// find (bit offsets) and decode (input bits + output symbols are its bound) for the TERMINATION check of the fuzzer.
struct VgGzHostStages {
	const uint8_t *gz; uint8_t *text; VgGzOpts op;
	std::vector<VgGzChunkRec> ck;
	std::vector<uint16_t> stag;
	std::vector<uint64_t> off;
	uint32_t n_chunks = 0;
	VgInfTables t;
	uint64_t needs = 0;
	VgGzHostStages(const uint8_t *gz_, uint8_t *text_, const VgGzOpts &op_) : gz(gz_), text(text_), op(op_) {}

	int chain(uint64_t in_off, uint64_t in_len, uint32_t entry_bit, VgGzSlotRec *rec, uint64_t *text_len)
	{
		const uint8_t *in = gz + in_off;
		const uint64_t area = op.chunk_bytes * op.max_ratio, n_bits = in_len * 8;
		n_chunks = (uint32_t)((in_len + op.chunk_bytes - 1) / op.chunk_bytes);
		ck.assign(n_chunks, VgGzChunkRec{});
		stag.resize((size_t)n_chunks * area);
		off.assign(n_chunks + 1, 0);
		VgGzHostSyms io;
		io.in = in; io.len = in_len;
		uint32_t tested = 0;
		for (uint32_t c = 0; c < n_chunks; c++) {                                 // find
			ck[c].guess = c == 0 ? entry_bit : vg_gz_find_chunk(io, t, in, in_len, c, op.chunk_bytes, &tested);
			ck[c].rc = 0; ck[c].state = VG_GZ_ST_NONE;
		}
		for (uint32_t c = 0; c < n_chunks; c++) {                                 // decode
			if (ck[c].guess == VG_GZ_NONE) continue;
			const uint32_t nx = vg_gz_next_guess(ck.data(), n_chunks, c);
			io.set_out(stag.data() + (size_t)c * area);
			vg_gz_decode_chunk(io, t, ck[c].guess, nx < n_chunks ? ck[nx].guess : n_bits, (uint64_t)(nx - c) * area, &ck[c]);
		}
		bool all_ok = true;                                                       // confirm
		for (uint32_t c = 1; c < n_chunks; c++) if (ck[c].guess != VG_GZ_NONE && !vg_gz_confirm_one(ck.data(), c)) all_ok = false;
		vg_gz_repair_chain(io, t, ck.data(), n_chunks, n_bits, area, stag.data(), all_ok, rec);
		rec->tested = tested;
		needs += io.needs;
		for (uint32_t c = 0; c < n_chunks; c++) off[c + 1] = off[c] + (ck[c].state == VG_GZ_ST_VALID ? ck[c].out_len : 0);      // output offsets
		*text_len = off[n_chunks];
		return 0;
	}
	int resolve(uint64_t text_off, uint64_t before, uint64_t text_len, uint32_t *crc, uint64_t *bad_bit)
	{
		uint8_t *tx = text + text_off;
		const uint64_t area = op.chunk_bytes * op.max_ratio;
		for (uint32_t c = 0; c < n_chunks; c++) {                                 // windows and resolve are one pass here: chunks in order
			if (ck[c].state != VG_GZ_ST_VALID) continue;
			const uint16_t *s = stag.data() + (size_t)c * area;
			for (uint32_t j = 0; j < ck[c].out_len; j++)
				if (!vg_gz_resolve_sym(s[j], tx, (int64_t)off[c], (int64_t)before, tx + off[c] + j) && ck[c].entry < *bad_bit) *bad_bit = ck[c].entry;
		}
		*crc = vg_crc32(vg_crc_tab_host(), 0, tx, text_len);
		return 0;
	}
};

// ---- the chunked route over PUSHES: the same decisions as vg_gunzip_chunked, the compressed bytes arriving cut anywhere -----------
// The bytes not yet consumed (the incomplete tail block of the last slot, a header or trailer cut short) wait on the host in `carry`
// for the next push, as BgzfStream::carry does.  A slot is run when slot_len bytes are there, or at end() with what is left: the
// slots, and with them every result, are those of vg_gunzip_chunked over the whole file (a slot that ends exactly at the end of
// the file is run once more at end(): the driver could not know that nothing follows; only the chunk counts see that).  Every slot's entry is a CHECKPOINT: its
// compressed bit offset, the text offset there, and the member's text in front of it (at most 32 KiB: the window a decoder needs
// to go on from there) -- what a caller that takes over after a refusal asks for.
// The backend runs a slot's stages on bytes the driver hands it and keeps the text:
//   int chain_at(in, in_len, entry_bit, VgGzSlotRec *rec, uint64_t *text_len)        as chain(), the slot at `in`
//   int resolve_next(before, text_len, uint32_t *crc, uint64_t *bad_bit)              as resolve(), the text behind the text so far
//   int window(uint8_t *dst, before)                                                  the last `before` bytes of the text so far; dst is
//                                                                                     read after the chain_at that follows, not before
struct VgGzCheckpoint { uint64_t comp_bit, text_off; std::vector<uint8_t> window; };

template <class B>
struct VgGzPush {
	B &be;
	VgGzOpts op;
	std::vector<uint8_t> carry;                                           // compressed bytes from file offset comp_pos on: carry[head..]
	size_t head = 0;
	uint64_t comp_pos = 0;
	uint32_t bit = 0;                                                     // inside a member: the entry's bit in carry[head]
	enum { HEADER, BODY, TRAILER } state = HEADER;
	uint64_t text = 0, member_text = 0, member_pos = 0, slot_len = 0;
	uint32_t crc = 0;
	bool stopped = false;                                                 // bad data or a refused slot: nothing more is decoded
	VgGzResult r;
	std::vector<VgGzCheckpoint> cks;

	VgGzPush(B &be_, const VgGzOpts &op_) : be(be_), op(op_) { slot_len = op.slot_bytes; }
	int push(const uint8_t *p, uint64_t n)
	{
		if (stopped || !n) return 0;
		if (head) { carry.erase(carry.begin(), carry.begin() + (long)head); head = 0; }
		carry.insert(carry.end(), p, p + n);
		return pump(false);
	}
	int end() { return stopped ? 0 : pump(true); }
	// the last checkpoint at or before a text offset (null: none was taken)
	const VgGzCheckpoint *checkpoint(uint64_t text_offset) const
	{
		const VgGzCheckpoint *best = nullptr;
		for (const VgGzCheckpoint &c : cks) if (c.text_off <= text_offset) best = &c;
		return best;
	}
private:
	void eat(uint64_t n) { head += (size_t)n; comp_pos += n; }
	int stop(int rc, uint64_t bad)
	{
		stopped = true;
		r.rc = rc; r.bad_offset = bad; r.text_len = member_text; r.consumed = member_pos;      // nothing of the member counts
		return 0;
	}
	int pump(bool fin)
	{
		for (;;) {                                                        // every turn consumes bytes of the carry, doubles slot_len, or returns
			const uint8_t *p = carry.data() + head;
			const uint64_t avail = carry.size() - head, n = comp_pos + avail;
			if (state == HEADER) {
				r.text_len = text; r.consumed = comp_pos;
				if (!avail) return 0;
				uint64_t hl = 0;
				const int hrc = vg_gz_header(p, avail, &hl);
				if (hrc == 1) { member_text = text; member_pos = comp_pos; return fin ? stop(VG_INF_EINPUT, n) : 0; }
				if (hrc) { member_text = text; member_pos = comp_pos; return stop(hrc, comp_pos); }
				member_text = text; member_pos = comp_pos;
				eat(hl);
				state = BODY; bit = 0; crc = 0; slot_len = op.slot_bytes;
				continue;
			}
			if (state == BODY) {
				if (avail < slot_len && !fin) return 0;
				if (!avail) return stop(VG_INF_EINPUT, n);
				const uint64_t in_len = avail < slot_len ? avail : slot_len;
				const bool last = fin && in_len == avail;
				const uint64_t before = text - member_text < VG_GZ_WINDOW ? text - member_text : VG_GZ_WINDOW;
				if (cks.empty() || cks.back().comp_bit != comp_pos * 8 + bit) {
					cks.push_back(VgGzCheckpoint{comp_pos * 8 + bit, text, std::vector<uint8_t>((size_t)before)});
					if (before) { const int wrc = be.window(cks.back().window.data(), before); if (wrc) return wrc; }
				}
				VgGzSlotRec rec = {};
				uint64_t slot_text = 0;
				int brc = be.chain_at(p, in_len, bit, &rec, &slot_text);
				if (brc) return brc;
				r.st.chunks += (in_len + op.chunk_bytes - 1) / op.chunk_bytes;
				r.st.guessed += rec.guessed; r.st.confirmed += rec.confirmed; r.st.repaired += rec.repaired; r.st.tested += rec.tested;
				int rc = rec.rc;
				uint64_t bad = comp_pos + rec.err_bit / 8;
				if (rc == VG_INF_EINPUT && !last) {                           // the slot's tail block is incomplete: it waits in the carry
					rc = 0;
					if (rec.exit_bit == bit) {                                // ... not one whole block: the same entry again with more bytes behind it
						if (slot_len * 2 <= op.slot_max) { slot_len *= 2; continue; }
						rc = VG_GZ_EBLOCK;
					}
					bad = comp_pos;
				}
				slot_len = op.slot_bytes;
				if (rc == VG_GZ_ECAP || rc == VG_GZ_EREPAIRS) {               // refused: nothing of the slot counts
					r.st.slots_refused++; r.st.resume_bit = comp_pos * 8 + bit;
					r.text_len = text; r.consumed = comp_pos;
					stopped = true;
					return 0;
				}
				if (rc) return stop(rc, bad < n ? bad : n);
				uint32_t slot_crc = 0;
				uint64_t bad_bit = VG_GZ_NONE;
				brc = be.resolve_next(before, slot_text, &slot_crc, &bad_bit);
				if (brc) return brc;
				if (bad_bit != VG_GZ_NONE) return stop(VG_INF_EDIST, comp_pos + bad_bit / 8);
				crc = vg_crc_mul(crc, vg_crc_x8n((uint32_t)slot_text)) ^ slot_crc;
				text += slot_text;
				eat(rec.exit_bit >> 3);
				bit = (uint32_t)(rec.exit_bit & 7u);
				r.st.resume_bit = comp_pos * 8 + bit;
				if (rec.ended) state = TRAILER;
				continue;
			}
			const uint64_t tb = (bit + 7u) >> 3;                              // TRAILER
			if (avail < tb + 8) return fin ? stop(VG_INF_EINPUT, n) : 0;
			if (crc != vg_gz_le32(p + tb)) return stop(VG_INF_ECRC, comp_pos + tb);
			if ((uint32_t)(text - member_text) != vg_gz_le32(p + tb + 4)) return stop(VG_INF_ESIZE, comp_pos + tb + 4);
			eat(tb + 8);
			bit = 0; state = HEADER;
			r.st.members++; r.st.resume_bit = comp_pos * 8;
		}
	}
};

// the host stages behind the push driver: the text grows in `out`
struct VgGzHostPushStages {
	VgGzHostStages st;
	std::vector<uint8_t> out;
	explicit VgGzHostPushStages(const VgGzOpts &op) : st(nullptr, nullptr, op) {}
	int chain_at(const uint8_t *in, uint64_t in_len, uint32_t entry_bit, VgGzSlotRec *rec, uint64_t *text_len)
	{
		st.gz = in;
		return st.chain(0, in_len, entry_bit, rec, text_len);
	}
	int resolve_next(uint64_t before, uint64_t text_len, uint32_t *crc, uint64_t *bad_bit)
	{
		const size_t o = out.size();
		out.resize(o + text_len);
		st.text = out.data();
		return st.resolve(o, before, text_len, crc, bad_bit);
	}
	int window(uint8_t *dst, uint64_t before) { memcpy(dst, out.data() + out.size() - before, before); return 0; }
};

// BGZF (blocked gzip, RFC 1952 members with a `BC` extra subfield) and raw DEFLATE (RFC 1951): ONE inflate core for the host and
// for the device.  Under hipcc every function here is __host__ __device__; under g++ they are ordinary functions.  No zlib.
//
// The core is written once, in SPMD form, over an IO policy:
//   lane() / lanes()      who I am among the cooperating lanes (host: 0 of 1; device: one wave of 64)
//   sync()                every earlier write to the shared tables / the output is visible to every lane (host: nothing)
//   u(x)                  x, known to be the same in every lane (device: readfirstlane; host: x)
//   need()                at least 32 bits are in the bit buffer (zeros behind the end of the input -- overrun() then says so)
//   peek() bits(n) drop(n) align_byte() overrun()
//   put(o, byte)  copy(o, dist, len)  stored_copy(o, len)      the output, [0, isize)
// Decode state (bit buffer, positions, symbols) is the same in every lane; the lanes share the work that is parallel: building the
// code tables, copies, the CRC.  HostIO below is the host's policy; the wave policy lives next to the kernel (vargeno_hip.hip).
//
// TERMINATION.  Every loop of the decoder consumes at least one input bit or writes at least one output byte per iteration; the
// input is [in, in + len) and the output [out, out + isize), isize <= 65536, and both ends are checked inside the loop.  Each loop
// carries a comment that says which of the two it is.  A corrupt file therefore costs at most len * 8 + isize iterations.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#if defined(__HIPCC__)
#define VG_HD __host__ __device__ __attribute__((always_inline)) inline
#else
#define VG_HD inline
#endif

enum {
	VG_INF_OK = 0,
	VG_INF_EINPUT = 1,        // input exhausted
	VG_INF_EBTYPE = 2,        // block type 3
	VG_INF_ESTORED = 3,       // stored block: LEN != ~NLEN
	VG_INF_EOVER = 4,         // over-subscribed code lengths
	VG_INF_EINCOMPLETE = 5,   // incomplete code lengths (other than the single-code distance tree)
	VG_INF_ESYMBOL = 6,       // a symbol that does not exist (or a header that names too many)
	VG_INF_EDIST = 7,         // a distance that reaches before the block's own output
	VG_INF_ESIZE = 8,         // output longer or shorter than ISIZE
	VG_INF_ECRC = 9,          // CRC32 of the output differs from the trailer's
	VG_INF_EHEADER = 10       // not a BGZF block header (host walk only)
};
VG_HD const char *vg_inflate_strerror(int rc)
{
	switch (rc) {
	case VG_INF_OK: return "ok";
	case VG_INF_EINPUT: return "deflate error: input exhausted";
	case VG_INF_EBTYPE: return "deflate error: invalid block type";
	case VG_INF_ESTORED: return "deflate error: stored block LEN / NLEN mismatch";
	case VG_INF_EOVER: return "deflate error: over-subscribed code lengths";
	case VG_INF_EINCOMPLETE: return "deflate error: incomplete code lengths";
	case VG_INF_ESYMBOL: return "deflate error: invalid symbol";
	case VG_INF_EDIST: return "deflate error: distance reaches before the block";
	case VG_INF_ESIZE: return "size: output differs from ISIZE";
	case VG_INF_ECRC: return "CRC: output differs from the trailer's CRC32";
	case VG_INF_EHEADER: return "not a BGZF block header";
	}
	return "unknown";
}

constexpr uint32_t VG_BGZF_MAX_ISIZE = 65536;
constexpr unsigned VG_INF_LIT_FAST = 10, VG_INF_DIST_FAST = 8;       // bits the one-look-up tables resolve; longer codes walk the counts

// one BGZF block, as the header walk reports it and as the kernel's block table holds it (32 bytes)
struct vg_bgzf_block {
	uint64_t comp_off;        // offset of the block (its 1f 8b) in the compressed stream
	uint64_t text_off;        // offset of its first output byte in the uncompressed stream
	uint32_t in_off;          // payload (raw DEFLATE): offset in the scanned buffer ...
	uint32_t in_len;          // ... and length
	uint32_t isize;           // uncompressed size, <= 65536
	uint32_t crc;             // CRC32 of the uncompressed bytes
};

// The code tables of one DEFLATE block (host: on the stack; device: LDS).  A fast entry is (symbol << 4 | code length), 0 where the
// code is longer than the table's index (or does not exist): the decoder then walks cnt[] / sym[] bit by bit.
struct VgInfTables {
	uint16_t lit_fast[1u << VG_INF_LIT_FAST];
	uint16_t dist_fast[1u << VG_INF_DIST_FAST];
	uint16_t lit_sym[288], dist_sym[32];          // symbols in canonical order
	uint16_t lit_cnt[16], dist_cnt[16];           // codes per length
	uint8_t lens[320];                            // code lengths as read: literal/length codes, then distance codes
};

// ---- code tables -------------------------------------------------------------------------------------------------------------
VG_HD uint32_t vg_inf_bitrev(uint32_t code, uint32_t len)
{
	uint32_t r = 0;
	for (uint32_t i = 0; i < len; i++) { r = (r << 1) | (code & 1u); code >>= 1; }      // (len <= 15)
	return r;
}

// lens[0, n) -> fast / cnt / sym.  Lane l counts the codes of length l, then places them: 15 lanes at work, n steps each.
template <class IO>
VG_HD int vg_inf_build(IO &io, const uint8_t *lens, uint32_t n, uint16_t *fast, uint32_t fbits, uint16_t *cnt, uint16_t *sym, bool single_ok)
{
	const uint32_t L = io.lane(), NL = io.lanes();
	for (uint32_t i = L; i < (1u << fbits); i += NL) fast[i] = 0;
	for (uint32_t l = L; l < 16; l += NL) {
		uint32_t c = 0;
		for (uint32_t s = 0; s < n; s++) c += lens[s] == l;
		cnt[l] = (uint16_t)c;
	}
	io.sync();
	int32_t left = 1;
	uint32_t total = 0;
	for (uint32_t l = 1; l <= 15; l++) {
		const uint32_t c = io.u(cnt[l]);
		left = (left << 1) - (int32_t)c;
		if (left < 0) return VG_INF_EOVER;
		total += c;
	}
	// no code at all is a table in which nothing decodes (a block of literals needs no distance code); otherwise the set must
	// be complete, but for the single distance code of length 1 that zlib's deflate writes
	if (left > 0 && total != 0 && !(single_ok && total == 1 && io.u(cnt[1]) == 1)) return VG_INF_EINCOMPLETE;
	for (uint32_t l = 1 + L; l <= 15; l += NL) {
		if (cnt[l] == 0) continue;
		uint32_t idx = 0, code = 0;
		for (uint32_t k = 1; k < l; k++) { idx += cnt[k]; code = (code + cnt[k]) << 1; }
		for (uint32_t s = 0; s < n; s++) {
			if (lens[s] != l) continue;
			sym[idx++] = (uint16_t)s;
			if (l <= fbits) for (uint32_t f = vg_inf_bitrev(code, l); f < (1u << fbits); f += 1u << l) fast[f] = (uint16_t)(s << 4 | l);
			code++;
		}
	}
	io.sync();
	return VG_INF_OK;
}

// one symbol; -1: no such code.  need() came before: at least 15 bits are there.
template <class IO>
VG_HD int vg_inf_decode(IO &io, const uint16_t *fast, uint32_t fbits, const uint16_t *cnt, const uint16_t *sym)
{
	uint32_t b = io.peek();
	const uint32_t e = io.u(fast[b & ((1u << fbits) - 1u)]);
	if (e & 15u) { io.drop(e & 15u); return (int)(e >> 4); }
	uint32_t code = 0, first = 0, index = 0;
	for (uint32_t len = 1; len <= 15; len++) {                       // at most 15 steps; the caller consumes `len` bits or stops
		code |= b & 1u; b >>= 1;
		const uint32_t c = io.u(cnt[len]);
		if (code < first + c) { io.drop(len); return (int)io.u(sym[index + (code - first)]); }
		index += c; first = (first + c) << 1; code <<= 1;
	}
	return -1;
}

// ---- raw DEFLATE ---------------------------------------------------------------------------------------------------------------
template <class IO>
VG_HD int vg_inf_dynamic_header(IO &io, VgInfTables &t, uint32_t *n_lit, uint32_t *n_dist)
{
	io.need();
	const uint32_t hlit = io.bits(5) + 257, hdist = io.bits(5) + 1, hclen = io.bits(4) + 4;
	if (io.overrun()) return VG_INF_EINPUT;
	if (hlit > 286 || hdist > 30) return VG_INF_ESYMBOL;
	// the code-length code, read into lens[0, 19) and built into the distance tables (7-bit codes: one look-up each)
	for (uint32_t i = io.lane(); i < 19; i += io.lanes()) t.lens[i] = 0;
	io.sync();
	for (uint32_t i = 0; i < hclen; i++) {                            // 3 bits each, hclen <= 19
		if ((i & 7u) == 0) io.need();
		const uint32_t v = io.bits(3);
		// the order of RFC 1951 3.2.7: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
		const uint32_t pos = i < 3 ? 16 + i : i == 3 ? 0 : (i & 1u) ? 8 - ((i - 3) >> 1) : 8 + ((i - 4) >> 1);
		if (io.lane() == 0) t.lens[pos] = (uint8_t)v;
	}
	if (io.overrun()) return VG_INF_EINPUT;
	io.sync();
	int rc = vg_inf_build(io, t.lens, 19, t.dist_fast, 7, t.dist_cnt, t.dist_sym, false);
	if (rc) return rc;
	const uint32_t n = hlit + hdist;
	uint32_t i = 0, last = 0;
	while (i < n) {                                                   // every iteration consumes at least one input bit (a code)
		io.need();
		const int s = vg_inf_decode(io, t.dist_fast, 7, t.dist_cnt, t.dist_sym);
		if (s < 0) return VG_INF_ESYMBOL;
		if (io.overrun()) return VG_INF_EINPUT;
		if (s < 16) {
			last = (uint32_t)s;
			if (io.lane() == 0) t.lens[i] = (uint8_t)s;
			i++;
			continue;
		}
		uint32_t rep, v = 0;
		if (s == 16) { if (i == 0) return VG_INF_ESYMBOL; v = last; rep = 3 + io.bits(2); }
		else if (s == 17) rep = 3 + io.bits(3);
		else rep = 11 + io.bits(7);
		if (io.overrun()) return VG_INF_EINPUT;
		if (i + rep > n) return VG_INF_ESYMBOL;
		for (uint32_t j = io.lane(); j < rep; j += io.lanes()) t.lens[i + j] = (uint8_t)v;
		i += rep;
		last = v;
	}
	io.sync();
	*n_lit = hlit; *n_dist = hdist;
	return VG_INF_OK;
}

// One BGZF block's payload -> [0, isize) of the IO's output.  See TERMINATION at the top.
template <class IO>
VG_HD int vg_inflate_raw(IO &io, VgInfTables &t, uint32_t isize)
{
	uint32_t o = 0;                                                   // bytes written; o <= isize throughout
	for (;;) {                                                        // one DEFLATE block per iteration: consumes at least its 3 header bits
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
			if (len > isize - o) return VG_INF_ESIZE;
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
					if (o >= isize) return VG_INF_ESIZE;
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
				if (dist > o) return VG_INF_EDIST;                    // BGZF blocks share no window
				if (len > isize - o) return VG_INF_ESIZE;
				io.copy(o, dist, len);
				o += len;
			}
		}
		if (hdr & 1u) break;
	}
	return o == isize ? VG_INF_OK : VG_INF_ESIZE;
}

// ---- CRC32 (the gzip polynomial, reflected), slicing by 4 ------------------------------------------------------------------------
constexpr uint32_t VG_CRC_POLY = 0xedb88320u;
struct VgCrcTab { uint32_t t[4][256]; };

// the table, built by the cooperating lanes (device: into LDS, once per block)
template <class IO>
VG_HD void vg_crc_tab_build(IO &io, VgCrcTab &tab)
{
	for (uint32_t i = io.lane(); i < 256; i += io.lanes()) {
		uint32_t c = i;
		for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ VG_CRC_POLY : c >> 1;
		tab.t[0][i] = c;
	}
	io.sync();
	for (uint32_t s = 1; s < 4; s++) {
		for (uint32_t i = io.lane(); i < 256; i += io.lanes()) { const uint32_t c = tab.t[s - 1][i]; tab.t[s][i] = (c >> 8) ^ tab.t[0][c & 0xffu]; }
		io.sync();
	}
}

// CRC32 of [p, p + n) continued from `crc` (0 to start): what zlib's crc32() returns
VG_HD uint32_t vg_crc32(const VgCrcTab &tab, uint32_t crc, const uint8_t *p, size_t n)
{
	crc = ~crc;
	while (n && ((uintptr_t)p & 3u)) { crc = (crc >> 8) ^ tab.t[0][(crc ^ *p++) & 0xffu]; n--; }
	for (; n >= 4; n -= 4, p += 4) {
		uint32_t w;
		__builtin_memcpy(&w, __builtin_assume_aligned(p, 4), 4);
		crc ^= w;
		crc = tab.t[3][crc & 0xffu] ^ tab.t[2][(crc >> 8) & 0xffu] ^ tab.t[1][(crc >> 16) & 0xffu] ^ tab.t[0][crc >> 24];
	}
	while (n--) crc = (crc >> 8) ^ tab.t[0][(crc ^ *p++) & 0xffu];
	return ~crc;
}

// a(x) * b(x) mod P, and x^(8 n) mod P: CRC32(A || B) = CRC32(A) * x^(8 |B|) + CRC32(B)
VG_HD uint32_t vg_crc_mul(uint32_t a, uint32_t b)
{
	uint32_t p = 0;
	for (uint32_t m = 1u << 31; m; m >>= 1) {                         // 32 steps
		if (a & m) p ^= b;
		b = (b & 1u) ? (b >> 1) ^ VG_CRC_POLY : b >> 1;
	}
	return p;
}
VG_HD uint32_t vg_crc_x8n(uint32_t nbytes)
{
	uint32_t sq = 1u << 30;                                           // x^1
	for (int k = 0; k < 3; k++) sq = vg_crc_mul(sq, sq);              // x^8
	uint32_t r = 1u << 31;                                            // x^0
	for (; nbytes; nbytes >>= 1) {                                    // 32 steps at most
		if (nbytes & 1u) r = vg_crc_mul(sq, r);
		sq = vg_crc_mul(sq, sq);
	}
	return r;
}
// Lane `lane` of `lanes`: its share of CRC32([p, p + n)) -- the XOR over all lanes is the CRC.  Slices are multiples of 4 bytes.
VG_HD uint32_t vg_crc32_share(const VgCrcTab &tab, const uint8_t *p, uint32_t n, uint32_t lane, uint32_t lanes)
{
	const uint32_t slice = ((n + lanes - 1) / lanes + 3u) & ~3u;
	const uint32_t lo = lane * slice < n ? lane * slice : n, hi = lo + slice < n ? lo + slice : n;
	if (hi == lo) return 0;
	return vg_crc_mul(vg_crc_x8n(n - hi), vg_crc32(tab, 0, p + lo, hi - lo));
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
struct VgHostLanes {
	static uint32_t lane() { return 0; }
	static uint32_t lanes() { return 1; }
	static void sync() {}
};
inline const VgCrcTab &vg_crc_tab_host()
{
	static const VgCrcTab tab = [] { VgCrcTab t; VgHostLanes l; vg_crc_tab_build(l, t); return t; }();
	return tab;
}

// the host's IO policy: plain memory, one lane.  Reads in[0, len) and writes out[0, isize), nothing else.
struct VgHostIO : VgHostLanes {
	const uint8_t *in; uint32_t len, pos = 0;
	uint8_t *out;
	uint64_t bitbuf = 0; uint32_t bitcnt = 0;
	int64_t bits_left;                                                // input bits not yet consumed; negative: the decoder ran past the end
	VgHostIO(const uint8_t *in_, uint32_t len_, uint8_t *out_) : in(in_), len(len_), out(out_), bits_left((int64_t)len_ * 8) {}
	static uint32_t u(uint32_t x) { return x; }
	void need() { while (bitcnt <= 56) { bitbuf |= (uint64_t)(pos < len ? in[pos] : 0) << bitcnt; pos++; bitcnt += 8; } }   // (8 steps at most)
	uint32_t peek() const { return (uint32_t)bitbuf; }
	void drop(uint32_t n) { bitbuf >>= n; bitcnt -= n; bits_left -= n; }
	uint32_t bits(uint32_t n) { const uint32_t v = (uint32_t)bitbuf & ((1u << n) - 1u); drop(n); return v; }
	void align_byte() { drop(bitcnt & 7u); }
	bool overrun() const { return bits_left < 0; }
	void put(uint32_t o, uint8_t b) { out[o] = b; }
	void copy(uint32_t o, uint32_t dist, uint32_t n) { for (uint32_t j = 0; j < n; j++) out[o + j] = out[o + j - dist]; }     // n output bytes
	bool stored_copy(uint32_t o, uint32_t n)
	{
		const uint32_t at = len - (uint32_t)(bits_left >> 3);         // byte-aligned here, and not past the end (the caller checked)
		if (n > len - at) return false;
		if (n) memcpy(out + o, in + at, n);
		pos = at + n; bitbuf = 0; bitcnt = 0; bits_left -= (int64_t)n * 8;
		return true;
	}
};

// one block on the host: payload -> out[0, isize), then the CRC
inline int vg_inflate_block_host(const uint8_t *in, uint32_t len, uint8_t *out, uint32_t isize, uint32_t crc)
{
	if (isize > VG_BGZF_MAX_ISIZE) return VG_INF_ESIZE;
	VgInfTables t;
	VgHostIO io(in, len, out);
	const int rc = vg_inflate_raw(io, t, isize);
	if (rc) return rc;
	return vg_crc32(vg_crc_tab_host(), 0, out, isize) == crc ? VG_INF_OK : VG_INF_ECRC;
}

// The header of the block at p, of which `avail` bytes are there.  0: a whole block, *b filled (offsets relative to p);
// 1: more bytes are needed; VG_INF_EHEADER: this is no BGZF block.
inline int vg_bgzf_header(const uint8_t *p, uint64_t avail, vg_bgzf_block *b)
{
	static const uint8_t magic[4] = {0x1f, 0x8b, 0x08, 0x04};
	for (uint64_t i = 0; i < 4 && i < avail; i++) if (p[i] != magic[i]) return VG_INF_EHEADER;
	if (avail < 12) return 1;
	const uint32_t xlen = p[10] | (uint32_t)p[11] << 8;
	if (avail < 12u + xlen) return 1;
	uint32_t at = 0, bsize = 0;
	bool found = false;
	while (at + 4 <= xlen) {                                          // the subfield list: each step moves at least 4 bytes on
		const uint8_t *s = p + 12 + at;
		const uint32_t slen = s[2] | (uint32_t)s[3] << 8;
		if (at + 4 + slen > xlen) return VG_INF_EHEADER;
		if (!found && s[0] == 'B' && s[1] == 'C' && slen == 2) { bsize = s[4] | (uint32_t)s[5] << 8; found = true; }
		at += 4 + slen;
	}
	if (at != xlen || !found) return VG_INF_EHEADER;
	const uint32_t total = bsize + 1, hdr = 12 + xlen;
	if (total < hdr + 8) return VG_INF_EHEADER;
	if (avail < total) return 1;
	const uint8_t *tr = p + total - 8;
	b->in_off = hdr; b->in_len = total - hdr - 8;
	b->crc = tr[0] | (uint32_t)tr[1] << 8 | (uint32_t)tr[2] << 16 | (uint32_t)tr[3] << 24;
	b->isize = tr[4] | (uint32_t)tr[5] << 8 | (uint32_t)tr[6] << 16 | (uint32_t)tr[7] << 24;
	if (b->isize > VG_BGZF_MAX_ISIZE) return VG_INF_EHEADER;
	return 0;
}

// gzip magic at all (a plain .gz is refused by name, not framed as text)
inline bool vg_is_gzip(const uint8_t *p, uint64_t avail) { return avail >= 3 && p[0] == 0x1f && p[1] == 0x8b && p[2] == 0x08; }

// The header walk over [p, p + n), bytes cut anywhere: every whole block is appended to `out` (comp_off / text_off continue from
// the given bases, in_off is relative to p); *tail = trailing bytes that belong to an incomplete block.  0, or VG_INF_EHEADER with
// *bad_off = compressed offset of the block that is none (the blocks before it are in `out`).  A block's total size is at least
// 20 bytes, so the walk takes at most n / 20 steps.
inline int vg_bgzf_scan(const uint8_t *p, uint64_t n, uint64_t comp_base, uint64_t text_base, std::vector<vg_bgzf_block> &out, uint64_t *tail, uint64_t *bad_off)
{
	uint64_t at = 0, text = text_base;
	*tail = 0;
	while (at < n) {
		vg_bgzf_block b;
		const int rc = vg_bgzf_header(p + at, n - at, &b);
		if (rc == 1) { *tail = n - at; break; }
		if (rc) { *bad_off = comp_base + at; return rc; }
		const uint64_t total = (uint64_t)b.in_off + b.in_len + 8;
		b.comp_off = comp_base + at; b.text_off = text;
		b.in_off += (uint32_t)at;
		out.push_back(b);
		text += b.isize;
		at += total;
	}
	return 0;
}

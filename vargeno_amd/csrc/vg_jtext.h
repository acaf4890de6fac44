// vg_jtext.h -- the data lines of the joint (multi-sample) VCF, stated once for the host loop and the device kernels.
//
// Input: the calls of n_samples samples, gt (0 not called, 1 hom-ref, 2 hom-alt, 3 het) and gq (any int32) per site, and a PLAN of
// the lines: one vg_jtext_record per data line of the SNP list that names a key of the call book (host/caller_vcf.cpp):
//   head_off, head_len   the line's first eight fields, bytes heads[head_off, head_off + head_len)
//   site_at, n_sites     sites[site_at, site_at + n_sites): the site indices of the record's key in genome order (they need not be
//                        consecutive: two chromosomes with one name share a key space)
//   * CELL of a sample with call (gt, gq), gt 1 / 2 / 3:  "\t" + "0/0" / "1/1" / "0/1" + ":" + gq as "%d" prints an int32 -- 6 to 16
//     bytes ("\t0/1:-2147483648"); the cell of a sample without a call is "\t./.:." ;
//   * LINE of a record: every sample shows the call of the LAST site of the run at which its gt != 0, or the missing cell.  If no
//     sample has a called site the record produces NO bytes; otherwise
//         heads[head_off, +head_len)  "\tGT:GQ"  the cells in sample order  "\n"
//   * BOUND of a span of records: the sum of head_len + n_records * (7 + 16 * n_samples).
// The INFO mode VG_JT_INFO_COUNTS (opt-in; VG_JT_INFO_NONE writes the bytes above) adds the record's allele counts to the head's INFO:
//   * COUNTS of a record that produces a line, over the calls its line SHOWS (one per sample, see LINE): NS = samples whose shown call
//     has gt != 0, het = shown calls with gt 3, hom = with gt 2; AN = 2 NS, AC = het + 2 hom, AF = AC / AN rounded half up to six
//     decimals and stripped of trailing zeros and of a bare point ("0", "1", "0.5", "0.333333") -- in integers alone:
//     q = (2 000 000 AC + AN) / (2 AN) in 64 bits, 1 000 000 prints "1", 0 prints "0", the rest "0." + six digits, stripped.
//   * TAG: "NS=<NS>;AN=<AN>;AC=<AC>;AF=<AF>", at most 38 bytes at 16 384 samples.
//   * SPLICE, a function of the head's bytes alone: a head with exactly seven tabs has eight fields and its INFO follows the seventh
//     tab.  INFO "." : that byte is replaced by the tag; INFO empty (the head ends in a tab): the tag is appended; otherwise ";" and
//     the tag are appended.  A head with another number of tabs is written as it is.  "\tGT:GQ", the cells and "\n" follow as above.
//   * the BOUND grows by VG_JT_INFO_MAX = 40 bytes per record.
// The kernels of vargeno_hip.hip compile vg_jt_cell, vg_jt_pick, vg_jt_splice and vg_jt_tag; the host loop below is the same rule on
// threads.
#pragma once
#include <stdint.h>
#include <string.h>

#include <thread>
#include <vector>

#if defined(__HIPCC__)
#define VG_JT_HD __host__ __device__
#else
#define VG_JT_HD
#endif

#ifndef VG_JTEXT_RECORD_DEFINED
#define VG_JTEXT_RECORD_DEFINED
typedef struct vg_jtext_record {
	uint64_t head_off;     /* the first eight fields: heads[head_off, head_off + head_len) */
	uint64_t site_at;      /* the key's sites: sites[site_at, site_at + n_sites) */
	uint32_t head_len;
	uint32_t n_sites;
} vg_jtext_record;
#endif

constexpr uint32_t VG_JT_CELL_MAX = 16, VG_JT_LINE_FIXED = 7;        // "\tGT:GQ" and "\n"
constexpr uint32_t VG_JT_GQ_ESCAPE = 16383;                         // the 14-bit gq field of a narrow word that says: look in the wide column

// A cell as 16 bytes in two little-endian words (byte i of the cell is byte i of lo, then of hi): no array a kernel would have to
// index dynamically.
struct vg_jt_cell_t { uint64_t lo, hi; uint32_t len; };
VG_JT_HD inline void vg_jt_put(vg_jt_cell_t &c, uint32_t at, uint32_t byte)
{
	if (at < 8) c.lo |= (uint64_t)byte << (8 * at);
	else c.hi |= (uint64_t)byte << (8 * (at - 8));
}
VG_JT_HD inline uint32_t vg_jt_byte(const vg_jt_cell_t &c, uint32_t at) { return (uint32_t)((at < 8 ? c.lo >> (8 * at) : c.hi >> (8 * (at - 8))) & 0xffu); }

VG_JT_HD inline vg_jt_cell_t vg_jt_cell(uint32_t gt, int32_t gq)
{
	vg_jt_cell_t c;
	if (gt == 0 || gt > 3) {                                         // "\t./.:."
		c.lo = 0x2e3a2e2f2e09ull; c.hi = 0; c.len = 6;
		return c;
	}
	// "\t" a "/" b ":"   0/0 hom-ref, 1/1 hom-alt, 0/1 het
	const uint64_t a = gt == 2 ? '1' : '0', b = gt == 1 ? '0' : '1';
	c.lo = 0x09ull | a << 8 | (uint64_t)'/' << 16 | b << 24 | (uint64_t)':' << 32;
	c.hi = 0;
	uint32_t at = 5;
	uint32_t u = (uint32_t)gq;
	if (gq < 0) { vg_jt_put(c, at++, '-'); u = 0u - u; }             // (INT_MIN: 2147483648 as an unsigned number)
	uint32_t nd = 1;
	for (uint32_t v = u; v >= 10; v /= 10) nd++;
	for (uint32_t k = nd; k-- > 0;) { vg_jt_put(c, at + k, '0' + u % 10); u /= 10; }
	c.len = at + nd;
	return c;
}

// What a sample shows for a record: the call of the last site of the run at which call(site) has a gt -- call is a functor
// site index -> (gt << 32 | (uint32_t)gq) -- or 0 (gt 0) when there is none.
template <class Call>
VG_JT_HD inline uint64_t vg_jt_pick(const uint32_t *sites, uint32_t n, Call call)
{
	for (uint32_t q = n; q-- > 0;) {
		const uint64_t v = call(sites[q]);
		if (v >> 32) return v;
	}
	return 0;
}

VG_JT_HD inline uint64_t vg_jt_bound(uint64_t head_bytes, uint64_t n_records, uint32_t n_samples)
{
	return head_bytes + n_records * (VG_JT_LINE_FIXED + (uint64_t)VG_JT_CELL_MAX * n_samples);
}

// ---- the INFO mode ----
#ifndef VG_JT_INFO_NONE                                             /* (include/vargeno_hip.h has the same three) */
#define VG_JT_INFO_NONE   0
#define VG_JT_INFO_COUNTS 1
#define VG_JT_INFO_MAX    40                                        /* what a record's line may grow by: ";" + the tag's 38 bytes at most */
#endif
constexpr uint32_t VG_JT_SPLICE_NONE = 0, VG_JT_SPLICE_DOT = 1, VG_JT_SPLICE_EMPTY = 2, VG_JT_SPLICE_APPEND = 3;

// which shown calls count as what
VG_JT_HD inline bool vg_jt_is_called(uint32_t gt) { return gt != 0; }
VG_JT_HD inline bool vg_jt_is_het(uint32_t gt) { return gt == 3; }
VG_JT_HD inline bool vg_jt_is_hom(uint32_t gt) { return gt == 2; }

VG_JT_HD inline uint64_t vg_jt_bound_info(uint64_t head_bytes, uint64_t n_records, uint32_t n_samples, int info)
{
	return vg_jt_bound(head_bytes, n_records, n_samples) + (info == VG_JT_INFO_COUNTS ? n_records * VG_JT_INFO_MAX : 0);
}

// The splice kind of a head from its number of tabs and its last two bytes (prev: the byte in front of the last; either is
// ignored where the head is too short to have it)
VG_JT_HD inline uint32_t vg_jt_splice(uint64_t tabs, uint32_t head_len, uint32_t last, uint32_t prev)
{
	if (tabs != 7 || head_len == 0) return VG_JT_SPLICE_NONE;       // (seven tabs take seven bytes: head_len >= 7 from here on)
	if (last == '\t') return VG_JT_SPLICE_EMPTY;
	if (last == '.' && prev == '\t') return VG_JT_SPLICE_DOT;
	return VG_JT_SPLICE_APPEND;
}
// bytes of the head that stay, and whether a ';' follows them
VG_JT_HD inline uint32_t vg_jt_splice_keep(uint32_t kind, uint32_t head_len) { return head_len - (kind == VG_JT_SPLICE_DOT ? 1u : 0u); }
VG_JT_HD inline uint32_t vg_jt_splice_sep(uint32_t kind) { return kind == VG_JT_SPLICE_APPEND ? 1u : 0u; }

// The tag of a record with the counts (ns >= 1, het + hom <= ns <= 2^30): put(i, byte) receives byte i of it, in order; returns
// its length.  No floating point: the host and the device cannot differ.
template <class Put>
VG_JT_HD inline uint32_t vg_jt_tag(uint32_t ns, uint32_t het, uint32_t hom, Put put)
{
	uint32_t at = 0;
	auto number = [&](uint32_t c0, uint32_t c1, uint32_t v) {        // ";" c0 c1 "=" v, without the ";" in front of the first
		if (at) put(at++, (uint32_t)';');
		put(at++, c0); put(at++, c1); put(at++, (uint32_t)'=');
		uint32_t nd = 1;
		for (uint32_t w = v; w >= 10; w /= 10) nd++;
		for (uint32_t k = nd; k-- > 0;) { uint32_t w = v; for (uint32_t j = 0; j < k; j++) w /= 10; put(at++, '0' + w % 10); }
	};
	const uint32_t an = 2 * ns, ac = het + 2 * hom;
	number('N', 'S', ns);
	number('A', 'N', an);
	number('A', 'C', ac);
	put(at++, (uint32_t)';'); put(at++, (uint32_t)'A'); put(at++, (uint32_t)'F'); put(at++, (uint32_t)'=');
	const uint32_t q = (uint32_t)((2000000ull * ac + an) / (2ull * an));
	if (q == 0 || q >= 1000000) { put(at++, q ? (uint32_t)'1' : (uint32_t)'0'); return at; }
	put(at++, (uint32_t)'0'); put(at++, (uint32_t)'.');
	uint32_t nd = 6, v = q;
	while (v % 10 == 0) { v /= 10; nd--; }                          // (q != 0: a digit stays)
	for (uint32_t k = nd; k-- > 0;) { uint32_t w = v; for (uint32_t j = 0; j < k; j++) w /= 10; put(at++, '0' + w % 10); }
	return at;
}
VG_JT_HD inline uint32_t vg_jt_tag_len(uint32_t ns, uint32_t het, uint32_t hom) { return vg_jt_tag(ns, het, hom, [](uint32_t, uint32_t) {}); }
// the length of a line's head piece -- the head with its splice, and "\tGT:GQ"
VG_JT_HD inline uint32_t vg_jt_head_piece_len(uint32_t kind, uint32_t head_len, uint32_t ns, uint32_t het, uint32_t hom)
{
	if (kind == VG_JT_SPLICE_NONE) return head_len + 6;
	return vg_jt_splice_keep(kind, head_len) + vg_jt_splice_sep(kind) + vg_jt_tag_len(ns, het, hom) + 6;
}

// ---- the host loop (plain host functions; a device compiler only parses them) ----
struct vg_jt_counts_t { uint32_t ns, het, hom; };
inline uint32_t vg_jt_head_splice(const uint8_t *head, uint32_t head_len)
{
	uint64_t tabs = 0;
	for (uint32_t i = 0; i < head_len; i++) tabs += head[i] == '\t';
	return vg_jt_splice(tabs, head_len, head_len ? head[head_len - 1] : 0u, head_len > 1 ? head[head_len - 2] : 0u);
}
// what every sample shows for a record, counted (a record with ns == 0 produces no line)
inline vg_jt_counts_t vg_jt_counts_host(const uint8_t *const *gt, const int32_t *const *gq, uint32_t n_samples, const vg_jtext_record &r, const uint32_t *sites)
{
	vg_jt_counts_t c{0, 0, 0};
	for (uint32_t s = 0; s < n_samples; s++) {
		const uint8_t *g = gt[s];
		const int32_t *q = gq[s];
		const uint32_t shown = g ? (uint32_t)(vg_jt_pick(sites + r.site_at, r.n_sites, [&](uint32_t site) { return (uint64_t)g[site] << 32 | (uint32_t)q[site]; }) >> 32) : 0u;
		c.ns += vg_jt_is_called(shown); c.het += vg_jt_is_het(shown); c.hom += vg_jt_is_hom(shown);
	}
	return c;
}
// the head of a line with its splice and "\tGT:GQ" at out; returns the bytes written
inline uint32_t vg_jt_head_host(const uint8_t *head, uint32_t head_len, int info, const vg_jt_counts_t &c, uint8_t *out)
{
	const uint32_t kind = info == VG_JT_INFO_COUNTS ? vg_jt_head_splice(head, head_len) : VG_JT_SPLICE_NONE;
	uint32_t at = vg_jt_splice_keep(kind, head_len);
	memcpy(out, head, at);
	if (vg_jt_splice_sep(kind)) out[at++] = ';';
	if (kind != VG_JT_SPLICE_NONE) at += vg_jt_tag(c.ns, c.het, c.hom, [&](uint32_t i, uint32_t byte) { out[at + i] = (uint8_t)byte; });
	memcpy(out + at, "\tGT:GQ", 6);
	return at + 6;
}
// gt[s], gq[s]: sample s's columns (a null gt[s]: a sample never set, all missing).  One record -> at most its bound's bytes at
// out; returns the bytes written (0: the record is dropped).  The cells are written where the longest head piece would end and
// moved down behind the head piece once the counts say how long it is (mode 0: they are written in place).
inline uint64_t vg_jt_line_host_info(const uint8_t *const *gt, const int32_t *const *gq, uint32_t n_samples, const uint8_t *heads, const vg_jtext_record &r, const uint32_t *sites, int info, uint8_t *out)
{
	uint8_t *const cells = out + r.head_len + 6 + (info == VG_JT_INFO_COUNTS ? VG_JT_INFO_MAX : 0u);
	uint8_t *p = cells;
	vg_jt_counts_t n{0, 0, 0};
	for (uint32_t s = 0; s < n_samples; s++) {
		const uint8_t *g = gt[s];
		const int32_t *q = gq[s];
		const uint64_t v = g ? vg_jt_pick(sites + r.site_at, r.n_sites, [&](uint32_t site) { return (uint64_t)g[site] << 32 | (uint32_t)q[site]; }) : 0;
		const uint32_t shown = (uint32_t)(v >> 32);
		n.ns += vg_jt_is_called(shown); n.het += vg_jt_is_het(shown); n.hom += vg_jt_is_hom(shown);
		const vg_jt_cell_t c = vg_jt_cell(shown, (int32_t)(uint32_t)v);
		for (uint32_t i = 0; i < c.len; i++) p[i] = (uint8_t)vg_jt_byte(c, i);
		p += c.len;
	}
	if (!n.ns) return 0;
	*p++ = '\n';
	const uint32_t head = vg_jt_head_host(heads + r.head_off, r.head_len, info, n, out);
	if (out + head != cells) memmove(out + head, cells, (size_t)(p - cells));
	return head + (uint64_t)(p - cells);
}
inline uint64_t vg_jt_line_host(const uint8_t *const *gt, const int32_t *const *gq, uint32_t n_samples, const uint8_t *heads, const vg_jtext_record &r, const uint32_t *sites, uint8_t *out)
{
	return vg_jt_line_host_info(gt, gq, n_samples, heads, r, sites, VG_JT_INFO_NONE, out);
}

// the bound of a span of records
inline uint64_t vg_jt_span_bound_info(const vg_jtext_record *recs, uint64_t n_records, uint32_t n_samples, int info)
{
	uint64_t heads_sum = 0;
	for (uint64_t i = 0; i < n_records; i++) heads_sum += recs[i].head_len;
	return vg_jt_bound_info(heads_sum, n_records, n_samples, info);
}
inline uint64_t vg_jt_span_bound(const vg_jtext_record *recs, uint64_t n_records, uint32_t n_samples) { return vg_jt_span_bound_info(recs, n_records, n_samples, VG_JT_INFO_NONE); }

// A span of records on `threads` threads -> text[0, *len); *n_lines = records that produced a line.  false, and nothing is
// written: cap is below the span's bound.  Every thread renders a slice of the records at the slice's bound offset; the slices
// are then moved down.  Throws what std::vector and std::thread throw.
inline bool vg_jtext_host_run_info(const uint8_t *const *gt, const int32_t *const *gq, uint32_t n_samples, const uint8_t *heads, const vg_jtext_record *recs, uint64_t n_records,
                                   const uint32_t *sites, int info, int threads, uint8_t *text, uint64_t cap, uint64_t *len, uint64_t *n_lines)
{
	if (cap < vg_jt_span_bound_info(recs, n_records, n_samples, info)) return false;
	const uint64_t T = (uint64_t)(threads < 1 ? 1 : threads) < n_records ? (uint64_t)(threads < 1 ? 1 : threads) : (n_records ? n_records : 1);
	std::vector<uint64_t> at(T + 1, 0), got(T, 0), lines(T, 0);
	for (uint64_t t = 0; t < T; t++) {
		uint64_t heads_sum = 0;
		for (uint64_t i = n_records * t / T; i < n_records * (t + 1) / T; i++) heads_sum += recs[i].head_len;
		at[t + 1] = at[t] + vg_jt_bound_info(heads_sum, n_records * (t + 1) / T - n_records * t / T, n_samples, info);
	}
	auto work = [&](uint64_t t) {
		uint8_t *p = text + at[t];
		for (uint64_t i = n_records * t / T; i < n_records * (t + 1) / T; i++) {
			const uint64_t n = vg_jt_line_host_info(gt, gq, n_samples, heads, recs[i], sites, info, p);
			p += n;
			lines[t] += n != 0;
		}
		got[t] = (uint64_t)(p - (text + at[t]));
	};
	std::vector<std::thread> th;
	for (uint64_t t = 1; t < T; t++) th.emplace_back(work, t);
	work(0);
	for (auto &x : th) x.join();
	uint64_t total = 0, nl = 0;
	for (uint64_t t = 0; t < T; t++) {
		if (t && got[t]) memmove(text + total, text + at[t], (size_t)got[t]);
		total += got[t];
		nl += lines[t];
	}
	*len = total;
	*n_lines = nl;
	return true;
}
inline bool vg_jtext_host_run(const uint8_t *const *gt, const int32_t *const *gq, uint32_t n_samples, const uint8_t *heads, const vg_jtext_record *recs, uint64_t n_records,
                              const uint32_t *sites, int threads, uint8_t *text, uint64_t cap, uint64_t *len, uint64_t *n_lines)
{
	return vg_jtext_host_run_info(gt, gq, n_samples, heads, recs, n_records, sites, VG_JT_INFO_NONE, threads, text, cap, len, n_lines);
}

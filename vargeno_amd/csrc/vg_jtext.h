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
// The kernels of vargeno_hip.hip compile vg_jt_cell and vg_jt_pick; the host loop below is the same rule on threads.
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

// ---- the host loop (plain host functions; a device compiler only parses them) ----
// gt[s], gq[s]: sample s's columns (a null gt[s]: a sample never set, all missing).  One record -> at most its bound's bytes at
// out; returns the bytes written (0: the record is dropped).
inline uint64_t vg_jt_line_host(const uint8_t *const *gt, const int32_t *const *gq, uint32_t n_samples, const uint8_t *heads, const vg_jtext_record &r, const uint32_t *sites, uint8_t *out)
{
	uint8_t *p = out + r.head_len + 6;
	bool any = false;
	for (uint32_t s = 0; s < n_samples; s++) {
		const uint8_t *g = gt[s];
		const int32_t *q = gq[s];
		const uint64_t v = g ? vg_jt_pick(sites + r.site_at, r.n_sites, [&](uint32_t site) { return (uint64_t)g[site] << 32 | (uint32_t)q[site]; }) : 0;
		any = any || (v >> 32) != 0;
		const vg_jt_cell_t c = vg_jt_cell((uint32_t)(v >> 32), (int32_t)(uint32_t)v);
		for (uint32_t i = 0; i < c.len; i++) p[i] = (uint8_t)vg_jt_byte(c, i);
		p += c.len;
	}
	if (!any) return 0;
	memcpy(out, heads + r.head_off, r.head_len);
	memcpy(out + r.head_len, "\tGT:GQ", 6);
	*p++ = '\n';
	return (uint64_t)(p - out);
}

// the bound of a span of records
inline uint64_t vg_jt_span_bound(const vg_jtext_record *recs, uint64_t n_records, uint32_t n_samples)
{
	uint64_t heads_sum = 0;
	for (uint64_t i = 0; i < n_records; i++) heads_sum += recs[i].head_len;
	return vg_jt_bound(heads_sum, n_records, n_samples);
}

// A span of records on `threads` threads -> text[0, *len); *n_lines = records that produced a line.  false, and nothing is
// written: cap is below the span's bound.  Every thread renders a slice of the records at the slice's bound offset; the slices
// are then moved down.  Throws what std::vector and std::thread throw.
inline bool vg_jtext_host_run(const uint8_t *const *gt, const int32_t *const *gq, uint32_t n_samples, const uint8_t *heads, const vg_jtext_record *recs, uint64_t n_records,
                              const uint32_t *sites, int threads, uint8_t *text, uint64_t cap, uint64_t *len, uint64_t *n_lines)
{
	if (cap < vg_jt_span_bound(recs, n_records, n_samples)) return false;
	const uint64_t T = (uint64_t)(threads < 1 ? 1 : threads) < n_records ? (uint64_t)(threads < 1 ? 1 : threads) : (n_records ? n_records : 1);
	std::vector<uint64_t> at(T + 1, 0), got(T, 0), lines(T, 0);
	for (uint64_t t = 0; t < T; t++) {
		uint64_t heads_sum = 0;
		for (uint64_t i = n_records * t / T; i < n_records * (t + 1) / T; i++) heads_sum += recs[i].head_len;
		at[t + 1] = at[t] + vg_jt_bound(heads_sum, n_records * (t + 1) / T - n_records * t / T, n_samples);
	}
	auto work = [&](uint64_t t) {
		uint8_t *p = text + at[t];
		for (uint64_t i = n_records * t / T; i < n_records * (t + 1) / T; i++) {
			const uint64_t n = vg_jt_line_host(gt, gq, n_samples, heads, recs[i], sites, p);
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

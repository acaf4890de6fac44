// vg_vcfidx.h -- the tabix index (.tbi) of a BGZF VCF, stated once for the host scanner, the scan kernels and a stand-alone test.
//
// The text is cut at '\n' (a last line without one is a line).  A line that is empty or starts with '#' is SKIPPED wherever it
// stands; every other line is a DATA line  CHROM \t POS \t ID \t REF [\t ...]:
//   beg = POS - 1, end = beg + len(REF)      POS: one or more ASCII digits, POS >= 1; len(REF) >= 1; end <= 2^29.  INFO/END is not read.
//   tid = rank of the CHROM string by first appearance; within a tid beg never decreases; a CHROM never comes back after another.
// A data line that breaks a rule REFUSES the index (vg_vi_rule names the rule; the line's text offset goes with it); the refusal is
// sticky and concerns the index alone.  The rules of one line are tried in the order of the VG_VI_* numbers below.
//   bin      reg2bin(beg, end) of the 5-level, 14-bit scheme;  CHUNK: a maximal run of consecutive data lines of one tid and one bin
//            (skipped lines do not break it), [vo(start of the first line), vo(end of the last: behind its '\n', or the end of text)]
//   vo(u)    cstart[u / block] << 16 | u % block, cstart[k] the file offset of block k (k = number of blocks: of the marker)
//   linear   n_intv = ((max end - 1) >> 14) + 1; ioff[w] = vo(start) of the first line in file order with beg >> 14 <= w <= (end - 1) >> 14;
//            a window without a line takes the next higher window's value
//   per tid  the bins ascending, chunks in file order, then pseudo-bin 37450: (vo(first start), vo(last end)), (data lines, 0).
// Small bins are not merged into their parents (htslib does; both are valid).
//
// Three layers, none with a HIP type: vg_vi_parse (one line; also compiled into the parse kernel), vg_vi_scan_lines (whole lines ->
// RECORDS: a run of joining lines is one record -- what the kernels produce too), VgVcfIdx (the streaming handle: carry of a cut
// line, replay of records with the sequential algorithm, BGZF block offsets, the serialiser).
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <map>
#include <string>
#include <thread>
#include <vector>

#if defined(__HIPCC__)
#define VG_VI_HD __host__ __device__
#else
#define VG_VI_HD
#endif

enum {
	VG_VI_SKIP = 0, VG_VI_DATA = 1,
	VG_VI_FEW_FIELDS = 2, VG_VI_POS_NOT_NUMBER = 3, VG_VI_POS_ZERO = 4, VG_VI_REF_EMPTY = 5, VG_VI_END_BEYOND = 6,      // one line's rules, in this order
	VG_VI_UNSORTED = 7, VG_VI_NOT_CONTIGUOUS = 8                                                                         // the order of lines
};
inline const char *vg_vi_rule(uint32_t kind)
{
	switch (kind) {
	case VG_VI_FEW_FIELDS: return "fewer than four fields";
	case VG_VI_POS_NOT_NUMBER: return "POS is not a number";
	case VG_VI_POS_ZERO: return "POS is 0";
	case VG_VI_REF_EMPTY: return "REF is empty";
	case VG_VI_END_BEYOND: return "the end lies beyond 2^29";
	case VG_VI_UNSORTED: return "unsorted positions";
	case VG_VI_NOT_CONTIGUOUS: return "chromosome blocks not continuous";
	default: return nullptr;
	}
}
constexpr uint32_t VG_VI_MAX_END = 1u << 29, VG_VI_PSEUDO_BIN = 37450;

struct vg_vi_line { uint32_t kind, clen, beg, end; };                  // one line: VG_VI_*, bytes of CHROM, [beg, end) of a data line

// the line p[0, n), its '\n' not included
VG_VI_HD inline vg_vi_line vg_vi_parse(const uint8_t *p, uint64_t n)
{
	vg_vi_line r = {VG_VI_SKIP, 0, 0, 0};
	if (n == 0 || p[0] == '#') return r;
	uint64_t i = 0;
	while (i < n && p[i] != '\t') i++;
	r.clen = (uint32_t)(i < 0xffffffffull ? i : 0xffffffffull);
	r.kind = VG_VI_FEW_FIELDS;
	if (i >= n) return r;
	const uint64_t pos_at = ++i;
	uint64_t pos = 0;
	bool digits = true;
	for (; i < n && p[i] != '\t'; i++) {
		const uint32_t c = p[i];
		if (c < '0' || c > '9') digits = false;
		else if (pos < (1ull << 40)) pos = pos * 10 + (c - '0');       // (saturates far above 2^29)
	}
	const uint64_t pos_end = i;
	if (i >= n) return r;
	for (++i; i < n && p[i] != '\t'; i++) {}                           // ID
	if (i >= n) return r;
	const uint64_t ref_at = ++i;
	while (i < n && p[i] != '\t') i++;
	const uint64_t ref_len = i - ref_at;
	if (!digits || pos_end == pos_at) { r.kind = VG_VI_POS_NOT_NUMBER; return r; }
	if (pos == 0) { r.kind = VG_VI_POS_ZERO; return r; }
	if (ref_len == 0) { r.kind = VG_VI_REF_EMPTY; return r; }
	if (pos - 1 + ref_len > VG_VI_MAX_END) { r.kind = VG_VI_END_BEYOND; return r; }
	r.kind = VG_VI_DATA; r.beg = (uint32_t)(pos - 1); r.end = (uint32_t)(pos - 1 + ref_len);
	return r;
}

VG_VI_HD inline uint32_t vg_vi_reg2bin(uint32_t beg, uint32_t end)
{
	--end;
	if (beg >> 14 == end >> 14) return 4681 + (beg >> 14);
	if (beg >> 17 == end >> 17) return 585 + (beg >> 17);
	if (beg >> 20 == end >> 20) return 73 + (beg >> 20);
	if (beg >> 23 == end >> 23) return 9 + (beg >> 23);
	if (beg >> 26 == end >> 26) return 1 + (beg >> 26);
	return 0;
}

// does data line `cur` join the record its predecessor `prev` (the line right before it) belongs to?  Both lie in one 16 kb
// window, on the same chromosome, in order: the record then needs no more than its first line's facts and its last line's beg.
VG_VI_HD inline bool vg_vi_joins(const vg_vi_line &prev, const vg_vi_line &cur, bool same_chrom)
{
	return prev.kind == VG_VI_DATA && cur.kind == VG_VI_DATA && same_chrom && prev.beg >> 14 == (prev.end - 1) >> 14 && cur.beg >> 14 == (cur.end - 1) >> 14
	       && prev.beg >> 14 == cur.beg >> 14 && cur.beg >= prev.beg;
}

// What crosses the link, and what the host scanner makes too: a run of joining data lines (or one data line, or one line that
// breaks a rule).  start / end: text offsets of the first line's first byte and of the byte behind the last line.
struct vg_vi_rec {
	uint64_t start, end;
	uint32_t first_line, last_line;        // line numbers within the scanned piece (their difference + 1 = the data lines)
	uint32_t beg_first, end_first;         // the first line's [beg, end)
	uint32_t beg_last;                     // the last line's beg
	uint32_t clen;                         // bytes of CHROM at `start`
	uint32_t kind;                         // VG_VI_DATA, or the rule the one line breaks
	uint32_t same;                         // 1: CHROM equals that of the data line right before `start` (no name needs to be read)
};

// whole lines text[0, n) (a last line without '\n' ends with the text) at text offset `base`
inline void vg_vi_scan_lines(const uint8_t *text, uint64_t n, uint64_t base, std::vector<vg_vi_rec> &out)
{
	vg_vi_line prev = {VG_VI_SKIP, 0, 0, 0};
	const uint8_t *prev_name = nullptr;
	bool open = false;
	uint32_t line = 0;
	for (uint64_t a = 0; a < n; line++) {
		const uint8_t *q = (const uint8_t *)memchr(text + a, '\n', (size_t)(n - a));
		const uint64_t e = q ? (uint64_t)(q - text) : n, next = q ? e + 1 : n;
		const vg_vi_line cur = vg_vi_parse(text + a, e - a);
		if (cur.kind == VG_VI_SKIP) open = false;
		else {
			const bool same = prev.kind == VG_VI_DATA && cur.kind == VG_VI_DATA && prev.clen == cur.clen && memcmp(prev_name, text + a, cur.clen) == 0;
			if (open && vg_vi_joins(prev, cur, same)) { vg_vi_rec &r = out.back(); r.end = base + next; r.last_line = line; r.beg_last = cur.beg; }
			else {
				out.push_back(vg_vi_rec{base + a, base + next, line, line, cur.beg, cur.end, cur.beg, cur.clen, cur.kind, same ? 1u : 0u});
				open = cur.kind == VG_VI_DATA;
			}
		}
		prev = cur; prev_name = text + a;
		a = next;
	}
}

struct VgVcfIdx {
	struct Tid {
		std::string name;
		std::map<uint32_t, std::vector<std::pair<uint64_t, uint64_t>>> bins;      // chunks as text offsets
		std::vector<uint64_t> ioff;                                               // text offsets, ~0: no line yet
		uint64_t first = 0, last = 0, lines = 0;
		uint32_t last_beg = 0, open_bin = ~0u;
	};
	uint32_t B = 65280;
	std::vector<Tid> tids;
	std::map<std::string, uint32_t> by_name;
	std::string carry;                     // the bytes of a line whose '\n' has not come yet
	uint64_t carry_at = 0, fed = 0;        // its text offset; text bytes fed
	bool ended = false;
	uint32_t err = 0;                      // the rule that refused the index (0: none), and the line's offset
	uint64_t err_at = 0;
	std::vector<uint64_t> cstart;          // file offsets of the text blocks
	uint64_t file_at = 0, text_end = 0;    // bytes of BGZF fed; the file offset behind the last text block (where the marker stands)
	uint64_t n_lines = 0, n_chunks = 0, n_bins = 0;
	double seconds = 0;                    // spent scanning (for the caller's report)

	void refuse(uint32_t rule, uint64_t at) { if (!err) { err = rule; err_at = at; } }

	// one record, in file order; name: the CHROM bytes at r.start (may be null when r.same)
	void replay(const vg_vi_rec &r, const uint8_t *name)
	{
		if (err) return;
		if (r.kind != VG_VI_DATA) { refuse(r.kind, r.start); return; }
		if (!(r.same && !tids.empty())) {
			Tid *cur = tids.empty() ? nullptr : &tids.back();
			if (!cur || cur->name.size() != r.clen || memcmp(cur->name.data(), name, r.clen) != 0) {
				std::string nm((const char *)name, r.clen);
				if (by_name.count(nm)) { refuse(VG_VI_NOT_CONTIGUOUS, r.start); return; }
				by_name.emplace(nm, (uint32_t)tids.size());
				tids.emplace_back();
				tids.back().name = std::move(nm);
				tids.back().first = r.start;
			}
		}
		Tid &t = tids.back();
		if (t.lines && r.beg_first < t.last_beg) { refuse(VG_VI_UNSORTED, r.start); return; }
		const uint32_t bin = vg_vi_reg2bin(r.beg_first, r.end_first);
		if (t.open_bin == bin) t.bins[bin].back().second = r.end;
		else { auto &v = t.bins[bin]; if (v.empty()) n_bins++; v.emplace_back(r.start, r.end); n_chunks++; t.open_bin = bin; }
		const uint32_t w0 = r.beg_first >> 14, w1 = (r.end_first - 1) >> 14;
		if (t.ioff.size() <= w1) t.ioff.resize((size_t)w1 + 1, ~0ull);
		for (uint32_t w = w0; w <= w1; w++) if (t.ioff[w] == ~0ull) t.ioff[w] = r.start;
		const uint64_t k = (uint64_t)(r.last_line - r.first_line) + 1;
		t.lines += k; n_lines += k;
		t.last_beg = r.beg_last; t.last = r.end;
	}

	// The next n text bytes, cut anywhere.  `scan` makes the records of whole lines text[off, off + len) (text offset fed + off) and
	// returns 0, or fails before anything of the handle has changed; names are read from `text`.
	typedef std::function<int(uint64_t off, uint64_t len, std::vector<vg_vi_rec> &out)> Scan;
	int feed(const uint8_t *text, uint64_t n, const Scan &scan)
	{
		if (err || ended || n == 0) { fed += n; return 0; }
		uint64_t at = 0;
		const uint8_t *first_nl = nullptr;
		if (!carry.empty()) {
			first_nl = (const uint8_t *)memchr(text, '\n', (size_t)n);
			if (!first_nl) { carry.append((const char *)text, (size_t)n); fed += n; return 0; }
			at = (uint64_t)(first_nl - text) + 1;
		}
		uint64_t whole = n;                                            // text[at, whole): whole lines
		while (whole > at && text[whole - 1] != '\n') whole--;
		std::vector<vg_vi_rec> recs;
		if (whole > at) { const int rc = scan(at, whole - at, recs); if (rc) return rc; }
		if (first_nl) {
			carry.append((const char *)text, (size_t)(at - 1));
			line_of_carry(fed + at);
		}
		for (const vg_vi_rec &r : recs) replay(r, text + (r.start - fed));
		if (whole < n) { carry.assign((const char *)text + whole, (size_t)(n - whole)); carry_at = fed + whole; }
		fed += n;
		return 0;
	}
	void line_of_carry(uint64_t end)
	{
		const vg_vi_line l = vg_vi_parse((const uint8_t *)carry.data(), carry.size());
		if (l.kind != VG_VI_SKIP) replay(vg_vi_rec{carry_at, end, 0, 0, l.beg, l.end, l.beg, l.clen, l.kind, 0}, (const uint8_t *)carry.data());
		carry.clear();
	}
	int feed_host(const uint8_t *text, uint64_t n, int threads)
	{
		return feed(text, n, [&](uint64_t off, uint64_t len, std::vector<vg_vi_rec> &out) {
			const uint64_t per = 1 << 16;                              // a thread is worth starting for 64 KiB of lines
			const int nt = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(1, std::min(threads, 256)), len / per));
			if (nt == 1) { vg_vi_scan_lines(text + off, len, fed + off, out); return 0; }
			// segments that end behind a '\n', one per thread; their records in order
			std::vector<uint64_t> cut((size_t)nt + 1, off + len);
			cut[0] = off;
			for (int t = 1; t < nt; t++) {
				uint64_t c = std::max(cut[(size_t)t - 1], off + len / (uint64_t)nt * (uint64_t)t);
				const uint8_t *q = c < off + len ? (const uint8_t *)memchr(text + c, '\n', (size_t)(off + len - c)) : nullptr;
				cut[(size_t)t] = q ? (uint64_t)(q - text) + 1 : off + len;
			}
			std::vector<std::vector<vg_vi_rec>> part((size_t)nt);
			std::vector<std::thread> th;
			for (int t = 0; t < nt; t++) th.emplace_back([&, t] { vg_vi_scan_lines(text + cut[(size_t)t], cut[(size_t)t + 1] - cut[(size_t)t], fed + cut[(size_t)t], part[(size_t)t]); });
			for (auto &x : th) x.join();
			for (auto &p : part) out.insert(out.end(), p.begin(), p.end());
			return 0;
		});
	}
	// whole lines that are not in host memory (the caller made `recs` from them, `name_of` fetches a record's CHROM bytes)
	bool feed_records(uint64_t n, const std::vector<vg_vi_rec> &recs, const std::function<const uint8_t *(const vg_vi_rec &)> &name_of)
	{
		if (!carry.empty()) return false;
		if (!err && !ended) for (const vg_vi_rec &r : recs) { if (err) break; replay(r, r.same && !tids.empty() ? nullptr : name_of(r)); }
		fed += n;
		return true;
	}
	void end_text()
	{
		if (ended) return;
		ended = true;
		if (!err && !carry.empty()) line_of_carry(fed);
	}

	// whole BGZF blocks, as the compressor hands them out; the end-of-file marker (ISIZE 0) is not a text block
	bool feed_bgzf(const uint8_t *z, uint64_t n)
	{
		uint64_t at = 0;
		while (at < n) {
			if (n - at < 18 || z[at] != 0x1f || z[at + 1] != 0x8b || z[at + 12] != 'B' || z[at + 13] != 'C') return false;
			const uint64_t size = (uint64_t)(z[at + 16] | z[at + 17] << 8) + 1;
			if (size < 26 || size > n - at) return false;
			const uint8_t *t = z + at + size - 4;
			const uint32_t isize = t[0] | t[1] << 8 | t[2] << 16 | (uint32_t)t[3] << 24;
			if (isize) { cstart.push_back(file_at + at); text_end = file_at + at + size; }
			at += size;
		}
		file_at += n;
		return true;
	}

	uint64_t blocks_of_text() const { return (fed + B - 1) / B; }
	uint64_t raw_bytes() const
	{
		uint64_t s = 4 + 8 * 4;
		for (const Tid &t : tids) {
			s += t.name.size() + 1 + 4 + 4;
			for (const auto &b : t.bins) s += 8 + 16 * b.second.size();
			s += 8 + 32 + 8 * t.ioff.size();
		}
		return s + 8;
	}
	// 0, or: 1 the index was refused, 2 the blocks fed are not those of the text fed
	int serialise(std::vector<uint8_t> &out)
	{
		end_text();
		if (err) return 1;
		const uint64_t nb = blocks_of_text();
		if (cstart.size() != nb) return 2;
		auto vo = [&](uint64_t u) { const uint64_t k = u / B; return (k < nb ? cstart[(size_t)k] : text_end) << 16 | u % B; };      // (block nb: the marker)
		out.clear();
		out.reserve((size_t)raw_bytes());
		auto u32 = [&](uint32_t v) { for (int i = 0; i < 4; i++) out.push_back((uint8_t)(v >> (8 * i))); };
		auto u64 = [&](uint64_t v) { for (int i = 0; i < 8; i++) out.push_back((uint8_t)(v >> (8 * i))); };
		out.insert(out.end(), {'T', 'B', 'I', 1});
		uint32_t l_nm = 0;
		for (const Tid &t : tids) l_nm += (uint32_t)t.name.size() + 1;
		u32((uint32_t)tids.size()); u32(2); u32(1); u32(2); u32(0); u32('#'); u32(0); u32(l_nm);
		for (const Tid &t : tids) { out.insert(out.end(), t.name.begin(), t.name.end()); out.push_back(0); }
		for (const Tid &t : tids) {
			u32((uint32_t)t.bins.size() + 1);
			for (const auto &b : t.bins) {
				u32(b.first); u32((uint32_t)b.second.size());
				for (const auto &c : b.second) { u64(vo(c.first)); u64(vo(c.second)); }
			}
			u32(VG_VI_PSEUDO_BIN); u32(2); u64(vo(t.first)); u64(vo(t.last)); u64(t.lines); u64(0);
			u32((uint32_t)t.ioff.size());
			std::vector<uint64_t> io(t.ioff);
			for (size_t w = io.size(); w-- > 0;) if (io[w] == ~0ull) io[w] = io[w + 1];      // (the highest window always has a line)
			for (uint64_t u : io) u64(vo(u));
		}
		u64(0);
		return 0;
	}
};

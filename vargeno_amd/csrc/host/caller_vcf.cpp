// caller_vcf.cpp -- genotype caller and VCF annotator of the drop-in `vargeno geno`.
//
// Behaviour to reproduce (reference src/qv.cc:1573-1747 caller loop + VCF pass, :1789-1848 posterior):
//   * per SNP site: likelihood of (ref_cnt, alt_cnt) under hom-ref / het / hom-alt with a 1 % error rate, Hardy-Weinberg
//     prior from the two allele frequencies stored as n/255, times a Poisson(7.1) depth term; a site with no reads or
//     with both counters saturated is not called; GQ = (int)(-10 ln(confidence));
//   * the SNP list is echoed with GT:GQ for every record whose "chr<CHROM>$<POS>" names a called site; other records
//     are dropped; FORMAT header lines are injected unless the input declares them.
// The arithmetic is IEEE double through libm in the reference's operation order (GQ truncates, so a last-bit
// difference can show).  Everything else is organised for a 10 M-record dbSNP file: calls live in per-chromosome sorted
// arrays instead of a string-keyed hash map, the input is scanned in place, and record chunks are annotated by all
// host threads.
#include <ctype.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/vargeno_hip.h"
#include "vg_host.h"
#include "../vg_caller.h"
#include "../vg_jtext.h"

namespace vgh {

// ------------------------------------------------------------------------------------------------
// posterior: ../vg_caller.h, shared with the device's caller kernel
// ------------------------------------------------------------------------------------------------
namespace {
const vg_caller_tables &caller_tables()
{
	static const vg_caller_tables t = [] { vg_caller_tables x; vg_caller_tables_fill(x); return x; }();
	return t;
}
}  // namespace

Genotype call_genotype(unsigned ref_cnt, unsigned alt_cnt, uint8_t ref_freq, uint8_t alt_freq)
{
	const vg_site_call c = vg_call_site(caller_tables(), ref_cnt, alt_cnt, ref_freq, alt_freq);
	return Genotype{c.gt, c.confidence};
}

int genotype_quality(double confidence) { return vg_genotype_quality(confidence); }

// ------------------------------------------------------------------------------------------------
// chromosome table (<prefix>.chrlens: "name length" per line; a name is at most 32 non-space characters)
// ------------------------------------------------------------------------------------------------
std::vector<ChrLen> read_chrlens(const std::string &path)
{
	FILE *f = fopen(path.c_str(), "r");
	if (!f) throw Error{"cannot open " + path};
	std::vector<ChrLen> table;
	char line[256];
	while (fgets(line, sizeof line, f)) {
		const char *p = line;
		while (*p && !isspace((unsigned char)*p) && p - line < 32) p++;
		ChrLen c{std::string((const char *)line, (size_t)(p - line)), 0};
		while (isspace((unsigned char)*p)) p++;
		c.len = (uint64_t)atol(p);
		table.push_back(c);
	}
	fclose(f);
	return table;
}

// the calls themselves are independent of one another: threads, a slice of the sites each (r05: 10 M sites at 30-fold coverage
// are all genotyped; one thread took 0.3 s of the job's tail for them)
void call_sites(const SiteCounts &s, SiteCalls &out)
{
	const size_t ns = s.pos.size();
	out.gt.resize(ns); out.gq.resize(ns);
	unsigned nt = std::max(1u, std::min(std::thread::hardware_concurrency(), 16u));
	if (ns < (1u << 16)) nt = 1;
	auto work = [&](unsigned t) {
		for (size_t i = ns * t / nt; i < ns * (t + 1) / nt; i++) {
			const Genotype k = call_genotype(s.ref_cnt[i], s.alt_cnt[i], s.ref_freq[i], s.alt_freq[i]);
			out.gt[i] = k.gt;
			out.gq[i] = k.gt == GT_NONE ? 0 : genotype_quality(k.confidence);
		}
	};
	if (nt == 1) work(0);
	else { std::vector<std::thread> th; for (unsigned t = 0; t < nt; t++) th.emplace_back(work, t); for (auto &x : th) x.join(); }
}

// ------------------------------------------------------------------------------------------------
// called sites, addressable the way the reference's "name$position" keys are
// ------------------------------------------------------------------------------------------------
namespace {

struct CalledSite {
	uint64_t local;        // 1-based position inside its chromosome
	uint32_t order;        // rank in genome order (a later site replaces an earlier one under the same key)
	uint8_t gt;
	int gq;
};

class CallBook {
public:
	// the host call loop, then the book of its calls
	CallBook(const SiteCounts &s, const std::vector<ChrLen> &chrs, CallSummary &sum)
	{
		SiteCalls calls;
		call_sites(s, calls);
		build(s.pos, chrs, calls.gt.data(), calls.gq.data(), &sum);
	}
	// from precomputed calls, one per site (the device caller's: vg_sample_calls_fetch)
	CallBook(const std::vector<uint32_t> &pos, const std::vector<ChrLen> &chrs, const SiteCalls &calls, CallSummary &sum) { build(pos, chrs, calls.gt.data(), calls.gq.data(), &sum); }
	// EVERY site under its key, called or not, sites of one key in genome order: the key -> sites structure of a joint file, built once
	// for all samples (find() returns the first site of a key, the others follow it)
	CallBook(const std::vector<uint32_t> &pos, const std::vector<ChrLen> &chrs) { build(pos, chrs, nullptr, nullptr, nullptr); }

private:
	void build(const std::vector<uint32_t> &pos, const std::vector<ChrLen> &chrs, const uint8_t *gts, const int32_t *gqs, CallSummary *sum)
	{
		const size_t ns = pos.size();
		// sites ascend over the concatenated genome: walk the chromosome table alongside them
		size_t c = 0, c_of_list = SIZE_MAX;
		std::vector<CalledSite> *list = nullptr;                 // by_name_[chrs[c].name], looked up once per chromosome
		uint64_t before = 0;                                     // bases in chromosomes 0 .. c-1
		for (size_t i = 0; i < ns; i++) {
			const uint64_t g = pos[i];
			while (c < chrs.size() && g - before > chrs[c].len) before += chrs[c++].len;
			const uint8_t gt = gts ? gts[i] : (uint8_t)GT_NONE;
			if (gts) {
				if (gt == GT_NONE) continue;
				(gt == GT_HOM_REF ? sum->ref : gt == GT_HOM_ALT ? sum->alt : sum->het)++;
			}
			if (c == chrs.size()) continue;                      // beyond the last chromosome: no name to print it under
			if (c != c_of_list) { list = &by_name_[chrs[c].name]; c_of_list = c; list->reserve(list->size() + (gts ? (ns - i) / 4 : 0)); }
			list->push_back(CalledSite{g - before, (uint32_t)i, gt, gts ? (int)gqs[i] : 0});
		}
		// two chromosomes with one name share a key space; keep, per position, the site that comes last in genome order (a book of
		// every site keeps them all: which of them is a sample's last CALLED one differs from sample to sample)
		for (auto &kv : by_name_) {
			std::vector<CalledSite> &v = kv.second;
			if (std::is_sorted(v.begin(), v.end(), [](const CalledSite &a, const CalledSite &b) { return a.local < b.local; }) &&
			    std::adjacent_find(v.begin(), v.end(), [](const CalledSite &a, const CalledSite &b) { return a.local == b.local; }) == v.end())
				continue;
			std::stable_sort(v.begin(), v.end(), [](const CalledSite &a, const CalledSite &b) { return a.local != b.local ? a.local < b.local : a.order < b.order; });
			if (!gts) continue;
			size_t w = 0;
			for (size_t r = 0; r < v.size(); r++) { if (w && v[w - 1].local == v[r].local) v[w - 1] = v[r]; else v[w++] = v[r]; }
			v.resize(w);
		}
	}

public:
	// The reference compares the strings  name + "$" + decimal(position)  and  chrom + "$" + POS-column.  A decimal number
	// holds no '$', so the two are equal exactly when the text after the LAST '$' of the right-hand side is the canonical
	// decimal form of the position and the text before it is the name.
	// (a SNP list is nearly always sorted: the caller's Hint remembers the list of the last name and the place of the last hit in
	// it, and the search gallops forward from there; any other order merely falls back to the full search)
	struct Hint { std::string name; const std::vector<CalledSite> *list = nullptr; size_t at = 0; };
	const CalledSite *find(const std::string &key, Hint &h) const
	{
		const size_t cut = key.rfind('$');
		const char *d = key.c_str() + cut + 1;
		const size_t nd = key.size() - cut - 1;
		if (nd == 0 || nd > 19 || (d[0] == '0' && nd > 1)) return nullptr;
		uint64_t v = 0;
		for (size_t i = 0; i < nd; i++) { if (d[i] < '0' || d[i] > '9') return nullptr; v = v * 10 + (uint64_t)(d[i] - '0'); }
		if (!(h.list && h.name.size() == cut && key.compare(0, cut, h.name) == 0)) {
			h.name.assign(key, 0, cut);
			const auto it = by_name_.find(h.name);
			h.list = it == by_name_.end() ? nullptr : &it->second;
			h.at = 0;
		}
		if (!h.list) return nullptr;
		const std::vector<CalledSite> &list = *h.list;
		auto lo = list.begin(), hi = list.end();
		if (h.at < list.size() && list[h.at].local <= v) {
			// gallop: the answer is at or after the last hit
			size_t step = 1, a = h.at;
			while (a + step < list.size() && list[a + step].local < v) { a += step; step *= 2; }
			lo = list.begin() + (ptrdiff_t)a;
			hi = list.begin() + (ptrdiff_t)std::min(list.size(), a + step + 1);
		}
		const auto at = std::lower_bound(lo, hi, v, [](const CalledSite &a, uint64_t x) { return a.local < x; });
		if (at == list.end() || at->local != v) return nullptr;
		h.at = (size_t)(at - list.begin());
		return &*at;
	}

	// one past the last site of the list the hint's last find() looked in
	static const CalledSite *list_end(const Hint &h) { return h.list->data() + h.list->size(); }

private:
	std::map<std::string, std::vector<CalledSite>> by_name_;
};

// ------------------------------------------------------------------------------------------------
// the VCF pass
// ------------------------------------------------------------------------------------------------
const char kGtDecl[] = "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n";
const char kGqDecl[] = "##FORMAT=<ID=GQ,Number=1,Type=Integer,Description=\"Genotype Quality\">\n";
// the joint file under JointTextRoute::info_counts: the keys of ../vg_jtext.h's tag, in its order
const char *const kJointInfoKeys[4] = {"NS", "AN", "AC", "AF"};
const char kJointInfoDecl[] = "##INFO=<ID=NS,Number=1,Type=Integer,Description=\"Number of samples with a called genotype\">\n"
                              "##INFO=<ID=AN,Number=1,Type=Integer,Description=\"Total number of alleles in called genotypes\">\n"
                              "##INFO=<ID=AC,Number=A,Type=Integer,Description=\"Allele count in called genotypes\">\n"
                              "##INFO=<ID=AF,Number=A,Type=Float,Description=\"Allele frequency in called genotypes, AC / AN\">\n";

struct Span {
	const char *b, *e;
	size_t size() const { return (size_t)(e - b); }
	bool is(const char *lit) const { return size() == strlen(lit) && memcmp(b, lit, size()) == 0; }
};

// What the header decided for every record that follows it.
struct Layout {
	bool declares_gt = false, declares_gq = false;   // the input already has "ID=GT," / "ID=GQ," meta lines
	bool sample_columns = true;                      // the #CHROM line has FORMAT + a sample column (>= 10 fields)
	int gt_slot = -1, gq_slot = -1;                  // sub-field of the sample column to overwrite; settled by the first annotated record
};

size_t count_fields(Span s, char sep) { return (size_t)std::count(s.b, s.e, sep) + 1; }
Span field(Span s, char sep, size_t k)            // k-th sep-separated field (must exist)
{
	const char *p = s.b;
	for (; k; k--) p = (const char *)memchr(p, sep, (size_t)(s.e - p)) + 1;
	const char *q = (const char *)memchr(p, sep, (size_t)(s.e - p));
	return Span{p, q ? q : s.e};
}
int slot_of(Span format, const char *tag)
{
	const size_t n = count_fields(format, ':');
	for (size_t k = 0; k < n; k++) if (field(format, ':', k).is(tag)) return (int)k;
	return -1;
}

const char *gt_text(uint8_t gt) { return gt == GT_HET ? "0/1" : gt == GT_HOM_ALT ? "1/1" : "0/0"; }

// One data line -> `out` (nothing if its key names no called site).  Returns false if the layout's slots are still open
// and this record would have to settle them (the caller does that on one thread, in file order).
struct Scratch { std::string key, fmt, smp; CallBook::Hint hint; };           // one per thread: no allocation per line
bool annotate(Span line, const CallBook &book, const Layout &lay, bool may_settle, Layout *settled, std::string &out, Scratch &sc)
{
	const size_t nf = count_fields(line, '\t');
	if (nf < 2) return true;
	const Span chrom = field(line, '\t', 0), pos = field(line, '\t', 1);
	std::string &key = sc.key;
	key.clear();
	if (chrom.size() == 0 || chrom.b[0] != 'c') key = "chr";
	key.append(chrom.b, chrom.e).push_back('$');
	key.append(pos.b, pos.e);
	const CalledSite *site = book.find(key, sc.hint);
	if (!site) return true;

	const bool in_place = lay.sample_columns && nf >= 10;      // rewrite fields 8 and 9; otherwise append two fields
	int gt_slot = lay.gt_slot, gq_slot = lay.gq_slot;
	if ((lay.declares_gt && gt_slot < 0) || (lay.declares_gq && gq_slot < 0)) {
		if (!may_settle) return false;
		const Span fmt = in_place ? field(line, '\t', 8) : Span{line.e, line.e};
		if (lay.declares_gt && gt_slot < 0) gt_slot = slot_of(fmt, "GT");
		if (lay.declares_gq && gq_slot < 0) gq_slot = slot_of(fmt, "GQ");
		// the reference asserts that a declared GT is present in the first annotated record's FORMAT (qv.cc:1701); a declared
		// GQ drives it into an out-of-range write (it never looks the column up), so there the intent is followed instead
		if ((lay.declares_gt && gt_slot < 0) || (lay.declares_gq && gq_slot < 0))
			throw Error{"the SNP list declares GT/GQ in its header but the FORMAT column of a genotyped record lacks it"};
		settled->gt_slot = gt_slot; settled->gq_slot = gq_slot;
	}
	char gq_text[16];
	snprintf(gq_text, sizeof gq_text, "%d", site->gq);

	std::string &fmt = sc.fmt, &smp = sc.smp;
	fmt.clear(); smp.clear();
	size_t n_sub = 0;
	if (in_place) {
		const Span f8 = field(line, '\t', 8), f9 = field(line, '\t', 9);
		fmt.assign(f8.b, f8.e);
		n_sub = count_fields(f9, ':');
		for (size_t k = 0; k < n_sub; k++) {
			if (k) smp.push_back(':');
			if (lay.declares_gt && (int)k == gt_slot) smp += gt_text(site->gt);
			else if (lay.declares_gq && (int)k == gq_slot) smp += gq_text;
			else { const Span v = field(f9, ':', k); smp.append(v.b, v.e); }
		}
		if ((lay.declares_gt && (size_t)gt_slot >= n_sub) || (lay.declares_gq && (size_t)gq_slot >= n_sub))
			throw Error{"a genotyped record's sample column has fewer sub-fields than its FORMAT"};
	}
	auto push = [&](const char *tag, const char *val) {
		if (!fmt.empty() || n_sub) { fmt.push_back(':'); smp.push_back(':'); }
		fmt += tag; smp += val;
		n_sub++;
	};
	if (!lay.declares_gt) push("GT", gt_text(site->gt));
	if (!lay.declares_gq) push("GQ", gq_text);

	if (in_place) {
		const Span f8 = field(line, '\t', 8), f9 = field(line, '\t', 9);
		out.append(line.b, f8.b).append(fmt).push_back('\t');
		out.append(smp).append(f9.e, line.e);
	} else {
		out.append(line.b, line.e).push_back('\t');
		out.append(fmt).push_back('\t');
		out.append(smp);
	}
	out.push_back('\n');
	return true;
}

std::string slurp(const std::string &path, bool &ok)
{
	std::string text;
	FILE *f = fopen(path.c_str(), "rb");
	ok = f != nullptr;
	if (!f) return text;
	char buf[1 << 16];
	size_t got;
	while ((got = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, got);
	fclose(f);
	return text;
}

inline Span next_line(const char *&p, const char *end)
{
	const char *nl = (const char *)memchr(p, '\n', (size_t)(end - p));
	Span s{p, nl ? nl : end};
	p = nl ? nl + 1 : end;
	return s;
}

}  // namespace

// Lines that are read by one thread in file order: meta lines ("##..."), column headers ("#..."), and -- while the input
// declares GT/GQ but no annotated record has shown yet which sub-field holds them -- data lines.  Stops in front of the
// first data line that can be annotated independently of its neighbours.
static void ordered_lines(const char *&p, const char *end, Layout &lay, const CallBook &book, std::string &dst)
{
	while (p < end) {
		const char *at = p;
		const Span ln = next_line(p, end);
		if (ln.size() == 0) continue;
		if (ln.b[0] != '#') {
			const bool slots_open = (lay.declares_gt && lay.gt_slot < 0) || (lay.declares_gq && lay.gq_slot < 0);
			if (!slots_open) { p = at; return; }
			Scratch sc;
			annotate(ln, book, lay, true, &lay, dst, sc);
		} else if (ln.size() > 1 && ln.b[1] == '#') {
			dst.append(ln.b, ln.e).push_back('\n');
			const std::string meta(ln.b, ln.e);
			if (meta.find("ID=GT,") != std::string::npos) lay.declares_gt = true;
			else if (meta.find("ID=GQ,") != std::string::npos) lay.declares_gq = true;
		} else {
			if (!lay.declares_gt) dst += kGtDecl;
			if (!lay.declares_gq) dst += kGqDecl;
			dst.append(ln.b, ln.e);
			if (count_fields(ln, '\t') < 10) { lay.sample_columns = false; dst += "\tFORMAT\tDONOR"; }
			dst.push_back('\n');
		}
	}
}

bool read_whole_file(const std::string &path, std::string &text)
{
	bool ok = false;
	text = slurp(path, ok);
	return ok;
}

// ------------------------------------------------------------------------------------------------
// where the text goes (vg_host.h: VcfSink)
// ------------------------------------------------------------------------------------------------
namespace {

class PlainSink : public VcfSink {
public:
	PlainSink(const std::string &path) : path_(path), f_(fopen(path.c_str(), "wb")) { if (!f_) throw Error{"cannot write " + path}; }
	~PlainSink() override { if (f_) fclose(f_); }
	void write(const char *p, size_t n) override { fwrite(p, 1, n, f_); }
	void close() override
	{
		FILE *f = f_;
		f_ = nullptr;
		if (fclose(f) != 0) throw Error{"cannot write " + path_};
	}
private:
	const std::string path_;
	FILE *f_;
};

std::atomic<unsigned> g_index_refusals{0};

// <vcf_path>.tbi from a handle that has seen the whole text and every block of the file, after the VCF has closed cleanly
void write_tbi(vg_vcfidx *idx, const std::string &vcf_path, const VcfOutput &how, const char *route)
{
	const std::string path = vcf_path + ".tbi";
	std::vector<uint8_t> raw((size_t)vg_vcfidx_bound(idx));
	uint64_t len = 0, at = 0;
	const int rc = vg_vcfidx_finish(idx, raw.data(), raw.size(), &len);
	if (const char *rule = vg_vcfidx_error(idx, &at)) {
		fprintf(stderr, "vargeno: %s cannot be indexed: %s (the line at byte %lu of the text); the VCF is complete, no .tbi is written\n", vcf_path.c_str(), rule, (unsigned long)at);
		remove(path.c_str());
		g_index_refusals++;
		return;
	}
	if (rc != VG_OK) throw Error{std::string("vg_vcfidx_finish failed: ") + vg_last_error()};
	std::vector<uint8_t> z((size_t)vg_bgzf_deflate_bound(len, 0));
	uint64_t zlen = 0;
	if (vg_bgzf_deflate_host_coded(raw.data(), len, 0, 1, 1, VG_DEFLATE_FIXED, z.data(), z.size(), &zlen) != VG_OK) throw Error{std::string("vg_bgzf_deflate_host_coded failed: ") + vg_last_error()};
	FILE *f = fopen(path.c_str(), "wb");
	const bool wrote = f && fwrite(z.data(), 1, (size_t)zlen, f) == (size_t)zlen;
	if ((f && fclose(f) != 0) || !wrote) throw Error{"cannot write " + path};
	if (how.verbose) {
		uint64_t st[5] = {0, 0, 0, 0, 0};
		(void)vg_vcfidx_stats(idx, st);
		fprintf(stderr, "vcf index: %s, %lu data lines, %lu chromosomes, %lu bins, %lu chunks, %lu bytes, %.3f s\n", route, (unsigned long)st[0], (unsigned long)st[1], (unsigned long)st[2], (unsigned long)st[3], (unsigned long)zlen, (double)st[4] / 1e6);
	}
}

// Spans of span_ bytes (a multiple of the block: the blocks of the file are those of one call over the whole text) go to a worker
// thread, which compresses and writes them in order; the producer waits while two are queued.
class BgzfSink : public VcfSink {
public:
	BgzfSink(const std::string &path, const VcfOutput &how) : path_(path), how_(how), f_(fopen(path.c_str(), "wb"))
	{
		if (!f_) throw Error{"cannot write " + path};
		const uint64_t block = how.block ? how.block : 65280;
		span_ = (size_t)(block * std::max<uint64_t>(1, (16ull << 20) / block));
		device_ = how.bgzf == VcfBgzf::Device;
		if (how.index && vg_vcfidx_create(how.block, &idx_) != VG_OK) { fclose(f_); throw Error{std::string("vg_vcfidx_create failed: ") + vg_last_error()}; }
		worker_ = std::thread([this] { work(); });
	}
	~BgzfSink() override
	{
		stop(true);
		if (f_) fclose(f_);
		vg_vcfidx_destroy(idx_);
	}
	void write(const char *p, size_t n) override
	{
		while (n) {                                                   // one span at most per step
			const size_t take = std::min(n, span_ - cur_.size());
			cur_.insert(cur_.end(), p, p + take);
			p += take; n -= take;
			if (cur_.size() == span_) push(false);
		}
	}
	void close() override
	{
		push(true);                                                   // the rest of the text (or none), and the end-of-file marker behind it
		stop(false);
		FILE *f = f_;
		f_ = nullptr;
		const bool closed = fclose(f) == 0;
		if (!error_.empty()) throw Error{error_};
		if (!closed) throw Error{"cannot write " + path_};
		if (idx_) write_tbi(idx_, path_, how_, how_.bgzf != VcfBgzf::Device ? "host" : device_ ? "device" : "device, then host");
	}
private:
	struct Span { std::vector<uint8_t> text; bool last; };
	void push(bool last)
	{
		std::unique_lock<std::mutex> g(mu_);
		cv_.wait(g, [&] { return q_.size() < 2; });
		q_.push_back(Span{std::move(cur_), last});
		cur_ = std::vector<uint8_t>();
		if (!last) cur_.reserve(span_);
		cv_.notify_all();
	}
	void stop(bool abandon)
	{
		{ std::lock_guard<std::mutex> g(mu_); done_ = true; if (abandon) { abandon_ = true; q_.clear(); } }
		cv_.notify_all();
		if (worker_.joinable()) worker_.join();
	}
	// one span -> its BGZF bytes in out; "" or what went wrong
	std::string compress(const Span &s, std::vector<uint8_t> &out)
	{
		const uint64_t cap = vg_bgzf_deflate_bound(s.text.size(), how_.block);
		out.resize((size_t)cap);
		uint64_t len = 0;
		const uint8_t *text = s.text.empty() ? out.data() : s.text.data();      // (no text: any pointer that is not null)
		if (device_) {
			const int rc = idx_ ? vg_bgzf_deflate_device_indexed(how_.device, text, s.text.size(), how_.block, s.last, how_.codes, idx_, out.data(), cap, &len)
			                    : vg_bgzf_deflate_device_coded(how_.device, text, s.text.size(), how_.block, s.last, how_.codes, out.data(), cap, &len);
			if (rc == VG_ENOMEM) {
				if (how_.verbose) fprintf(stderr, "vcf: no device memory for the deflate kernel (%s): the rest of %s is compressed on the host\n", vg_last_error(), path_.c_str());
				device_ = false;
			} else if (rc != VG_OK) return std::string("vg_bgzf_deflate_device_coded failed: ") + vg_last_error();
		}
		if (!device_) {                                               // (the index: the host scanner and the blocks, around the compressor)
			if (idx_ && vg_vcfidx_text_host(idx_, text, s.text.size(), how_.threads) != VG_OK) return std::string("vg_vcfidx_text_host failed: ") + vg_last_error();
			if (vg_bgzf_deflate_host_coded(text, s.text.size(), how_.block, s.last, how_.threads, how_.codes, out.data(), cap, &len) != VG_OK)
				return std::string("vg_bgzf_deflate_host_coded failed: ") + vg_last_error();
			if (idx_ && vg_vcfidx_bgzf(idx_, out.data(), len) != VG_OK) return std::string("vg_vcfidx_bgzf failed: ") + vg_last_error();
		}
		out.resize((size_t)len);
		return std::string();
	}
	void work()
	{
		std::vector<uint8_t> out;
		for (;;) {                                                    // one span per step
			Span s;
			{
				std::unique_lock<std::mutex> g(mu_);
				cv_.wait(g, [&] { return !q_.empty() || done_; });
				if (q_.empty() || abandon_) return;
				s = std::move(q_.front());                            // (it stays queued while it is compressed: two spans are in flight, not three)
			}
			if (error_.empty()) {
				std::string e = compress(s, out);
				if (e.empty() && fwrite(out.data(), 1, out.size(), f_) != out.size()) e = "cannot write " + path_;
				if (!e.empty()) error_ = e;                           // (read by close(), after the join)
			}
			{ std::lock_guard<std::mutex> g(mu_); if (!q_.empty()) q_.pop_front(); }
			cv_.notify_all();
			if (s.last) return;
		}
	}
	const std::string path_;
	const VcfOutput how_;
	FILE *f_;
	size_t span_ = 0;
	bool device_ = false;
	vg_vcfidx *idx_ = nullptr;                                        // VcfOutput::index: fed by the worker alone, read by close() after the join
	std::vector<uint8_t> cur_;
	std::thread worker_;
	std::mutex mu_; std::condition_variable cv_;
	std::deque<Span> q_;
	bool done_ = false, abandon_ = false;
	std::string error_;
};

}  // namespace

unsigned vcf_index_refusals() { return g_index_refusals; }

std::unique_ptr<VcfSink> open_vcf_sink(const std::string &path, const VcfOutput &how)
{
	if (how.bgzf == VcfBgzf::Off) return std::unique_ptr<VcfSink>(new PlainSink(path));
	return std::unique_ptr<VcfSink>(new BgzfSink(path, how));
}

namespace {

unsigned vcf_threads()
{
	unsigned threads = std::max(1u, std::min(std::thread::hardware_concurrency(), 32u));
	if (const char *e = getenv("VARGENO_THREADS")) if (atoi(e) > 0) threads = (unsigned)atoi(e);
	return threads;
}

// The pass over the SNP list's bytes, shared by the single-sample and the joint writer.  header(p, end, dst) takes the lines that
// one thread reads in file order and stops in front of the first data line that can be annotated independently of its
// neighbours; line(ln, dst, scratch) annotates one such line.  Returns the seconds spent handing text to the sink.
template <class Header, class Line>
double vcf_pass(const std::string &text, VcfSink &out, unsigned threads, Header header, Line line)
{
	double t_write = 0;
	auto lap = [](const timespec &a, const timespec &b) { return (double)(b.tv_sec - a.tv_sec) + 1e-9 * (double)(b.tv_nsec - a.tv_nsec); };
	const char *p = text.data(), *const end = p + text.size();
	while (p < end) {
		std::string seq;
		header(p, end, seq);
		out.write(seq.data(), seq.size());
		// a run of data lines: up to the next line that starts with '#' (the reference re-reads header lines wherever they
		// stand, so they fence the run), cut at line starts into one piece per thread
		const char *stop = end;
		for (const char *q = p; q < end;) {
			const char *h = (const char *)memchr(q, '#', (size_t)(end - q));
			if (!h) break;
			if (h == text.data() || h[-1] == '\n') { stop = h; break; }
			q = h + 1;
		}
		const size_t bytes = (size_t)(stop - p);
		const unsigned nt = bytes < (1u << 20) ? 1u : threads;
		std::vector<const char *> cut(nt + 1, stop);
		cut[0] = p;
		for (unsigned t = 1; t < nt; t++) {
			const char *c = p + bytes / nt * t;
			const char *nl = (const char *)memchr(c, '\n', (size_t)(stop - c));
			cut[t] = nl ? nl + 1 : stop;
		}
		std::vector<std::string> piece(nt), err(nt);
		auto work = [&](unsigned t) {
			const char *q = cut[t], *const e = cut[t + 1];
			piece[t].reserve((size_t)(e - q) + (size_t)(e - q) / 4 + 4096);          // (a line grows by ~":GT:GQ" + the two values)
			Scratch sc;
			try {
				while (q < e) { const Span ln = next_line(q, e); if (ln.size()) line(ln, piece[t], sc); }
			} catch (const Error &x) { err[t] = x.msg; }
		};
		if (nt == 1) work(0);
		else {
			std::vector<std::thread> th;
			for (unsigned t = 0; t < nt; t++) th.emplace_back(work, t);
			for (auto &x : th) x.join();
		}
		for (unsigned t = 0; t < nt; t++) if (!err[t].empty()) throw Error{err[t]};
		struct timespec c2, c3; clock_gettime(CLOCK_MONOTONIC, &c2);
		for (unsigned t = 0; t < nt; t++) out.write(piece[t].data(), piece[t].size());          // (positioned writes by several threads are slower: one inode lock)
		clock_gettime(CLOCK_MONOTONIC, &c3);
		t_write += lap(c2, c3);
		p = stop;
	}
	return t_write;
}

}  // namespace

CallSummary write_genotyped_vcf(const SiteCounts &s, const std::vector<ChrLen> &chrlens, const std::string &vcf_in, const std::string &vcf_out, const std::string *vcf_text, const SiteCalls *calls, const VcfOutput &how)
{
	CallSummary sum;
	const bool clocks = getenv("VARGENO_VCF_CLOCKS") != nullptr;
	struct timespec c0, c1; clock_gettime(CLOCK_MONOTONIC, &c0);
	auto lap = [](const timespec &a, const timespec &b) { return (double)(b.tv_sec - a.tv_sec) + 1e-9 * (double)(b.tv_nsec - a.tv_nsec); };
	const CallBook book = calls ? CallBook(s.pos, chrlens, *calls, sum) : CallBook(s, chrlens, sum);
	clock_gettime(CLOCK_MONOTONIC, &c1);
	bool ok = vcf_text != nullptr;
	std::string own;
	if (!vcf_text) own = slurp(vcf_in, ok);
	const std::string &text = vcf_text ? *vcf_text : own;
	struct timespec c1b; clock_gettime(CLOCK_MONOTONIC, &c1b);
	if (!ok) { fprintf(stderr, "Error opening: %s . You have failed.\n", vcf_in.c_str()); return sum; }
	const std::unique_ptr<VcfSink> out = open_vcf_sink(vcf_out, how);

	Layout lay;
	const double t_write = vcf_pass(text, *out, vcf_threads(),
	                                [&](const char *&p, const char *end, std::string &dst) { ordered_lines(p, end, lay, book, dst); },
	                                [&](Span ln, std::string &dst, Scratch &sc) { annotate(ln, book, lay, false, nullptr, dst, sc); });
	out->close();
	if (clocks) { struct timespec c4; clock_gettime(CLOCK_MONOTONIC, &c4); fprintf(stderr, "vcf: calls + book %.3f s, SNP list read %.3f s, lines %.3f s, write %.3f s\n", lap(c0, c1), lap(c1, c1b), lap(c1b, c4) - t_write, t_write); }
	return sum;
}

// ------------------------------------------------------------------------------------------------
// the joint file: one line per site, one column per sample (no reference counterpart; README "Cohorts")
// ------------------------------------------------------------------------------------------------
// A data line is written iff at least one sample's own VCF would contain it: its first eight fields, GT:GQ, then per sample what
// that sample's own VCF shows for the record -- the call of the LAST site of the record's key, in genome order, that the sample
// has called -- or ./.:. if its VCF drops the record.
namespace {

Span joint_first_eight(Span ln)
{
	const char *q = ln.b;
	for (int k = 0; k < 8 && q; k++) { q = (const char *)memchr(q, '\t', (size_t)(ln.e - q)); if (q && k < 7) q++; }
	return Span{ln.b, q ? q : ln.e};
}

// The plan of a run of data lines (../vg_jtext.h), built by the pass's threads: head offsets count from the start of the SNP list's text
struct JointPlan {
	std::vector<vg_jtext_record> recs;
	std::vector<uint32_t> sites;
	void clear() { recs.clear(); sites.clear(); }
};

// The planned routes of write_joint_vcf (vg_host.h: JointText::Planned and ::Device).  false: the device has no memory for the
// handle and nothing has been written -- the caller's own loop writes the file.
bool write_joint_vcf_planned(const std::vector<uint32_t> &pos, const std::vector<ChrLen> &chrlens, const std::vector<JointSample> &samples, const std::string &vcf_in, const std::string &vcf_out, const std::string *vcf_text,
                             const VcfOutput &how, const JointTextRoute &tr)
{
	struct timespec c0, c1; clock_gettime(CLOCK_MONOTONIC, &c0);
	const bool on_device = tr.route == JointText::Device;
	const char *const route = on_device ? "device" : "planned";
	const size_t n = samples.size();
	if (n == 0 || n > 16384) throw Error{std::string("VARGENO_JOINT_TEXT=") + route + " takes 1 to 16384 samples"};
	// a span: at most `lines` records, SPAN_HEADS bytes of the list from its first head to its last, and site_cap site references
	const int info = tr.info_counts ? VG_JT_INFO_COUNTS : VG_JT_INFO_NONE;      // the mode of every span's text
	const uint64_t per_line = VG_JT_LINE_FIXED + (uint64_t)VG_JT_CELL_MAX * n + (tr.info_counts ? VG_JT_INFO_MAX : 0), SPAN_HEADS = 32ull << 20;
	const uint64_t lines = tr.lines ? std::min<uint64_t>(tr.lines, 1u << 22) : std::max<uint64_t>(1, std::min<uint64_t>(1u << 20, (128ull << 20) / (per_line + 64)));
	const uint64_t site_cap = 4 * lines + 4096;
	const bool stream = on_device && how.bgzf == VcfBgzf::Device;         // the text leaves the device compressed
	vg_jtext *jt = nullptr;
	struct Closer { vg_jtext *&h; ~Closer() { if (h) vg_jtext_destroy(h); } } closer{jt};
	if (on_device) {
		uint32_t wide = 0;                                                // samples with a gq the 2-byte column cannot hold
		for (const JointSample &js : samples) {
			bool w = false;
			for (size_t i = 0; i < js.calls.gt.size() && !w; i++) w = js.calls.gt[i] != GT_NONE && (js.calls.gq[i] < 0 || js.calls.gq[i] >= (int32_t)VG_JT_GQ_ESCAPE);
			wide += w;
		}
		const int rc = vg_jtext_create_info(tr.device, pos.size(), (uint32_t)n, wide, lines, SPAN_HEADS, site_cap, stream, info, &jt);
		if (rc == VG_ENOMEM) {
			if (how.verbose) fprintf(stderr, "joint text: no device memory for the text kernels (%s): %s is written by the host loop\n", vg_last_error(), vcf_out.c_str());
			return false;
		}
		if (rc != VG_OK) throw Error{std::string("VARGENO_JOINT_TEXT=device: ") + vg_last_error()};
		for (size_t j = 0; j < n && !pos.empty(); j++)
			if (vg_jtext_set(jt,(uint32_t)j, samples[j].calls.gt.data(), samples[j].calls.gq.data()) != VG_OK) throw Error{"vg_jtext_set failed for sample " + samples[j].name + ": " + vg_last_error()};
	}
	const CallBook book(pos, chrlens);
	bool ok = vcf_text != nullptr;
	std::string own;
	if (!vcf_text) own = slurp(vcf_in, ok);
	const std::string &text = vcf_text ? *vcf_text : own;
	if (!ok) throw Error{"Error opening: " + vcf_in + " . You have failed."};

	// where the bytes go: the sink of every other route, or -- the stream -- BGZF blocks from the handle straight into the file
	std::unique_ptr<VcfSink> out;
	FILE *f = nullptr;
	struct FileCloser { FILE *&f; ~FileCloser() { if (f) fclose(f); } } file_closer{f};
	vg_vcfidx *idx = nullptr;
	struct IndexCloser { vg_vcfidx *&h; ~IndexCloser() { vg_vcfidx_destroy(h); } } index_closer{idx};
	std::vector<uint8_t> buf;
	auto put = [&](uint64_t len) { if (len && fwrite(buf.data(), 1, (size_t)len, f) != (size_t)len) throw Error{"cannot write " + vcf_out}; };
	if (stream) {
		f = fopen(vcf_out.c_str(), "wb");
		if (!f) throw Error{"cannot write " + vcf_out};
		if (vg_jtext_bgzf_begin(jt, how.block, how.codes) != VG_OK) throw Error{std::string("vg_jtext_bgzf_begin failed: ") + vg_last_error()};
		// the index follows the stream: the rendered lines are scanned where they are, on the device
		if (how.index && (vg_vcfidx_create(how.block, &idx) != VG_OK || vg_jtext_bgzf_index(jt, idx) != VG_OK)) throw Error{std::string("the index could not be attached to the stream: ") + vg_last_error()};
	} else out = open_vcf_sink(vcf_out, how);

	std::vector<const uint8_t *> gts(n);
	std::vector<const int32_t *> gqs(n);
	for (size_t j = 0; j < n; j++) { gts[j] = samples[j].calls.gt.data(); gqs[j] = samples[j].calls.gq.data(); }

	bool declares_gt = false, declares_gq = false;
	auto header = [&](const char *&p, const char *end, std::string &dst) {
		while (p < end) {
			const char *at = p;
			const Span ln = next_line(p, end);
			if (ln.size() == 0) continue;
			if (ln.b[0] != '#') { p = at; return; }
			if (ln.size() > 1 && ln.b[1] == '#') {
				dst.append(ln.b, ln.e).push_back('\n');
				const std::string meta(ln.b, ln.e);
				if (meta.find("ID=GT,") != std::string::npos) declares_gt = true;
				else if (meta.find("ID=GQ,") != std::string::npos) declares_gq = true;
			} else {
				if (!declares_gt) dst += kGtDecl;
				if (!declares_gq) dst += kGqDecl;
				if (tr.info_counts) dst += kJointInfoDecl;
				dst += tr.prior_line;
				const Span cols = joint_first_eight(ln);
				dst.append(cols.b, cols.e) += "\tFORMAT";
				for (const JointSample &js : samples) { dst.push_back('\t'); dst += js.name; }
				dst.push_back('\n');
			}
		}
	};
	// one data line -> its record, if its key is in the book
	auto plan_line = [&](Span ln, JointPlan &pl, Scratch &sc) {
		if (count_fields(ln, '\t') < 2) return;
		const Span chrom = field(ln, '\t', 0), ps = field(ln, '\t', 1);
		std::string &key = sc.key;
		key.clear();
		if (chrom.size() == 0 || chrom.b[0] != 'c') key = "chr";
		key.append(chrom.b, chrom.e).push_back('$');
		key.append(ps.b, ps.e);
		const CalledSite *first = book.find(key, sc.hint);
		if (!first) return;
		const Span head = joint_first_eight(ln);
		if (head.size() > SPAN_HEADS) throw Error{"a record of the SNP list has more than " + std::to_string(SPAN_HEADS) + " bytes in its first eight fields: VARGENO_JOINT_TEXT=host writes such a file"};
		vg_jtext_record r;
		r.head_off = (uint64_t)(head.b - text.data()); r.head_len = (uint32_t)head.size(); r.site_at = pl.sites.size(); r.n_sites = 0;
		for (const CalledSite *q = first, *e = CallBook::list_end(sc.hint); q < e && q->local == first->local; q++) { pl.sites.push_back(q->order); r.n_sites++; }      // the sites of this key, in genome order
		if (r.n_sites > site_cap) throw Error{"a key of the SNP list names more than " + std::to_string(site_cap) + " sites: VARGENO_JOINT_TEXT=host writes such a file"};
		pl.recs.push_back(r);
	};

	uint64_t n_records = 0, n_lines = 0, n_spans = 0, n_text = 0;
	std::vector<vg_jtext_record> span_recs;
	// records [i0, i1) of the run's plan -> their text, to the sink or the stream
	auto render_span = [&](const JointPlan &pl, size_t i0, size_t i1) {
		const vg_jtext_record &a = pl.recs[i0], &z = pl.recs[i1 - 1];
		const uint64_t heads_len = z.head_off + z.head_len - a.head_off, refs = z.site_at + z.n_sites - a.site_at;
		span_recs.assign(pl.recs.begin() + (ptrdiff_t)i0, pl.recs.begin() + (ptrdiff_t)i1);
		uint64_t head_sum = 0;
		for (vg_jtext_record &r : span_recs) { r.head_off -= a.head_off; r.site_at -= a.site_at; head_sum += r.head_len; }
		const uint8_t *heads = (const uint8_t *)text.data() + a.head_off;
		const uint32_t *sites = pl.sites.data() + a.site_at;
		const uint64_t bound = vg_jtext_text_bound_info(head_sum, i1 - i0, (uint32_t)n, info);
		uint64_t len = 0, got_lines = 0;
		if (stream) {
			uint64_t text_len = 0;
			buf.resize((size_t)vg_jtext_bgzf_bound(bound, how.block));
			if (vg_jtext_bgzf_lines(jt, heads, heads_len, span_recs.data(), span_recs.size(), sites, refs, buf.data(), buf.size(), &len, &text_len, &got_lines) != VG_OK) throw Error{std::string("vg_jtext_bgzf_lines failed: ") + vg_last_error()};
			put(len);
			n_text += text_len;
		} else {
			buf.resize((size_t)std::max<uint64_t>(1, bound));
			const int rc = on_device ? vg_jtext_render(jt, heads, heads_len, span_recs.data(), span_recs.size(), sites, refs, buf.data(), buf.size(), &len, &got_lines)
			                         : vg_jtext_render_host_info(pos.size(), (uint32_t)n, gts.data(), gqs.data(), heads, heads_len, span_recs.data(), span_recs.size(), sites, refs, info, (int)vcf_threads(), buf.data(), buf.size(), &len, &got_lines);
			if (rc != VG_OK) throw Error{std::string(on_device ? "vg_jtext_render" : "vg_jtext_render_host") + " failed: " + vg_last_error()};
			out->write((const char *)buf.data(), (size_t)len);
			n_text += len;
		}
		n_lines += got_lines; n_spans++;
	};

	// the pass: vcf_pass's structure -- header lines on one thread in file order, then the run of data lines up to the next line
	// that starts with '#', cut at line starts into one piece per thread; the threads plan, the spans render
	const unsigned threads = vcf_threads();
	const char *p = text.data(), *const end = p + text.size();
	JointPlan run;
	while (p < end) {
		std::string seq;
		header(p, end, seq);
		if (stream) {
			uint64_t len = 0;
			buf.resize((size_t)vg_jtext_bgzf_bound(seq.size(), how.block));
			if (vg_jtext_bgzf_text(jt, (const uint8_t *)seq.data(), seq.size(), buf.data(), buf.size(), &len) != VG_OK) throw Error{std::string("vg_jtext_bgzf_text failed: ") + vg_last_error()};
			put(len);
		} else out->write(seq.data(), seq.size());
		const char *stop = end;
		for (const char *q = p; q < end;) {
			const char *h = (const char *)memchr(q, '#', (size_t)(end - q));
			if (!h) break;
			if (h == text.data() || h[-1] == '\n') { stop = h; break; }
			q = h + 1;
		}
		const size_t bytes = (size_t)(stop - p);
		const unsigned nt = bytes < (1u << 20) ? 1u : threads;
		std::vector<const char *> cut(nt + 1, stop);
		cut[0] = p;
		for (unsigned t = 1; t < nt; t++) {
			const char *c = p + bytes / nt * t;
			const char *nl = (const char *)memchr(c, '\n', (size_t)(stop - c));
			cut[t] = nl ? nl + 1 : stop;
		}
		std::vector<JointPlan> piece(nt);
		std::vector<std::string> err(nt);
		auto work = [&](unsigned t) {
			const char *q = cut[t], *const e = cut[t + 1];
			Scratch sc;
			try {
				while (q < e) { const Span ln = next_line(q, e); if (ln.size()) plan_line(ln, piece[t], sc); }
			} catch (const Error &x) { err[t] = x.msg; }
		};
		if (nt == 1) work(0);
		else {
			std::vector<std::thread> th;
			for (unsigned t = 0; t < nt; t++) th.emplace_back(work, t);
			for (auto &x : th) x.join();
		}
		for (unsigned t = 0; t < nt; t++) if (!err[t].empty()) throw Error{err[t]};
		run.clear();
		for (unsigned t = 0; t < nt; t++) {                               // the pieces' plans, joined in file order
			const uint64_t base = run.sites.size();
			for (vg_jtext_record r : piece[t].recs) { r.site_at += base; run.recs.push_back(r); }
			run.sites.insert(run.sites.end(), piece[t].sites.begin(), piece[t].sites.end());
		}
		n_records += run.recs.size();
		for (size_t i0 = 0; i0 < run.recs.size();) {                      // one span per step
			size_t i1 = i0 + 1;
			const vg_jtext_record &a = run.recs[i0];
			while (i1 < run.recs.size() && i1 - i0 < lines) {
				const vg_jtext_record &r = run.recs[i1];
				if (r.head_off + r.head_len - a.head_off > SPAN_HEADS || r.site_at + r.n_sites - a.site_at > site_cap) break;
				i1++;
			}
			render_span(run, i0, i1);
			i0 = i1;
		}
		p = stop;
	}
	if (stream) {
		uint64_t len = 0;
		buf.resize((size_t)vg_jtext_bgzf_bound(0, how.block));
		if (vg_jtext_bgzf_end(jt, buf.data(), buf.size(), &len) != VG_OK) throw Error{std::string("vg_jtext_bgzf_end failed: ") + vg_last_error()};
		put(len);
		FILE *g = f;
		f = nullptr;
		if (fclose(g) != 0) throw Error{"cannot write " + vcf_out};
		if (idx) write_tbi(idx, vcf_out, how, "device stream");
	} else out->close();
	clock_gettime(CLOCK_MONOTONIC, &c1);
	if (how.verbose)
		fprintf(stderr, "joint text: %s%s%s, %lu records, %lu lines written, %lu spans of at most %lu records, %lu text bytes, %.3f s\n", route, stream ? " (BGZF stream)" : "", tr.info_counts ? ", info counts" : "", (unsigned long)n_records, (unsigned long)n_lines,
		        (unsigned long)n_spans, (unsigned long)lines, (unsigned long)n_text, (double)(c1.tv_sec - c0.tv_sec) + 1e-9 * (double)(c1.tv_nsec - c0.tv_nsec));
	return true;
}

}  // namespace

std::string joint_info_declared(const std::string &vcf_in)
{
	FILE *f = fopen(vcf_in.c_str(), "rb");
	if (!f) return std::string();
	std::string found, line;
	bool more = true;
	while (more && found.empty()) {                                       // the lines in front of the first data line, whatever their length
		line.clear();
		int c;
		while ((c = fgetc(f)) != EOF && c != '\n') line.push_back((char)c);
		more = c != EOF;
		if (!line.empty() && line.back() == '\r') line.pop_back();
		if (line.empty()) continue;
		if (line[0] != '#') break;
		for (const char *key : kJointInfoKeys) if (found.empty() && line.compare(0, 11, "##INFO=<ID=") == 0 && line.compare(11, strlen(key) + 1, std::string(key) + ",") == 0) found = key;
	}
	fclose(f);
	return found;
}

void write_joint_vcf(const std::vector<uint32_t> &pos, const std::vector<ChrLen> &chrlens, const std::vector<JointSample> &samples, const std::string &vcf_in, const std::string &vcf_out, const std::string *vcf_text, const VcfOutput &how,
                     const JointTextRoute &text_route)
{
	for (const JointSample &js : samples)
		if (js.calls.gt.size() != pos.size() || js.calls.gq.size() != pos.size()) throw Error{"sample " + js.name + " has calls for another number of sites than the index has"};
	if (text_route.route != JointText::Host && write_joint_vcf_planned(pos, chrlens, samples, vcf_in, vcf_out, vcf_text, how, text_route)) return;
	const CallBook book(pos, chrlens);
	bool ok = vcf_text != nullptr;
	std::string own;
	if (!vcf_text) own = slurp(vcf_in, ok);
	const std::string &text = vcf_text ? *vcf_text : own;
	if (!ok) throw Error{"Error opening: " + vcf_in + " . You have failed."};
	const std::unique_ptr<VcfSink> out = open_vcf_sink(vcf_out, how);

	const size_t n = samples.size();
	bool declares_gt = false, declares_gq = false;
	auto first_eight = [](Span ln) {
		const char *q = ln.b;
		for (int k = 0; k < 8 && q; k++) { q = (const char *)memchr(q, '\t', (size_t)(ln.e - q)); if (q && k < 7) q++; }
		return Span{ln.b, q ? q : ln.e};
	};
	auto header = [&](const char *&p, const char *end, std::string &dst) {
		while (p < end) {
			const char *at = p;
			const Span ln = next_line(p, end);
			if (ln.size() == 0) continue;
			if (ln.b[0] != '#') { p = at; return; }
			if (ln.size() > 1 && ln.b[1] == '#') {
				dst.append(ln.b, ln.e).push_back('\n');
				const std::string meta(ln.b, ln.e);
				if (meta.find("ID=GT,") != std::string::npos) declares_gt = true;
				else if (meta.find("ID=GQ,") != std::string::npos) declares_gq = true;
			} else {
				if (!declares_gt) dst += kGtDecl;
				if (!declares_gq) dst += kGqDecl;
				if (text_route.info_counts) dst += kJointInfoDecl;
				dst += text_route.prior_line;
				const Span cols = first_eight(ln);
				dst.append(cols.b, cols.e) += "\tFORMAT";
				for (const JointSample &js : samples) { dst.push_back('\t'); dst += js.name; }
				dst.push_back('\n');
			}
		}
	};
	auto line = [&](Span ln, std::string &dst, Scratch &sc) {
		if (count_fields(ln, '\t') < 2) return;
		const Span chrom = field(ln, '\t', 0), ps = field(ln, '\t', 1);
		std::string &key = sc.key;
		key.clear();
		if (chrom.size() == 0 || chrom.b[0] != 'c') key = "chr";
		key.append(chrom.b, chrom.e).push_back('$');
		key.append(ps.b, ps.e);
		const CalledSite *first = book.find(key, sc.hint);
		if (!first) return;
		const CalledSite *last = first + 1;                        // [first, last): the sites of this key, in genome order
		for (const CalledSite *e = CallBook::list_end(sc.hint); last < e && last->local == first->local; last++) {}
		std::string &cols = sc.smp;
		cols.clear();
		bool any = false;
		vg_jt_counts_t shown{0, 0, 0};                             // the line's counts over the calls it shows (../vg_jtext.h)
		for (size_t j = 0; j < n; j++) {
			const SiteCalls &c = samples[j].calls;
			const CalledSite *hit = nullptr;
			for (const CalledSite *q = last; q > first && !hit;) { q--; if (c.gt[q->order] != GT_NONE) hit = q; }
			if (!hit) { cols += "\t./.:."; continue; }
			any = true;
			shown.ns += vg_jt_is_called(c.gt[hit->order]); shown.het += vg_jt_is_het(c.gt[hit->order]); shown.hom += vg_jt_is_hom(c.gt[hit->order]);
			char buf[24];
			snprintf(buf, sizeof buf, "\t%s:%d", gt_text(c.gt[hit->order]), (int)c.gq[hit->order]);
			cols += buf;
		}
		if (!any) return;
		const Span head = first_eight(ln);
		if (text_route.info_counts) {                              // the head with its splice and "\tGT:GQ", by the header's function
			const size_t at = dst.size();
			dst.resize(at + head.size() + VG_JT_INFO_MAX + 6);
			dst.resize(at + vg_jt_head_host((const uint8_t *)head.b, (uint32_t)head.size(), VG_JT_INFO_COUNTS, shown, (uint8_t *)&dst[at]));
		} else dst.append(head.b, head.e) += "\tGT:GQ";
		dst.append(cols).push_back('\n');
	};
	vcf_pass(text, *out, vcf_threads(), header, line);
	out->close();
}

}  // namespace vgh

// jinfo_check.cpp -- the INFO mode of csrc/vg_jtext.h's host loop under AddressSanitizer + UBSan (tests/test_joint_info_cpu.py compiles
// and runs it): every array is a heap array of exactly its size, the text buffer exactly the span's bound in the mode, and the result
// is compared with a naive loop that prints every cell and the tag with snprintf (the frequency by long division a digit at a
// time, not the header's expression).  Heads of every splice kind and of 0 .. 6 tabs, n_samples in
// {1, 63, 64, 65, 129}, one and three threads; with a buffer one byte below the bound the loop must refuse and write nothing.
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "vg_jtext.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n)
{
	rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
	return (uint32_t)((rng_state >> 20) % n);
}

static const int32_t EDGES[] = {0, 9, 10, 99, 100, 999, 1000, 9999, 10000, 16382, 16383, 16384, INT_MAX, -1, INT_MIN};

// AC / AN to six decimals, half up, by long division a digit at a time: seven digits, then the rounding
static std::string naive_af(uint32_t ac, uint32_t an)
{
	uint64_t digits = 0, rem = ac % an;
	for (int k = 0; k < 7; k++) { rem *= 10; digits = digits * 10 + rem / an; rem %= an; }
	uint64_t six = (uint64_t)(ac / an) * 1000000 + digits / 10 + (digits % 10 >= 5 ? 1 : 0);
	char buf[32];
	snprintf(buf, sizeof buf, "%lu.%06lu", (unsigned long)(six / 1000000), (unsigned long)(six % 1000000));
	std::string s = buf;
	while (s.back() == '0') s.pop_back();
	if (s.back() == '.') s.pop_back();
	return s;
}

static std::string naive_head(const std::string &head, uint32_t ns, uint32_t het, uint32_t hom)
{
	size_t tabs = 0, seventh = 0;
	for (size_t i = 0; i < head.size(); i++) if (head[i] == '\t' && ++tabs == 7) seventh = i;
	if (tabs != 7) return head;
	char tag[64];
	snprintf(tag, sizeof tag, "NS=%u;AN=%u;AC=%u;AF=%s", ns, 2 * ns, het + 2 * hom, naive_af(het + 2 * hom, 2 * ns).c_str());
	const std::string info = head.substr(seventh + 1);
	if (info == "." || info.empty()) return head.substr(0, seventh + 1) + tag;
	return head + ";" + tag;
}

static std::string naive(const std::vector<std::unique_ptr<uint8_t[]>> &gt, const std::vector<std::unique_ptr<int32_t[]>> &gq, const uint8_t *heads, const vg_jtext_record *recs, uint64_t n_records, const uint32_t *sites, int info)
{
	std::string out;
	for (uint64_t i = 0; i < n_records; i++) {
		std::string cols;
		uint32_t ns = 0, het = 0, hom = 0;
		for (size_t s = 0; s < gt.size(); s++) {
			int hit = -1;
			for (uint32_t q = 0; q < recs[i].n_sites; q++) if (gt[s] && gt[s][sites[recs[i].site_at + q]]) hit = (int)sites[recs[i].site_at + q];
			if (hit < 0) { cols += "\t./.:."; continue; }
			char buf[32];
			const uint8_t g = gt[s][hit];
			ns++; het += g == 3; hom += g == 2;
			snprintf(buf, sizeof buf, "\t%s:%d", g == 3 ? "0/1" : g == 2 ? "1/1" : "0/0", (int)gq[s][hit]);
			cols += buf;
		}
		if (!ns) continue;
		const std::string head((const char *)heads + recs[i].head_off, recs[i].head_len);
		out += info ? naive_head(head, ns, het, hom) : head;
		out += "\tGT:GQ";
		out += cols;
		out += "\n";
	}
	return out;
}

static std::string make_head(uint64_t i)
{
	static const char *const infos[] = {".", "RS=7;VC=SNV", "", "..", "x.", "DP=0"};
	char buf[160];
	if (i % 7 == 6) {                                                   // 0 .. 6 tabs
		std::string h = "c";
		for (uint64_t t = 0; t < (i / 7) % 7; t++) h += t % 2 ? "\t" : "\t.";
		return h;
	}
	snprintf(buf, sizeof buf, "%u\t%u\trs%u\tA\tC\t.\t.\t%s", 1 + (unsigned)(i % 22), 100 + (unsigned)i, (unsigned)rnd(100000), infos[i % 7]);
	return buf;
}

static int run_case(uint32_t n_samples, uint64_t n_records, int threads, int info)
{
	std::vector<uint32_t> run_len(n_records);
	uint64_t n_refs = 0;
	for (auto &r : run_len) { r = 1 + rnd(4); n_refs += r; }
	const uint64_t n_sites = n_refs + 5;
	std::unique_ptr<uint32_t[]> sites(new uint32_t[n_refs ? n_refs : 1]);
	for (uint64_t i = 0; i < n_refs; i++) sites[i] = (uint32_t)((i * 7919) % n_sites);
	std::unique_ptr<vg_jtext_record[]> recs(new vg_jtext_record[n_records ? n_records : 1]);
	std::string all;
	uint64_t at = 0;
	for (uint64_t i = 0; i < n_records; i++) {
		const std::string h = make_head(i);
		all.append(i % 3, '#');
		recs[i] = vg_jtext_record{all.size(), at, (uint32_t)h.size(), run_len[i]};
		all += h;
		at += run_len[i];
	}
	std::unique_ptr<uint8_t[]> heads(new uint8_t[all.size() ? all.size() : 1]);
	memcpy(heads.get(), all.data(), all.size());
	std::vector<std::unique_ptr<uint8_t[]>> gt(n_samples);
	std::vector<std::unique_ptr<int32_t[]>> gq(n_samples);
	std::vector<const uint8_t *> pg(n_samples);
	std::vector<const int32_t *> pq(n_samples);
	for (uint32_t s = 0; s < n_samples; s++) {
		if (n_samples > 1 && s == n_samples - 1) continue;                  // the last sample was never set
		gt[s].reset(new uint8_t[n_sites]);
		gq[s].reset(new int32_t[n_sites]);
		for (uint64_t i = 0; i < n_sites; i++) {
			gt[s][i] = (uint8_t)(rnd(3) ? rnd(4) : 0);
			gq[s][i] = rnd(2) ? EDGES[rnd(sizeof EDGES / sizeof EDGES[0])] : (int32_t)rnd(100);
		}
		pg[s] = gt[s].get(); pq[s] = gq[s].get();
	}
	for (uint64_t i = n_records / 3; i < n_records / 2; i++)               // a run of dropped records in the middle
		for (uint32_t q = 0; q < recs[i].n_sites; q++) for (uint32_t s = 0; s < n_samples; s++) if (gt[s]) gt[s][sites[recs[i].site_at + q]] = 0;
	const std::string want = naive(gt, gq, heads.get(), recs.get(), n_records, sites.get(), info);
	const uint64_t bound = vg_jt_span_bound_info(recs.get(), n_records, n_samples, info);
	if (bound != vg_jt_span_bound(recs.get(), n_records, n_samples) + (info ? 40 * n_records : 0)) { printf("the bound is not the formula\n"); return 1; }
	uint64_t len = 123, lines = 456;
	{
		std::unique_ptr<uint8_t[]> text(new uint8_t[bound ? bound : 1]);
		if (!vg_jtext_host_run_info(pg.data(), pq.data(), n_samples, heads.get(), recs.get(), n_records, sites.get(), info, threads, text.get(), bound, &len, &lines)) { printf("refused at the bound\n"); return 1; }
		if (len != want.size() || memcmp(text.get(), want.data(), want.size()) != 0) { printf("text differs: %u samples, %lu records, %d threads, mode %d\n", n_samples, (unsigned long)n_records, threads, info); return 1; }
		uint64_t nl = 0;
		for (char c : want) nl += c == '\n';
		if (lines != nl) { printf("line count differs\n"); return 1; }
	}
	// a record alone in a buffer of exactly its own bound: the cells are parked where the longest head piece would end, inside it
	for (uint64_t i = 0; i < n_records; i++) {
		const uint64_t b = vg_jt_bound_info(recs[i].head_len, 1, n_samples, info);
		std::unique_ptr<uint8_t[]> one(new uint8_t[b]);
		const uint64_t n = vg_jt_line_host_info(pg.data(), pq.data(), n_samples, heads.get(), recs[i], sites.get(), info, one.get());
		const vg_jt_counts_t c = vg_jt_counts_host(pg.data(), pq.data(), n_samples, recs[i], sites.get());
		if (n > b || (n == 0) != (c.ns == 0) || c.het + c.hom > c.ns) { printf("record %lu alone: %lu bytes, bound %lu\n", (unsigned long)i, (unsigned long)n, (unsigned long)b); return 1; }
	}
	if (bound) {
		std::unique_ptr<uint8_t[]> small(new uint8_t[bound - 1 ? bound - 1 : 1]);
		len = 123; lines = 456;
		if (vg_jtext_host_run_info(pg.data(), pq.data(), n_samples, heads.get(), recs.get(), n_records, sites.get(), info, threads, small.get(), bound - 1, &len, &lines) || len != 123 || lines != 456) { printf("a buffer below the bound was taken\n"); return 1; }
	}
	return 0;
}

int main()
{
	// the tag through the header's function alone, at the widths where a digit appears or the rounding decides, up to the widest
	const uint32_t ns_of[] = {1, 2, 3, 5, 7, 9, 10, 64, 99, 100, 128, 130, 999, 1000, 5000, 9999, 10000, 16383, 16384};
	for (uint32_t ns : ns_of)
		for (uint32_t het = 0; het <= ns; het += 1 + het / 3)
			for (uint32_t hom = 0; het + hom <= ns; hom += 1 + hom / 2) {
				char got[64] = {0};
				const uint32_t n = vg_jt_tag(ns, het, hom, [&](uint32_t i, uint32_t byte) { if (i < 63) got[i] = (char)byte; });
				char want[64];
				snprintf(want, sizeof want, "NS=%u;AN=%u;AC=%u;AF=%s", ns, 2 * ns, het + 2 * hom, naive_af(het + 2 * hom, 2 * ns).c_str());
				if (n != strlen(want) || n + 1 > VG_JT_INFO_MAX || n != vg_jt_tag_len(ns, het, hom) || strcmp(want, got) != 0) { printf("tag (%u, %u, %u): %s, not %s\n", ns, het, hom, got, want); return 1; }
			}
	const uint32_t widths[] = {1, 63, 64, 65, 129};
	const uint64_t spans[] = {0, 1, 2, 67};
	for (int info : {VG_JT_INFO_COUNTS, VG_JT_INFO_NONE})
		for (uint32_t n : widths)
			for (uint64_t r : spans)
				for (int threads : {1, 3})
					if (run_case(n, r, threads, info)) return 1;
	printf("ok\n");
	return 0;
}

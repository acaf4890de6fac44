// jtext_check.cpp -- the host loop of csrc/vg_jtext.h under AddressSanitizer + UBSan (tests/test_joint_text_cpu.py compiles and runs it):
// every array is a heap array of exactly its size, the text buffer exactly the span's bound, and the result is compared with a naive
// loop that prints every cell with snprintf.  n_samples in {1, 63, 64, 65, 129}, one and three threads; with a buffer one byte
// below the bound the loop must refuse and write nothing (the buffer it gets then is one byte short: a write would be caught).
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

static std::string naive(const std::vector<std::unique_ptr<uint8_t[]>> &gt, const std::vector<std::unique_ptr<int32_t[]>> &gq, const uint8_t *heads, const vg_jtext_record *recs, uint64_t n_records, const uint32_t *sites)
{
	std::string out;
	for (uint64_t i = 0; i < n_records; i++) {
		std::string cols;
		bool any = false;
		for (size_t s = 0; s < gt.size(); s++) {
			int hit = -1;
			for (uint32_t q = 0; q < recs[i].n_sites; q++) if (gt[s] && gt[s][sites[recs[i].site_at + q]]) hit = (int)sites[recs[i].site_at + q];
			if (hit < 0) { cols += "\t./.:."; continue; }
			any = true;
			char buf[32];
			const uint8_t g = gt[s][hit];
			snprintf(buf, sizeof buf, "\t%s:%d", g == 3 ? "0/1" : g == 2 ? "1/1" : "0/0", (int)gq[s][hit]);
			cols += buf;
		}
		if (!any) continue;
		out.append((const char *)heads + recs[i].head_off, recs[i].head_len);
		out += "\tGT:GQ";
		out += cols;
		out += "\n";
	}
	return out;
}

static int run_case(uint32_t n_samples, uint64_t n_records, int threads)
{
	// site runs of 1 .. 4 sites each, taken from a pool in a stride that makes them non-consecutive
	std::vector<uint32_t> run_len(n_records);
	uint64_t n_refs = 0;
	for (auto &r : run_len) { r = 1 + rnd(4); n_refs += r; }
	const uint64_t n_sites = n_refs + 5;
	std::unique_ptr<uint32_t[]> sites(new uint32_t[n_refs ? n_refs : 1]);
	for (uint64_t i = 0; i < n_refs; i++) sites[i] = (uint32_t)((i * 7919) % n_sites);
	std::unique_ptr<vg_jtext_record[]> recs(new vg_jtext_record[n_records ? n_records : 1]);
	uint64_t heads_len = 0, at = 0;
	for (uint64_t i = 0; i < n_records; i++) {
		const uint32_t hl = i % 5 == 0 ? 1 + rnd(60) : 1 + (uint32_t)(i % 5);
		recs[i] = vg_jtext_record{heads_len + (i % 3), at, hl, run_len[i]};
		heads_len += (i % 3) + hl;
		at += run_len[i];
	}
	std::unique_ptr<uint8_t[]> heads(new uint8_t[heads_len ? heads_len : 1]);
	for (uint64_t i = 0; i < heads_len; i++) heads[i] = (uint8_t)(33 + rnd(90));
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
	// a run of dropped records in the middle
	for (uint64_t i = n_records / 3; i < n_records / 2; i++)
		for (uint32_t q = 0; q < recs[i].n_sites; q++) for (uint32_t s = 0; s < n_samples; s++) if (gt[s]) gt[s][sites[recs[i].site_at + q]] = 0;
	const std::string want = naive(gt, gq, heads.get(), recs.get(), n_records, sites.get());
	const uint64_t bound = vg_jt_span_bound(recs.get(), n_records, n_samples);
	uint64_t len = 123, lines = 456;
	{
		std::unique_ptr<uint8_t[]> text(new uint8_t[bound ? bound : 1]);
		if (!vg_jtext_host_run(pg.data(), pq.data(), n_samples, heads.get(), recs.get(), n_records, sites.get(), threads, text.get(), bound, &len, &lines)) { printf("refused at the bound\n"); return 1; }
		if (len != want.size() || memcmp(text.get(), want.data(), want.size()) != 0) { printf("text differs: %u samples, %lu records, %d threads\n", n_samples, (unsigned long)n_records, threads); return 1; }
		uint64_t nl = 0;
		for (char c : want) nl += c == '\n';
		if (lines != nl) { printf("line count differs\n"); return 1; }
	}
	if (bound) {
		std::unique_ptr<uint8_t[]> small(new uint8_t[bound - 1 ? bound - 1 : 1]);
		len = 123; lines = 456;
		if (vg_jtext_host_run(pg.data(), pq.data(), n_samples, heads.get(), recs.get(), n_records, sites.get(), threads, small.get(), bound - 1, &len, &lines) || len != 123 || lines != 456) { printf("a buffer below the bound was taken\n"); return 1; }
	}
	return 0;
}

int main()
{
	// every cell length there is, through the cell function alone
	for (int32_t q : EDGES)
		for (uint32_t g = 0; g < 5; g++) {
			const vg_jt_cell_t c = vg_jt_cell(g, q);
			char want[32], got[17] = {0};
			if (g == 0 || g > 3) snprintf(want, sizeof want, "\t./.:.");
			else snprintf(want, sizeof want, "\t%s:%d", g == 3 ? "0/1" : g == 2 ? "1/1" : "0/0", (int)q);
			for (uint32_t i = 0; i < c.len && i < 16; i++) got[i] = (char)vg_jt_byte(c, i);
			if (c.len != strlen(want) || c.len > VG_JT_CELL_MAX || strcmp(want, got) != 0) { printf("cell (%u, %d): %s, not %s\n", g, (int)q, got, want); return 1; }
		}
	const uint32_t widths[] = {1, 63, 64, 65, 129};
	const uint64_t spans[] = {0, 1, 2, 67};
	for (uint32_t n : widths)
		for (uint64_t r : spans)
			for (int threads : {1, 3})
				if (run_case(n, r, threads)) return 1;
	printf("ok\n");
	return 0;
}

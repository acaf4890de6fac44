// vcfidx_check.cpp -- the host scanner, the builder and the serialiser of csrc/vg_vcfidx.h under AddressSanitizer + UBSan
// (tests/test_vcf_index_cpu.py compiles and runs it).  Seeded VCF-like texts whose lines are mutated (tabs dropped, letters in POS,
// POS 0, an end beyond 2^29, empty fields, empty lines, '#' lines, chromosomes that come back, positions out of order, no final
// newline) are fed three ways -- whole on one thread; at fuzzed cuts, every piece a heap array of exactly its size, on three
// threads; and line by line as one record per line, no runs -- and must end in the same index bytes or the same refusal.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "vg_vcfidx.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n)
{
	rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
	return (uint32_t)((rng_state >> 20) % n);
}

static std::string make_text(uint32_t n_lines, uint32_t mutate_one_in)
{
	std::string t = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\n";
	const char *chroms[] = {"chr1", "chr1_alt", "2", "a_rather_long_chromosome_name_a_rather_long_chromosome_name"};
	uint32_t c = 0, pos = 1;
	for (uint32_t i = 0; i < n_lines; i++) {
		if (rnd(n_lines / 3 + 1) == 0 && c < 3) { c++; pos = 1; }
		pos += rnd(4) == 0 ? rnd(40000) : rnd(30);
		if (pos > (1u << 29) - 200) pos = (1u << 29) - 200;
		std::string ref(1 + (rnd(50) == 0 ? rnd(40000) : rnd(3)), 'A');
		std::string line = std::string(chroms[c]) + "\t" + std::to_string(pos) + "\tid" + std::to_string(i) + "\t" + ref + "\tC\t.\n";
		if (mutate_one_in && rnd(mutate_one_in) == 0) {
			switch (rnd(10)) {
			case 0: line = "\n"; break;
			case 1: line = "#mid-file header\n"; break;
			case 2: line[line.find('\t')] = ' '; break;                                   // one field fewer
			case 3: line = std::string(chroms[c]) + "\t12x\t.\tA\n"; break;
			case 4: line = std::string(chroms[c]) + "\t0\t.\tA\n"; break;
			case 5: line = std::string(chroms[c]) + "\t536870912\t.\tAC\n"; break;
			case 6: line = std::string(chroms[c]) + "\t" + std::to_string(pos) + "\t.\t\tC\n"; break;
			case 7: line = std::string(chroms[0]) + "\t" + std::to_string(pos) + "\t.\tA\n"; break;      // may come back
			case 8: line = std::string(chroms[c]) + "\t" + std::to_string(pos > 50 ? pos - 50 : 1) + "\t.\tA\n"; break;      // may be unsorted
			default: line = std::string(chroms[c]) + "\t\t\t\n"; break;
			}
		}
		t += line;
	}
	if (rnd(2)) t.pop_back();
	return t;
}

// blocks of B text bytes as 26-byte BGZF blocks without payload (the handle reads BSIZE and ISIZE alone), then the marker
static void feed_blocks(VgVcfIdx &ix, uint64_t text_bytes)
{
	for (uint64_t at = 0; at < text_bytes + 1; at += ix.B) {
		const uint32_t isize = at >= text_bytes ? 0 : (uint32_t)std::min<uint64_t>(ix.B, text_bytes - at);
		std::unique_ptr<uint8_t[]> z(new uint8_t[26]());
		z[0] = 0x1f; z[1] = 0x8b; z[12] = 'B'; z[13] = 'C'; z[16] = 25; z[17] = 0;
		memcpy(z.get() + 22, &isize, 4);
		if (!ix.feed_bgzf(z.get(), 26)) { printf("FAIL: a block was refused\n"); exit(1); }
		if (!isize) break;
	}
}

struct Result { int what; uint32_t err; uint64_t err_at; std::vector<uint8_t> raw; };
static Result finish(VgVcfIdx &ix, uint64_t text_bytes)
{
	feed_blocks(ix, text_bytes);
	Result r;
	r.what = ix.serialise(r.raw);
	r.err = ix.err; r.err_at = ix.err_at;
	if (r.what == 0 && r.raw.size() != ix.raw_bytes()) { printf("FAIL: raw_bytes() is not the serialiser's size\n"); exit(1); }
	return r;
}
static bool same(const Result &a, const Result &b) { return a.what == b.what && a.err == b.err && a.err_at == b.err_at && a.raw == b.raw; }

int main()
{
	unsigned refused = 0, indexed = 0;
	for (uint32_t round = 0; round < 60; round++) {
		const uint32_t B = round % 3 == 0 ? 65280 : round % 3 == 1 ? 97 : 1 + rnd(5000);
		const std::string text = make_text(50 + rnd(3000), round % 4 == 0 ? 0 : 200 + rnd(3000));
		const uint64_t n = text.size();
		VgVcfIdx whole;
		whole.B = B;
		{
			std::unique_ptr<uint8_t[]> p(new uint8_t[n]);
			memcpy(p.get(), text.data(), n);
			whole.feed_host(p.get(), n, 1);
		}
		const Result a = finish(whole, n);
		if (a.what == 2) { printf("FAIL: round %u: block count\n", round); return 1; }
		VgVcfIdx cut;
		cut.B = B;
		for (uint64_t at = 0; at < n;) {
			const uint64_t k = std::min<uint64_t>(n - at, rnd(3) == 0 ? 1 + rnd(7) : rnd(3) == 0 ? 1 + rnd(200000) : 1 + rnd(3000));
			std::unique_ptr<uint8_t[]> p(new uint8_t[k]);
			memcpy(p.get(), text.data() + at, k);
			cut.feed_host(p.get(), k, 3);
			at += k;
		}
		const Result b = finish(cut, n);
		VgVcfIdx lines;
		lines.B = B;
		for (uint64_t at = 0; at < n;) {
			const char *q = (const char *)memchr(text.data() + at, '\n', n - at);
			const uint64_t e = q ? (uint64_t)(q - text.data()) : n, next = q ? e + 1 : n;
			std::unique_ptr<uint8_t[]> p(new uint8_t[e - at + 1]);
			memcpy(p.get(), text.data() + at, e - at);
			const vg_vi_line l = vg_vi_parse(p.get(), e - at);
			if (l.kind != VG_VI_SKIP) lines.replay(vg_vi_rec{at, next, 0, 0, l.beg, l.end, l.beg, l.clen, l.kind, 0}, p.get());
			at = next;
		}
		lines.fed = n;
		const Result c = finish(lines, n);
		if (!same(a, b) || !same(a, c)) {
			printf("FAIL: round %u (block %u, %lu bytes): whole %d/%u@%lu/%zu, cuts %d/%u@%lu/%zu, lines %d/%u@%lu/%zu\n", round, B, (unsigned long)n, a.what, a.err, (unsigned long)a.err_at, a.raw.size(), b.what, b.err,
			       (unsigned long)b.err_at, b.raw.size(), c.what, c.err, (unsigned long)c.err_at, c.raw.size());
			return 1;
		}
		(a.what ? refused : indexed)++;
	}
	if (!refused || !indexed) { printf("FAIL: %u refused, %u indexed: the texts do not cover both\n", refused, indexed); return 1; }
	printf("ok: %u indexed, %u refused\n", indexed, refused);
	return 0;
}

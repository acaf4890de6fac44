// Stand-alone fuzz driver of the dynamic mode of the host build of the deflate core (vargeno_amd/csrc/vg_deflate.h); built by
// tests/test_deflate_dynamic_cpu.py with -fsanitize=address,undefined and run directly.
//
//   deflate_dyn_fuzz [texts [seed]]
//
// Seeded texts and a fixed list of edge cases are cut into blocks and compressed block by block through vg_bgzf_deflate_block_host_dyn
// into exactly-sized heap buffers (text, token buffer of n words, slot, the block's worst case) with the shared state poisoned.
// Every block is read back by vg_inflate.h's host core and compared with its text; it is never larger than the fixed mode's block,
// and the same bytes where it takes the stored or the fixed form.  A decoder of its own (bit by bit, canonical codes built here)
// walks every dynamic block and measures each token's bits: the run must have met a token of more than 32 bits, or the window's
// three-word straddle went untested.  The code-length builder is driven directly on Fibonacci counts, which a Huffman tree built
// here shows to need the limit.
#include "../vargeno_amd/csrc/vg_deflate.h"

#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <memory>
#include <vector>

static uint64_t rng_state;
static uint64_t rnd()
{
	rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;     // xorshift64
	return rng_state;
}

static long n_form[3] = {0, 0, 0};                                    // stored, fixed, dynamic
static uint32_t widest_token = 0;
static uint64_t text_bytes = 0, file_bytes = 0;

// ---- this file's own reader of a dynamic block: canonical codes decoded bit by bit ----
struct Bits {
	const uint8_t *p; size_t n; size_t at = 0;
	bool bad = false;
	uint32_t get(uint32_t k) { uint32_t v = 0; for (uint32_t i = 0; i < k; i++) { if (at >= 8 * n) { bad = true; return 0; } v |= (uint32_t)(p[at >> 3] >> (at & 7) & 1u) << i; at++; } return v; }
};
struct Canon {
	std::vector<uint32_t> count = std::vector<uint32_t>(16, 0), sym;
	explicit Canon(const std::vector<uint8_t> &len)
	{
		for (uint8_t l : len) count[l]++;
		count[0] = 0;
		for (uint32_t l = 1; l < 16; l++) for (uint32_t s = 0; s < len.size(); s++) if (len[s] == l) sym.push_back(s);
	}
	int decode(Bits &b) const
	{
		uint32_t code = 0, first = 0, index = 0;
		for (uint32_t l = 1; l < 16; l++) {
			code |= b.get(1);
			if (b.bad) return -1;
			if (code - first < count[l]) return (int)sym[index + (code - first)];
			index += count[l]; first = (first + count[l]) << 1; code <<= 1;
		}
		return -1;
	}
};
// walks a BTYPE 2 payload of a block of n text bytes; 0 when it is well formed and has n bytes of tokens; notes the widest token
static int walk_dynamic(const uint8_t *in, uint32_t in_len, uint32_t n)
{
	static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
	Bits b{in, in_len};
	if (b.get(3) != 5) return 1;
	const uint32_t hlit = b.get(5) + 257, hdist = b.get(5) + 1, hclen = b.get(4) + 4;
	if (hlit > 286 || hdist > 30) return 2;
	std::vector<uint8_t> cl(19, 0);
	for (uint32_t i = 0; i < hclen; i++) cl[order[i]] = (uint8_t)b.get(3);
	if (hclen > 4 && cl[order[hclen - 1]] == 0) return 3;             // HCLEN is trimmed
	Canon cc(cl);
	std::vector<uint8_t> lens;
	while (lens.size() < hlit + hdist) {
		const int s = cc.decode(b);
		if (s < 0) return 4;
		if (s < 16) lens.push_back((uint8_t)s);
		else if (s == 16) { if (lens.empty()) return 5; const uint8_t v = lens.back(); for (uint32_t r = 3 + b.get(2); r; r--) lens.push_back(v); }
		else for (uint32_t r = s == 17 ? 3 + b.get(3) : 11 + b.get(7); r; r--) lens.push_back(0);
	}
	if (lens.size() != hlit + hdist) return 6;
	if (hlit > 257 && lens[hlit - 1] == 0) return 7;                  // HLIT and HDIST are trimmed
	if (hdist > 1 && lens[hlit + hdist - 1] == 0) return 8;
	std::vector<uint8_t> ll(lens.begin(), lens.begin() + hlit), dl(lens.begin() + hlit, lens.end());
	for (const std::vector<uint8_t> *v : {&ll, &dl}) {                // complete, and at least two codes
		uint64_t kraft = 0; uint32_t used = 0;
		for (uint8_t l : *v) if (l) { kraft += 1ull << (15 - l); used++; }
		if (kraft != 1ull << 15 || used < 2) return 9;
	}
	Canon lc(ll), dc(dl);
	uint32_t out = 0;
	for (;;) {
		const size_t at0 = b.at;
		const int s = lc.decode(b);
		if (s < 0) return 10;
		if (s == 256) break;
		if (s < 256) { out++; continue; }
		static const uint16_t lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
		static const uint8_t lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
		if (s > 285) return 11;
		const uint32_t len = lbase[s - 257] + b.get(lext[s - 257]);
		const int d = dc.decode(b);
		if (d < 0 || d > 29) return 12;
		const uint32_t de = d < 4 ? 0 : (uint32_t)d / 2 - 1, dbase = d < 4 ? (uint32_t)d + 1 : ((2u + (d & 1)) << de) + 1;
		const uint32_t dist = dbase + b.get(de);
		if (dist > out || dist > 32768) return 13;
		out += len;
		widest_token = std::max<uint32_t>(widest_token, (uint32_t)(b.at - at0));
	}
	if (b.bad || out != n || (b.at + 7) / 8 != in_len) return 14;
	return 0;
}

// one block with exactly-sized heap buffers; 0 when it reads back as its text
static int one_block(const uint8_t *text, uint32_t n)
{
	uint8_t *tb = (uint8_t *)malloc(n);
	memcpy(tb, text, n);
	const uint32_t worst = n + 5 + VG_BGZF_HEADER + VG_BGZF_TRAILER;
	uint8_t *dst = (uint8_t *)malloc(worst), *fix = (uint8_t *)malloc(worst);
	uint32_t *slot = (uint32_t *)malloc(n + VG_DEF_SLACK), *tok = (uint32_t *)malloc(4 * (size_t)n);
	std::unique_ptr<VgDefDynShared> sh(new VgDefDynShared);
	std::unique_ptr<VgDefShared> shf(new VgDefShared);
	memset(sh.get(), 0xa5, sizeof(VgDefDynShared));                   // (the core must set up what it reads)
	memset(shf.get(), 0xa5, sizeof(VgDefShared));
	memset(tok, 0xa5, 4 * (size_t)n);
	const uint32_t total = vg_bgzf_deflate_block_host_dyn(tb, n, dst, *sh, slot, tok);
	const uint32_t total_fixed = vg_bgzf_deflate_block_host(tb, n, fix, *shf, slot);
	int bad = 0;
	vg_bgzf_block b;
	if (total > worst || total > 65536) { fprintf(stderr, "block of %u text bytes takes %u\n", n, total); bad = 1; }
	else if (total > total_fixed) { fprintf(stderr, "block of %u text bytes: %u in dynamic mode, %u in fixed mode\n", n, total, total_fixed); bad = 1; }
	else if (vg_bgzf_header(dst, total, &b) != 0 || b.in_off != VG_BGZF_HEADER || b.in_off + b.in_len + VG_BGZF_TRAILER != total) { fprintf(stderr, "header of a %u-byte block does not parse\n", n); bad = 1; }
	else if (b.isize != n) { fprintf(stderr, "trailer of a %u-byte block: ISIZE %u\n", n, b.isize); bad = 1; }
	else {
		uint8_t *in = (uint8_t *)malloc(b.in_len), *back = (uint8_t *)malloc(n);
		memcpy(in, dst + b.in_off, b.in_len);
		const int rc = vg_inflate_block_host(in, b.in_len, back, n, b.crc);
		if (rc != VG_INF_OK) { fprintf(stderr, "block of %u text bytes does not inflate: %s\n", n, vg_inflate_strerror(rc)); bad = 1; }
		else if (memcmp(back, text, n) != 0) { fprintf(stderr, "block of %u text bytes inflates to other bytes\n", n); bad = 1; }
		const uint32_t form = (in[0] >> 1) & 3u;
		if (form > 2 || !(in[0] & 1u)) { fprintf(stderr, "first byte %02x\n", in[0]); bad = 1; }
		else {
			n_form[form]++;
			if (form == 0 && b.in_len != n + 5) { fprintf(stderr, "stored block of %u bytes with a payload of %u\n", n, b.in_len); bad = 1; }
			if (form != 0 && b.in_len >= n) { fprintf(stderr, "coded block of %u bytes with a payload of %u\n", n, b.in_len); bad = 1; }
			if (form != 0 && (sh->t.form != form || (sh->t.bits + 7) / 8 != b.in_len)) { fprintf(stderr, "block of %u bytes: the plan said form %u, %u bits; the payload has form %u, %u bytes\n", n, sh->t.form, sh->t.bits, form, b.in_len); bad = 1; }
			if (form != 2 && (total != total_fixed || memcmp(dst, fix, total) != 0)) { fprintf(stderr, "block of %u bytes in form %u is not the fixed mode's block\n", n, form); bad = 1; }
			if (form == 2) { const int w = walk_dynamic(in, b.in_len, n); if (w) { fprintf(stderr, "dynamic block of %u bytes: this file's reader stops with %d\n", n, w); bad = 1; } }
		}
		free(in); free(back);
	}
	text_bytes += n; file_bytes += total;
	free(tb); free(dst); free(fix); free(slot); free(tok);
	return bad;
}

static int whole_text(const std::vector<uint8_t> &t, uint32_t block)
{
	for (size_t at = 0; at < t.size(); at += block)
		if (one_block(t.data() + at, (uint32_t)std::min<size_t>(block, t.size() - at))) return 1;
	return 0;
}

static void draw_text(std::vector<uint8_t> &t)
{
	t.clear();
	const size_t want = 1 + rnd() % 140000;
	const unsigned alphabet = 1u + (unsigned)(rnd() % 3 == 0 ? 255 : rnd() % 20);
	while (t.size() < want) {
		const unsigned kind = (unsigned)(rnd() % 6);
		if (kind == 0 || t.empty()) { const size_t n = 1 + rnd() % 300; for (size_t i = 0; i < n; i++) t.push_back((uint8_t)(rnd() % alphabet + (alphabet < 200 ? 60 : 0))); }     // literals
		else if (kind == 1) { const size_t n = 1 + rnd() % 700; const uint8_t c = (uint8_t)rnd(); t.insert(t.end(), n, c); }                                                   // a run
		else if (kind == 2) { const size_t per = 2 + rnd() % 6, n = 1 + rnd() % 900, from = t.size(); for (size_t i = 0; i < n; i++) t.push_back(i < per ? (uint8_t)rnd() : t[from + i % per]); }
		else {
			size_t dist = kind == 3 ? 1 + rnd() % 64 : kind == 4 ? 1 + rnd() % t.size() : 32768 - 2 + rnd() % 5;      // a copy: near, anywhere, or around the window's edge
			if (dist > t.size()) dist = t.size();
			const size_t n = 3 + rnd() % 400, from = t.size() - dist;
			for (size_t i = 0; i < n; i++) t.push_back(t[from + i]);
		}
	}
	t.resize(want);
}

// A block with one match of length 227 or more at a distance above 16 384 among many short near matches: its length and distance
// symbols are rare, so their codes are long, and both carry the most extra bits -- the token of more than 32 bits.
static void wide_token_text(std::vector<uint8_t> &t)
{
	t.clear();
	for (uint32_t i = 0; i < 240; i++) t.push_back((uint8_t)(128 + rnd() % 128));             // the far match's source: bytes the rest never uses
	while (t.size() < 30000) { const uint32_t w = (uint32_t)(rnd() % 16); for (uint32_t i = 0; i < 6; i++) t.push_back((uint8_t)("ACGTNacgtn01.|/\t"[(w + i * 5) % 16])); }
	for (uint32_t i = 0; i < 240; i++) t.push_back(t[i]);
	while (t.size() < 60000) { const uint32_t w = (uint32_t)(rnd() % 16); for (uint32_t i = 0; i < 6; i++) t.push_back((uint8_t)("ACGTNacgtn01.|/\t"[(w + i * 5) % 16])); }
}

// ---- the code-length builder alone ----
static uint32_t huffman_depth(const std::vector<uint32_t> &freq, uint64_t *cost)     // an unlimited Huffman tree, built here: its depth and cost
{
	struct Node { uint64_t w; uint32_t depth_below; uint64_t leaves_cost; };
	std::vector<Node> q;
	for (uint32_t f : freq) if (f) q.push_back({f, 0, 0});
	while (q.size() > 1) {
		std::sort(q.begin(), q.end(), [](const Node &a, const Node &b) { return a.w > b.w; });
		const Node a = q.back(); q.pop_back();
		const Node b = q.back(); q.pop_back();
		q.push_back({a.w + b.w, std::max(a.depth_below, b.depth_below) + 1, a.leaves_cost + b.leaves_cost + a.w + b.w});
	}
	*cost = q[0].leaves_cost;
	return q[0].depth_below;
}
static int check_lengths(const std::vector<uint32_t> &freq, uint32_t limit, bool must_need_limit)
{
	const uint32_t n = (uint32_t)freq.size();
	uint32_t *f = (uint32_t *)malloc(4 * n);
	uint8_t *len = (uint8_t *)malloc(n);
	memcpy(f, freq.data(), 4 * n);
	memset(len, 0xa5, n);
	std::unique_ptr<VgDefLenScratch> sc(new VgDefLenScratch);
	memset(sc.get(), 0xa5, sizeof(VgDefLenScratch));
	DefHostIO io;
	vg_def_code_lengths(io, f, n, limit, len, *sc);
	uint64_t kraft = 0, cost = 0, best = 0;
	uint32_t most = 0;
	int bad = 0;
	for (uint32_t s = 0; s < n; s++) {
		if ((len[s] != 0) != (freq[s] != 0)) bad = 1;
		if (len[s]) { kraft += 1ull << (15 - len[s]); most = std::max<uint32_t>(most, len[s]); cost += (uint64_t)freq[s] * len[s]; }
	}
	const uint32_t depth = huffman_depth(freq, &best);
	if (kraft != 1ull << 15 || most > limit || cost < best || (depth <= limit && cost != best)) bad = 1;
	if (must_need_limit && depth <= limit) { fprintf(stderr, "a histogram meant to need the limit %u has depth %u\n", limit, depth); bad = 1; }
	if (bad) fprintf(stderr, "code lengths of %u symbols at limit %u: Kraft %llu / 32768, longest %u, cost %llu against %llu at depth %u\n", n, limit, (unsigned long long)kraft, most, (unsigned long long)cost, (unsigned long long)best, depth);
	free(f); free(len);
	return bad;
}

int main(int argc, char **argv)
{
	const long n_texts = argc > 1 ? atol(argv[1]) : 300;
	rng_state = argc > 2 ? strtoull(argv[2], nullptr, 10) | 1u : 0x9e3779b97f4a7c15ull;
	static const uint32_t blocks[] = {65280, 1, 7, 311, 4096, 65280, 64, 65, 63, 258, 259, 32768, 32769, 65279};
	int bad = 0;
	std::vector<uint8_t> t;
	// the builder: Fibonacci counts over 22 symbols and as far as 32 bits hold their sum (44 of them, the other 242 symbols at 1)
	{
		std::vector<uint32_t> fib22, fib286(286, 1);
		uint32_t a = 1, b = 1;
		for (uint32_t i = 0; i < 44; i++) { if (i < 22) fib22.push_back(a); fib286[(i * 131) % 286] = a; const uint32_t c = a + b; a = b; b = c; }
		for (uint32_t limit : {7u, 15u}) { bad |= check_lengths(fib22, limit, true); }
		bad |= check_lengths(fib286, 15, true);
		std::vector<uint32_t> h(19);
		for (int round = 0; round < 200 && !bad; round++) {
			h.assign(round % 2 ? 19 : 286, 0);
			for (uint32_t &x : h) x = rnd() % 3 == 0 ? 0 : (uint32_t)(rnd() % (1u << (rnd() % 20))) ;
			h[0] += 1; h[h.size() - 1] += 2;                          // (two in use at least)
			bad |= check_lengths(h, round % 2 ? 7 : 15, false);
		}
	}
	// the edge cases of the fixed mode's driver, and those of this mode
	{
		t.assign(131072, 'I');
		for (uint32_t b : {65280u, 258u, 259u, 260u, 64u, 65u, 4096u}) bad |= whole_text(t, b);
		for (unsigned per : {2u, 3u, 5u}) { t.clear(); for (size_t i = 0; i < 70000; i++) t.push_back((uint8_t)("ACGTN"[i % per])); bad |= whole_text(t, 65280); bad |= whole_text(t, 311); }
		for (uint32_t dist : {32768u, 32769u}) {
			t.clear();
			for (uint32_t i = 0; i < 300; i++) t.push_back((uint8_t)rnd());
			while (t.size() < dist) t.push_back('\n');
			for (uint32_t i = 0; i < 300; i++) t.push_back(t[i]);
			while (t.size() < 65280) t.push_back('\n');
			bad |= whole_text(t, 65280);
		}
		t.clear();
		for (uint32_t i = 0; i < 5000; i++) t.push_back((uint8_t)(rnd() % 4 + 'A'));
		for (uint32_t i = 0; i < 200; i++) t.push_back(t[1000 + i]);                  // ends the block
		bad |= whole_text(t, 65280);
		t.clear();
		for (uint32_t i = 0; i < 65280; i++) t.push_back((uint8_t)rnd());             // noise: stored
		bad |= whole_text(t, 65280);
		for (uint32_t n = 1; n <= 70 && !bad; n++) { t.assign(n, 'a'); bad |= whole_text(t, 65280); }
		t.clear();
		for (uint32_t i = 0; i < 256; i++) t.push_back((uint8_t)(i * 167 + 13));      // 256 distinct bytes: no match at all
		bad |= whole_text(t, 65280);
		wide_token_text(t);
		const uint32_t before = widest_token;
		bad |= whole_text(t, 65280);
		if (widest_token <= 32 || widest_token <= before) { fprintf(stderr, "the block built for it holds no token of more than 32 bits (widest %u)\n", widest_token); bad = 1; }
	}
	for (long i = 0; i < n_texts && !bad; i++) {
		draw_text(t);
		const uint32_t block = blocks[rnd() % (sizeof blocks / sizeof blocks[0])];
		if (block < 64 && t.size() > 4000) t.resize(4000);                           // (tiny blocks: each costs a set of heap buffers)
		bad |= whole_text(t, block);
	}
	if (n_form[2] == 0 || n_form[0] == 0) { fprintf(stderr, "no dynamic or no stored block met\n"); bad = 1; }
	printf("deflate_dyn_fuzz: %ld texts, %ld dynamic, %ld fixed and %ld stored blocks, widest token %u bits, %llu text bytes in %llu\n%s\n", n_texts, n_form[2], n_form[1], n_form[0], widest_token,
	       (unsigned long long)text_bytes, (unsigned long long)file_bytes, bad ? "FAILED" : "ok");
	return bad ? 1 : 0;
}

// Stand-alone fuzz driver of the host build of the deflate core (vargeno_amd/csrc/vg_deflate.h); built by tests/test_deflate_cpu.py
// with -fsanitize=address,undefined and run directly.
//
//   deflate_fuzz [texts [seed]]
//
// `texts` seeded texts -- mixtures of literal runs, copies at drawn distances (the window's edge among them), short periods, long
// runs -- and a fixed list of edge cases are cut into blocks of a drawn length and compressed block by block through the host
// policy into exactly-sized heap buffers (the sanitizer sees any byte touched outside the text, the slot or the block's worst
// case).  Every block is then read back by vg_inflate.h's host core and compared with its text; its header fields are checked, and
// its CRC32 is recomputed here bit by bit, not with the core's tables.
#include "../vargeno_amd/csrc/vg_deflate.h"

#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <vector>

static uint32_t crc_bitwise(const uint8_t *p, size_t n)
{
	uint32_t c = 0xffffffffu;
	for (size_t i = 0; i < n; i++) {
		c ^= p[i];
		for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ 0xedb88320u : c >> 1;
	}
	return ~c;
}

static uint64_t rng_state;
static uint64_t rnd()
{
	rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;     // xorshift64
	return rng_state;
}

static long n_stored = 0, n_coded = 0;
static uint64_t text_bytes = 0, file_bytes = 0;

// one block with exactly-sized heap buffers; 0 when it reads back as its text
static int one_block(const uint8_t *text, uint32_t n)
{
	uint8_t *tb = (uint8_t *)malloc(n);
	memcpy(tb, text, n);
	uint8_t *dst = (uint8_t *)malloc(n + 5 + VG_BGZF_HEADER + VG_BGZF_TRAILER);
	uint32_t *slot = (uint32_t *)malloc(n + VG_DEF_SLACK);
	std::unique_ptr<VgDefShared> sh(new VgDefShared);
	memset(sh.get(), 0xa5, sizeof(VgDefShared));                      // (the core must set up what it reads)
	const uint32_t total = vg_bgzf_deflate_block_host(tb, n, dst, *sh, slot);
	int bad = 0;
	vg_bgzf_block b;
	if (total > n + 5 + VG_BGZF_HEADER + VG_BGZF_TRAILER || total > 65536) { fprintf(stderr, "block of %u text bytes takes %u\n", n, total); bad = 1; }
	else if (vg_bgzf_header(dst, total, &b) != 0 || b.in_off != VG_BGZF_HEADER || b.in_off + b.in_len + VG_BGZF_TRAILER != total) { fprintf(stderr, "header of a %u-byte block does not parse\n", n); bad = 1; }
	else if (b.isize != n || b.crc != crc_bitwise(text, n)) { fprintf(stderr, "trailer of a %u-byte block: ISIZE %u, CRC %08x\n", n, b.isize, b.crc); bad = 1; }
	else {
		static const uint8_t fixed12[12] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0};
		if (memcmp(dst, fixed12, 12) != 0) { fprintf(stderr, "the 12 fixed header bytes differ\n"); bad = 1; }
		uint8_t *in = (uint8_t *)malloc(b.in_len), *back = (uint8_t *)malloc(n);
		memcpy(in, dst + b.in_off, b.in_len);
		const int rc = vg_inflate_block_host(in, b.in_len, back, n, b.crc);
		if (rc != VG_INF_OK) { fprintf(stderr, "block of %u text bytes does not inflate: %s\n", n, vg_inflate_strerror(rc)); bad = 1; }
		else if (memcmp(back, text, n) != 0) { fprintf(stderr, "block of %u text bytes inflates to other bytes\n", n); bad = 1; }
		if ((in[0] & 6u) == 0) { n_stored++; if (b.in_len != n + 5) { fprintf(stderr, "stored block of %u bytes with a payload of %u\n", n, b.in_len); bad = 1; } }
		else { n_coded++; if (b.in_len >= n) { fprintf(stderr, "coded block of %u bytes with a payload of %u\n", n, b.in_len); bad = 1; } }
		free(in); free(back);
	}
	text_bytes += n; file_bytes += total;
	free(tb); free(dst); free(slot);
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
			// a copy: near, anywhere, or around the window's edge
			size_t dist = kind == 3 ? 1 + rnd() % 64 : kind == 4 ? 1 + rnd() % t.size() : 32768 - 2 + rnd() % 5;
			if (dist > t.size()) dist = t.size();
			const size_t n = 3 + rnd() % 400, from = t.size() - dist;
			for (size_t i = 0; i < n; i++) t.push_back(t[from + i]);
		}
	}
	t.resize(want);
}

int main(int argc, char **argv)
{
	const long n_texts = argc > 1 ? atol(argv[1]) : 300;
	rng_state = argc > 2 ? strtoull(argv[2], nullptr, 10) | 1u : 0x9e3779b97f4a7c15ull;
	static const uint32_t blocks[] = {65280, 1, 7, 311, 4096, 65280, 64, 65, 63, 258, 259, 32768, 32769, 65279};
	int bad = 0;
	std::vector<uint8_t> t;
	// the edge cases: runs (distance 1, length-258 chains), short periods, repeats at the window's edge, a match to the last byte
	{
		t.assign(131072, 'I');
		for (uint32_t b : {65280u, 258u, 259u, 260u, 64u, 65u, 4096u}) bad |= whole_text(t, b);
		for (unsigned per : {2u, 3u, 5u}) { t.clear(); for (size_t i = 0; i < 70000; i++) t.push_back((uint8_t)("ACGTN"[i % per])); bad |= whole_text(t, 65280); bad |= whole_text(t, 311); }
		for (uint32_t dist : {32768u, 32769u}) {
			t.clear();
			for (uint32_t i = 0; i < dist; i++) t.push_back((uint8_t)rnd());
			for (uint32_t i = 0; i < 300; i++) t.push_back(t[i]);
			while (t.size() < 65280) t.push_back((uint8_t)rnd());
			bad |= whole_text(t, 65280);
		}
		t.clear();
		for (uint32_t i = 0; i < 5000; i++) t.push_back((uint8_t)(rnd() % 4 + 'A'));
		for (uint32_t i = 0; i < 200; i++) t.push_back(t[1000 + i]);                  // ends the block
		bad |= whole_text(t, 65280);
		for (uint32_t run : {258u, 259u}) { t.clear(); for (int k = 0; k < 3; k++) { for (int i = 0; i < 100; i++) t.push_back((uint8_t)rnd()); t.insert(t.end(), run, 'x'); } bad |= whole_text(t, 65280); }
		t.clear();
		for (uint32_t i = 0; i < 65280; i++) t.push_back((uint8_t)rnd());             // noise: stored
		bad |= whole_text(t, 65280);
		for (uint32_t n = 1; n <= 70 && !bad; n++) { t.assign(n, 'a'); bad |= whole_text(t, 65280); }
	}
	for (long i = 0; i < n_texts && !bad; i++) {
		draw_text(t);
		const uint32_t block = blocks[rnd() % (sizeof blocks / sizeof blocks[0])];
		if (block < 64 && t.size() > 4000) t.resize(4000);                           // (tiny blocks: each costs a set of heap buffers)
		bad |= whole_text(t, block);
	}
	printf("deflate_fuzz: %ld texts, %ld coded and %ld stored blocks, %llu text bytes in %llu\n%s\n", n_texts, n_coded, n_stored, (unsigned long long)text_bytes, (unsigned long long)file_bytes, bad ? "FAILED" : "ok");
	return bad ? 1 : 0;
}

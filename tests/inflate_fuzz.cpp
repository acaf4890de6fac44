// Stand-alone fuzz driver of the host build of the inflate core (vargeno_amd/csrc/vg_inflate.h); built by tests/test_bgzf_cpu.py
// with -fsanitize=address,undefined and run directly.
//
//   inflate_fuzz FILE.bgzf [mutations [seed]]
//
// Every block of the (valid) file is inflated once unchanged: it must succeed.  Then `mutations` seeded mutations -- bit flips,
// truncations, length-field edits -- of randomly chosen blocks go through vg_inflate_block_host with exactly-sized heap buffers
// (the sanitizer sees any byte touched outside [in, in + len) or [out, out + isize)).  Passes when every call returns and its
// status is an error or the output has the expected CRC (recomputed here bit by bit, not with the core's tables).
#include "../vargeno_amd/csrc/vg_inflate.h"

#include <stdio.h>
#include <stdlib.h>

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

// one call with exactly-sized heap buffers; returns the status, checks an accepted output
static int run(const uint8_t *in, uint32_t len, uint32_t isize, uint32_t crc, int *bad)
{
	uint8_t *ib = (uint8_t *)malloc(len ? len : 1), *ob = (uint8_t *)malloc(isize && isize <= VG_BGZF_MAX_ISIZE ? isize : 1);
	if (len) memcpy(ib, in, len);
	const int rc = vg_inflate_block_host(len ? ib : ib + 1, len, ob, isize, crc);           // (len == 0: a pointer with no byte behind it)
	if (rc == VG_INF_OK) {
		if (crc_bitwise(ob, isize) != crc) { fprintf(stderr, "accepted an output with another CRC\n"); *bad = 1; }
		uint32_t x = 0;
		for (uint32_t l = 0; l < 64; l++) x ^= vg_crc32_share(vg_crc_tab_host(), ob, isize, l, 64);
		if (x != crc) { fprintf(stderr, "the 64 lanes' CRC shares do not add up\n"); *bad = 1; }
	}
	free(ib); free(ob);
	return rc;
}

int main(int argc, char **argv)
{
	if (argc < 2) { fprintf(stderr, "usage: inflate_fuzz FILE.bgzf [mutations [seed]]\n"); return 2; }
	const long n_mut = argc > 2 ? atol(argv[2]) : 20000;
	rng_state = argc > 3 ? strtoull(argv[3], nullptr, 10) | 1u : 0x9e3779b97f4a7c15ull;
	FILE *f = fopen(argv[1], "rb");
	if (!f) { perror(argv[1]); return 2; }
	std::vector<uint8_t> file;
	uint8_t buf[65536];
	for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) file.insert(file.end(), buf, buf + n);
	fclose(f);
	std::vector<vg_bgzf_block> blocks;
	uint64_t tail = 0, bad_off = 0;
	if (vg_bgzf_scan(file.data(), file.size(), 0, 0, blocks, &tail, &bad_off) || tail || blocks.empty()) { fprintf(stderr, "not a whole BGZF file\n"); return 2; }
	int bad = 0;
	for (const vg_bgzf_block &b : blocks)
		if (run(file.data() + b.in_off, b.in_len, b.isize, b.crc, &bad) != VG_INF_OK) { fprintf(stderr, "valid block at %llu refused\n", (unsigned long long)b.comp_off); bad = 1; }
	long by_status[16] = {0};
	std::vector<uint8_t> m;
	for (long i = 0; i < n_mut && !bad; i++) {
		const vg_bgzf_block &b = blocks[rnd() % blocks.size()];
		m.assign(file.data() + b.in_off, file.data() + b.in_off + b.in_len);
		uint32_t isize = b.isize, crc = b.crc;
		const unsigned kind = (unsigned)(rnd() % 8);
		if (kind < 3 && !m.empty()) { const unsigned flips = 1 + (unsigned)(rnd() % 3); for (unsigned k = 0; k < flips; k++) m[rnd() % m.size()] ^= (uint8_t)(1u << (rnd() % 8)); }
		else if (kind == 3 && !m.empty()) { const uint64_t at = rnd() % m.size(); m[at] ^= (uint8_t)(1u << (rnd() % 8)); }                    // a flip, mostly in the header: at small offsets
		else if (kind == 4) m.resize(m.empty() ? 0 : rnd() % m.size());                                  // truncation
		else if (kind == 5) isize = (rnd() & 1u) ? isize + 1 + (uint32_t)(rnd() % 3) : (uint32_t)(rnd() % (isize + 1));   // ISIZE edits
		else if (kind == 6 && m.size() >= 2) { const uint64_t at = rnd() % (m.size() - 1) % 64; m[at] = (uint8_t)rnd(); m[at + 1] = (uint8_t)rnd(); }   // a 16-bit field near the front (LEN / NLEN, HLIT...)
		else if (!m.empty()) { const uint64_t at = rnd() % m.size(); for (uint64_t k = at; k < m.size() && k < at + 8; k++) m[k] = (uint8_t)rnd(); }
		const int rc = run(m.data(), (uint32_t)m.size(), isize, crc, &bad);
		by_status[rc & 15]++;
	}
	printf("inflate_fuzz: %zu blocks, %ld mutations; by status:", blocks.size(), n_mut);
	for (int s = 0; s < 11; s++) printf(" %d:%ld", s, by_status[s]);
	printf("\n%s\n", bad ? "FAILED" : "ok");
	return bad ? 1 : 0;
}

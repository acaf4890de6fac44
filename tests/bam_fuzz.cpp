// Stand-alone fuzz driver of the host build of the BAM record parser (vargeno_amd/csrc/vg_bam.h); built by tests/test_bam_cpu.py
// with -fsanitize=address,undefined and run directly.
//
//   bam_fuzz STREAM.bin [mutations [seed]]
//
// STREAM.bin is an INFLATED BAM stream (header + records).  It is walked once unchanged: header, every record, the conversion of
// every kept record -- that must succeed and end at the stream's end.  Then `mutations` seeded mutations of record bytes (bit flips,
// field edits, truncations) go through the field view, the plausibility predicate, the speculation chain, the window walk (with the
// conversion pieces of every record it keeps) and the header parser, always on a heap copy of EXACTLY the mutated length: the
// sanitizer sees any byte read outside it.  Last, a walk and a speculation chain are started at every offset of a 4 KiB sample.
// A clean run means no out-of-bounds read and no walk that fails to end.
#include "../vargeno_amd/csrc/vg_bam.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

static uint64_t rng_state;
static uint64_t rnd()
{
	rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;     // xorshift64
	return rng_state;
}

static unsigned long long g_touched = 0;

// everything the device does with a buffer, from `entry`: speculation, the walk over every window, the conversion pieces
static bool exercise(const uint8_t *data, size_t n, uint64_t entry, int32_t n_ref)
{
	uint8_t *b = (uint8_t *)malloc(n ? n : 1);                   // exactly n bytes
	if (n) memcpy(b, data, n);
	const uint8_t *p = n ? b : b + 1;
	std::vector<uint32_t> offs(VG_BAM_WIN_RECS);
	bool ok = true;
	VgBamRec r;
	(void)vg_bam_plausible(p, n, entry, n_ref, &r);
	g_touched += vg_bam_chain(p, n, entry, n_ref);
	uint64_t at = entry, steps = 0;
	while (at < n) {
		const uint64_t win_end = (at / VG_BAM_WINDOW + 1) * VG_BAM_WINDOW;
		VgBamWalk w;
		vg_bam_walk(p, n, at, win_end, offs.data(), (uint32_t)offs.size(), &w);
		if (w.exit < at || w.exit > n + VG_BAM_WINDOW || w.n_kept > offs.size()) { fprintf(stderr, "walk: exit %u from %llu\n", w.exit, (unsigned long long)at); ok = false; break; }
		for (uint32_t i = 0; i < w.n_kept; i++) {
			const uint32_t off = offs[i];
			if (vg_bam_view(p, n, off, &r) != VG_BAM_OK || !vg_bam_sizes_ok(r) || n - off < 4ull + r.block_size) { fprintf(stderr, "walk kept a record that is not inside the buffer\n"); ok = false; break; }
			const uint64_t so = r.seq_off(off), qo = r.qual_off(off);
			for (uint32_t j = 0; j < r.l_seq; j++) g_touched += vg_bam_base(p, so, r.l_seq, r.reversed(), j);
			for (uint32_t c = 0; c < 64; c++) g_touched += vg_bam_gate_bit(p, qo, r.l_seq, r.reversed(), c);
		}
		if (w.bad || w.exit == at || !ok) break;                  // a bad record, or the data ends inside the record at `at`
		at = w.exit;
		if (++steps > n / 37 + 2) { fprintf(stderr, "the walk does not end\n"); ok = false; break; }
	}
	uint64_t end = 0; int32_t nr = 0;
	g_touched += (unsigned)vg_bam_header(p, n, &end, &nr);
	std::string text; uint64_t used = 0; VgBamCounts cnt;
	(void)vg_bam_convert(p, n, entry <= n ? entry : n, text, &used, cnt);
	if (used > n) { fprintf(stderr, "convert: used %llu of %zu\n", (unsigned long long)used, n); ok = false; }
	free(b);
	return ok;
}

int main(int argc, char **argv)
{
	if (argc < 2) { fprintf(stderr, "usage: bam_fuzz STREAM.bin [mutations [seed]]\n"); return 2; }
	const long n_mut = argc > 2 ? atol(argv[2]) : 20000;
	rng_state = argc > 3 ? strtoull(argv[3], nullptr, 10) | 1u : 0x9e3779b97f4a7c15ull;
	FILE *f = fopen(argv[1], "rb");
	if (!f) { perror(argv[1]); return 2; }
	std::vector<uint8_t> raw;
	uint8_t buf[65536];
	for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) raw.insert(raw.end(), buf, buf + n);
	fclose(f);
	uint64_t hdr_end = 0; int32_t n_ref = 0;
	if (vg_bam_header(raw.data(), raw.size(), &hdr_end, &n_ref) != VG_BAM_OK) { fprintf(stderr, "no BAM header\n"); return 2; }
	// the valid stream: every record in turn, to the end
	std::vector<uint64_t> starts;
	{
		std::string text; uint64_t used = 0; VgBamCounts cnt;
		if (vg_bam_convert(raw.data(), raw.size(), hdr_end, text, &used, cnt) != VG_BAM_OK || used != raw.size() || !cnt.kept) { fprintf(stderr, "the valid stream does not convert to its end\n"); return 1; }
		VgBamRec r;
		for (uint64_t at = hdr_end; at < raw.size(); at += 4ull + r.block_size) { if (vg_bam_view(raw.data(), raw.size(), at, &r) != VG_BAM_OK) return 1; starts.push_back(at); }
	}
	bool ok = exercise(raw.data(), raw.size(), hdr_end, n_ref);
	// mutations of a run of records (up to 4 KiB from a record's start), exactly sized
	std::vector<uint8_t> m;
	for (long i = 0; i < n_mut && ok; i++) {
		const uint64_t at = starts[rnd() % starts.size()];
		const size_t len = (size_t)std::min<uint64_t>(raw.size() - at, 64 + rnd() % 4096);
		m.assign(raw.begin() + (long)at, raw.begin() + (long)(at + len));
		const unsigned kind = (unsigned)(rnd() % 8);
		if (kind < 2) { const unsigned flips = 1 + (unsigned)(rnd() % 3); for (unsigned k = 0; k < flips; k++) m[rnd() % m.size()] ^= (uint8_t)(1u << (rnd() % 8)); }
		else if (kind == 2) { const uint64_t o = rnd() % 36; m[o] ^= (uint8_t)(1u << (rnd() % 8)); }                       // a bit of the first record's fixed fields
		else if (kind == 3) { const uint32_t v = (rnd() & 1u) ? (uint32_t)rnd() : (uint32_t)(rnd() % 70000); memcpy(m.data(), &v, 4); }        // block_size
		else if (kind == 4) { const uint32_t v = (rnd() & 1u) ? (uint32_t)rnd() : (uint32_t)(rnd() % 70000); memcpy(m.data() + 20, &v, 4); }   // l_seq
		else if (kind == 5) { m[12] = (uint8_t)rnd(); m[16] = (uint8_t)rnd(); m[17] = (uint8_t)rnd(); }                      // l_read_name, n_cigar_op
		else if (kind == 6) m.resize(rnd() % m.size());                                                                      // truncation
		else { const uint64_t o = rnd() % m.size(); for (uint64_t k = o; k < m.size() && k < o + 8; k++) m[k] = (uint8_t)rnd(); }
		const uint64_t entry = (rnd() % 8) ? 0 : rnd() % (m.size() + 1);
		ok = exercise(m.data(), m.size(), entry, n_ref);
	}
	// a walk from EVERY offset of a 4 KiB sample
	const size_t sample = std::min<size_t>(raw.size() - (size_t)hdr_end, 4096);
	for (size_t o = 0; o <= sample && ok; o++) ok = exercise(raw.data() + hdr_end, sample, o, n_ref);
	// the header parser on every prefix of the header, and on mutated headers
	for (uint64_t n = 0; n <= hdr_end && n < 6000 && ok; n++) {
		uint8_t *b = (uint8_t *)malloc(n ? n : 1);
		if (n) memcpy(b, raw.data(), n);
		uint64_t end = 0; int32_t nr = 0;
		const int rc = vg_bam_header(n ? b : b + 1, n, &end, &nr);
		if (n < hdr_end ? rc != VG_BAM_MORE : rc != VG_BAM_OK) { fprintf(stderr, "header of %llu bytes: %d\n", (unsigned long long)n, rc); ok = false; }
		if (n >= 12) { b[rnd() % n] ^= (uint8_t)(1u << (rnd() % 8)); g_touched += (unsigned)vg_bam_header(b, n, &end, &nr); }
		free(b);
	}
	printf("bam_fuzz: %zu records, %ld mutations, %zu offsets (%llu)\n%s\n", starts.size(), n_mut, sample + 1, g_touched, ok ? "ok" : "FAILED");
	return ok ? 0 : 1;
}

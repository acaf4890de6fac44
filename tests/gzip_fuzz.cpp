// gzip_fuzz.cpp -- the host build of vargeno_amd/csrc/vg_gunzip.h alone, for a sanitizer build (tests/test_gzip_cpu.py builds it with
// -fsanitize=address,undefined and runs it directly):  gzip_fuzz <valid.gz> <iterations> <seed>
// Every iteration mutates the valid file (bit flips, a truncation, a spliced run of bytes) into an exactly sized heap buffer and runs
// it through the sequential decoder and through the chunked stages on the host, at a chunk and slot size drawn per iteration, with
// exactly sized text buffers.  Checked: the two agree -- one accepts iff the other does (a refused slot aside), with the same text and
// offsets --; the unmutated file decodes to the same text at every setting; and no decode took more steps than TERMINATION allows.
#include "../vargeno_amd/csrc/vg_gunzip.h"

#include <stdio.h>
#include <stdlib.h>

#include <memory>

static uint64_t rng_state;
static uint64_t rnd()
{
	rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
	return rng_state;
}

int main(int argc, char **argv)
{
	if (argc < 4) { fprintf(stderr, "usage: gzip_fuzz <valid.gz> <iterations> <seed>\n"); return 2; }
	FILE *f = fopen(argv[1], "rb");
	if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
	std::vector<uint8_t> good;
	uint8_t tmp[65536];
	size_t k;
	while ((k = fread(tmp, 1, sizeof tmp, f)) > 0) good.insert(good.end(), tmp, tmp + k);
	fclose(f);
	const long iters = atol(argv[2]);
	rng_state = strtoull(argv[3], nullptr, 10) * 0x9e3779b97f4a7c15ull + 1;

	// the valid file: its text, by the sequential decoder
	std::vector<uint8_t> want(64u << 20);
	VgGzResult g;
	vg_gunzip_sequential(good.data(), good.size(), want.data(), want.size(), &g);
	if (g.rc || g.consumed != good.size()) { fprintf(stderr, "the valid file does not decode: rc %d\n", g.rc); return 1; }
	want.resize(g.text_len);
	const uint64_t cap = want.size() + 257;

	uint64_t accepted = 0, refused = 0, max_steps_seq = 0, max_steps_chk = 0;
	for (long it = 0; it <= iters; it++) {
		// iteration 0 is the unmutated file
		uint64_t n = good.size();
		const uint64_t kind = it ? rnd() % 8 : 99;
		if (kind == 0) n = rnd() % (good.size() + 1);                                  // a truncation
		std::unique_ptr<uint8_t[]> in(new uint8_t[n ? n : 1]);
		memcpy(in.get(), good.data(), n);
		if (kind >= 1 && kind <= 5 && n) for (uint64_t j = 0; j <= kind % 3; j++) in[rnd() % n] ^= (uint8_t)(1u << (rnd() % 8));      // 1 to 3 bit flips
		if (kind == 6 && n > 64) { const uint64_t len = 1 + rnd() % 32, a = rnd() % (n - len), b = rnd() % (n - len); memmove(in.get() + a, in.get() + b, len); }    // a spliced run
		if (kind == 7 && n > 40) in[rnd() % 40] ^= (uint8_t)(1u << (rnd() % 8));         // a flip among the first headers

		std::unique_ptr<uint8_t[]> t1(new uint8_t[cap]), t2(new uint8_t[cap]);
		VgGzResult a;
		vg_gunzip_sequential(in.get(), n, t1.get(), cap, &a);
		if (a.steps > 2 * (n * 8 + cap) + 4096) { printf("iteration %ld: the sequential decoder took %lu steps for %lu bytes\n", it, (unsigned long)a.steps, (unsigned long)n); return 1; }
		max_steps_seq = std::max(max_steps_seq, a.steps);

		static const uint64_t chunks[] = {64, 100, 1024, 8192, 32768, 1u << 20};
		VgGzOpts op = {chunks[rnd() % 6], 0, 1 + rnd() % 12, 0};
		const uint64_t slots[] = {n + 1, n / 4 + 1, n / 40 + 1, 3000};
		op.slot_bytes = slots[rnd() % 4];
		op = vg_gz_opts_checked(op, n);
		VgGzHostStages be(in.get(), t2.get(), op);
		VgGzResult b;
		if (vg_gunzip_chunked(be, in.get(), n, cap, op, &b)) { printf("iteration %ld: the host stages failed\n", it); return 1; }
		// TERMINATION: every decode is bounded by its slot's bits plus its capacity, every full test by one header parse
		// (a slot that held no whole block was tried again twice as long: at most log2 tries of at most slot_max bytes each)
		const uint64_t slot_bits = op.slot_max * 8, slot_cap = (op.slot_max / op.chunk_bytes + 1) * op.chunk_bytes * op.max_ratio, n_slots = 32 * (n / op.slot_bytes + b.st.members + 2);
		const uint64_t bound = (b.st.guessed + b.st.repaired + n_slots) * (2 * (slot_bits + slot_cap) + 4096) + (b.st.tested + 1) * 1024;
		if (be.needs > bound) { printf("iteration %ld: the chunked stages took %lu steps, bound %lu\n", it, (unsigned long)be.needs, (unsigned long)bound); return 1; }
		max_steps_chk = std::max(max_steps_chk, be.needs);

		// every fourth file also through the push driver (what a gzip stream runs), cut into pushes of a drawn size: the same verdict,
		// offsets, members and text as the route that sees the whole file (the chunk counts may differ: a slot that ends exactly at the
		// end of the file is tried once more by a driver that cannot know that nothing follows)
		if (it % 4 == 0) {
			const uint64_t pushes[] = {1, 7, 4099, n + 1};
			const uint64_t push = pushes[rnd() % 4];
			VgGzHostPushStages pbe(op);
			VgGzPush<VgGzHostPushStages> drv(pbe, op);
			for (uint64_t at = 0; at < n; at += push) if (drv.push(in.get() + at, std::min(push, n - at))) { printf("iteration %ld: the pushed host stages failed\n", it); return 1; }
			if (drv.end()) { printf("iteration %ld: the pushed host stages failed\n", it); return 1; }
			const VgGzResult &c = drv.r;
			if (c.rc != b.rc || c.bad_offset != b.bad_offset || c.text_len != b.text_len || c.consumed != b.consumed || c.st.members != b.st.members || c.st.slots_refused != b.st.slots_refused || c.st.resume_bit != b.st.resume_bit || c.text_len > pbe.out.size() || (c.text_len && memcmp(pbe.out.data(), t2.get(), c.text_len))) {
				printf("iteration %ld: pushes of %lu differ from the whole file: rc %d / %d, bad offset %lu / %lu, text %lu / %lu, consumed %lu / %lu (chunk %lu slot %lu ratio %lu)\n", it, (unsigned long)push, c.rc, b.rc, (unsigned long)c.bad_offset,
				       (unsigned long)b.bad_offset, (unsigned long)c.text_len, (unsigned long)b.text_len, (unsigned long)c.consumed, (unsigned long)b.consumed, (unsigned long)op.chunk_bytes, (unsigned long)op.slot_bytes, (unsigned long)op.max_ratio);
				return 1;
			}
		}

		const bool b_refused = b.st.slots_refused != 0 || b.rc == VG_GZ_EBLOCK;            // (the ratio bound or the slot size of this draw: no verdict on the data)
		if (b_refused) refused++;
		if (!b_refused && (a.rc == 0) != (b.rc == 0)) { printf("iteration %ld: sequential rc %d, chunked rc %d (chunk %lu slot %lu)\n", it, a.rc, b.rc, (unsigned long)op.chunk_bytes, (unsigned long)op.slot_bytes); return 1; }
		// the text: the same bytes -- all of them, or (a refused slot: the text before it, of a member not yet verified) a prefix of a valid file's
		if ((!b_refused || a.rc == 0) && (b.text_len > a.text_len || memcmp(t1.get(), t2.get(), b.text_len))) { printf("iteration %ld: the chunked text differs from the sequential text (rc %d / %d, text %lu / %lu, chunk %lu slot %lu ratio %lu)\n", it, a.rc, b.rc, (unsigned long)a.text_len, (unsigned long)b.text_len, (unsigned long)op.chunk_bytes, (unsigned long)op.slot_bytes, (unsigned long)op.max_ratio); return 1; }
		if (!b_refused && (b.text_len != a.text_len || b.consumed != a.consumed)) { printf("iteration %ld: text %lu / %lu, consumed %lu / %lu\n", it, (unsigned long)a.text_len, (unsigned long)b.text_len, (unsigned long)a.consumed, (unsigned long)b.consumed); return 1; }
		if (it == 0 && (a.rc || a.text_len != want.size() || memcmp(t1.get(), want.data(), want.size()))) { printf("the unmutated file decodes differently\n"); return 1; }
		if (a.rc == 0) accepted++;
	}
	printf("%ld mutations: %lu still valid, %lu with a refused slot; most steps %lu (sequential) %lu (chunked)\nok\n", iters, (unsigned long)accepted, (unsigned long)refused, (unsigned long)max_steps_seq, (unsigned long)max_steps_chk);
	return 0;
}

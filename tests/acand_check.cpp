// Stage A's candidates of a chunk (vargeno_amd/csrc/vg_acand.h) against a plain restatement of the per-site look-up it replaced,
// site by site in source order; stand-alone, built with -fsanitize=address,undefined by tests/test_acand_cpu.py.
// Every combination of: pass 0 / 1; the chunk's strand bit; palindrome; reverse block usable or not; 0 .. 4 matching entries, each
// reference or SNP, of either strand, with flags from {hit, hit at POS_AMBIGUOUS, ambiguous (a row), PAIR, quiet A, quiet B, quiet A + B}.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "vg_acand.h"
#include "vg_quiet.h"

static const uint32_t POS_AMBIGUOUS = 0xFFFFFFFFu;
enum Kind { REV_PUSH, FWD_PUSH, ROW_REF, ROW_SNP };
struct Op { int kind; uint32_t value, quiet; bool operator==(const Op &o) const { return kind == o.kind && value == o.value && quiet == o.quiet; } };
struct Entry { bool is_snp; uint32_t es, p1, p2, f; };

// the quiet bits a push carries, as the kernel's quiet_bit() takes them from the hit's flags
static uint32_t quiet_of_flags(uint32_t hf) { return (hf & 6u) == 0u ? hf & VG_QUIET_MASK : 0u; }

// The per-site form: note() at every matching entry in bucket order -- the entry of the other strand goes to the reverse block at
// once, while the block is usable --, then the reference hit, then the SNP hit.  (What the key table answers -- no room, a chunk
// voting twice -- is not part of the rule: the table here takes everything.)
static std::vector<Op> per_site(uint32_t pass, uint32_t ks, bool pal, bool rc_usable, const std::vector<Entry> &es, bool &rc_after)
{
	std::vector<Op> out;
	bool rc_ok = pass == 0u && rc_usable;                       // rc_top != RC_BAD
	uint32_t rp = 0, rp2 = 0, rf = 0, sp = 0, sp2 = 0, sf = 0;
	for (const Entry &e : es) {
		if (pal || e.es == ks) { if (e.is_snp) { sp = e.p1; sp2 = e.p2; sf = e.f; } else { rp = e.p1; rp2 = e.p2; rf = e.f; } }
		if ((pal || e.es != ks) && rc_ok) {
			if (e.f & 2u) rc_ok = false;
			else if (e.p1 != POS_AMBIGUOUS) out.push_back({REV_PUSH, e.p1, quiet_of_flags(e.f)});
		}
	}
	const bool r_ok = (rf & 1u) && ((rf & 4u) || rp != POS_AMBIGUOUS), s_ok = (sf & 1u) && ((sf & 4u) || sp != POS_AMBIGUOUS);
	const bool r_ax = r_ok && (rf & 6u) == 2u, s_ax = s_ok && (sf & 6u) == 2u;
	if (r_ok) {
		if (r_ax) out.push_back({ROW_REF, rp, 0u});
		else { out.push_back({FWD_PUSH, rp, quiet_of_flags(rf)}); if (rf & 4u) out.push_back({FWD_PUSH, rp2, 0u}); }
	}
	if (s_ok) {
		if (s_ax) out.push_back({ROW_SNP, sp, 0u});
		else { out.push_back({FWD_PUSH, sp, 0u}); if (sf & 4u) out.push_back({FWD_PUSH, sp2, 0u}); }
	}
	rc_after = rc_ok;
	return out;
}

// the header's list, read the way the kernel's drain reads it: slot by slot from the meta word
static std::vector<Op> from_header(uint32_t pass, uint32_t ks, bool pal, bool rc_usable, const std::vector<Entry> &es, bool &rc_after)
{
	VgAChunk st;
	vg_acand_begin(st, pass, rc_usable);
	for (const Entry &e : es) vg_acand_note(st, ks, pal, e.is_snp, e.es, e.p1, e.p2, e.f);
	const uint32_t meta = vg_acand_meta(st);
	std::vector<Op> out;
	for (uint32_t s = 0; s < VG_AC_SLOTS; s++) if ((meta >> s) & 1u) {
		const int kind = vg_acand_is_reverse(s) ? REV_PUSH : vg_acand_is_row(meta, s) ? (s == 2u ? ROW_REF : ROW_SNP) : FWD_PUSH;
		out.push_back({kind, st.v[s], vg_acand_quiet_of(meta, s)});
	}
	rc_after = st.usable;
	return out;
}

static long checks = 0, wide = 0, max_len = 0;
static void fail(const char *what, uint32_t pass, uint32_t ks, bool pal, bool rc, const std::vector<Entry> &es)
{
	printf("FAIL %s: pass %u ks %u pal %d rc %d entries", what, pass, ks, (int)pal, (int)rc);
	for (const Entry &e : es) printf(" (snp %d es %u p1 %u f %u)", (int)e.is_snp, e.es, e.p1, e.f);
	printf("\n");
	exit(1);
}

int main()
{
	const uint32_t flagset[7] = {1u, 1u, 1u | 2u, 1u | 2u | 4u, 1u | VG_QUIET_A, 1u | VG_QUIET_B, 1u | VG_QUIET_MASK};   // [1]: at POS_AMBIGUOUS
	const uint32_t per = 2u * 2u * 7u;                          // an entry: dictionary x strand x flags
	for (uint32_t hdr = 0; hdr < 16u; hdr++) {
		const uint32_t pass = hdr & 1u, ks = (hdr >> 1) & 1u;
		const bool pal = (hdr >> 2) & 1u, rc = (hdr >> 3) & 1u;
		for (uint32_t n = 0; n <= 4u; n++) {
			uint64_t total = 1;
			for (uint32_t i = 0; i < n; i++) total *= per;
			for (uint64_t code = 0; code < total; code++) {
				std::vector<Entry> es;
				uint64_t x = code;
				for (uint32_t i = 0; i < n; i++) {
					const uint32_t e = (uint32_t)(x % per); x /= per;
					const uint32_t fi = e / 4u;
					es.push_back({(e & 1u) != 0u, (e >> 1) & 1u, fi == 1u ? POS_AMBIGUOUS : 1000u * (i + 1u), 1000u * (i + 1u) + 7u, flagset[fi]});
				}
				bool rc_a = false, rc_b = false;
				const std::vector<Op> want = per_site(pass, ks, pal, rc, es, rc_a), got = from_header(pass, ks, pal, rc, es, rc_b);
				long nrev = 0;
				for (const Op &o : want) nrev += o.kind == REV_PUSH;
				if (got.size() > 6u) fail("more than six candidates", pass, ks, pal, rc, es);
				if ((long)got.size() > max_len) max_len = (long)got.size();
				if (nrev <= 2) {
					if (!(want == got) || rc_a != rc_b) fail("list or block state differs", pass, ks, pal, rc, es);
				} else {
					// three or more reverse-strand candidates in one chunk (no index has them): the block is given up -- pass 1 is then
					// looked up the plain way --, the first two and every forward candidate stand as before
					wide++;
					if (rc_b) fail("block kept after a third reverse candidate", pass, ks, pal, rc, es);
					std::vector<Op> w2;
					long k = 0;
					for (const Op &o : want) if (o.kind != REV_PUSH || k++ < 2) w2.push_back(o);
					if (!(w2 == got)) fail("forward list differs beside a wide reverse list", pass, ks, pal, rc, es);
				}
				checks++;
			}
		}
	}
	// the quiet bits a candidate carries give the same free-chunk proof as the flags themselves
	for (uint32_t f = 0; f < 256u; f++) for (uint32_t n = 1; n <= 5u; n++) for (uint32_t c = 0; c < 5u; c++) {
		const uint32_t want = (f & 6u) == 0u ? vg_quiet_chunks(f, c, n) : 0u;
		const uint32_t q2 = vg_acand_quiet2(f), got = q2 ? vg_quiet_chunks(q2 << VG_AC_QUIET_SHIFT, c, n) : 0u;
		if (want != got) { printf("FAIL quiet bits f %u c %u n %u\n", f, c, n); return 1; }
		checks++;
	}
	if (max_len != 6) { printf("FAIL the bound of six is never reached (%ld)\n", max_len); return 1; }
	printf("ok %ld checks, %ld with a wide reverse list, longest list %ld\n", checks, wide, max_len);
	return 0;
}

// vg_caller.h -- the genotype caller (reference src/qv.cc:1789-1848, GQ at :1681), once, for the host tools and the device.
//
// Per SNP site: likelihood of (ref_cnt, alt_cnt) under hom-ref / het / hom-alt with a 1 % error rate, Hardy-Weinberg prior from
// the two allele frequencies stored as n/255, times a Poisson(7.1) depth term; a site with no reads or with both counters
// saturated is not called; GQ = (int)(-10 ln(confidence)).
//
// GQ truncates, so a last-bit difference in the confidence can show.  Three rules keep host and device bit-identical:
//   * the per-count factors (powers, the Poisson mass, k/255) are computed ONCE, on the host, with libm (vg_caller_tables_fill);
//     device code takes them from an uploaded copy of that table and never recomputes them;
//   * the arithmetic on them is f64 add, multiply and divide only, under `fp contract(off)`: a device compiler fuses a*b+c by
//     default, the host build (-march=x86-64-v2) cannot, and the fused form rounds once where the reference rounds twice;
//   * the logarithm is NOT shared: vg_genotype_quality() is libm's and host-only.  Device code settles a site only when its own
//     log is far enough from an integer for the difference not to matter (vg_gq_settled) and leaves the rest to the host.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define VG_CALLER_HD __host__ __device__
#else
#define VG_CALLER_HD
#endif

enum { VGC_CAP = 63 };                     // counter saturation, src/vartype.h:27
enum { VGC_NONE = 0, VGC_HOM_REF = 1, VGC_HOM_ALT = 2, VGC_HET = 3 };     // numbering of the reference's GTYPE_* (vartype.h)

// Per-count factors.  The reference tabulates the three likelihoods per (ref_cnt, alt_cnt) pair; a product of two tabulated
// powers is the same pair of libm calls and the same multiply, so 3 x 64 numbers replace 3 x 4096.
struct vg_caller_tables {
	double keep[VGC_CAP + 1];              // (1 - e)^k
	double flip[VGC_CAP + 1];              // e^k
	double half[2 * VGC_CAP + 1];          // 0.5^k
	double depth[2 * VGC_CAP + 1];         // Poisson(7.1) mass at k
	double freq[256];                      // k / 255.0
};

struct vg_site_call {
	uint8_t gt;                            // VGC_*
	double confidence;                     // posterior of the winning genotype x Poisson(7.1) mass of the depth
};

// host only (libm)
inline void vg_caller_tables_fill(vg_caller_tables &t)
{
	const double err = 0.01;               // src/vartype.h:13
	const double mean_depth = 7.1;         // src/vartype.h:14
	for (unsigned k = 0; k <= VGC_CAP; k++) { t.keep[k] = pow(1.0 - err, (int)k); t.flip[k] = pow(err, (int)k); }
	const double m = exp(-mean_depth);
	for (unsigned k = 0; k <= 2 * VGC_CAP; k++) {
		t.half[k] = pow(0.5, (int)k);
		t.depth[k] = (m * pow(mean_depth, (int)k)) / exp(lgamma(k + 1.0));
	}
	for (unsigned k = 0; k < 256; k++) t.freq[k] = k / 255.0;
}
// the GQ column: (int)(-10 ln c), libm's logarithm
inline int vg_genotype_quality(double confidence) { return (int)(-10 * log(confidence)); }

// counts above the cap are saturated first; frequencies are the dictionary's n/255 encodings
VG_CALLER_HD inline vg_site_call vg_call_site(const vg_caller_tables &t, unsigned ref_cnt, unsigned alt_cnt, uint8_t ref_freq, uint8_t alt_freq)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	vg_site_call out{VGC_NONE, 0.0};
	if (ref_cnt > VGC_CAP) ref_cnt = VGC_CAP;
	if (alt_cnt > VGC_CAP) alt_cnt = VGC_CAP;
	if ((ref_cnt | alt_cnt) == 0 || (ref_cnt == VGC_CAP && alt_cnt == VGC_CAP)) return out;
	const double pr = t.freq[ref_freq], pa = t.freq[alt_freq];
	const double rr = pr * pr, aa = pa * pa;
	const double w[3] = {
		rr * (t.keep[ref_cnt] * t.flip[alt_cnt]),            // hom-ref
		(1.0 - rr - aa) * t.half[ref_cnt + alt_cnt],         // het
		aa * (t.flip[ref_cnt] * t.keep[alt_cnt]),            // hom-alt
	};
	const double sum = w[0] + w[1] + w[2];
	// strict maximum wins, hom-ref tested before het; anything else (ties included) is hom-alt
	int best = 2;
	if (w[0] > w[1] && w[0] > w[2]) best = 0;
	else if (w[1] > w[0] && w[1] > w[2]) best = 1;
	out.gt = best == 0 ? VGC_HOM_REF : best == 1 ? VGC_HET : VGC_HOM_ALT;
	const double top = best == 0 ? w[0] : best == 1 ? w[1] : w[2];
	out.confidence = (top / sum) * t.depth[ref_cnt + alt_cnt];
	return out;
}

// A per-site call in two bytes: gt << 14 | gq.  A gq field of VG_CALL_ESCAPE says "not settled here": whoever reads it recomputes
// that site with vg_call_site + vg_genotype_quality.
enum { VG_CALL_ESCAPE = 0x3FFF };

// y = -10 * log(confidence) by a logarithm that is not libm's: may (int)y be taken for libm's?  Only for a confidence inside
// (0, 1) (outside it the reference's GQ is an accident of its conversion, INT_MIN for a logarithm of a negative number), with y
// farther than `guard` from the nearest integer -- the two logarithms differ by a few ulp, ~1e-12 at |y| <= 2500 -- and below the
// escape code.
VG_CALLER_HD inline bool vg_gq_settled(double confidence, double y, double guard)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	if (!(confidence > 0.0 && confidence < 1.0)) return false;
	if (!(y >= 0.0 && y < (double)VG_CALL_ESCAPE)) return false;
	const double below = y - (double)(int)y;                 // y >= 0: (int) is floor
	return below > guard && 1.0 - below > guard;
}
#define VG_CALL_GUARD_DEFAULT 1e-6

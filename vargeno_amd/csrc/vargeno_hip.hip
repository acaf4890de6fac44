// vargeno_hip.hip -- HIP kernels (gfx950) and the C-ABI of include/vargeno_hip.h.
//
// Path: the per-read loop of `vargeno geno` (reference src/qv.cc:760-1558): 2-bit encode of the
// 32-base chunks, exact ref/SNP dictionary lookups, quality-gated Hamming-1 neighbour search bounded
// by two bit vectors, order-dependent position vote, pile-up counter updates.
//
// Build: hipcc --offload-arch=gfx950 -O3 -fPIC -shared (see Makefile).  No CPU fallback exists:
// every entry point fails with VG_ENODEV when no HIP device is usable.
#include "../../include/vargeno_hip.h"
#include "vg_device.h"
#include "vg_wave.h"
#include "vg_hostpack.h"
#include "vg_allreduce_plan.h"
#include "vg_arena.h"
#include "vg_inflate.h"
#include "vg_deflate.h"
#include "vg_bam.h"
#include "vg_gunzip.h"
#include "vg_caller.h"
#include "vg_pairs.h"
#include "vg_cprior.h"
#include "vg_jtext.h"
#include "vg_vcfidx.h"

#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <chrono>
#include <initializer_list>
#include <map>
#include <memory>
#include <string>
#include <thread>
#include <vector>

using namespace vg;

// ------------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
static int fail(int code, const char *fmt, const char *a = "", const char *b = "")
{
	snprintf(g_err, sizeof g_err, fmt, a, b);
	return code;
}
#define HIP_TRY(expr)                                                                              \
	do {                                                                                           \
		hipError_t e_ = (expr);                                                                    \
		if (e_ != hipSuccess) return fail(e_ == hipErrorOutOfMemory ? VG_ENOMEM : VG_ENODEV, "%s: %s", #expr, hipGetErrorString(e_)); \
	} while (0)

// No C++ exception may cross the C boundary: host allocations (new[], std::vector) inside an entry point are guarded.
template <class F>
static int guarded(F &&body)
{
	try { return body(); }
	catch (const std::bad_alloc &) { return fail(VG_ENOMEM, "host allocation failed"); }
	catch (...) { return fail(VG_EINVAL, "unexpected C++ exception"); }
}

extern "C" const char *vg_last_error(void) { return g_err; }
#ifndef VG_LIB_BUILD_ID
#define VG_LIB_BUILD_ID "unknown"
#endif
extern "C" const char *vg_build_id(void) { return VG_LIB_BUILD_ID; }

// page-locked host memory for callers without HIP headers (the CLI reads FASTQ chunks straight into it: H2D then runs
// at link speed instead of through the runtime's pageable staging)
extern "C" void *vg_host_alloc_pinned(size_t bytes)
{
	void *p = nullptr;
	if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) return nullptr;
	return p;
}
extern "C" void vg_host_free_pinned(void *p) { if (p) (void)hipHostFree(p); }
extern "C" int vg_device_count(void)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) return 0;
	return n;
}
extern "C" uint64_t vg_device_memory(int device)
{
	hipDeviceProp_t prop;
	if (hipGetDeviceProperties(&prop, device) != hipSuccess) { (void)hipGetLastError(); return 0; }
	return (uint64_t)prop.totalGlobalMem;
}
// host -> device rate of page-locked memory over this device's link, bytes per second (0 on failure): two timed copies of 64 MiB
extern "C" double vg_link_rate(int device)
{
	if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return 0.0; }
	const size_t n = 64ull << 20;
	void *h = nullptr, *d = nullptr;
	hipStream_t s = nullptr;
	double best = 0.0;
	if (hipHostMalloc(&h, n, hipHostMallocDefault) == hipSuccess && hipMalloc(&d, n) == hipSuccess && hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess) {
		memset(h, 1, n);
		for (int it = 0; it < 3; it++) {
			const auto t0 = std::chrono::steady_clock::now();
			if (hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) break;
			const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
			if (it && dt > 0 && (double)n / dt > best) best = (double)n / dt;        // (the first copy warms the path up)
		}
	}
	(void)hipGetLastError();
	if (s) (void)hipStreamDestroy(s);
	if (d) (void)hipFree(d);
	if (h) (void)hipHostFree(h);
	return best;
}
extern "C" uint64_t vg_share_budget(int device, int replicas)
{
	uint64_t total = vg_device_memory(device);
	const uint64_t reserve = 12ull << 30;
	if (total == 0 || replicas < 1) return 0;
	// what is free NOW, when that is less (another process on the device, the read stores the command line has just taken)
	size_t fr = 0, tot = 0;
	if (hipSetDevice(device) == hipSuccess && hipMemGetInfo(&fr, &tot) == hipSuccess) total = std::min<uint64_t>(total, (uint64_t)fr);
	(void)hipGetLastError();
	return (total > reserve ? total - reserve : total) / (uint64_t)replicas;
}

// ------------------------------------------------------------------------------------------------
// kernels: index construction
// ------------------------------------------------------------------------------------------------
constexpr int JG_SPAN = 16384;                       // bucket ids per workgroup
constexpr int JG_LDS = JG_SPAN + JG_SPAN / 32;       // padded: one spare word per 32 keeps the per-thread runs off one bank

__device__ inline uint64_t lower_bound_dev(const uint64_t *a, uint64_t n, uint64_t key)
{
	uint64_t lo = 0, hi = n;
	while (lo < hi) { uint64_t m = lo + ((hi - lo) >> 1); if (a[m] < key) lo = m + 1; else hi = m; }
	return lo;
}

// jump table: jg[h] = number of entries whose (kmer >> SHIFT) < h  (= index of the first entry with
// HI >= h, = n past the last used HI: exactly what src/qv.cc:539-584 / :622-678 build).  One
// workgroup owns JG_SPAN consecutive h: LDS histogram of its slice of the sorted array, LDS scan,
// coalesced write.  jg has n_buckets + 1 entries; the last one is the sentinel n.
__global__ __launch_bounds__(256) void vg_build_jumpgate(const uint64_t *__restrict__ kmer, uint64_t n, uint32_t *__restrict__ jg, uint64_t n_buckets, const int SHIFT)
{
	__shared__ uint32_t hist[JG_LDS];
	__shared__ uint64_t range[2];
	__shared__ uint32_t wave_tot[4];
	const uint64_t h0 = (uint64_t)blockIdx.x * JG_SPAN;
	const uint32_t t = threadIdx.x;
	if (t < 2) {
		const uint64_t h = h0 + (t ? JG_SPAN : 0);
		range[t] = (h >= n_buckets) ? n : lower_bound_dev(kmer, n, h << SHIFT);
	}
	for (uint32_t i = t; i < JG_LDS; i += 256) hist[i] = 0;
	__syncthreads();
	const uint64_t e0 = range[0], e1 = range[1];
	for (uint64_t e = e0 + t; e < e1; e += 256) {
		const uint32_t b = (uint32_t)((kmer[e] >> SHIFT) - h0);
		atomicAdd(&hist[b + (b >> 5)], 1u);
	}
	__syncthreads();
	// thread t owns buckets [64t, 64t+64): serial exclusive scan in place, then a block scan of the 256 run totals
	uint32_t run = 0;
	for (uint32_t j = 0; j < 64; j++) {
		const uint32_t b = t * 64 + j, at = b + (b >> 5);
		const uint32_t v = hist[at];
		hist[at] = run;
		run += v;
	}
	uint32_t incl = run;
	const uint32_t lane = t & 63, wv = t >> 6;
	for (int o = 1; o < 64; o <<= 1) { uint32_t y = __shfl_up(incl, o); if ((int)lane >= o) incl += y; }
	if (lane == 63) wave_tot[wv] = incl;
	__syncthreads();
	uint32_t base = incl - run;
	for (uint32_t w = 0; w < wv; w++) base += wave_tot[w];
	__syncthreads();
	for (uint32_t j = 0; j < 64; j++) { const uint32_t b = t * 64 + j, at = b + (b >> 5); hist[at] += base; }
	__syncthreads();
	for (uint32_t i = t; i < JG_SPAN; i += 256) {
		const uint64_t h = h0 + i;
		if (h < n_buckets) jg[h] = (uint32_t)(e0 + hist[i + (i >> 5)]);
	}
	if (blockIdx.x == gridDim.x - 1 && t == 0) jg[n_buckets] = (uint32_t)n;
}

size_t vg_dev_sort_pairs_temp_bytes(size_t n);                                                          // vg_sort.hip
int vg_dev_sort_pairs_u64_u32(uint64_t *keys_a, uint64_t *keys_b, uint32_t *vals_a, uint32_t *vals_b, size_t n, hipStream_t stream, void *tmp, size_t tmp_bytes, bool *result_in_b);

__global__ void vg_make_sec_keys(const uint64_t *__restrict__ kmer, uint64_t n, uint64_t *__restrict__ key, uint32_t *__restrict__ val)
{
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t k = kmer[i];
		key[i] = (k << 32) | (k >> 32);            // LO32 major, HI32 minor
		val[i] = (uint32_t)i;
	}
}

// 12-byte records of the LO32-ordered view (DevIndex::sec3) from the sorted keys (LO32 << 32 | HI32) and the entries they name
__global__ void vg_make_sec3(const uint64_t *__restrict__ skey, const uint32_t *__restrict__ sidx, const RefEnt *__restrict__ ref, uint64_t n, uint32_t *__restrict__ out)
{
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t k = skey[i];
		const RefEnt e = ref[sidx[i]];
		out[3 * i] = (uint32_t)k;
		out[3 * i + 1] = e.pos;
		out[3 * i + 2] = ((uint32_t)(k >> 32) & 0x7FFFFFFFu) | (e.amb ? 0x80000000u : 0u);
	}
}
// ... and of the SNP dictionary's (DevIndex::ssec3): the low word keeps 26 bits of LO32 and carries SNP_INFO_POS (where in the k-mer the SNP
// sits: a neighbour whose mutated base is the SNP base itself is not a hit, qv.cc:1308-1352) and the ambiguity flag
__global__ void vg_make_ssec3(const uint64_t *__restrict__ skey, const uint32_t *__restrict__ sidx, const SnpEnt *__restrict__ snp, uint64_t n, uint32_t *__restrict__ out)
{
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t k = skey[i];
		const SnpEnt e = snp[sidx[i]];
		out[3 * i] = (uint32_t)k;
		out[3 * i + 1] = e.pos;
		out[3 * i + 2] = ((uint32_t)(k >> 32) & 0x03FFFFFFu) | ((uint32_t)((e.key >> 43) & 0x1Fu) << 26) | (((e.key >> 48) & 0xFFu) ? 0x80000000u : 0u);
	}
}
// Is the reference bit vector exactly the set of LO32 values of the dictionary (qv.cc:955 tests bit hash32(LO32), and hash32 is a
// bijection)?  out[0]: dictionary LO32 values whose bit is NOT set; out[1]: distinct LO32 values; out[2]: bits set in the vector.
__global__ void vg_sec_bf_check(const uint64_t *__restrict__ skey, uint64_t n, const uint64_t *__restrict__ bf, unsigned long long *__restrict__ out)
{
	unsigned long long miss = 0, distinct = 0;
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		const uint32_t lo = (uint32_t)(skey[i] >> 32);
		if (i == 0 || lo != (uint32_t)(skey[i - 1] >> 32)) {
			distinct++;
			const uint32_t h = hash32(lo);
			if (!((bf[h >> 6] >> (h & 63u)) & 1ull)) miss++;
		}
	}
	if (miss) atomicAdd(&out[0], miss);
	if (distinct) atomicAdd(&out[1], distinct);
}
__global__ void vg_popcount_words(const uint64_t *__restrict__ w, uint64_t n, unsigned long long *__restrict__ out)
{
	unsigned long long c = 0;
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) c += (unsigned long long)__popcll(w[i]);
	for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
	if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, c);
}
// The merged view is keyed by the CANONICAL form of a k-mer (the smaller of it and its reverse complement, mixed so that the
// buckets fill evenly; r03): one look-up of a read's chunk then answers both strands -- the entry of the k-mer itself
// (a hit of the current pass) and the entry of its reverse complement (a hit of the OTHER pass, for the mirrored chunk).  A read of
// the reverse strand, whose forward pass finds nothing, then runs its one useful pass on the look-ups it has just made.
// strand bit of entry i (1: the dictionary's k-mer is the reverse complement of its canonical form)
__global__ void vg_canon_keys(uint64_t *__restrict__ key, uint64_t n, uint32_t *__restrict__ strand_bits)
{
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t k = key[i], r = revcomp64(k), ck = k < r ? k : r;
		if (k != ck) atomicOr(&strand_bits[i >> 5], 1u << (i & 31));
		key[i] = fmix64(ck);
	}
}
// merged exact-match view: after the stable sort, val = index into the concatenation [ref | snp].  Position and ambiguity come
// from the dictionaries' 16-byte entries (r05: the columns they were unpacked from are long gone by now -- the construction keeps
// as little alive as it can, vg_arena.h).  The entry's last word carries HI32 of its key, i.e. its bucket, until the direct
// table has been built from it (vg_make_direct; vg_inline_pairs then puts the word to its real use).
// dx_bits < 32 (DevIndex::dx_bits): bits 16-31 of the flags word carry field F, the key's high-word bits below the bucket, left-aligned.
// Quiet bits (vg_quiet.h; srank_words != nullptr): a reference entry with a single position says whether the site bits to the left
// and to the right of its k-mer are all clear -- flags 64 (A) and 128 (B), which vg_make_direct copies into the dx record.  SNP
// entries, ambiguous entries (PAIR or not) and POS_AMBIGUOUS get neither.  quiet_cnt: entries with A, with B, with both.
__global__ void vg_make_mx_entries(const uint64_t *__restrict__ key, const uint32_t *__restrict__ val, uint64_t n, uint64_t n_ref,
                                   const RefEnt *__restrict__ ref, const SnpEnt *__restrict__ snp, uint4 *__restrict__ out, const uint32_t *__restrict__ strand_bits, const uint32_t dx_bits,
                                   const unsigned long long *__restrict__ srank_words, const uint64_t pile_len, unsigned long long *__restrict__ quiet_cnt)
{
	uint32_t na = 0, nb = 0, nab = 0;
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		const uint32_t v = val[i];
		const bool is_snp = v >= n_ref;
		uint32_t pos, amb;
		if (is_snp) { const SnpEnt e = snp[v - n_ref]; pos = e.pos; amb = (uint32_t)(e.key >> 48) & 0xFFu; }
		else { const RefEnt e = ref[v]; pos = e.pos; amb = e.amb; }
		const uint32_t strand = (strand_bits[v >> 5] >> (v & 31)) & 1u;                          // flag 8: the dictionary's k-mer is the reverse complement of its canonical form
		const uint32_t hi = (uint32_t)(key[i] >> 32), F = dx_bits < 32u ? (hi << dx_bits) & 0xFFFF0000u : 0u;
		uint32_t quiet = 0;
		if (srank_words && !is_snp && !(amb & 1u) && pos != POS_AMBIGUOUS) {
			quiet = vg_quiet_bits(srank_words, pile_len, pos);
			na += (quiet & VG_QUIET_A) != 0u; nb += (quiet & VG_QUIET_B) != 0u; nab += quiet == VG_QUIET_MASK;
		}
		out[i] = make_uint4((uint32_t)key[i], pos, (is_snp ? 1u : 0u) | ((amb & 1u) << 1) | (strand << 3) | quiet | F, hi);
	}
	if (quiet_cnt) {
		if (na) atomicAdd(&quiet_cnt[0], (unsigned long long)na);
		if (nb) atomicAdd(&quiet_cnt[1], (unsigned long long)nb);
		if (nab) atomicAdd(&quiet_cnt[2], (unsigned long long)nab);
	}
}
// An ambiguous k-mer (2-10 copies) points at an auxiliary row; when the row holds exactly two positions -- the usual case --
// both fit the entry itself (flag PAIR: y = first position, w = second), and stage A needs no row gather for it.
__device__ inline bool aux_pair(const uint32_t *__restrict__ aux, uint32_t row, uint32_t &p0, uint32_t &p1)
{
	if (row == POS_AMBIGUOUS) return false;
	const uint32_t *r = aux + (uint64_t)row * AUX_COLS;
	p0 = r[0]; p1 = r[1];
	return p1 != 0 && r[2] == 0;
}
// direct table: the first entry of every HI32 bucket of the merged view, inline.  flags: 1 non-empty, 2 SNP entry, 4 ambiguous,
// 8 PAIR (single-entry buckets only: a longer bucket needs w for the index of its entries), 16 TIE (the second entry has the
// first one's k-mer: a query that matches the first entry of a bucket without it needs no further entry), bits 8.. = entries.
// r05: built from the entries themselves -- each carries its bucket in its last word (vg_make_mx_entries), the thread of a
// bucket's first entry writes the record, the table was zeroed before -- so that no 16 GiB jump table has to exist next to the
// 64 GiB table while it is filled: that was the one moment at which construction held more than the finished index.
__global__ void vg_make_direct(const uint4 *__restrict__ mx, uint64_t n, uint4 *__restrict__ dx,
                               const uint32_t *__restrict__ ref_aux, const uint32_t *__restrict__ snp_aux_pos, uint32_t *__restrict__ too_big, const uint32_t dx_bits)
{
	// dx_bits < 32: a bucket = the top dx_bits bits of the key's high word; the record's flags word carries the first entry's field F
	// (copied from the entry, bits 16-31) and an 8-bit count; TIE compares the whole of what is left of the key, (F, lo32)
	const uint32_t sh = 32u - dx_bits;
	const uint64_t cmax = dx_bits < 32u ? 0xFFull : 0xFFFFFFull;
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		const uint4 e = mx[i];
		const uint32_t bkt = e.w >> sh;
		if (i && (mx[i - 1].w >> sh) == bkt) continue;             // not the first of its bucket
		uint64_t hi = i + 1;
		while (hi < n && hi - i <= cmax && (mx[hi].w >> sh) == bkt) hi++;
		uint32_t cnt = (uint32_t)(hi - i);
		if (cnt > cmax) { atomicOr(too_big, 1u); cnt = (uint32_t)cmax; }        // the count field is 24 (8) bits wide: the host keeps the jump-table form (drops the view)
		uint4 r = make_uint4(e.x, e.y, 1u | ((e.z & 1u) << 1) | (((e.z >> 1) & 1u) << 2) | (((e.z >> 3) & 1u) << 5) | (e.z & VG_QUIET_MASK) | (cnt << 8) | (e.z & 0xFFFF0000u), (uint32_t)i);   // (flag 32: strand; 64, 128: quiet bits)
		if (cnt > 1u && mx[i + 1].x == e.x && mx[i + 1].w == e.w) r.z |= 16u;            // TIE: the second entry carries the same k-mer (reference + SNP dictionary)
		uint32_t p0, p1;
		if (cnt == 1u && (e.z & 2u) && aux_pair((e.z & 1u) ? snp_aux_pos : ref_aux, e.y, p0, p1)) { r.y = p0; r.w = p1; r.z = (r.z | 8u) & ~VG_QUIET_MASK; }   // (an ambiguous entry has no quiet bit; a PAIR must not)
		dx[bkt] = r;
	}
}
// the jump table of the merged view from the same bucket words (only when the direct table could not be kept after all)
__global__ void vg_jumpgate_from_buckets(const uint4 *__restrict__ mx, uint64_t n, uint32_t *__restrict__ jg)
{
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t h1 = i < n ? (uint64_t)mx[i].w : (1ull << 32), h0 = i ? (uint64_t)mx[i - 1].w + 1 : 0ull;     // buckets (previous entry's, this entry's] start here
		for (uint64_t h = h0; h <= h1; h++) jg[h] = (uint32_t)i;
	}
}
// the same for the entries of the merged view themselves (read for buckets of several entries); mx flags: 1 SNP, 2 ambiguous, 4 PAIR
__global__ void vg_inline_pairs(uint4 *__restrict__ mx, uint64_t n, const uint32_t *__restrict__ ref_aux, const uint32_t *__restrict__ snp_aux_pos)
{
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		uint4 e = mx[i];
		uint32_t p0, p1;
		e.w = 0u;                                                   // (the bucket word has done its job)
		if ((e.z & 2u) && aux_pair((e.z & 1u) ? snp_aux_pos : ref_aux, e.y, p0, p1)) { e.y = p0; e.w = p1; e.z = (e.z | 4u) & ~VG_QUIET_MASK; }   // (a PAIR carries no quiet bit)
		mx[i] = e;
	}
}
// strided-probe view of the SNP dictionary (DevIndex::snp_probe)
__global__ void vg_make_snp_probe(const uint64_t *__restrict__ kmer, const uint32_t *__restrict__ jg, uint64_t n, uint64_t *__restrict__ out)
{
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += (uint64_t)gridDim.x * blockDim.x) {
		if (i == n) { out[i] = 0ull; continue; }                    // (the kernel reads the view two entries at a time)
		const uint64_t slo = jg[kmer[i] >> 40];
		const uint64_t t = slo + (i - slo) * SNP_STRIDE;
		out[i] = t < n ? (kmer[t] & LO40_MASK) : 0ull;
	}
}
// paired HI32 table (DevIndex::hx), r05: from the dictionaries' entries, each of which carries its HI32 bucket in its spare word --
// no jump table is built for it (r03-r04 built two of 16 GiB each, one after the other, next to the 64 GiB table).  The table is
// zeroed first; the thread of a bucket's first entry writes the bucket's part of the record: the reference side writes whole
// records, the SNP side completes them.  A filter is computed over at most 64 entries; a longer bucket gets the mask that lets
// everything through.  Counts saturate at 0xFFFF: the bucket's end is then the NEXT record's start, which the same thread
// writes too (an empty bucket has no thread of its own; a non-empty one writes the same value).
__global__ void vg_hx_fill_ref(const RefEnt *__restrict__ ref, uint64_t n, uint4 *__restrict__ hx)
{
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		const uint32_t h = ref[i].pad;
		if (i && ref[i - 1].pad == h) continue;
		uint64_t hi = i + 1;
		while (hi < n && ref[hi].pad == h) hi++;
		const uint64_t cnt = hi - i;
		uint32_t f = 0;
		if (cnt == 1u) f = hx_fp16(ref[i].lo);
		else if (cnt > 64u) f = 0xFFFFu;
		else for (uint64_t e = i; e < hi; e++) f |= hx_bit(ref[e].lo);
		hx[h] = make_uint4((uint32_t)i, 0u, cnt < 0xFFFFu ? (uint32_t)cnt : 0xFFFFu, f);
		if (cnt >= 0xFFFFu) atomicMax(&hx[(uint64_t)h + 1].x, (uint32_t)hi);      // (atomic: the next bucket's own thread may write its record at the same moment -- with this very start)
	}
}
__global__ void vg_hx_fill_snp(const SnpEnt *__restrict__ snp, uint64_t n, uint4 *__restrict__ hx)
{
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		const uint32_t h = snp[i].pad;
		if (i && snp[i - 1].pad == h) continue;
		uint64_t hi = i + 1;
		while (hi < n && snp[hi].pad == h) hi++;
		const uint64_t cnt = hi - i;
		uint32_t f = 0;
		if (cnt == 1u) f = hx_fp16((uint32_t)snp[i].key);
		else if (cnt > 64u) f = 0xFFFFu;
		else for (uint64_t e = i; e < hi; e++) f |= hx_bit((uint32_t)snp[e].key);
		// (the reference side ran before: its words of the record stand)
		uint32_t *r = reinterpret_cast<uint32_t *>(hx + h);
		r[1] = (uint32_t)i;
		atomicOr(&r[2], (cnt < 0xFFFFu ? (uint32_t)cnt : 0xFFFFu) << 16);
		atomicOr(&r[3], f << 16);
		if (cnt >= 0xFFFFu) atomicMax(&hx[(uint64_t)h + 1].y, (uint32_t)hi);
	}
}
__global__ void vg_hx_sentinel(uint4 *__restrict__ hx, uint32_t n_ref, uint32_t n_snp) { hx[1ull << 32] = make_uint4(n_ref, n_snp, 0u, 0u); }
// signature form of the strided-probe view (DevIndex::snp_sig); 16 zero signatures behind the last entry (items read eight at a time)
__global__ void vg_make_snp_sig(const uint64_t *__restrict__ kmer, const uint32_t *__restrict__ jg, uint64_t n, uint16_t *__restrict__ out)
{
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n + 16; i += (uint64_t)gridDim.x * blockDim.x) {
		if (i >= n) { out[i] = 0; continue; }
		const uint64_t slo = jg[kmer[i] >> 40];
		const uint64_t t = slo + (i - slo) * SNP_STRIDE;
		out[i] = (uint16_t)sig16(t < n ? (kmer[t] & LO40_MASK) : 0ull);
	}
}
__global__ void vg_iota_u32(uint32_t *v, uint64_t n) { for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) v[i] = (uint32_t)i; }

// SoA as the dictionary file has it -> one 16-byte entry per k-mer (a hit then costs one line)
__global__ void vg_make_ref_entries(const uint64_t *__restrict__ kmer, const uint32_t *__restrict__ pos, const uint8_t *__restrict__ amb, uint64_t n, RefEnt *__restrict__ out)
{
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
		out[i] = RefEnt{(uint32_t)kmer[i], pos[i], (uint32_t)amb[i], (uint32_t)(kmer[i] >> 32)};       // (the spare word: HI32, the entry's bucket -- see vg_hx_fill_ref)
}
__global__ void vg_make_snp_entries(const uint64_t *__restrict__ kmer, const uint32_t *__restrict__ pos, const uint8_t *__restrict__ info, const uint8_t *__restrict__ amb, uint64_t n, SnpEnt *__restrict__ out)
{
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
		out[i] = SnpEnt{(kmer[i] & LO40_MASK) | ((uint64_t)info[i] << 40) | ((uint64_t)amb[i] << 48), pos[i], (uint32_t)(kmer[i] >> 32)};
}

// ------------------------------------------------------------------------------------------------
// kernels: the read loop
// ------------------------------------------------------------------------------------------------

// Streaming pre-pass: ASCII -> chunk k-mers + one flag word per read (gate bits: chunk c is gate-open iff
// qual[c] < '8', src/qv.cc:836, 943 -- the chunk NUMBER indexes the quality string).  Chunk c of read r
// lands at pk_kmer[(offsets[r] >> 5) + c]; slots of different reads cannot collide.
//
// r05: the text is packed POSITION by position, not read by read.  A wave takes a tile of 64 consecutive reads: their bases are
// one contiguous span of text, which the lanes fetch as aligned 16-byte pieces (coalesced, PACK_G per lane in flight), pack to
// 32 bits each (pack16: v_perm_b32 + v_dot4_u32_u8, ~8 instructions per 4 bases) and lay side by side in LDS -- the tile's text
// as a 2-bit stream.  A read's k-mers are then 64-bit windows of that stream at bit offset 2 x (its byte offset): five LDS
// words and four v_alignbit_b32 per pair of chunks.  The r04 kernel staged the ASCII text in LDS and let every lane pack its own
// read with 64-bit SWAR arithmetic: ~1 500 vector instructions per tile, 147 VGPRs, three waves per SIMD -- its 0.38 ms per
// 8 M reads were 0.31 ms of vector issue (125 000 tiles x 1 500 instructions over 1 024 SIMDs at one per four cycles), not the
// memory system.  Pieces that hold a byte other than ACGTacgt are flagged per piece (one ballot per round of 64 pieces); only
// a read whose chunks touch a flagged piece -- an N run, in practice -- classifies its own text (classify_bad_wide).
// Workgroups are four INDEPENDENT waves (a CU takes at most 16 workgroups; with ~48 VGPRs the kernel wants 32 waves per CU):
// no barrier, wave-scope fences only.  Only the first n quality characters of a read are ever looked at.
constexpr uint32_t PACK_T = 64;                 // reads per tile = lanes of the wave that packs it
constexpr uint32_t PACK_WPB = 4;                // waves per workgroup
constexpr uint32_t PACK_MAXLEN = 160;           // tiles whose reads average at most this many bases go through LDS; longer reads take the direct path
constexpr uint32_t PACK_PIECES = PACK_T * PACK_MAXLEN / 16 + 1;      // aligned 16-byte pieces under a tile (one more than the span needs)
constexpr uint32_t PACK_ROUNDS = (PACK_PIECES + 63) / 64;
#ifndef VG_PACK_G
#define VG_PACK_G 5                             // pieces per lane in flight together (150 bp reads: two groups per tile)
#endif
#ifndef VG_PACK_NT
#define VG_PACK_NT 1                            // `nt` on the loads of the base text, read once
#endif
__global__ __launch_bounds__(PACK_T * PACK_WPB) void vg_pack_kernel(const uint8_t *__restrict__ bases, const uint8_t *__restrict__ quals, const uint64_t *__restrict__ offsets,
                                                      uint64_t n_reads_arg, uint64_t *__restrict__ pk_kmer, uint64_t *__restrict__ pk_meta, uint32_t *__restrict__ invalid_reads,
                                                      const uint32_t *__restrict__ n_reads_dev, const uint32_t *__restrict__ gate, const uint32_t TR)
{
	// TR: reads per tile (<= 64; the host picks it from the batch's mean read length so that a tile's text fits the LDS stream:
	// 64 for reads of up to 160 bases, 40 for 250 bp ...; lanes beyond TR only help to fetch and pack the text)
	// gate != nullptr: the batch comes with one gate word per read (bit c = quality character c < '8') instead of quality strings --
	// the kernel then streams the bases only.  (With strings it fetches one line per read for the <= 4 characters a 150 bp read's
	// gate can see: at a 150-byte stride that is every line of the quality array, nearly as much traffic again as the bases.)
	__shared__ uint32_t sm_pk[PACK_WPB][PACK_PIECES + 7];                 // the tile's text, 16 bases per word
	__shared__ unsigned long long sm_bad[PACK_WPB][PACK_ROUNDS + 1];      // bit p: piece p holds a byte other than ACGTacgt
	const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), ln = threadIdx.x & 63u;
	const uint64_t n_reads = n_reads_dev ? (uint64_t)*n_reads_dev : n_reads_arg;     // a batch framed on the device knows its size there
	const uint64_t n_tiles = (n_reads + TR - 1) / TR, stride = (uint64_t)gridDim.x * PACK_WPB;
	uint64_t t = (uint64_t)blockIdx.x * PACK_WPB + wv;
	// a tile's own offsets (and gate words) are fetched while the tile before it is packed: one dependent wait per tile, not two
	uint64_t off = 0, off1 = 0;
	uint32_t gw = 0;
	auto fetch = [&](uint64_t tile, uint64_t &o, uint64_t &o1, uint32_t &g) {
		const uint64_t r = tile * TR + ln;
		o = o1 = 0; g = 0;
		if (ln < TR && r < n_reads) { o = offsets[r]; o1 = offsets[r + 1]; if (gate) g = gate[r]; }
	};
	if (t < n_tiles) fetch(t, off, off1, gw);
	for (; t < n_tiles; t += stride) {
		const uint64_t r0 = t * TR;
		const uint64_t r = ln < TR ? r0 + ln : n_reads;                                                    // (lanes beyond the tile have no read)
		const uint32_t last = (uint32_t)((r0 + TR < n_reads ? r0 + TR : n_reads) - r0) - 1u;               // last live lane of the tile
		const uint64_t base0 = __shfl(off, 0), span = __shfl(off1, (int)last) - base0;
		uint64_t noff = 0, noff1 = 0;
		uint32_t ngw = 0;
		if (t + stride < n_tiles) fetch(t + stride, noff, noff1, ngw);
		const uint32_t n = (uint32_t)((off1 - off) >> 5);
		uint32_t q4 = 0;
		if (!gate && n && r < n_reads) __builtin_memcpy(&q4, quals + off, 4);           // 4 <= n + 3 <= the read's own length: never past it
		// aligned 16-byte pieces: a piece that holds a byte of the text lies in that byte's page, so the first and the last piece
		// may reach past the text (a batch may start at any byte)
		const uint64_t a_text = (uint64_t)(bases + base0);
		const uint32_t shift = (uint32_t)(a_text & 15u);
		const uint8_t *abase = (const uint8_t *)(a_text - shift);
		const bool staged = (uint64_t)shift + span <= (uint64_t)PACK_T * PACK_MAXLEN;
		int cls = 0;
		if (staged) {
			const uint32_t n_pieces = (uint32_t)__builtin_amdgcn_readfirstlane((int)((shift + (uint32_t)span + 15u) >> 4));
			bool tile_bad = false;                                        // wave-uniform
			constexpr uint32_t G = VG_PACK_G;
			for (uint32_t j0 = 0; j0 * 64u < n_pieces; j0 += G) {
				uint4 v[G];
				#pragma unroll
				for (uint32_t q = 0; q < G; q++) {
					const uint32_t p = (j0 + q) * 64u + ln;
					v[q] = make_uint4(0x41414141u, 0x41414141u, 0x41414141u, 0x41414141u);
					if (p < n_pieces) v[q] = load_policy<VG_PACK_NT != 0, uint4, 16>(abase + 16ull * p);
				}
				#pragma unroll
				for (uint32_t q = 0; q < G; q++) {
					const uint32_t p = (j0 + q) * 64u + ln;
					uint32_t br = 0;
#ifdef VG_PACK_DRY
					const uint32_t w = v[q].x ^ v[q].y ^ v[q].z ^ v[q].w;      // timing experiment only (wrong results): the kernel's traffic without its arithmetic
#else
					const uint32_t w = pack16(v[q], br);
#endif
					if (p < n_pieces) sm_pk[wv][p] = w;
					const unsigned long long bm = __ballot((br & PACK_CASE_MASK) != 0u);
					tile_bad = tile_bad || bm != 0ull;
					if (ln == 0 && (j0 + q) * 64u < n_pieces) sm_bad[wv][j0 + q] = bm;
				}
			}
			VG_WAVE_SYNC();
			if (r < n_reads && n) {
				const uint32_t o = shift + (uint32_t)(off - base0);          // byte offset of the read in the tile's pieces
				const uint32_t w0 = o >> 4, s = 2u * (o & 15u);
				uint64_t *dst = pk_kmer + (off >> 5);
				auto win = [&](uint32_t hi, uint32_t lo) -> uint32_t { return __builtin_amdgcn_alignbit(hi, lo, s); };
				uint32_t c = 0;
				for (; c + 2 <= n; c += 2) {                               // a read's k-mers are contiguous: 16-byte stores
					uint32_t d[5];
					__builtin_memcpy(d, &sm_pk[wv][w0 + 2u * c], 20);
					const ulonglong2 kv = make_ulonglong2((uint64_t)win(d[1], d[0]) | ((uint64_t)win(d[2], d[1]) << 32), (uint64_t)win(d[3], d[2]) | ((uint64_t)win(d[4], d[3]) << 32));
					__builtin_memcpy(dst + c, &kv, 16);
				}
				if (c < n) {
					uint32_t d[3];
					__builtin_memcpy(d, &sm_pk[wv][w0 + 2u * c], 12);
					dst[c] = (uint64_t)win(d[1], d[0]) | ((uint64_t)win(d[2], d[1]) << 32);
				}
				if (tile_bad) {
					// does one of the pieces under this read's chunks hold an offending byte?  (the flags are per piece: the bases a read's
					// trim drops, and its neighbours' bases, may be what was seen -- the read's own text decides)
					bool any = false;
					for (uint32_t p = w0, left = ((o + 32u * n - 1u) >> 4) - w0 + 1u; left;) {          // (a 150 bp read lies under 9 pieces: one or two words)
						const uint32_t b = p & 63u, take = 64u - b < left ? 64u - b : left;
						unsigned long long m = sm_bad[wv][p >> 6] >> b;
						if (take < 64u) m &= (1ull << take) - 1ull;
						any = any || m != 0ull;
						p += take; left -= take;
					}
					if (any) cls = classify_bad_wide(bases + off, n);
				}
			}
		} else if (r < n_reads) {
			uint64_t bad = 0;
			for (uint32_t c = 0; c < n; c++) pk_kmer[(off >> 5) + c] = encode32(bases + off + 32 * c, bad);
			if (bad) cls = classify_bad(bases + off, n);
		}
		if (r < n_reads) {
			// quality gate bits (qv.cc:836): character c of the quality line, four characters per gather (the first four are in hand)
			uint64_t meta = 0;
			if (gate) meta = n >= 32 ? gw : (gw & ((1u << n) - 1u));
			else for (uint32_t c0 = 0; c0 < n && c0 < 32; c0 += 4) {
				if (c0) __builtin_memcpy(&q4, quals + off + c0, 4);       // c0 + 4 <= n + 3 <= the read's own length
				for (uint32_t j = 0; j < 4 && c0 + j < n && c0 + j < 32; j++) if ((int)(int8_t)(q4 >> (8 * j)) - '8' < 0) meta |= 1ull << (c0 + j);
			}
			if (cls) meta |= cls == 1 ? PK_SKIP_N : PK_INVALID;
			if (n > 32) meta |= gate ? PK_INVALID : PK_LONG;            // (a gate word has 32 bits; the reference's line buffer admits 31 chunks)
			if (meta & PK_INVALID) atomicAdd(invalid_reads, 1u);       // the reference aborts on such a read (util.c:103): the caller is told
			pk_meta[r] = meta;
		}
		VG_WAVE_SYNC();                                                // the tile's LDS words are read: the next tile may overwrite them
		off = noff; off1 = noff1; gw = ngw;
	}
}

// base-indexed counters of the wave kernel -> the ref / alt sums (and zero them for the next round): one launch for every sample
// plane that has taken increments since the last fold -- blockIdx.y walks the list of their numbers (one entry, plane 0, for a
// handle that never reserved a second plane)
__global__ void vg_fold_counters(const PlanePtr *__restrict__ planes, const uint32_t *__restrict__ dirty, const uint8_t *__restrict__ site_ba, uint64_t n_sites)
{
	const PlanePtr pl = planes[dirty[blockIdx.y]];
	uint32_t *__restrict__ const cnt4 = pl.cnt4, *__restrict__ const cnt = pl.cnt;
	for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n_sites; s += (uint64_t)gridDim.x * blockDim.x) {
		uint4 v = ((const uint4 *)cnt4)[s];
		if ((v.x | v.y | v.z | v.w) == 0) continue;
		const uint32_t q[4] = {v.x, v.y, v.z, v.w};
		const uint32_t ba = site_ba[s];
		cnt[2 * s] += q[ba & 3u];
		cnt[2 * s + 1] += q[(ba >> 2) & 3u];
		((uint4 *)cnt4)[s] = make_uint4(0u, 0u, 0u, 0u);
	}
}

// MAX_COV saturation (src/vartype.h:27, qv.cc:1411, 1419) of the exact sums, on the way to the host: 2 bytes per site cross the link instead of 8
__global__ void vg_clamp_counters(const uint32_t *__restrict__ cnt, uint64_t n_sites, uint8_t *__restrict__ ref_cnt, uint8_t *__restrict__ alt_cnt)
{
	for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n_sites; s += (uint64_t)gridDim.x * blockDim.x) {
		const uint2 v = ((const uint2 *)cnt)[s];
		ref_cnt[s] = (uint8_t)(v.x < 63u ? v.x : 63u);
		alt_cnt[s] = (uint8_t)(v.y < 63u ? v.y : 63u);
	}
}

// One lane = one read: forward pass, then the reverse-complement retry (src/qv.cc:1504-1510).
// A read touches the counters only at the end of its last pass, so a lane that runs out of scratch
// simply drops the read onto the overflow list and the same kernel re-runs it with a deep scratch.
// packed: the batch came 2-bit packed (vg_reads_submit_packed, the host-packed FASTQ stream): chunk k-mers and flag words
// are read from pk_kmer / pk_meta (the layout the pack kernel writes) instead of being encoded from text.
template <bool STATS>
__global__ __launch_bounds__(256) void vg_lane_kernel(DevIndex d, Scratch s, const uint8_t *__restrict__ bases, const uint8_t *__restrict__ quals,
                                                      const uint64_t *__restrict__ offsets, uint64_t n_reads_arg, const uint32_t *__restrict__ read_ids,
                                                      const uint32_t *__restrict__ n_ids, uint32_t *overflow_list, uint32_t *overflow_count, unsigned long long *stats, uint32_t *invalid_reads,
                                                      const uint32_t *__restrict__ gate, const uint64_t *__restrict__ pk_kmer, const uint64_t *__restrict__ pk_meta, const bool packed,
                                                      const PlanePtr *__restrict__ planes, const uint16_t *__restrict__ plane_tag)
{
	// planes != nullptr (the run over the late store only): read r counts into the sample plane its tag names, not into d.cnt
	const uint64_t n_reads = n_ids ? (uint64_t)*n_ids : n_reads_arg;          // a list launch (or a device-framed batch) is sized on the device: no host round trip
	const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t stride = gridDim.x * blockDim.x;
	Lane<STATS> L(d, s, gtid);
	LaneStats<STATS> tot;
	if constexpr (STATS) for (int i = 0; i < S_COUNT; i++) tot.v[i] = 0;
	// entry r of the work goes to lane r / n_waves of wave r % n_waves: a list of a dozen deep reads lands on a dozen waves,
	// not on twelve lanes of one wave that would run their divergent walks one after the other
	const uint32_t n_waves = stride >> 6;
	for (uint64_t r = (uint64_t)(gtid & 63u) * n_waves + (gtid >> 6); r < n_reads; r += stride) {
		const uint64_t rid = read_ids ? read_ids[r] : r;
		const uint64_t off = offsets[rid];
		const uint32_t n = (uint32_t)((offsets[rid + 1] - off) >> 5);            // src/qv.cc:778-779: len = (read_len/32)*32
		const uint8_t *p = bases + off;
		const uint64_t pmeta = packed ? pk_meta[rid] : 0ull;
		// src/qv.cc:836, 943: the chunk NUMBER indexes the quality string (which is NOT reversed for the second pass, qv.cc:786-806);
		// a batch may bring the comparison's results as one word per read instead of the strings (a read has at most 31 chunks)
		const uint32_t gw = packed ? (uint32_t)pmeta : gate ? gate[rid] : 0u;
		auto gate_open = [&](uint32_t c) -> bool { return (gate || packed) ? ((gw >> (c & 31u)) & 1u) != 0u : (int)(int8_t)quals[off + c] - '8' < 0; };
		auto kmer_at = [&](uint32_t c) -> uint64_t { uint64_t b2 = 0; return packed ? pk_kmer[(off >> 5) + c] : encode32(p + 32 * c, b2); };
		if constexpr (STATS) { for (int i = 0; i < S_COUNT; i++) L.st.v[i] = 0; }
		L.st.add(S_READS, 1);
		L.st.add(S_INGEST, 9 * n);
		L.overflow = false;
		if (planes) L.cnt = planes[plane_tag[rid]].cnt;

		int cls = 0;
		if (packed) cls = (pmeta & PK_INVALID) ? 2 : (pmeta & PK_SKIP_N) ? 1 : 0;
		else {
			uint64_t bad = 0;
			for (uint32_t c = 0; c < n; c++) (void)encode32(p + 32 * c, bad);
			if (bad) cls = classify_bad(p, n);
		}
		if (cls == 1) L.st.add(S_READS_N, 1);
		if (cls == 0 && (gate || packed) && n > 32u) cls = 2;                       // (a gate word has 32 bits: the pack kernel counts such a read invalid too)
		if (cls == 2) { L.st.add(S_READS_INVALID, 1); if (invalid_reads) atomicAdd(invalid_reads, 1u); }
		if (cls == 0) {
			bool ok = false;
			L.reset_pass();
			for (uint32_t c = 0; c < n && !L.overflow; c++) L.do_chunk(kmer_at(c), c, gate_open(c));
			if (!L.overflow) ok = L.finish_pass();
			if (!L.overflow && !ok) {
				L.reset_pass();
				for (uint32_t c = 0; c < n && !L.overflow; c++) L.do_chunk(revcomp64(kmer_at(n - 1 - c)), c, gate_open(c));
				if (!L.overflow) (void)L.finish_pass();
			}
		}
		if (L.overflow) {
			const uint32_t at = atomicAdd(overflow_count, 1u);
			overflow_list[at] = (uint32_t)rid;
		} else if constexpr (STATS) {
			for (int i = 0; i < S_COUNT; i++) tot.v[i] += L.st.v[i];
		}
	}
	if constexpr (STATS) {
		for (int i = 0; i < S_COUNT; i++) if (tot.v[i]) atomicAdd(&stats[i], (unsigned long long)tot.v[i]);
	}
}



// The reads the deep tier leaves behind (listB: more vote keys or neighbour contexts than its LDS tables hold) are finished by the
// lane machine, one read per lane with its lists in HBM: 6-12 ms for the handful of 250 bp reads per 8 M that reach it, during
// which the batch's slot -- and with three slots the main stream -- waited (r05: 6.9 ms per step for 5.1 ms of kernels).  Counters
// are sums, so WHEN such a read is finished does not matter: this kernel copies the packed form of those reads (chunk k-mers + flag
// word) out of the batch's slot into a small store that belongs to the handle, the slot is free at once, and the lane machine runs
// over the store ONCE, when the caller next synchronises (finish_pending).  One 64-bit atomic reserves a read's place and its
// chunks' (reads << 32 | chunks: both cursors move together, so the offsets stay a prefix sum); what does not fit -- or has more
// chunks than a flag word has gate bits -- goes to the residual list and takes the per-batch lane launch as before.
// The store mixes the reads of every batch since the last synchronisation, and those batches may belong to different samples:
// each read carries the number of its sample plane (tag), and the lane machine's run bumps that plane.
constexpr uint32_t VG_MAX_SAMPLES = 65535;                               // (a tag is 16 bits wide)
struct LateStore {
	uint64_t *kmers = nullptr, *meta = nullptr, *offsets = nullptr;      // [cap_chunks + 2], [cap_reads], [cap_reads + 1] (offsets in bases: 32 x chunks before)
	uint16_t *tag = nullptr;                                             // [cap_reads] sample plane of the read's batch
	unsigned long long *state = nullptr;                                 // [0] reads << 32 | chunks reserved so far, [1] reads that fit (a prefix)
	uint32_t *lost = nullptr, *lost_n = nullptr;                         // reads that outgrew the lane machine's deep scratch too
	uint32_t cap_reads = 0, cap_chunks = 0;
};
__global__ __launch_bounds__(256) void vg_late_collect(LateStore ls, const uint64_t *__restrict__ pk_kmer, const uint64_t *__restrict__ pk_meta, const uint64_t *__restrict__ offsets,
                                                       const uint32_t *__restrict__ list, const uint32_t *__restrict__ n_list, uint32_t *__restrict__ residual, uint32_t *__restrict__ n_residual,
                                                       const uint32_t plane)
{
	const uint32_t n = *n_list;
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
		const uint32_t rid = list[i];
		const uint64_t off = offsets[rid];
		const uint32_t nch = (uint32_t)((offsets[rid + 1] - off) >> 5);
		bool kept = false;
		if (nch <= 32u) {
			const unsigned long long old = atomicAdd(&ls.state[0], (1ull << 32) | (unsigned long long)nch);
			const uint64_t r = old >> 32, c0 = old & 0xFFFFFFFFull;
			if (r < ls.cap_reads && c0 + nch <= ls.cap_chunks) {
				for (uint32_t c = 0; c < nch; c++) ls.kmers[c0 + c] = pk_kmer[(off >> 5) + c];
				ls.meta[r] = pk_meta[rid];
				ls.tag[r] = (uint16_t)plane;
				ls.offsets[r] = 32ull * c0;
				ls.offsets[r + 1] = 32ull * (c0 + nch);
				atomicMax(&ls.state[1], (unsigned long long)(r + 1));
				kept = true;
			}
		}
		if (!kept) residual[atomicAdd(n_residual, 1u)] = rid;
	}
}

// ------------------------------------------------------------------------------------------------
// kernels: FASTQ framing on the device (reference src/qv.cc:760-784: four fgets() per record)
//
// The text arrives as a STREAM of arbitrary byte chunks (vg_fastq_stream_push).  Everything a chunk's framing needs to know
// about its predecessor -- the bytes of the record the previous chunk ended in the middle of -- stays on the device, so the
// host never waits for a result: it only moves bytes.  A chunk's buffer keeps FQ_CARRY bytes free in front of the copied
// text; the carried bytes are put right before it and the chunk's text starts there.
// ------------------------------------------------------------------------------------------------
size_t vg_dev_scan_temp_bytes(size_t n_u32, size_t n_u64);                                             // vg_sort.hip
int vg_dev_exclusive_scan_u32(const uint32_t *in, uint32_t *out, size_t n, hipStream_t stream, void *tmp, size_t tmp_bytes);
int vg_dev_exclusive_scan_u64(const uint64_t *in, uint64_t *out, size_t n, hipStream_t stream, void *tmp, size_t tmp_bytes);

constexpr uint32_t FQ_TILE = 4096;                   // bytes per workgroup tile (256 lanes x 16 bytes)
constexpr uint32_t FQ_CARRY = 1u << 16;              // room in front of a chunk for the unfinished record of the chunk before (4 lines <= 4 KiB)

struct FqStream {                                    // one per handle, device resident
	unsigned long long consumed;                     // bytes of the stream framed into complete records so far
	unsigned long long records;                      // ... and their number
	unsigned long long last_record;                  // stream offset of the last of them
	uint32_t carry;                                  // bytes of the previous chunk's text that belong to its unfinished last record
	uint32_t poisoned;                               // a chunk could not be framed here: it and everything after it is left to the host
	// BAM streams (vg_fastq_stream_begin_bam): consumed / last_record are offsets in the inflated BAM stream, records counts kept records
	unsigned long long skipped_flag, skipped_empty;  // records skipped: secondary / supplementary; l_seq == 0
	unsigned long long repairs;                      // windows whose speculated entry was wrong and that were walked again
};
struct FqChunk {                                     // one per batch slot, device resident
	uint32_t start, len;                             // the chunk's text is buf[start, start + len)
	uint32_t n_reads;                                // complete records framed (0 when refused)
	uint32_t bad;                                    // this chunk needs the host's framing (a line beyond fgets' 1023 characters, ...)
	unsigned long long total;                        // bases of the batch
};

// carried bytes in front of the new text; start / length of the chunk's text.  bad_key (BGZF streams, else null): the inflate kernel's
// verdict on this chunk's blocks and all before them -- a bad block makes the chunk a refused one: nothing of it or behind it is framed
__global__ __launch_bounds__(256) void vg_fqs_prepare(const FqStream *__restrict__ st, FqChunk *__restrict__ ck, const uint8_t *__restrict__ prev_end, uint8_t *__restrict__ buf, uint32_t nbytes,
                                                      const unsigned long long *__restrict__ bad_key)
{
	const uint32_t c = prev_end ? st->carry : 0u;
	for (uint32_t i = threadIdx.x; i < c; i += 256) buf[FQ_CARRY - c + i] = prev_end[(int64_t)i - (int64_t)c];
	if (threadIdx.x == 0) { ck->start = FQ_CARRY - c; ck->len = c + nbytes; ck->n_reads = 0; ck->bad = st->poisoned | (bad_key && *bad_key != ~0ull ? 1u : 0u); ck->total = 0; }
}

// newlines per 4 KiB tile of the buffer (bytes outside the chunk's text do not count)
__global__ __launch_bounds__(256) void vg_fq_count_newlines(const uint8_t *__restrict__ buf, const FqChunk *__restrict__ ck, uint32_t *__restrict__ tile_cnt)
{
	__shared__ uint32_t wsum[4];
	const uint32_t lo = ck->start, hi = lo + ck->len;
	const uint32_t base = blockIdx.x * FQ_TILE + threadIdx.x * 16;
	uint32_t c = 0;
	if (base + 16 > lo && base < hi) {
		uint4 v;
		__builtin_memcpy(&v, buf + base, 16);                     // the buffer is padded to a whole tile
		const uint8_t *b = (const uint8_t *)&v;
		for (uint32_t j = 0; j < 16; j++) if (base + j >= lo && base + j < hi && b[j] == '\n') c++;
	}
	for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
	if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
	__syncthreads();
	if (threadIdx.x == 0) tile_cnt[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// line_start[g + 1] = byte after the g-th newline; line_start[0] = start of the text
__global__ __launch_bounds__(256) void vg_fq_line_starts(const uint8_t *__restrict__ buf, FqChunk *__restrict__ ck, const uint32_t *__restrict__ tile_off, uint32_t *__restrict__ line_start, uint32_t cap_lines)
{
	__shared__ uint32_t wsum[4];
	const uint32_t lo = ck->start, hi = lo + ck->len;
	const uint32_t base = blockIdx.x * FQ_TILE + threadIdx.x * 16;
	uint32_t mask = 0;
	if (base + 16 > lo && base < hi) {
		uint4 v;
		__builtin_memcpy(&v, buf + base, 16);
		const uint8_t *b = (const uint8_t *)&v;
		for (uint32_t j = 0; j < 16; j++) if (base + j >= lo && base + j < hi && b[j] == '\n') mask |= 1u << j;
	}
	const uint32_t c = (uint32_t)__popc(mask);
	uint32_t incl = c;
	const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(incl, o); if ((int)lane >= o) incl += y; }
	if (lane == 63) wsum[wv] = incl;
	__syncthreads();
	uint32_t g = tile_off[blockIdx.x] + incl - c;
	for (uint32_t w = 0; w < wv; w++) g += wsum[w];
	if (blockIdx.x == 0 && threadIdx.x == 0) line_start[0] = lo;
	while (mask) {
		const uint32_t j = (uint32_t)__ffs((int)mask) - 1;
		mask &= mask - 1;
		++g;
		if (g < cap_lines) line_start[g] = base + j + 1; else ck->bad = 1u;     // lines shorter than 8 bytes on average: host framing
	}
}

// one lane per record: read length = strlen(read line) - 1 (qv.cc:778); slots past the last record get length 0 (the scan
// that follows runs over the whole capacity).  A line longer than fgets' 1023 characters, or a quality line without a
// character for every chunk (it would expose the reference's stale buffer contents), refuses the chunk.
__global__ void vg_fq_record_lengths(const uint32_t *__restrict__ line_start, const uint32_t *__restrict__ n_lines_p, FqChunk *__restrict__ ck, uint64_t *__restrict__ rlen, uint32_t cap_rec, uint32_t cap_lines)
{
	const uint32_t n_lines = *n_lines_p;
	const uint32_t n_rec = n_lines + 1 <= cap_lines ? n_lines / 4 : 0u;
	if (blockIdx.x == 0 && threadIdx.x == 0 && (n_lines + 1 > cap_lines || n_rec > cap_rec)) ck->bad = 1u;
	for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= cap_rec; r += (uint64_t)gridDim.x * blockDim.x) {
		uint64_t len = 0;
		if (r < n_rec && r < cap_rec) {
			bool bad = false;
			for (int l = 0; l < 4; l++) bad |= (line_start[4 * r + l + 1] - line_start[4 * r + l]) > 1023u;
			len = line_start[4 * r + 2] - line_start[4 * r + 1] - 1u;             // the line's length minus its newline
			bad |= (line_start[4 * r + 4] - line_start[4 * r + 3] - 1u) < (len >> 5);
			if (bad) ck->bad = 1u;
		}
		rlen[r] = len;
	}
}

// after the offsets scan: the chunk's verdict, and the stream's state for the next chunk
__global__ void vg_fqs_finish(FqStream *__restrict__ st, FqChunk *__restrict__ ck, const uint32_t *__restrict__ n_lines_p, const uint32_t *__restrict__ line_start,
                              const uint64_t *__restrict__ offsets, uint32_t cap_rec)
{
	if (threadIdx.x != 0 || blockIdx.x != 0) return;
	if (st->poisoned || ck->bad) { st->poisoned = 1u; ck->bad = 1u; ck->n_reads = 0; ck->total = 0; return; }
	const uint32_t n_rec = *n_lines_p / 4;
	const uint32_t end = n_rec ? line_start[4 * n_rec] : ck->start;               // first byte after the last complete record
	const uint32_t used = end - ck->start, left = ck->len - used;
	if (left > FQ_CARRY) { st->poisoned = 1u; ck->bad = 1u; return; }            // an unfinished record of more than 64 KiB
	if (n_rec) st->last_record = st->consumed + (line_start[4 * (n_rec - 1)] - ck->start);
	st->consumed += used;
	st->records += n_rec;
	st->carry = left;
	ck->n_reads = n_rec;
	ck->total = offsets[n_rec < cap_rec ? n_rec : cap_rec];
}

// gather bases and quality characters of every record into the flat batch layout; a quality line shorter than the
// read keeps what the reference's buffer would hold there: its newline, then NULs (qv.cc:763, 836)
// The quality line is looked at here and nowhere else: all the path ever asks of it is whether character c is below '8' for the
// read's chunk numbers c (qv.cc:836, 943), so the batch carries one GATE WORD per read (bit c) instead of the strings.
__global__ __launch_bounds__(256) void vg_fq_gather(const uint8_t *__restrict__ text, const uint32_t *__restrict__ line_start, const uint64_t *__restrict__ offsets,
                                                    const FqChunk *__restrict__ ck, uint8_t *__restrict__ bases, uint32_t *__restrict__ gate)
{
	const uint64_t n_rec = ck->n_reads;
	const uint32_t lane = threadIdx.x & 63;
	const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
	for (uint64_t r = wave; r < n_rec; r += n_waves) {                          // one wave per record: coalesced copies
		const uint64_t o = offsets[r], len = offsets[r + 1] - o;
		const uint32_t s1 = line_start[4 * r + 1], s3 = line_start[4 * r + 3];
		const uint32_t qlen = line_start[4 * r + 4] - s3;                       // quality line incl. its newline
		for (uint64_t j = lane; j < len; j += 64) bases[o + j] = text[s1 + j];
		// (a record is only framed here when its quality line has a character for every chunk, vg_fq_record_lengths; a lane past
		// the line reads what the reference's buffer would hold there: its newline, then NULs)
		const uint32_t n = (uint32_t)(len >> 5);
		bool open = false;
		if (lane < n && lane < 32u) { const uint8_t q = lane < qlen ? text[s3 + lane] : (uint8_t)0; open = (int)(int8_t)q - '8' < 0; }
		const uint64_t m = __ballot(open);
		if (lane == 0) gate[r] = (uint32_t)m;
	}
}

// ------------------------------------------------------------------------------------------------
// kernel: BGZF blocks inflated on the device (vg_inflate.h is the decoder; this is its wave policy)
//
// ONE WAVE PER BGZF BLOCK, one-wave workgroups.  Symbol decoding inside a block is serial -- the position of a code is known only
// when the code before it has been read -- so the 64 lanes of the wave hold ONE decode state (bit buffer, positions: formed
// through readfirstlane, they live in SGPRs and the decode loop is scalar code with broadcast LDS look-ups) and share what is
// parallel: code tables, ring refills, match / stored copies, the CRC, the write-out.  A chunk holds some thousand blocks; they
// are independent (no shared window), and their output offsets are known from the ISIZE fields before a byte is decoded.
//
// LDS per workgroup (BzShared, 74 320 B: two blocks per CU of 160 KiB):
//   out   65 536 + 16   the block's output is assembled here: back-references never read global memory another lane has just
//                       written, and the text leaves in one coalesced pass at the end
//   ring   1 024        compressed input, refilled by one 16-byte load per lane; the next KiB waits in a register meanwhile
//   crc    4 096        slicing-by-4 table (second pass over the finished output: each lane a slice, combined by x^(8n) mod P)
//   t      3 648        code tables (vg_inflate.h)
// ------------------------------------------------------------------------------------------------
struct BzShared {
	uint32_t out32[VG_BGZF_MAX_ISIZE / 4 + 4];
	uint4 ring[64];
	VgCrcTab crc;
	VgInfTables t;
};

struct BzWaveIO {
	uint8_t *outp;                 // LDS: the block's output
	uint32_t *ring32;              // LDS: 256 words of input
	uint4 *ring16;
	const uint4 *src;              // global: the 16-byte aligned address at or below the payload
	const uint8_t *in;             // global: the payload
	uint32_t in_len, skew;         // payload bytes; in - (const uint8_t *)src
	uint32_t n_vec;                // 16-byte vectors of src that hold payload bytes: nothing beyond them is loaded
	uint32_t g0;                   // vector index of ring16[0]
	uint4 pre;                     // this lane's vector of the NEXT KiB (loaded while the ring's KiB is decoded)
	uint32_t wpos;                 // next word of the ring
	uint64_t bitbuf; uint32_t bitcnt;
	int32_t bits_left;             // payload bits not yet consumed; negative: the decoder ran past the end
	uint32_t ln;

	__device__ __forceinline__ uint32_t lane() const { return ln; }
	__device__ __forceinline__ static uint32_t lanes() { return 64; }
	__device__ __forceinline__ static void sync() { __syncthreads(); }            // (one wave: a wait for its own LDS traffic, no s_barrier)
	__device__ __forceinline__ static uint32_t u(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
	__device__ __forceinline__ uint4 load(uint32_t v) const { return v < n_vec ? src[v] : make_uint4(0, 0, 0, 0); }
	// the reader at payload byte `at` (<= in_len): ring and bit buffer start over
	__device__ __forceinline__ void seek(uint32_t at)
	{
		const uint32_t a = skew + at;
		g0 = a >> 4;
		sync();                                                              // (nobody still reads the ring's old contents)
		ring16[ln] = load(g0 + ln);
		pre = load(g0 + 64 + ln);
		sync();
		wpos = (a & 15u) >> 2;
		bitbuf = 0; bitcnt = 0;
		need();
		const uint32_t lead = (a & 3u) * 8u;                                 // bytes of the first word in front of `at`
		bitbuf >>= lead; bitcnt -= lead;
		bits_left = (int32_t)((in_len - at) * 8u);
	}
	__device__ __forceinline__ void need()
	{
		if (bitcnt <= 32) {
			if (wpos == 256) {                                               // the ring's KiB is used up: the waiting one takes its place
				sync();
				ring16[ln] = pre;
				g0 += 64;
				pre = load(g0 + 64 + ln);
				sync();
				wpos = 0;
			}
			const uint32_t w = u(ring32[wpos]);
			bitbuf |= (uint64_t)w << bitcnt;
			bitcnt += 32; wpos++;
		}
	}
	__device__ __forceinline__ uint32_t peek() const { return (uint32_t)bitbuf; }
	__device__ __forceinline__ void drop(uint32_t n) { bitbuf >>= n; bitcnt -= n; bits_left -= (int32_t)n; }
	__device__ __forceinline__ uint32_t bits(uint32_t n) { const uint32_t v = (uint32_t)bitbuf & ((1u << n) - 1u); drop(n); return v; }
	__device__ __forceinline__ void align_byte() { drop(bitcnt & 7u); }
	__device__ __forceinline__ bool overrun() const { return bits_left < 0; }
	__device__ __forceinline__ void put(uint32_t o, uint8_t b) { if (ln == 0) outp[o] = b; }
	// len bytes from `dist` back.  dist >= 64: a round of 64 lanes reads what earlier rounds (or earlier symbols) wrote.  dist < 64:
	// the copy replicates a period; every lane reads below o only -- bytes that were there before the copy began.
	__device__ __forceinline__ void copy(uint32_t o, uint32_t dist, uint32_t len)
	{
		sync();
		if (dist >= 64) {
			for (uint32_t base = 0; base < len; base += 64) {                // at most 5 rounds (len <= 258), 64 output bytes each
				const uint32_t j = base + ln;
				if (j < len) outp[o + j] = outp[o + j - dist];
				if (base + 64 < len) sync();
			}
		} else {
			for (uint32_t base = 0; base < len; base += 64) {
				const uint32_t j = base + ln;
				if (j < len) outp[o + j] = outp[o - dist + j % dist];
			}
		}
	}
	// a stored block's bytes straight from global memory; then the reader starts over behind them
	__device__ __forceinline__ bool stored_copy(uint32_t o, uint32_t n)
	{
		const uint32_t at = in_len - ((uint32_t)bits_left >> 3);             // byte-aligned here, and not past the end (the caller checked)
		if (n > in_len - at) return false;
		const uint8_t *s = in + at;
		for (uint32_t base = 0; base < n; base += 64 * 8) {                  // 512 output bytes per round
			uint8_t v[8];
#pragma unroll
			for (uint32_t k = 0; k < 8; k++) { const uint32_t j = base + k * 64 + ln; v[k] = j < n ? s[j] : (uint8_t)0; }
#pragma unroll
			for (uint32_t k = 0; k < 8; k++) { const uint32_t j = base + k * 64 + ln; if (j < n) outp[o + j] = v[k]; }
		}
		seek(at + n);
		return true;
	}
};

// grid = blocks of the chunk.  status[b] = the block's VG_INF_* result; a failing block writes no text and enters
// (its compressed offset << 4 | result) into *bad_key with atomicMin: the lowest failing block of the chunk / the stream.
__global__ __launch_bounds__(64) void vg_bgzf_inflate_kernel(const uint8_t *__restrict__ comp, const vg_bgzf_block *__restrict__ tab, uint32_t n_blocks,
                                                            uint8_t *__restrict__ text, uint32_t *__restrict__ status, unsigned long long *__restrict__ bad_key)
{
	__shared__ BzShared sh;
	const uint32_t b = blockIdx.x;
	if (b >= n_blocks) return;
	const vg_bgzf_block blk = tab[b];
	const uint32_t isize = blk.isize;
	BzWaveIO io;
	io.ln = threadIdx.x;
	io.outp = (uint8_t *)sh.out32;
	io.ring16 = sh.ring;
	io.ring32 = (uint32_t *)sh.ring;
	io.in = comp + blk.in_off;
	io.in_len = blk.in_len;
	io.skew = (uint32_t)((uintptr_t)io.in & 15u);
	io.src = (const uint4 *)(io.in - io.skew);
	io.n_vec = (io.skew + io.in_len + 15u) >> 4;
	int rc = VG_INF_ESIZE;
	if (isize <= VG_BGZF_MAX_ISIZE) {
		vg_crc_tab_build(io, sh.crc);
		io.seek(0);
		rc = vg_inflate_raw(io, sh.t, isize);
		if (rc == VG_INF_OK) {
			__syncthreads();
			uint32_t x = vg_crc32_share(sh.crc, io.outp, isize, io.ln, 64);
			for (int o = 32; o > 0; o >>= 1) x ^= __shfl_xor(x, o);
			if (x != blk.crc) rc = VG_INF_ECRC;
		}
	}
	rc = __builtin_amdgcn_readfirstlane(rc);
	if (rc == VG_INF_OK) {
		// the text leaves coalesced: bytes up to the destination's next word boundary, whole words (two LDS words funnelled), tail bytes
		uint8_t *dst = text + blk.text_off;
		const uint32_t head = min(isize, (4u - (uint32_t)((uintptr_t)dst & 3u)) & 3u);
		if (io.ln < head) dst[io.ln] = io.outp[io.ln];
		const uint32_t n_w = (isize - head) >> 2;
		uint32_t *dw = (uint32_t *)(dst + head);
		for (uint32_t w = io.ln; w < n_w; w += 64) {
			const uint32_t i = head + 4u * w, sft = (i & 3u) * 8u;
			const uint32_t lo = sh.out32[i >> 2], hi = sh.out32[(i >> 2) + 1];
			dw[w] = sft ? (lo >> sft) | (hi << (32u - sft)) : lo;
		}
		for (uint32_t i = head + 4u * n_w + io.ln; i < isize; i += 64) dst[i] = io.outp[i];
	}
	if (io.ln == 0) {
		status[b] = (uint32_t)rc;
		if (rc != VG_INF_OK) atomicMin(bad_key, (unsigned long long)blk.comp_off << 4 | (unsigned long long)rc);
	}
}

// ------------------------------------------------------------------------------------------------
// kernels: text deflated into BGZF blocks on the device (vg_deflate.h is the compressor; this is its wave policy)
//
// ONE WAVE PER BGZF BLOCK, one-wave workgroups, as above: blocks share no window, so a chunk of text is some thousand independent
// waves.  A lane owns one position of each group of 64: it hashes the four bytes there, measures the match against the table's
// candidate, forms the position's code if the group's scan emits it, and ORs the code's bits into the staging window at the
// offset the wave's prefix sum of the bit lengths gives it.  The text is read where it was uploaded (a block's 64 KiB stay in
// the caches for the few hundred groups that look back into them); only the tables live in LDS.
//
// LDS per workgroup (DfShared, 20 872 B: seven blocks per CU of 160 KiB):
//   hash  16 384        one word per hash value: position + 1 of the greatest position entered before the group (ds_max_u32)
//   stage    264        the group's bits (ds_or_b32); whole words leave for the block's slot in global memory, the rest is carried
//   mlen     128        the group's match lengths, read by the scan
//   crc    4 096        slicing-by-4 table (each lane a slice of the text, combined by x^(8n) mod P)
// The payload's length is known only when the block is done, so a block writes into a slot of its own (text bytes + VG_DEF_SLACK)
// and reports (payload bytes or 0 = stored, CRC32); the host sums the lengths and vg_bgzf_frame_kernel moves header, payload (or
// the stored text) and trailer to the block's place in the file.
// ------------------------------------------------------------------------------------------------
struct DfShared {
	VgDefShared d;
	VgCrcTab crc;
};
struct DfDynShared {
	VgDefDynShared d;
	VgCrcTab crc;
};

struct DefWaveIO {
	static constexpr uint32_t LANES = 64;
	uint32_t ln;
	__device__ __forceinline__ uint32_t lane() const { return ln; }
	__device__ __forceinline__ static uint32_t lanes() { return 64; }
	__device__ __forceinline__ static void sync() { __syncthreads(); }
	__device__ __forceinline__ static uint32_t u(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
	__device__ __forceinline__ static uint64_t ballot(uint64_t mine) { return __ballot(mine != 0); }       // (a lane's own bit is bit `lane`)
	__device__ __forceinline__ uint32_t scan(const uint32_t *v, uint32_t *off) const
	{
		uint32_t x = v[0];
		for (uint32_t d = 1; d < 64; d <<= 1) { const uint32_t y = (uint32_t)__shfl_up((int)x, d); if (ln >= d) x += y; }     // 6 steps
		off[0] = x - v[0];
		return u((uint32_t)__shfl((int)x, 63));
	}
	__device__ __forceinline__ static void max32(uint32_t *p, uint32_t v) { atomicMax(p, v); }
	__device__ __forceinline__ static void or32(uint32_t *p, uint32_t v) { atomicOr(p, v); }
	__device__ __forceinline__ static void add32(uint32_t *p, uint32_t v) { atomicAdd(p, v); }
};
// ... with the dynamic path's token buffer: the block's words of global memory
struct DefWaveDynIO : DefWaveIO {
	uint32_t *tok;
	__device__ __forceinline__ uint32_t *tokens() const { return tok; }
};

// text [0, nbytes) in blocks of `block` bytes (the last one shorter).  grid = blocks.  meta[b] = (payload bytes in the block's slot,
// or 0: store the block; CRC32 of its text).  A slot has slot_words words: at least (block + VG_DEF_SLACK) / 4.
__global__ __launch_bounds__(64) void vg_bgzf_deflate_kernel(const uint8_t *__restrict__ text, uint64_t nbytes, uint32_t block, uint32_t n_blocks,
                                                            uint32_t *__restrict__ slots, uint32_t slot_words, uint2 *__restrict__ meta)
{
	__shared__ DfShared sh;
	const uint32_t b = blockIdx.x;
	if (b >= n_blocks) return;
	const uint64_t at = (uint64_t)b * block;
	const uint32_t n = (uint32_t)min((uint64_t)block, nbytes - at);
	const uint8_t *t = text + at;
	DefWaveIO io;
	io.ln = threadIdx.x;
	vg_crc_tab_build(io, sh.crc);
	const uint32_t coded = vg_deflate_block(io, sh.d, t, n, slots + (uint64_t)b * slot_words);
	uint32_t x = vg_crc32_share(sh.crc, t, n, io.ln, 64);
	for (int o = 32; o > 0; o >>= 1) x ^= __shfl_xor(x, o);
	if (io.ln == 0) meta[b] = make_uint2(coded, x);
}

// The same in the dynamic mode (vg_deflate_block_dyn): pass 1 leaves the block's tokens in its tok_words words of `tokens` (at least
// the block's text bytes) and its symbol counts in LDS; the plan -- code lengths, header, the choice of the form -- is made in LDS,
// its serial part (the Huffman tree, the run-length coding of the lengths, the canonical codes) by lane 0; pass 2 reads the tokens
// back.  meta[b] means what it means above, so vg_bgzf_frame_kernel frames either kernel's blocks.  A kernel of its own, so that
// vg_bgzf_deflate_kernel keeps its LDS and registers.
//
// LDS per workgroup (DfDynShared, 22 152 B: seven blocks per CU of 160 KiB, as above):
//   pass 1's state 16 776   the table, window and match lengths of the kernel above; once pass 1 is done the same bytes hold
//                           the plan's tables: the 98-word window, three code tables, the header's symbols, the builder's scratch
//   counts          1 280   288 + 32 symbol counters (ds_add_u32)
//   crc             4 096
// Resources (the compiler's remarks for gfx950): 73 VGPRs, 104 SGPRs, no scratch, 2 waves per SIMD.
__global__ __launch_bounds__(64) void vg_bgzf_deflate_dyn_kernel(const uint8_t *__restrict__ text, uint64_t nbytes, uint32_t block, uint32_t n_blocks,
                                                                uint32_t *__restrict__ slots, uint32_t slot_words, uint32_t *tokens, uint32_t tok_words, uint2 *__restrict__ meta)
{
	__shared__ DfDynShared sh;
	const uint32_t b = blockIdx.x;
	if (b >= n_blocks) return;
	const uint64_t at = (uint64_t)b * block;
	const uint32_t n = (uint32_t)min((uint64_t)block, nbytes - at);
	const uint8_t *t = text + at;
	DefWaveDynIO io;
	io.ln = threadIdx.x;
	io.tok = tokens + (uint64_t)b * tok_words;
	vg_crc_tab_build(io, sh.crc);
	const uint32_t coded = vg_deflate_block_dyn(io, sh.d, t, n, slots + (uint64_t)b * slot_words);
	uint32_t x = vg_crc32_share(sh.crc, t, n, io.ln, 64);
	for (int o = 32; o > 0; o >>= 1) x ^= __shfl_xor(x, o);
	if (io.ln == 0) meta[b] = make_uint2(coded, x);
}

// vg_def_code_lengths alone: one wave per histogram.  grid = n_sets; freq and lens are [n_sets][n_sym], 2 <= n_sym <= 288.
struct DfLenShared {
	uint32_t freq[VG_DEF_LL_TAB];
	uint8_t len[VG_DEF_LL_TAB];
	VgDefLenScratch sc;
};
__global__ __launch_bounds__(64) void vg_def_code_lengths_kernel(const uint32_t *__restrict__ freq, uint32_t n_sets, uint32_t n_sym, uint32_t limit, uint8_t *__restrict__ lens)
{
	__shared__ DfLenShared sh;
	const uint32_t b = blockIdx.x;
	if (b >= n_sets) return;
	DefWaveIO io;
	io.ln = threadIdx.x;
	for (uint32_t s = io.ln; s < n_sym; s += 64) sh.freq[s] = freq[(uint64_t)b * n_sym + s];       // 64 counters per iteration
	__syncthreads();
	vg_def_code_lengths(io, sh.freq, n_sym, limit, sh.len, sh.sc);
	for (uint32_t s = io.ln; s < n_sym; s += 64) lens[(uint64_t)b * n_sym + s] = sh.len[s];        // 64 lengths per iteration
}

// grid = blocks.  Block b of the file goes to out + offs[b]: header, payload from its slot (or 01 LEN NLEN and the text), CRC32, ISIZE.
__global__ __launch_bounds__(64) void vg_bgzf_frame_kernel(const uint8_t *__restrict__ text, uint64_t nbytes, uint32_t block, uint32_t n_blocks,
                                                          const uint32_t *__restrict__ slots, uint32_t slot_words, const uint2 *__restrict__ meta,
                                                          const uint64_t *__restrict__ offs, uint8_t *__restrict__ out)
{
	const uint32_t b = blockIdx.x, ln = threadIdx.x;
	if (b >= n_blocks) return;
	const uint64_t at = (uint64_t)b * block;
	const uint32_t n = (uint32_t)min((uint64_t)block, nbytes - at);
	const uint8_t *t = text + at, *slot = (const uint8_t *)(slots + (uint64_t)b * slot_words);
	const uint32_t coded = meta[b].x, crc = meta[b].y;
	const uint32_t payload = coded ? coded : n + 5u, total = VG_BGZF_HEADER + payload + VG_BGZF_TRAILER;
	uint8_t *dst = out + offs[b];
	for (uint32_t i = ln; i < total; i += 64) {                       // 64 bytes of the block per iteration
		uint8_t v;
		if (i < VG_BGZF_HEADER) v = vg_bgzf_header_byte(i, payload);
		else if (i < VG_BGZF_HEADER + payload) {
			const uint32_t j = i - VG_BGZF_HEADER;
			v = coded ? slot[j] : j < 5 ? vg_def_stored_byte(j, n) : t[j - 5];
		} else {
			const uint32_t j = i - VG_BGZF_HEADER - payload;
			v = (uint8_t)((j < 4 ? crc : n) >> (8u * (j & 3u)));
		}
		dst[i] = v;
	}
}

// ------------------------------------------------------------------------------------------------
// kernels: plain gzip inflated on the device (vg_gunzip.h is the finder, the decoder and the resolve; this is their wave policy)
//
// A slot of compressed bytes is cut into fixed chunks; ONE WAVE PER CHUNK finds a block start in its range (vg_gz_find) and decodes
// from it into 16-bit symbols (vg_gz_decode), one decode state per wave as in BzWaveIO.  vg_gz_confirm compares each guess with its
// predecessor's exit, vg_gz_repair (one wave) decodes the mismatched chunks again in order and writes the slot's record and the
// chunks' output lengths; after the scan of those, vg_gz_windows (one workgroup, serial over the chunks) resolves each chunk's last
// 32 Ki symbols against a window it keeps in LDS, and vg_gz_resolve (a full grid) the rest; vg_gz_crc folds the text's CRC32.
//
// LDS per decode workgroup (GzShared, 70 144 B: two per CU of 160 KiB):
//   sym   65 536   the most recent 32 Ki symbols: back-references never read global memory another lane has just written
//   ring   1 024   compressed input, as in BzShared
//   t      3 648   code tables (vg_inflate.h)
// Symbols are also stored straight to the chunk's staging area in global memory, never read back by this kernel.
// ------------------------------------------------------------------------------------------------
struct GzFindShared { uint4 ring[64]; VgInfTables t; };
struct GzShared { uint16_t sym[VG_GZ_WINDOW]; uint4 ring[64]; VgInfTables t; };

struct GzWaveIO {
	typedef uint32_t opos;
	uint16_t *symp;                // LDS: the symbol ring (decode only)
	uint16_t *outg;                // global: the chunk's staging area
	uint32_t *ring32;              // LDS: 256 words of input
	uint4 *ring16;
	const uint4 *src;              // global: the 16-byte aligned address at or below the slot's first byte
	const uint8_t *in;             // global: the slot's bytes
	uint32_t in_len, skew;         // slot bytes; in - (const uint8_t *)src
	uint32_t n_vec;                // 16-byte vectors of src that hold slot bytes: nothing beyond them is loaded
	uint32_t g0;                   // vector index of ring16[0]
	uint4 pre;                     // this lane's vector of the NEXT KiB
	uint32_t wpos;                 // next word of the ring
	uint64_t bitbuf; uint32_t bitcnt;
	int32_t bits_left;             // slot bits not yet consumed; negative: the decoder ran past the end (in_len <= VG_GZ_SLOT_MAX: below 2^29)
	uint32_t ln;

	__device__ __forceinline__ void init(const uint8_t *in_, uint32_t in_len_, uint4 *ring, uint16_t *sym)
	{
		ln = threadIdx.x; symp = sym; outg = nullptr;
		ring16 = ring; ring32 = (uint32_t *)ring;
		in = in_; in_len = in_len_;
		skew = (uint32_t)((uintptr_t)in & 15u);
		src = (const uint4 *)(in - skew);
		n_vec = (skew + in_len + 15u) >> 4;
		g0 = 0; wpos = 0; bitbuf = 0; bitcnt = 0; bits_left = 0; pre = make_uint4(0, 0, 0, 0);
	}
	__device__ __forceinline__ void set_out(uint16_t *p) { outg = p; }
	__device__ __forceinline__ uint32_t lane() const { return ln; }
	__device__ __forceinline__ static uint32_t lanes() { return 64; }
	__device__ __forceinline__ static void sync() { __syncthreads(); }            // (one wave: a wait for its own LDS traffic, no s_barrier)
	__device__ __forceinline__ static uint32_t u(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
	__device__ __forceinline__ static uint64_t u64(uint64_t x) { return (uint64_t)u((uint32_t)x) | (uint64_t)u((uint32_t)(x >> 32)) << 32; }
	__device__ __forceinline__ static uint64_t ballot(bool p) { return __ballot(p); }
	__device__ __forceinline__ static uint32_t reduce_add(uint32_t x) { for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o); return x; }
	__device__ __forceinline__ static uint32_t reduce_max(uint32_t x) { for (int o = 32; o > 0; o >>= 1) x = max(x, (uint32_t)__shfl_xor(x, o)); return x; }
	__device__ __forceinline__ uint4 load(uint32_t v) const { return v < n_vec ? src[v] : make_uint4(0, 0, 0, 0); }
	// the reader at slot byte `at` (<= in_len): ring and bit buffer start over
	__device__ __forceinline__ void seek(uint32_t at)
	{
		const uint32_t a = skew + at;
		g0 = a >> 4;
		sync();                                                              // (nobody still reads the ring's old contents)
		ring16[ln] = load(g0 + ln);
		pre = load(g0 + 64 + ln);
		sync();
		wpos = (a & 15u) >> 2;
		bitbuf = 0; bitcnt = 0;
		need();
		const uint32_t lead = (a & 3u) * 8u;                                 // bytes of the first word in front of `at`
		bitbuf >>= lead; bitcnt -= lead;
		bits_left = (int32_t)((in_len - at) * 8u);
	}
	__device__ __forceinline__ void seek_bit(uint64_t bit)
	{
		const uint32_t at = (uint32_t)(bit >> 3);
		seek(at < in_len ? at : in_len);
		drop((uint32_t)bit & 7u);
	}
	__device__ __forceinline__ uint64_t bitpos() const { return (uint64_t)((int64_t)in_len * 8 - bits_left); }
	__device__ __forceinline__ void need()
	{
		if (bitcnt <= 32) {
			if (wpos == 256) {                                               // the ring's KiB is used up: the waiting one takes its place
				sync();
				ring16[ln] = pre;
				g0 += 64;
				pre = load(g0 + 64 + ln);
				sync();
				wpos = 0;
			}
			const uint32_t w = u(ring32[wpos]);
			bitbuf |= (uint64_t)w << bitcnt;
			bitcnt += 32; wpos++;
		}
	}
	__device__ __forceinline__ uint32_t peek() const { return (uint32_t)bitbuf; }
	__device__ __forceinline__ void drop(uint32_t n) { bitbuf >>= n; bitcnt -= n; bits_left -= (int32_t)n; }
	__device__ __forceinline__ uint32_t bits(uint32_t n) { const uint32_t v = (uint32_t)bitbuf & ((1u << n) - 1u); drop(n); return v; }
	__device__ __forceinline__ void align_byte() { drop(bitcnt & 7u); }
	__device__ __forceinline__ bool overrun() const { return bits_left < 0; }
	// symbol at output position s of this decode: in the ring, or (s < 0) a placeholder for the window in front of the entry
	__device__ __forceinline__ uint16_t sym_at(int32_t s) const { return s >= 0 ? symp[(uint32_t)s & (VG_GZ_WINDOW - 1u)] : (uint16_t)(0x8000 + (int32_t)VG_GZ_WINDOW + s); }
	__device__ __forceinline__ void store(uint32_t o, uint16_t v) { symp[o & (VG_GZ_WINDOW - 1u)] = v; outg[o] = v; }
	__device__ __forceinline__ void put(uint32_t o, uint8_t b) { if (ln == 0) store(o, b); }
	// len symbols from `dist` back (dist <= 32768: the ring holds them, or they are placeholders).  dist >= 64: a round of 64 lanes
	// reads what earlier rounds (or earlier symbols) wrote; a lane that writes the ring slot of position o + j - 32768 has read it
	// itself before.  dist < 64: the copy replicates a period; every lane reads below o only.
	__device__ __forceinline__ bool copy(uint32_t o, uint32_t dist, uint32_t len)
	{
		sync();
		if (dist >= 64) {
			for (uint32_t base = 0; base < len; base += 64) {                // at most 5 rounds (len <= 258), 64 output symbols each
				const uint32_t j = base + ln;
				if (j < len) store(o + j, sym_at((int32_t)(o + j) - (int32_t)dist));
				if (base + 64 < len) sync();
			}
		} else {
			for (uint32_t base = 0; base < len; base += 64) {
				const uint32_t j = base + ln;
				if (j < len) store(o + j, sym_at((int32_t)o - (int32_t)dist + (int32_t)(j % dist)));
			}
		}
		return true;
	}
	// a stored block's bytes straight from global memory; then the reader starts over behind them
	__device__ __forceinline__ bool stored_copy(uint32_t o, uint32_t n)
	{
		const uint32_t at = in_len - ((uint32_t)bits_left >> 3);             // byte-aligned here, and not past the end (the caller checked)
		if (n > in_len - at) return false;
		const uint8_t *s = in + at;
		sync();
		for (uint32_t j = ln; j < n; j += 64) store(o + j, s[j]);            // 64 output symbols per round
		seek(at + n);
		return true;
	}
};

// the device's buffers of one slot (all on the device)
struct GzSlotDev {
	const uint8_t *in; uint32_t in_len, n_chunks, chunk_bytes, entry_bit;
	uint64_t area;                 // staging symbols per chunk: chunk_bytes * ratio
	VgGzChunkRec *ck; uint16_t *stag; uint64_t *lens, *offs; VgGzSlotRec *rec; uint32_t *counters;     // counters: [0] mismatches, [1] full tests
};

// grid = chunks.  The record of every chunk starts over; chunk 0's guess is the slot's exact entry.
__global__ __launch_bounds__(64) void vg_gz_find(GzSlotDev d)
{
	__shared__ GzFindShared sh;
	const uint32_t c = blockIdx.x;
	if (c >= d.n_chunks) return;
	GzWaveIO io;
	io.init(d.in, d.in_len, sh.ring, nullptr);
	uint32_t tested = 0;
	uint64_t g = d.entry_bit;
	if (c) g = vg_gz_find_chunk(io, sh.t, d.in, (uint64_t)d.in_len, (uint64_t)c, (uint64_t)d.chunk_bytes, &tested);
	if (io.ln == 0) {
		VgGzChunkRec r = {};
		r.guess = g; r.entry = g;
		d.ck[c] = r;
		if (tested) atomicAdd(&d.counters[1], tested);
	}
}

// grid = chunks; a chunk without a guess has nothing to do.  From the guess to the first block boundary at or beyond the next guess.
__global__ __launch_bounds__(64) void vg_gz_decode(GzSlotDev d)
{
	__shared__ GzShared sh;
	const uint32_t c = blockIdx.x;
	if (c >= d.n_chunks) return;
	const uint64_t g = GzWaveIO::u64(d.ck[c].guess);
	if (g == VG_GZ_NONE) return;
	GzWaveIO io;
	io.init(d.in, d.in_len, sh.ring, sh.sym);
	const uint32_t nx = GzWaveIO::u(vg_gz_next_guess(d.ck, d.n_chunks, c));
	const uint64_t stop = nx < d.n_chunks ? GzWaveIO::u64(d.ck[nx].guess) : (uint64_t)d.in_len * 8;
	io.set_out(d.stag + (uint64_t)c * d.area);
	VgGzChunkRec r = {};
	r.guess = g;
	vg_gz_decode_chunk(io, sh.t, g, stop, (uint64_t)(nx - c) * d.area, &r);
	if (io.ln == 0) {
		VgGzChunkRec *o = d.ck + c;                                          // (the guess stays: other waves read it meanwhile)
		o->entry = r.entry; o->exit_bit = r.exit_bit; o->err_bit = r.err_bit; o->out_len = r.out_len; o->rc = r.rc; o->ended = r.ended; o->state = r.state;
	}
}

__global__ __launch_bounds__(256) void vg_gz_confirm(GzSlotDev d)
{
	const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c == 0 || c >= d.n_chunks || d.ck[c].guess == VG_GZ_NONE) return;
	if (!vg_gz_confirm_one(d.ck, c)) atomicAdd(&d.counters[0], 1u);
}

// one wave: the chain of the slot made final (at once when every chunk was confirmed), its record, the chunks' output lengths
__global__ __launch_bounds__(64) void vg_gz_repair(GzSlotDev d)
{
	__shared__ GzShared sh;
	GzWaveIO io;
	io.init(d.in, d.in_len, sh.ring, sh.sym);
	const bool all_ok = GzWaveIO::u(d.counters[0]) == 0;
	vg_gz_repair_chain(io, sh.t, d.ck, d.n_chunks, (uint64_t)d.in_len * 8, d.area, d.stag, all_ok, d.rec);
	__threadfence();                                                         // (lane 0's records, read by the other lanes below)
	__syncthreads();
	for (uint32_t c = io.ln; c <= d.n_chunks; c += 64) d.lens[c] = c < d.n_chunks && d.ck[c].state == VG_GZ_ST_VALID ? d.ck[c].out_len : 0;
	if (io.ln == 0) d.rec->tested = d.counters[1];
}

// One workgroup, serial over the chunks: the last 32 Ki symbols of every chunk on the chain -> bytes at text[offs[c] + ...], against
// the window of the 32 KiB in front of the chunk, which is kept in LDS (indexed by text position mod 32 KiB) -- no byte this kernel
// has written is read back from global memory.  `before` bytes of the member lie in front of text[0] (at most 32 KiB matter).
constexpr uint32_t GZ_WIN_T = 1024, GZ_WIN_PER = VG_GZ_WINDOW / GZ_WIN_T;
__global__ __launch_bounds__(GZ_WIN_T) void vg_gz_windows(GzSlotDev d, uint8_t *__restrict__ text, uint32_t before, unsigned long long *__restrict__ bad_bit)
{
	__shared__ uint8_t win[VG_GZ_WINDOW];
	const uint32_t tid = threadIdx.x;
	for (uint32_t i = tid; i < before; i += GZ_WIN_T) { const int64_t p = (int64_t)i - (int64_t)before; win[(uint64_t)p & (VG_GZ_WINDOW - 1u)] = text[p]; }
	__syncthreads();
	for (uint32_t c = 0; c < d.n_chunks; c++) {                              // serial over the chunks, 32 Ki symbols at most of each
		const uint32_t len = d.lens[c];
		if (len == 0) continue;
		const int64_t off = (int64_t)d.offs[c];
		const uint32_t first = len > VG_GZ_WINDOW ? len - VG_GZ_WINDOW : 0;
		const uint16_t *s = d.stag + (uint64_t)c * d.area;
		uint8_t v[GZ_WIN_PER];
		bool ok = true;
#pragma unroll
		for (uint32_t k = 0; k < GZ_WIN_PER; k++) {
			const uint32_t j = first + k * GZ_WIN_T + tid;
			v[k] = 0;
			if (j < len) {
				const uint16_t y = s[j];
				if (y < 0x8000u) v[k] = (uint8_t)y;
				else {
					const int64_t p = off - (int64_t)VG_GZ_WINDOW + (int64_t)(y - 0x8000u);
					if (p < -(int64_t)before) ok = false; else v[k] = win[(uint64_t)p & (VG_GZ_WINDOW - 1u)];
				}
			}
		}
		if (!ok) atomicMin(bad_bit, (unsigned long long)d.ck[c].entry);
		__syncthreads();                                                     // (every read of the old window is done)
#pragma unroll
		for (uint32_t k = 0; k < GZ_WIN_PER; k++) {
			const uint32_t j = first + k * GZ_WIN_T + tid;
			if (j < len) { win[(uint64_t)(off + j) & (VG_GZ_WINDOW - 1u)] = v[k]; text[off + j] = v[k]; }
		}
		__syncthreads();
	}
}

// A full grid over the slot's text: what vg_gz_windows left (all but the last 32 Ki symbols of a chunk) -> bytes.  A placeholder reads
// the 32 KiB in front of its chunk: written by vg_gz_windows, or text of the slot before.
constexpr uint32_t GZ_RES_T = 256, GZ_RES_PER = 16;
__global__ __launch_bounds__(GZ_RES_T) void vg_gz_resolve(GzSlotDev d, uint8_t *__restrict__ text, uint32_t text_len, uint32_t before, unsigned long long *__restrict__ bad_bit)
{
	const uint32_t base = blockIdx.x * (GZ_RES_T * GZ_RES_PER) + threadIdx.x;
	if (base >= text_len) return;
	// the chunk of text position `base`: the last c with offs[c] <= base
	uint32_t lo = 0, hi = d.n_chunks;
	while (hi - lo > 1) { const uint32_t m = lo + ((hi - lo) >> 1); if (d.offs[m] <= base) lo = m; else hi = m; }      // log2(chunks) steps
	uint32_t c = lo;
	for (uint32_t k = 0; k < GZ_RES_PER; k++) {
		const uint32_t i = base + k * GZ_RES_T;
		if (i >= text_len) break;
		while (c + 1 < d.n_chunks && d.offs[c + 1] <= i) c++;                // (forward only: at most the chunks of this tile)
		const uint32_t off = (uint32_t)d.offs[c], len = (uint32_t)d.lens[c], j = i - off;
		if (j >= len || j + VG_GZ_WINDOW >= len) continue;                   // (the tail is vg_gz_windows')
		uint8_t b;
		if (vg_gz_resolve_sym(d.stag[(uint64_t)c * d.area + j], text, (int64_t)off, (int64_t)before, &b)) text[i] = b;
		else atomicMin(bad_bit, (unsigned long long)d.ck[c].entry);
	}
}

// CRC32 of text[0, text_len), tiles of 64 KiB: each thread a slice (vg_crc32_share), the tile's CRC moved to its place by
// x^(8 * bytes behind it) mod P and folded into *crc by XOR.
constexpr uint32_t GZ_CRC_TILE = 65536;
struct GzBlockLanes {
	__device__ static uint32_t lane() { return threadIdx.x; }
	__device__ static uint32_t lanes() { return 256; }
	__device__ static void sync() { __syncthreads(); }
};
__global__ __launch_bounds__(256) void vg_gz_crc(const uint8_t *__restrict__ text, uint32_t text_len, uint32_t *__restrict__ crc)
{
	__shared__ VgCrcTab tab;
	__shared__ uint32_t acc;
	GzBlockLanes l;
	if (threadIdx.x == 0) acc = 0;
	vg_crc_tab_build(l, tab);
	const uint32_t t0 = blockIdx.x * GZ_CRC_TILE, n = min(GZ_CRC_TILE, text_len - t0);
	uint32_t x = vg_crc32_share(tab, text + t0, n, threadIdx.x, 256);
	for (int o = 32; o > 0; o >>= 1) x ^= __shfl_xor(x, o);
	if ((threadIdx.x & 63u) == 0) atomicXor(&acc, x);
	__syncthreads();
	if (threadIdx.x == 0) atomicXor(crc, vg_crc_mul(vg_crc_x8n(text_len - t0 - n), acc));
}

// ------------------------------------------------------------------------------------------------
// kernels: BAM records framed on the device (vg_bam.h is the record parser; this is its wave policy)
//
// A slot's BGZF blocks inflate into bam_raw (BAM_CARRY bytes free in front, like the text buffer); the unfinished record of the
// slot before is put right before them (vg_bam_prepare), so the slot's data starts at a record boundary -- in the first slot at
// the header's end.  Finding the records is a chain of block_size fields, serial by nature.  It is cut into FIXED WINDOWS of
// 64 KiB of the slot's data (VG_BAM_WINDOW; not BGZF blocks, which may hold one byte):
//   vg_bam_walk_windows   one wave per window.  The lanes test candidate offsets, 64 at a time from the window's start: the guess is the
//                    smallest one from which three consecutive records are plausible or the chain reaches the end of the data
//                    (offset 0 of the window is in the first round: files whose records never straddle BGZF blocks hit at once).
//                    Lane 0 then walks the chain from the guess to the window's end: kept records' offsets, counts, the exit
//   vg_bam_confirm   in parallel: window k is right iff its guess is window k-1's exit (window 0's entry is exact).  Counts the
//                    mismatches and finds the first
//   vg_bam_repair    one wave; returns at once when every window was confirmed.  Else the mismatched windows in order: each is
//                    walked again from its predecessor's (now final) exit, the new exit is compared with the next guess.  More than
//                    VG_BAM_MAX_REPAIRS of them refuse the chunk.  By induction from window 0 the result is exact whatever was guessed
//   vg_bam_lengths   per kept record: its offset into one table (behind a scan of the windows' counts), its length into the offsets
//                    array for the scan the text route uses too; the windows' verdicts and counts summed
//   vg_bam_finish    the chunk's verdict, the stream's state for the next slot
//   vg_bam_gather    one wave per record: bases as ASCII from the nibbles (reverse-complemented where flagged), the gate word
// Capacities follow from the slot's byte count alone: a record takes at least 37 bytes (records <= bytes / 36), and a read of l
// bases takes 36 + (l + 1) / 2 + l bytes of its record (bases <= 2/3 of the bytes).
// A chunk is refused -- the text stream's contract: FqChunk.bad, the stream poisoned, nothing of it or after it framed -- when a
// record's block_size is below what its fields announce or above VG_BAM_MAX_BLOCK, a read is longer than VG_BAM_MAX_READ bases, or
// the inflate kernel's bad_key is set.
// ------------------------------------------------------------------------------------------------
constexpr uint32_t BAM_CARRY = 1u << 16;             // room in front of a slot's bytes for the unfinished record of the slot before (at most 65 536 bytes)

struct BamWin {                                      // one per window
	uint32_t guess;                                  // the speculated entry (window 0: the exact one)
	uint32_t exit, n_kept, n_flag, n_empty, bad;     // VgBamWalk of the walk from the entry in force
};
struct BamSlotInfo {                                 // one per slot
	uint32_t n_mismatch, first_mismatch;             // vg_bam_confirm
	uint32_t repairs;
	uint32_t n_flag, n_empty;                        // sums over the windows (vg_bam_lengths)
	uint32_t bad;                                    // vg_bam_lengths' verdict: a window's walk was bad, or a record beyond the tables.  Not FqChunk.bad,
	                                                 // which that kernel's blocks read at entry: vg_bam_finish puts the two together
};

// carried bytes in front of the new ones; start / length of the slot's data (bad_key: see vg_fqs_prepare); first_record: stream offset
// of the header's end, used by the stream's first slot
__global__ __launch_bounds__(256) void vg_bam_prepare(FqStream *__restrict__ st, FqChunk *__restrict__ ck, BamSlotInfo *__restrict__ info, const uint8_t *__restrict__ prev_end,
                                                      uint8_t *__restrict__ buf, uint32_t nbytes, const unsigned long long *__restrict__ bad_key, unsigned long long first_record)
{
	uint32_t c = prev_end ? st->carry : 0u;
	if (c > BAM_CARRY) c = 0;                                               // (never: vg_bam_finish poisons the stream instead)
	for (uint32_t i = threadIdx.x; i < c; i += 256) buf[BAM_CARRY - c + i] = prev_end[(int64_t)i - (int64_t)c];
	if (threadIdx.x == 0) {
		ck->start = BAM_CARRY - c; ck->len = c + nbytes; ck->n_reads = 0; ck->bad = st->poisoned | (bad_key && *bad_key != ~0ull ? 1u : 0u); ck->total = 0;
		info->n_mismatch = 0; info->first_mismatch = VG_BAM_NONE; info->repairs = 0; info->n_flag = 0; info->n_empty = 0; info->bad = 0;
		if (!prev_end) st->consumed = first_record;                        // the stream's first slot: nothing is framed before the header's end
	}
}

// grid = windows the slot can have (its capacity: the carry's length is known on the device only)
__global__ __launch_bounds__(64) void vg_bam_walk_windows(const uint8_t *__restrict__ buf, const FqChunk *__restrict__ ck, BamWin *__restrict__ win, uint32_t *__restrict__ woff,
                                                  int32_t n_ref, uint32_t entry0)
{
	const uint32_t k = blockIdx.x, lane = threadIdx.x;
	const uint32_t len = ck->len;
	const uint8_t *d = buf + ck->start;
	const uint64_t w0 = (uint64_t)k * VG_BAM_WINDOW;
	if (ck->bad || (k > 0 && w0 >= len)) {                                  // a refused chunk; a window behind the data
		if (lane == 0) { BamWin e; e.guess = VG_BAM_NONE; e.exit = VG_BAM_NONE; e.n_kept = 0; e.n_flag = 0; e.n_empty = 0; e.bad = 0; win[k] = e; }
		return;
	}
	uint32_t guess = VG_BAM_NONE;
	if (k == 0) guess = entry0 <= len ? entry0 : len;
	else {
		// (each round tests 64 offsets; the loop is wave-uniform: it ends for all lanes at the first round with a hit, at the
		// window's end or at the data's)
		for (uint32_t base = 0; base < VG_BAM_WINDOW && w0 + base < len; base += 64) {
			const uint64_t c = w0 + base + lane;
			const bool hit = c < len && vg_bam_chain(d, len, c, n_ref);
			const uint64_t m = __ballot(hit);
			if (m) { guess = (uint32_t)(w0 + base) + (uint32_t)__ffsll((long long)m) - 1u; break; }
		}
	}
	if (lane == 0) {
		BamWin e;
		e.guess = guess;
		if (guess == VG_BAM_NONE) { e.exit = VG_BAM_NONE; e.n_kept = 0; e.n_flag = 0; e.n_empty = 0; e.bad = 0; }
		else {
			VgBamWalk w;
			vg_bam_walk(d, len, guess, w0 + VG_BAM_WINDOW, woff + (uint64_t)k * VG_BAM_WIN_RECS, VG_BAM_WIN_RECS, &w);
			e.exit = w.exit; e.n_kept = w.n_kept; e.n_flag = w.n_flag; e.n_empty = w.n_empty; e.bad = w.bad;
		}
		win[k] = e;
	}
}

// the windows of the slot's data: ceil(len / window), at least one
__device__ __forceinline__ uint32_t bam_windows(uint32_t len) { return len ? (uint32_t)(((uint64_t)len + VG_BAM_WINDOW - 1) / VG_BAM_WINDOW) : 1u; }

__global__ __launch_bounds__(256) void vg_bam_confirm(const FqChunk *__restrict__ ck, const BamWin *__restrict__ win, BamSlotInfo *__restrict__ info)
{
	if (ck->bad) return;
	const uint32_t n_win = bam_windows(ck->len);
	const uint32_t k = blockIdx.x * 256 + threadIdx.x;
	const bool miss = k >= 1 && k < n_win && (win[k].guess != win[k - 1].exit || win[k].guess == VG_BAM_NONE);
	const uint64_t m = __ballot(miss);
	if (m && (threadIdx.x & 63) == 0) {
		atomicAdd(&info->n_mismatch, (uint32_t)__popcll(m));
		atomicMin(&info->first_mismatch, k + (uint32_t)__ffsll((long long)m) - 1u);
	}
}

__global__ __launch_bounds__(64) void vg_bam_repair(const uint8_t *__restrict__ buf, FqChunk *__restrict__ ck, BamWin *__restrict__ win, uint32_t *__restrict__ woff, BamSlotInfo *__restrict__ info)
{
	if (ck->bad || info->n_mismatch == 0) return;                           // every window confirmed: nothing serial happens
	const uint32_t lane = threadIdx.x;
	const uint32_t len = ck->len, n_win = bam_windows(len);
	const uint8_t *d = buf + ck->start;
	uint32_t k = info->first_mismatch, repairs = 0;
	bool refuse = false;
	while (k < n_win) {                                                     // (k grows with every round)
		if (repairs == VG_BAM_MAX_REPAIRS) { refuse = true; break; }
		// window k - 1 is final: walk k again from its exit
		uint32_t next_guess_ok = 1;
		if (lane == 0) {
			const BamWin pv = win[k - 1];
			BamWin e = win[k];
			if (pv.bad) e.bad = 1;                                           // (the chunk is refused below)
			else {
				VgBamWalk w;
				w.exit = pv.exit; w.n_kept = 0; w.n_flag = 0; w.n_empty = 0; w.bad = 0;
				if (pv.exit != VG_BAM_NONE) vg_bam_walk(d, len, pv.exit, (uint64_t)(k + 1) * VG_BAM_WINDOW, woff + (uint64_t)k * VG_BAM_WIN_RECS, VG_BAM_WIN_RECS, &w);
				else w.bad = 1;
				e.exit = w.exit; e.n_kept = w.n_kept; e.n_flag = w.n_flag; e.n_empty = w.n_empty; e.bad = w.bad;
			}
			win[k] = e;
			if (e.bad) next_guess_ok = 2;
			else if (k + 1 < n_win) next_guess_ok = win[k + 1].guess == e.exit && e.exit != VG_BAM_NONE ? 1u : 0u;
		}
		repairs++;
		next_guess_ok = (uint32_t)__builtin_amdgcn_readfirstlane((int)next_guess_ok);
		if (next_guess_ok == 2) { refuse = true; break; }
		if (next_guess_ok == 0) { k++; continue; }
		// the next window whose guess is not its predecessor's exit (exits behind k + 1 have not changed), 64 windows per round
		uint32_t j = k + 2, found = VG_BAM_NONE;
		for (; j < n_win; j += 64) {
			const uint32_t q = j + lane;
			const bool miss = q < n_win && (win[q].guess != win[q - 1].exit || win[q].guess == VG_BAM_NONE);
			const uint64_t m = __ballot(miss);
			if (m) { found = j + (uint32_t)__ffsll((long long)m) - 1u; break; }
		}
		k = found;                                                           // VG_BAM_NONE: none is left
	}
	if (lane == 0) { info->repairs = repairs; if (refuse) ck->bad = 1u; }
}

// the windows' kept-record counts as an array for the scan (cnt[n_win_cap] = 0: the scan's last entry is the total)
__global__ __launch_bounds__(256) void vg_bam_counts(const FqChunk *__restrict__ ck, const BamWin *__restrict__ win, uint32_t n_win_cap, uint32_t *__restrict__ cnt)
{
	const uint32_t k = blockIdx.x * 256 + threadIdx.x;
	if (k <= n_win_cap) cnt[k] = k < n_win_cap && !ck->bad && k < bam_windows(ck->len) ? win[k].n_kept : 0u;
}

// per window (one wave each): its kept records' offsets and lengths into the slot's tables, at the window's place in the scan of
// the counts; the windows' verdicts (into info->bad); rlen behind the last record is zero (the scan that follows runs over the whole capacity)
__global__ __launch_bounds__(256) void vg_bam_lengths(const uint8_t *__restrict__ buf, const FqChunk *__restrict__ ck, const BamWin *__restrict__ win, const uint32_t *__restrict__ woff,
                                                      const uint32_t *__restrict__ rec_base, uint32_t n_win_cap, BamSlotInfo *__restrict__ info,
                                                      uint32_t *__restrict__ rec_off, uint64_t *__restrict__ rlen, uint32_t cap_rec)
{
	const bool chunk_bad = ck->bad != 0;
	const uint32_t len = ck->len, n_win = bam_windows(len);
	const uint8_t *d = buf + ck->start;
	const uint32_t total = chunk_bad ? 0u : min(rec_base[n_win_cap], cap_rec);
	const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, n_t = (uint64_t)gridDim.x * blockDim.x;
	for (uint64_t r = total + t; r <= cap_rec; r += n_t) rlen[r] = 0;
	if (chunk_bad) return;
	// one wave per window: the lanes share its records
	const uint32_t lane = threadIdx.x & 63;
	for (uint64_t k = t >> 6; k < n_win; k += n_t >> 6) {
		const BamWin e = win[k];
		if (lane == 0) {
			if (e.bad) info->bad = 1u;
			if (e.n_flag) atomicAdd(&info->n_flag, e.n_flag);
			if (e.n_empty) atomicAdd(&info->n_empty, e.n_empty);
		}
		const uint32_t b = rec_base[k];
		for (uint32_t i = lane; i < e.n_kept; i += 64) {
			const uint32_t off = woff[k * VG_BAM_WIN_RECS + i];
			VgBamRec rec;
			const uint32_t l = vg_bam_view(d, len, off, &rec) == VG_BAM_OK ? rec.l_seq : 0u;
			if (b + i < cap_rec) { rec_off[b + i] = off; rlen[b + i] = l; } else info->bad = 1u;
		}
	}
}

// after the offsets scan: the chunk's verdict, and the stream's state for the next slot.  text_off: offset in the inflated BAM
// stream of the slot's first new byte (buf[BAM_CARRY])
__global__ void vg_bam_finish(FqStream *__restrict__ st, FqChunk *__restrict__ ck, const BamWin *__restrict__ win, const BamSlotInfo *__restrict__ info, const uint32_t *__restrict__ rec_base,
                              uint32_t n_win_cap, const uint32_t *__restrict__ rec_off, const uint64_t *__restrict__ offsets, uint32_t cap_rec, unsigned long long text_off)
{
	if (threadIdx.x != 0 || blockIdx.x != 0) return;
	if (st->poisoned || ck->bad || info->bad) { st->poisoned = 1u; ck->bad = 1u; ck->n_reads = 0; ck->total = 0; return; }
	const uint32_t n_win = bam_windows(ck->len);
	const uint32_t end = win[n_win - 1].exit;                                // first byte not framed, relative to the data's start: a record boundary
	const uint32_t n_rec = rec_base[n_win_cap];
	if (end == VG_BAM_NONE || end > ck->len || ck->len - end > BAM_CARRY || n_rec > cap_rec) { st->poisoned = 1u; ck->bad = 1u; return; }
	const long long data0 = (long long)text_off - (long long)(BAM_CARRY - ck->start);   // stream offset of the data's first byte (the carried bytes' own)
	if (n_rec) st->last_record = (unsigned long long)(data0 + rec_off[n_rec - 1]);
	st->consumed = (unsigned long long)(data0 + end);
	st->records += n_rec;
	st->skipped_flag += info->n_flag; st->skipped_empty += info->n_empty; st->repairs += info->repairs;
	st->carry = ck->len - end;
	ck->n_reads = n_rec;
	ck->total = offsets[n_rec];
}

// one wave per record: the bases as ASCII from the nibbles, the gate word from the qualities
__global__ __launch_bounds__(256) void vg_bam_gather(const uint8_t *__restrict__ buf, const uint32_t *__restrict__ rec_off, const uint64_t *__restrict__ offsets,
                                                     const FqChunk *__restrict__ ck, uint8_t *__restrict__ bases, uint32_t *__restrict__ gate)
{
	const uint64_t n_rec = ck->n_reads;
	const uint32_t len = ck->len;
	const uint8_t *d = buf + ck->start;
	const uint32_t lane = threadIdx.x & 63;
	const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
	for (uint64_t r = wave; r < n_rec; r += n_waves) {
		const uint64_t o = offsets[r];
		const uint32_t off = rec_off[r];
		VgBamRec rec = {};
		// (the walk framed this record: its bytes are inside the data; the checks keep a lane from reading outside them all the same)
		const bool ok = vg_bam_view(d, len, off, &rec) == VG_BAM_OK && rec.l_seq == offsets[r + 1] - o && rec.min_block() <= rec.block_size && (uint64_t)len - off >= 4ull + rec.block_size;
		const uint32_t l = ok ? rec.l_seq : 0u;
		const uint64_t so = rec.seq_off(off), qo = rec.qual_off(off);
		const bool rev = rec.reversed();
		for (uint32_t j = lane; j < l; j += 64) bases[o + j] = vg_bam_base(d, so, l, rev, j);
		const bool open = ok && vg_bam_gate_bit(d, qo, l, rev, lane);
		const uint64_t m = __ballot(open);
		if (lane == 0) gate[r] = (uint32_t)m;
	}
}

// ------------------------------------------------------------------------------------------------
// host side of the handle
// ------------------------------------------------------------------------------------------------
static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// hipMalloc that waits for memory on its way back.  Device memory that a handle -- or a process that has just ended -- gave up is
// not there for the next allocation at once: the driver clears it first, about 88 GB in 2.4 s on this part, and until then the
// runtime's book (hipMemGetInfo) already counts it free while hipMalloc still says no (profiles/vram_release_lag_r06.txt: four
// small jobs one after the other, each with the whole device's widest tables, had 300 GB "in use" between them).  So a refusal is
// final only when the book agrees: while it says the bytes are free -- or the free figure is still growing -- the call is repeated,
// for at most $VG_ALLOC_WAIT_S seconds (default 20; 0 = one attempt).
static hipError_t vg_malloc_patient(void **p, size_t bytes)
{
	hipError_t e = hipMalloc(p, bytes);
	if (e == hipSuccess) return e;
	(void)hipGetLastError();
	const char *w = getenv("VG_ALLOC_WAIT_S");
	const double limit = w && *w ? atof(w) : 20.0;
	const double t0 = now_s();
	double grew = t0;
	size_t best = 0;
	while (now_s() - t0 < limit) {
		size_t fr = 0, tot = 0;
		if (hipMemGetInfo(&fr, &tot) != hipSuccess) { (void)hipGetLastError(); break; }
		if (fr > best + (256u << 20)) { best = fr; grew = now_s(); }
		if (fr < bytes && now_s() - grew > 4.0) break;           // somebody holds it: that is the answer
		usleep(100000);
		e = hipMalloc(p, bytes);
		if (e == hipSuccess) {
			if (getenv("VG_VERBOSE")) fprintf(stderr, "[vargeno_hip] hipMalloc(%.1f GB) waited %.1f s for memory the driver was still clearing\n", bytes / 1e9, now_s() - t0);
			return e;
		}
		(void)hipGetLastError();
	}
	return e;
}

// the driver calls behind vg_arena.h: one hipMalloc per handle
struct HipBlock {
	static void *alloc(uint64_t bytes)
	{
		void *p = nullptr;
		if (vg_malloc_patient(&p, bytes) != hipSuccess) return nullptr;
		return p;
	}
	static void free(void *p) { (void)hipFree(p); }
};
typedef DevArenaT<HipBlock> DevArena;

struct ScratchBuf {
	Scratch s{};
	size_t bytes = 0;
};

struct NoCopy { NoCopy() = default; NoCopy(const NoCopy &) = delete; NoCopy &operator=(const NoCopy &) = delete; };
// A buffer of a batch slot, device memory or page-locked host memory: grow-only, sized by its user before every batch.  A block that
// is too small is freed BEFORE the new one is asked for, and the capacity is zero meanwhile: a failed allocation leaves
// {nullptr, 0}, never a stale size.  The new block holds exactly `count` elements.
template <class T, bool PINNED>
struct SlotBuf : NoCopy {
	T *p = nullptr;
	uint64_t cap = 0;                                   // elements
	~SlotBuf() { release(); }
	int reserve(uint64_t count, const char *what)
	{
		if (count <= cap) return VG_OK;
		release();
		const hipError_t e = PINNED ? hipHostMalloc((void **)&p, (size_t)count * sizeof(T), hipHostMallocDefault) : hipMalloc((void **)&p, (size_t)count * sizeof(T));
		if (e != hipSuccess) { p = nullptr; return fail(e == hipErrorOutOfMemory ? VG_ENOMEM : VG_ENODEV, PINNED ? "hipHostMalloc(%s): %s" : "hipMalloc(%s): %s", what, hipGetErrorString(e)); }
		cap = count;
		return VG_OK;
	}
	void release()
	{
		if (p) (void)(PINNED ? hipHostFree(p) : hipFree(p));
		p = nullptr; cap = 0;
	}
};
template <class T> using DevBuf = SlotBuf<T, false>;
template <class T> using PinnedBuf = SlotBuf<T, true>;
// Buffers that share one capacity: all of them are freed before any is allocated (that bounds peak memory), and the last one has
// the size only when all of them have it.
template <class B>
static int reserve_together(std::initializer_list<B *> bufs, uint64_t count, const char *what)
{
	if (count <= (*(bufs.end() - 1))->cap) return VG_OK;
	for (B *b : bufs) b->release();
	for (B *b : bufs) { const int rc = b->reserve(count, what); if (rc) return rc; }
	return VG_OK;
}
struct SlotEvent : NoCopy {
	hipEvent_t e = nullptr;
	~SlotEvent() { if (e) (void)hipEventDestroy(e); }
	operator hipEvent_t() const { return e; }
};

// Per-batch resources.  A handle keeps NSLOT batches in flight: the wave tier of batch k+1 runs on the
// main stream while the (rare, latency-bound) lane tiers of batch k finish on the tail stream.
// (The buffers and events give themselves back when the handle is deleted: vg_index_close.)
constexpr int NSLOT = 3;            // (5 and 8 were measured: no gain at 8 M-read batches, 10-30 % slower at 1 M -- more pack kernels run ahead and get in the wave kernel's way)
struct Slot {
	DevBuf<uint32_t> listA, listB, listC;   // spill lists, one capacity (reserve_together): main -> deep tier (A), deep tier -> lane tier (B), lost (C)
	uint32_t *ctr = nullptr;              // this batch's counter block (the layout: vg_wave.h, CTR_WORK_MAIN)
	PinnedBuf<uint32_t> h_ctr;            // page-locked copy of ctr[0..7], made on the tail stream when the batch's tiers are done
	// what the generic lane tier needs should the deep tier leave reads behind: it is only launched then (harvest), never empty
	const uint8_t *lt_bases = nullptr, *lt_quals = nullptr; const uint64_t *lt_offsets = nullptr; const uint32_t *lt_gate = nullptr; bool lt_packed = false, lt_stats = false, lt_enqueued = false, lt_late = false;      // lt_late: the deep tier's leftovers went through vg_late_collect (the per-batch lane tier then only has the residual list: listA, ctr[6])
	DevBuf<uint64_t> pk_kmer, pk_meta;                                // packed reads of this batch
	DevBuf<uint8_t> st_bases, st_quals; DevBuf<uint64_t> st_offsets;  // staging of vg_reads_submit / vg_fastq_submit
	DevBuf<uint32_t> st_gate;                                         // gate words of a batch framed on the device
	PinnedBuf<uint64_t> hp_kmers, hp_meta, hp_offsets;                // page-locked HOST staging of a batch framed + packed on the host (hp_meta and hp_offsets: one capacity)
	DevBuf<uint8_t> fq_text; DevBuf<uint32_t> fq_lines, fq_tiles;     // FASTQ framing
	DevBuf<uint8_t> fq_tmp;                                           // scan scratch, bytes (grow-only: no allocation per chunk)
	DevBuf<FqChunk> fq_chunk;                                         // this chunk's framing results (one FqChunk), device resident
	uint64_t fq_text_len = 0;                                        // bytes of text copied into fq_text (after the FQ_CARRY gap)
	DevBuf<uint8_t> bz_comp; DevBuf<vg_bgzf_block> bz_tab; DevBuf<uint32_t> bz_status;   // a BGZF chunk: compressed bytes, block table, per-block results
	// a BAM chunk: the inflated bytes (BAM_CARRY free in front), per window its result and its kept records' offsets, the counts'
	// scan, the records' offsets in one table, the slot's sums
	DevBuf<uint8_t> bam_raw; DevBuf<BamWin> bam_win; DevBuf<uint32_t> bam_woff, bam_cnt, bam_rec; DevBuf<BamSlotInfo> bam_info;
	uint64_t bam_raw_len = 0;                                        // bytes inflated into bam_raw (after the BAM_CARRY gap)
	SlotEvent e_in;                                                  // the batch's buffers are complete (when another stream produced them)
	SlotEvent e_fq; bool fq_tail_wanted = false;                     // the NEXT chunk's prepare kernel reads this text's tail: recorded after it
	// the batch's timeline (harvest reads the times between them): the pack kernel on its stream; the wave kernel (main tier) on the main
	// stream; the deep tier behind it on the tail stream; the batch's counters on the host, behind the last of its tiers
	SlotEvent pack_begin, pack_end, wave_begin, wave_end, deep_end, batch_done;
	bool busy = false;
	uint32_t plane = 0;                                              // the sample this batch belongs to (acquire_slot): every tier of the batch counts into that plane
};

// One sample's counters and what else is kept per sample.  Plane 0 is d.cnt / d.cnt4 (inside the arena); a further plane is one
// block of 24 * n_sites + 16 bytes outside the plan (vg_samples_reserve): cnt4 first, cnt behind it.
struct Plane {
	PlanePtr p{nullptr, nullptr};
	bool dirty = false;                   // cnt4 holds increments not yet folded into cnt
	uint64_t invalid = 0;                 // reads of this sample the reference would have aborted on, since open / vg_counts_reset / vg_sample_reset
};

// Host state of a BGZF stream (vg_fastq_stream_begin_bgzf): pushes are cut anywhere, so the bytes of an incomplete block wait here
// for the next push; the block index (16 bytes per block) is what vg_fastq_stream_bgzf_locate answers from, until the next begin.
struct BgzfStream {
	std::vector<uint8_t> carry;                                   // an incomplete block's bytes (at most 64 KiB once a header is whole)
	uint64_t comp_pos = 0, text_pos = 0;                          // stream offsets of the first byte not yet handed to a slot: compressed, text
	std::vector<std::pair<uint64_t, uint64_t>> index;             // (text offset, compressed offset) of every block so far
	unsigned long long *d_key = nullptr;                          // device: lowest (compressed offset << 4 | VG_INF_*) of a failed block, ~0: none
	unsigned long long host_key = ~0ull;                          // the same for blocks checked on the host (chunks without text)
	uint64_t slot_text = 0;                                       // most text one slot takes: a longer push is split at block boundaries
	bool header_bad = false;                                      // a push met bytes that are no BGZF block: the stream is over
	std::vector<vg_bgzf_block> blocks, tab;                       // scratch of a push
	// a BAM stream (vg_fastq_stream_begin_bam): the leading blocks are inflated here until the header parses
	bool bam = false, bam_hdr_done = false, bam_not_bam = false;
	std::vector<uint8_t> bam_hdr;                                 // inflated bytes of the leading blocks, while the header is incomplete
	uint64_t bam_hdr_end = 0;                                     // offset of the first record in the inflated stream
	int32_t bam_n_ref = 0;
};

struct vg_index {
	int device = 0;
	hipStream_t stream = nullptr, tail = nullptr;   // pack + wave tier | deep wave tier of earlier batches, one after the other
	// ... and their lane tiers + the copies of their counters, on a stream of their own (r05).  On the one tail stream the deep wave
	// tier of batch k+1 waited for the lane tier of batch k: with 250 bp reads a batch's lane tier takes 5-12 ms (a handful of reads
	// with thousands of contexts, latency-bound) against 5 ms per step, and the main stream waited for its slots (6.9 ms per step).
	// (A stream per batch slot -- six streams in all -- was tried and cost the DEFAULT workload 6 % and chr22-scale 25 %
	// (profiles/ab_tail_streams_r05.txt): more streams than hardware queues, and the main stream shares one.)
	hipStream_t tail2 = nullptr;
	hipStream_t ingest = nullptr;                   // FASTQ framing + pack kernel of the next batch, under the current batch's wave kernel
	int pack_overlap = -1;                          // the pack kernel of batch k+1 on the ingest stream, under batch k's wave kernel: 1 always, 0 never (VG_PACK_OVERLAP), -1: small batches
	                                                // always, large ones when the main stream is busy (enqueue_batch has the rules and the measurements behind them).
	                                                // A pack workgroup (4 x 68 VGPRs, 10 752 B of LDS) does not fit beside FOUR main-tier workgroups of a CU (4 x 116 VGPRs per
	                                                // SIMD, 4 x 38 928 B), it fits beside three.  With its full grid (16 workgroups per CU) the pack kernel therefore takes the CUs
	                                                // in turns with the wave kernel and the step gains nothing (hg38 scale, 8 M reads: 2.742 against 2.750 / 2.764 ms); with ONE
	                                                // workgroup per CU it runs for about a wave kernel's duration beside three main-tier workgroups per CU: 2.60 against 2.69 / 2.71
	uint32_t pack_corun_wgs = 0;                    // the pack kernel's grid when it runs beside the wave kernel of a large batch: one workgroup per CU (VG_PACK_CORUN_WGS)
	uint64_t pack_small_reads = 2u << 20;           // batches of up to this many reads are "small" (VG_PACK_SMALL_READS: the tests send the fixtures' batches down the large batches' path)
	int pack_bpc = 16;                              // the pack kernel's full grid: workgroups (of PACK_WPB tiles at a time) per CU (VG_PACK_BPC)
	bool fuse_pack = VG_FUSE_PACK;                  // the main tier encodes the reads itself (experiment: a build with -DVG_FUSE_PACK; VG_NO_FUSE turns it off)
	hipEvent_t last_wave_end = nullptr;             // the end of the wave kernel enqueued last (a slot's wave_end): not reached yet = the main stream is busy
	bool ingest_stream = true;                      // VG_NO_INGEST_STREAM: FASTQ framing on the main stream too
	hipStream_t ingest_or_main() const { return ingest_stream ? ingest : stream; }     // where framing, and the copies of a packed batch, go
	DevIndex d{};
	DevArena arena;                       // the index's device memory (vg_arena.h): permanent arrays and the temporaries of its construction
	std::vector<void *> owned;            // device allocations of the index made with hipMalloc (small handle-lifetime buffers; everything, when the arena could not be set up)
	std::map<void *, uint64_t> owned_bytes;
	uint64_t arena_misses = 0, arena_miss_bytes = 0;      // requests the arena had no room for (served by hipMalloc)
	uint64_t dev_bytes = 0;               // device memory of the index: hipMalloc'ed buffers (counted as they are made) + the arena's mapped chunks (counted when construction is over)
	uint64_t n_sites = 0;
	std::vector<Plane> planes;                         // sample planes: [0] = d.cnt / d.cnt4; grown by vg_samples_reserve
	uint32_t cur_sample = 0;                           // the selected sample (vg_sample_select): new batches, fetch, all-reduce
	uint32_t fq_sample = 0;                            // the sample of the open FASTQ stream: the one selected at its begin
	PlanePtr *d_planes = nullptr;                      // [VG_MAX_SAMPLES] device copy of the planes' pointers (late-store run, fold)
	uint32_t *d_dirty = nullptr;                       // [VG_MAX_SAMPLES] numbers of the planes the next fold takes ...
	std::vector<uint32_t> dirty_up;                    // ... as last copied up: a handle with one plane never copies again
	std::vector<uint32_t> site_pos;
	std::vector<uint8_t> site_ref, site_alt, site_rf, site_af;
	ScratchBuf mid, big;                  // lane-tier scratch: every lane x 64 contexts; a few lanes x 16384 contexts
	Slot slot[NSLOT];
	int next_slot = 0;
	bool lane_tier_seen = false;          // some batch of this handle left reads for the per-batch lane tier (the late store did not take them): it is enqueued with every batch from then on
	LateStore late;                       // reads the deep tier left behind, kept for ONE lane-machine run at the next synchronisation (vg_late_collect)
	uint32_t late_h[4] = {0, 0, 0, 0};    // host copy of the store's counters at the last finish_pending
	bool late_dirty = false, late_stats = false;     // batches have been enqueued since the store was last run / they were counting-build batches
	uint64_t late_reads_run = 0;          // reads the late runs have finished since open
	bool spill_known = false;
	uint32_t spill_hint = 0;              // the deep tier's list of the last harvested batches (reads): sizes the next batch's deep-tier grid
	uint64_t cum[4] = {0, 0, 0, 0};       // since reset: [0] wave-tier overflow, [1] lane-tier overflow, [2] lost, [3] reads with a character other than ACGTN
	uint8_t *d_clamped = nullptr;         // [2 * n_sites] staging of vg_counts_fetch: min(63, sum), ref counts then alt counts
	// the caller kernel's buffers (vg_sample_calls_fetch): ONE block outside the plan, taken at the first call -- the sites' two
	// frequency columns, the u16 staging of the calls (4 bytes per site in all), the factor tables and the escape count
	void *d_call_block = nullptr;
	const uint8_t *d_site_rf = nullptr, *d_site_af = nullptr;
	uint16_t *d_calls = nullptr;
	const vg_caller_tables *d_call_tab = nullptr;
	unsigned long long *d_call_esc = nullptr;
	unsigned long long *d_stats = nullptr;
	bool stats_enabled = true;
	bool force_generic = false;           // VG_FORCE_GENERIC=1: skip the wave tier (tests compare the tiers)
	double t_pack = 0, t_main = 0, t_tail = 0, t_total = 0, t_w2 = 0; uint64_t t_batches = 0;   // harvested event times since the last vg_timing_get
	int cus = 256;
	int lane_grid_blocks = 0, wave_grid = 0;
	uint32_t work_chunk = 128;            // reads a main-tier wave pulls from the launch's work counter at a time (VG_WORK_CHUNK)
	uint32_t hold_pairs = VG_HOLD_PAIRS_DEFAULT;   // main tier: a wave runs stage B once this many gate-open pairs wait in it (VG_HOLD_PAIRS; 0: every iteration; at most PCAP -- vg_wave.h, "held pairs")
	uint32_t wave_wgs = 0;                // a cap on the main tier's workgroups (VG_WAVE_WGS; 0: none).  Tests and A/B runs only: one or two workgroups make a wave of a small batch live through dozens of refills
	uint64_t held_passes = 0;             // since reset: passes the main tier's waves have held (word CTR_HELD of a batch's counter block)
	uint32_t w2_chunk = 8, w2_wpc = 3;    // deep tier: reads a wave pulls at a time (VG_W2_CHUNK), workgroups per CU of its grid (VG_W2_WPC)
	bool w2_full_grid = false;            // ... and that grid for every batch, whatever the lists before were like (VG_W2_FULL_GRID)
	FqStream *d_fq = nullptr;             // FASTQ stream state (vg_fastq_stream_*)
	bool fq_open = false; int fq_prev_slot = -1;
	BgzfStream bz;                        // the BGZF side of a stream opened with vg_fastq_stream_begin_bgzf
	bool fq_bgzf = false;                 // the open FASTQ stream takes BGZF bytes
	struct GzipStream *gz = nullptr;      // the plain-gzip side of a stream opened with vg_fastq_stream_begin_gzip (kept until the next one: stats, checkpoints)
	bool fq_gzip = false;                 // the open FASTQ stream takes plain gzip bytes
	uint64_t max_device_bytes = 0;        // the caller's budget for this replica (vg_index_open_ex; 0: the whole device)
	std::string plan_text;                // what the budget bought: views kept / left out (vg_index_plan)
	std::string aux_note;                 // ... and what the loader found in the auxiliary rows, if anything
	std::string open_report;              // where vg_index_open's time went, phase by phase
	vgp::Packer *packer = nullptr;        // host-side framing + packing (vg_fastq_stream_begin_packed)
	bool fq_packed = false;               // the open FASTQ stream is framed + packed on the host
	uint64_t host_invalid = 0;            // reads with a character other than ACGTN found by the host packer since the last reset
};

// The index handle a thread is constructing (vg_index_open / vg_index_create run on the caller's thread; the CLI opens its replicas
// on one thread each): where TempDev finds the arena and the stream.
static thread_local vg_index *g_building = nullptr;
static thread_local double g_alloc_s = 0;                  // seconds spent inside allocation calls since the last lap (VG_VERBOSE)

// a permanent array of the index: out of the arena's bottom half; hipMalloc when the arena is not there (or `plain`: buffers that
// other libraries get to see -- RCCL reduces the counters in place)
template <class T>
static int dev_alloc(vg_index *ix, T **p, uint64_t count, bool zero = false, bool plain = false)
{
	void *q = nullptr;
	const size_t bytes = (size_t)(count ? count : 1) * sizeof(T);
	const double t0 = now_s();
	if (!plain) { q = ix->arena.take(bytes, false); if (!q && ix->arena.ready()) { ix->arena_misses++; ix->arena_miss_bytes += bytes; } }
	if (!q) {
		hipError_t e = vg_malloc_patient(&q, bytes);
		if (e != hipSuccess) { return fail(VG_ENOMEM, "hipMalloc(%s bytes): %s", std::to_string(bytes).c_str(), hipGetErrorString(e)); }
		ix->owned.push_back(q);
		ix->owned_bytes[q] = bytes;
		ix->dev_bytes += bytes;
	}
	g_alloc_s += now_s() - t0;
	if (zero) { hipError_t e = hipMemsetAsync(q, 0, bytes, ix->stream); if (e != hipSuccess) return fail(VG_ENODEV, "hipMemset: %s", hipGetErrorString(e)); }
	*p = (T *)q;
	return VG_OK;
}
// ... and one that is not needed any more (a jump table that a wider table has replaced); the device must be done with it
static void dev_release(vg_index *ix, const void *cp)
{
	void *p = const_cast<void *>(cp);
	if (!p) return;
	(void)hipStreamSynchronize(ix->stream);
	if (ix->arena.give(p)) return;
	for (size_t z = 0; z < ix->owned.size(); z++) if (ix->owned[z] == p) { ix->owned.erase(ix->owned.begin() + (long)z); break; }
	auto it = ix->owned_bytes.find(p);
	if (it != ix->owned_bytes.end()) { ix->dev_bytes -= it->second; ix->owned_bytes.erase(it); }
	(void)hipFree(p);
}
template <class T>
static int dev_upload(vg_index *ix, T **p, const T *src, uint64_t count)
{
	int rc = dev_alloc(ix, p, count);
	if (rc) return rc;
	if (count) HIP_TRY(hipMemcpy(*p, src, (size_t)count * sizeof(T), hipMemcpyHostToDevice));
	return VG_OK;
}
// a temporary of the construction, given back when it goes out of scope (or released earlier): out of the arena's top half while a
// handle is being built on this thread, hipMalloc otherwise.  Giving it back waits for the stream first, as hipFree does.
template <class T>
struct TempDev {
	T *p = nullptr;
	vg_index *ix = nullptr;                        // the handle whose arena holds p (nullptr: hipMalloc)
	~TempDev() { release(); }
	int alloc(uint64_t count)
	{
		release();
		const size_t bytes = (size_t)(count ? count : 1) * sizeof(T);
		const double t0 = now_s();
		if (g_building) { p = (T *)g_building->arena.take(bytes, true); if (p) ix = g_building; else if (g_building->arena.ready()) { g_building->arena_misses++; g_building->arena_miss_bytes += bytes; } }
		if (!p) {
			hipError_t e = vg_malloc_patient((void **)&p, bytes);
			if (e != hipSuccess) { p = nullptr; return fail(VG_ENOMEM, "hipMalloc(staging): %s", hipGetErrorString(e)); }
		}
		g_alloc_s += now_s() - t0;
		return VG_OK;
	}
	int upload(const T *src, uint64_t count)
	{
		int rc = alloc(count);
		if (rc) return rc;
		if (count) HIP_TRY(hipMemcpy(p, src, (size_t)count * sizeof(T), hipMemcpyHostToDevice));
		return VG_OK;
	}
	void release()
	{
		if (!p) return;
		const double t0 = now_s();
		if (ix) { (void)hipStreamSynchronize(ix->stream); (void)ix->arena.give(p); }
		else (void)hipFree(p);
		g_alloc_s += now_s() - t0;
		p = nullptr; ix = nullptr;
	}
};

static int alloc_scratch(vg_index *ix, ScratchBuf &b, uint32_t nlanes, uint32_t cap, uint32_t kcap)
{
	b.s.nlanes = nlanes; b.s.cap = cap; b.s.kcap = kcap;
	int rc;
	if ((rc = dev_alloc(ix, &b.s.ctx_kmer, (uint64_t)cap * nlanes))) return rc;
	if ((rc = dev_alloc(ix, &b.s.ctx_kpos, (uint64_t)cap * nlanes))) return rc;
	if ((rc = dev_alloc(ix, &b.s.ctx_meta, (uint64_t)cap * nlanes))) return rc;
	if ((rc = dev_alloc(ix, &b.s.key_index, (uint64_t)kcap * nlanes))) return rc;
	if ((rc = dev_alloc(ix, &b.s.key_first, (uint64_t)kcap * nlanes))) return rc;
	if ((rc = dev_alloc(ix, &b.s.key_fm, (uint64_t)kcap * nlanes))) return rc;
	b.bytes = ((uint64_t)cap * 16 + (uint64_t)kcap * 12) * nlanes;
	return VG_OK;
}

static void gzip_stream_free(struct GzipStream *gs);
extern "C" void vg_index_close(vg_index *ix)
{
	if (!ix) return;
	(void)hipSetDevice(ix->device);
	if (ix->stream) (void)hipStreamSynchronize(ix->stream);
	if (ix->tail) (void)hipStreamSynchronize(ix->tail);
	if (ix->tail2) (void)hipStreamSynchronize(ix->tail2);
	if (ix->ingest) (void)hipStreamSynchronize(ix->ingest);
	for (void *p : ix->owned) (void)hipFree(p);
	ix->arena.destroy();
	delete ix->packer;
	gzip_stream_free(ix->gz);
	if (ix->stream) (void)hipStreamDestroy(ix->stream);
	if (ix->tail) (void)hipStreamDestroy(ix->tail);
	if (ix->tail2) (void)hipStreamDestroy(ix->tail2);
	if (ix->ingest) (void)hipStreamDestroy(ix->ingest);
	delete ix;                            // (the batch slots' buffers and events go with it)
}

// Wall time of the phases of vg_index_open / vg_index_create (start-up is SURVEY.md §8f-4): kept in the handle (vg_index_open_report),
// and on stderr under VG_VERBOSE=1.  Every lap also says how much of it was spent inside allocation calls.
struct PhaseClock {
	vg_index *ix;
	const bool on = getenv("VG_VERBOSE") != nullptr;
	std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
	explicit PhaseClock(vg_index *h) : ix(h) { g_alloc_s = 0; }
	void lap(const char *what)
	{
		(void)hipDeviceSynchronize();
		const auto n = std::chrono::steady_clock::now();
		const double sec = std::chrono::duration<double>(n - t).count();
		char line[200];
		snprintf(line, sizeof line, "%s%s %.2f s (allocation calls %.2f s)", ix->open_report.empty() ? "" : "; ", what, sec, g_alloc_s);
		ix->open_report += line;
		if (on) fprintf(stderr, "[vargeno_hip] %-44s %.2f s  (allocation calls %.2f s)\n", what, sec, g_alloc_s);
		g_alloc_s = 0;
		t = n;
	}
};

// reader threads of the index loader
static unsigned host_threads()
{
	static const unsigned n = [] {
		unsigned h = std::thread::hardware_concurrency();
		if (const char *e = getenv("VG_HOST_THREADS")) h = (unsigned)std::max(1, atoi(e));
		return std::max(1u, std::min(h, 64u));
	}();
	return n;
}

// ------------------------------------------------------------------------------------------------
// index construction.  Everything from the dictionaries' columns onward happens on the device: the host only brings
// bytes (from the caller's arrays, or straight from the files -- read by several threads into pinned staging buffers and
// copied up while the next piece is being read; the packed records are unpacked by a kernel).
// ------------------------------------------------------------------------------------------------

// unpack the reference dictionary's 13-byte records {u64 k-mer, u32 pos, u8 ambig} (dictgen.c:63-154): a workgroup stages the
// 3 328 contiguous bytes of 256 records in LDS with 16-byte loads, then every lane takes its own record out of LDS
__global__ __launch_bounds__(256) void vg_unpack_ref(const uint8_t *__restrict__ raw, uint64_t n, uint64_t *__restrict__ kmer, uint32_t *__restrict__ pos, uint8_t *__restrict__ amb)
{
	__shared__ __attribute__((aligned(16))) uint8_t sm[256 * 13 + 48];
	for (uint64_t r0 = (uint64_t)blockIdx.x * 256; r0 < n; r0 += (uint64_t)gridDim.x * 256) {
		const uint64_t b0 = 13 * r0, a0 = b0 & ~15ull;              // the tile's first byte, and the 16-byte boundary below it (raw itself is aligned)
		const uint32_t shift = (uint32_t)(b0 - a0);
		const uint64_t nrec = n - r0 < 256 ? n - r0 : 256;
		const uint32_t nbytes = shift + 13u * (uint32_t)nrec;
		__syncthreads();                                            // previous tile fully consumed
		for (uint32_t i = threadIdx.x * 16; i < nbytes; i += 256 * 16) *reinterpret_cast<uint4 *>(sm + i) = *reinterpret_cast<const uint4 *>(raw + a0 + i);   // (the buffer has slack behind its last byte)
		__syncthreads();
		if (threadIdx.x < nrec) {
			const uint8_t *q = sm + shift + 13 * threadIdx.x;
			uint64_t k; uint32_t p2;
			__builtin_memcpy(&k, q, 8); __builtin_memcpy(&p2, q + 8, 4);
			const uint64_t i = r0 + threadIdx.x;
			kmer[i] = k; pos[i] = p2; amb[i] = q[12];
		}
	}
}
// ... the SNP dictionary's 16-byte records {u64 k-mer, u32 pos, u8 snp_info, ambig, ref_freq, alt_freq} (dictgen.c:156-275): one aligned 16-byte load each
__global__ void vg_unpack_snp(const uint8_t *__restrict__ raw, uint64_t n, uint64_t *__restrict__ kmer, uint32_t *__restrict__ pos,
                              uint8_t *__restrict__ info, uint8_t *__restrict__ amb, uint8_t *__restrict__ rf, uint8_t *__restrict__ af)
{
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		const uint4 v = *reinterpret_cast<const uint4 *>(raw + 16 * i);
		kmer[i] = ((uint64_t)v.y << 32) | v.x; pos[i] = v.z;
		info[i] = (uint8_t)v.w; amb[i] = (uint8_t)(v.w >> 8); rf[i] = (uint8_t)(v.w >> 16); af[i] = (uint8_t)(v.w >> 24);
	}
}
// ... auxiliary rows: the reference dictionary's are 10 x u32 already (copied bytewise: the file offset is not aligned); the SNP
// dictionary's are {u64 k-mer, 10 x {u32 pos, u8 snp_info, u8 ref_freq, u8 alt_freq}} = 78 bytes, of which the path reads pos and snp_info
__global__ void vg_unpack_ref_aux(const uint8_t *__restrict__ raw, uint64_t n_words, uint32_t *__restrict__ out)
{
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += (uint64_t)gridDim.x * blockDim.x) {
		const uint8_t *q = raw + 4 * i;
		out[i] = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
	}
}
__global__ void vg_unpack_snp_aux(const uint8_t *__restrict__ raw, uint64_t n_rows, uint32_t *__restrict__ pos, uint8_t *__restrict__ info)
{
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_rows * AUX_COLS; i += (uint64_t)gridDim.x * blockDim.x) {
		const uint8_t *q = raw + 78 * (i / AUX_COLS) + 8 + 7 * (i % AUX_COLS);
		pos[i] = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
		info[i] = q[4];
	}
}

// largest genome position any entry names (the reference sizes its pile-up table max(raw pos field) + 33, i.e. 2^32 + 32 entries as soon
// as one k-mer is POS_AMBIGUOUS; only real positions are ever indexed)
__global__ void vg_max_pos(const uint32_t *__restrict__ pos, const uint8_t *__restrict__ amb, uint64_t n, unsigned long long *out)
{
	unsigned long long m = 0;
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		const uint32_t p = pos[i];
		if ((!amb || amb[i] == 0) && p != POS_AMBIGUOUS && p > m) m = p;
	}
	for (int o = 32; o > 0; o >>= 1) { const unsigned long long y = __shfl_xor(m, o); m = y > m ? y : m; }
	if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}
// What the kernels take for granted about a dictionary and a corrupt file could violate: k-mers strictly increasing (the jump
// tables and every bisection), and an entry flagged "several positions" naming a row the auxiliary table has.  bad[0] / bad[1]
// count the violations; the caller refuses the index (a wild row index would be a wild read on the device).
__global__ void vg_check_columns(const uint64_t *__restrict__ kmer, const uint32_t *__restrict__ pos, const uint8_t *__restrict__ amb, uint64_t n, uint64_t n_aux,
                                 unsigned long long *bad)
{
	unsigned long long unsorted = 0, wild = 0;
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		if (i + 1 < n && kmer[i] >= kmer[i + 1]) unsorted++;
		if (amb[i] != 0 && pos[i] != POS_AMBIGUOUS && pos[i] >= n_aux) wild++;
	}
	if (unsorted) atomicAdd(&bad[0], unsorted);
	if (wild) atomicAdd(&bad[1], wild);
}
// An auxiliary row lists the positions of a k-mer with 2-10 occurrences (dictgen.c:63-154); they are distinct unless the SNP list
// holds the very same record several times (then the k-mer "occurs" that often at one position).  The wave kernel's key table
// gives a chunk one vote per key, so it has to know (DevIndex::aux_dups): it counts rows with a repeated position.
__global__ void vg_check_aux_rows(const uint32_t *__restrict__ rows, uint64_t n_rows, unsigned long long *dups)
{
	unsigned long long mine = 0;
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_rows; i += (uint64_t)gridDim.x * blockDim.x) {
		uint32_t v[AUX_COLS];
		for (int j = 0; j < AUX_COLS; j++) v[j] = rows[i * AUX_COLS + j];
		bool live = true, rep = false;
		for (int j = 0; j < AUX_COLS; j++) {
			live = live && v[j] != 0;
			if (!live) break;
			for (int k = 0; k < j; k++) rep = rep || v[k] == v[j];
		}
		if (rep) mine++;
	}
	if (mine) atomicAdd(dups, mine);
}
// Pile-up seeding in FILE ORDER, last writer wins (qv.cc:637-659): every position first learns the index of the LAST SNP-dictionary
// entry that seeds it ...
__global__ void vg_site_winner(const uint32_t *__restrict__ pos, const uint8_t *__restrict__ info, const uint8_t *__restrict__ amb, uint64_t n, uint32_t *__restrict__ winner)
{
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		const uint32_t f = info[i];
		if ((f & 4u) == 0 && pos[i] != POS_AMBIGUOUS && amb[i] == 0) atomicMax(&winner[(uint64_t)pos[i] + (f >> 3)], (uint32_t)(i + 1));   // n < 2^32 - 1
	}
}
// ... then every position applies that one entry: one wave per 64-position block -- the ballot of "is a site" is the block's rank mask
__global__ __launch_bounds__(256) void vg_site_blocks(const uint32_t *__restrict__ winner, const uint64_t *__restrict__ kmer, const uint8_t *__restrict__ info,
                                                      uint64_t plen, uint8_t *__restrict__ pile, ulonglong2 *__restrict__ rank, uint64_t *__restrict__ blk_sites)
{
	const uint64_t nblk = plen / 64 + 1;
	const uint32_t lane = threadIdx.x & 63;
	for (uint64_t b = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; b < nblk; b += ((uint64_t)gridDim.x * blockDim.x) >> 6) {
		const uint64_t p = b * 64 + lane;
		uint32_t w = 0;
		if (p < plen) {
			const uint32_t win = winner[p];
			if (win) {
				const uint32_t f = info[win - 1];
				w = (f & 3u) | (((uint32_t)(kmer[win - 1] >> (2 * (f >> 3))) & 3u) << 2);
			}
		}
		const bool site = (w & 3u) != ((w >> 2) & 3u);
		if (p < plen) pile[p] = (uint8_t)(w | (site ? 16u : 0u));
		const uint64_t m = __ballot(site);
		if (lane == 0) { rank[b] = make_ulonglong2(m, 0ull); blk_sites[b] = (uint64_t)__popcll(m); }
	}
}
__global__ __launch_bounds__(256) void vg_site_tables(const uint32_t *__restrict__ winner, const uint8_t *__restrict__ pile, const uint8_t *__restrict__ rf, const uint8_t *__restrict__ af,
                                                      uint64_t plen, ulonglong2 *__restrict__ rank, const uint64_t *__restrict__ blk_before,
                                                      uint32_t *__restrict__ s_pos, uint8_t *__restrict__ s_ref, uint8_t *__restrict__ s_alt, uint8_t *__restrict__ s_rf, uint8_t *__restrict__ s_af, uint8_t *__restrict__ s_ba)
{
	const uint64_t nblk = plen / 64 + 1;
	const uint32_t lane = threadIdx.x & 63;
	for (uint64_t b = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; b < nblk; b += ((uint64_t)gridDim.x * blockDim.x) >> 6) {
		const uint64_t before = blk_before[b], m = rank[b].x;
		if (lane == 0) rank[b].y = before;
		if ((m >> lane) & 1ull) {
			const uint64_t p = b * 64 + lane, s = before + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
			const uint32_t w = pile[p], win = winner[p];
			s_pos[s] = (uint32_t)p; s_ref[s] = (uint8_t)(w & 3u); s_alt[s] = (uint8_t)((w >> 2) & 3u); s_ba[s] = (uint8_t)(w & 15u);
			s_rf[s] = rf[win - 1]; s_af[s] = af[win - 1];
		}
	}
}

// the dictionaries' columns on the device: temporaries of the construction (freed when it is done)
struct DevCols {
	uint64_t n_ref = 0, n_ref_aux = 0, n_snp = 0, n_snp_aux = 0;
	TempDev<uint64_t> ref_kmer, snp_kmer;
	TempDev<uint32_t> ref_pos, snp_pos;
	TempDev<uint8_t> ref_amb, snp_info, snp_amb, snp_rf, snp_af;
	uint32_t *ref_aux = nullptr, *snp_aux_pos = nullptr; uint8_t *snp_aux_info = nullptr;     // final arrays, owned by the index
	int alloc()
	{
		int rc;
		if ((rc = ref_kmer.alloc(n_ref)) || (rc = ref_pos.alloc(n_ref)) || (rc = ref_amb.alloc(n_ref))) return rc;
		if ((rc = snp_kmer.alloc(n_snp)) || (rc = snp_pos.alloc(n_snp)) || (rc = snp_info.alloc(n_snp)) || (rc = snp_amb.alloc(n_snp)) || (rc = snp_rf.alloc(n_snp)) || (rc = snp_af.alloc(n_snp))) return rc;
		return VG_OK;
	}
};

static int init_handle(vg_index *ix, int device)
{
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(VG_ENODEV, "no HIP device available (this library has no CPU fallback)");
	if (device < 0 || device >= ndev) return fail(VG_EINVAL, "device index out of range");
	ix->device = device;
	HIP_TRY(hipSetDevice(device));
	HIP_TRY(hipStreamCreateWithFlags(&ix->stream, hipStreamNonBlocking));
	{
		// the spill tiers are a few hundred small workgroups that can only start when main-tier workgroups retire: with a
		// higher priority they are placed first at every such moment instead of queueing behind the next wave kernel
		int lo_p = 0, hi_p = 0;
		(void)hipDeviceGetStreamPriorityRange(&lo_p, &hi_p);
		if (getenv("VG_TAIL_PRIO") && atoi(getenv("VG_TAIL_PRIO")) == 0) hi_p = 0;
		HIP_TRY(hipStreamCreateWithPriority(&ix->tail, hipStreamNonBlocking, hi_p));
		HIP_TRY(hipStreamCreateWithPriority(&ix->tail2, hipStreamNonBlocking, hi_p));
	}
	HIP_TRY(hipStreamCreateWithFlags(&ix->ingest, hipStreamNonBlocking));
	if (const char *e = getenv("VG_PACK_OVERLAP")) ix->pack_overlap = atoi(e) != 0 ? 1 : 0;
	if (const char *e = getenv("VG_PACK_CORUN_WGS")) ix->pack_corun_wgs = (uint32_t)std::max(1, atoi(e));
	if (const char *e = getenv("VG_PACK_SMALL_READS")) ix->pack_small_reads = strtoull(e, nullptr, 10);
	if (const char *e = getenv("VG_PACK_BPC")) ix->pack_bpc = std::max(1, atoi(e));
	if (getenv("VG_NO_FUSE")) ix->fuse_pack = false;
	ix->ingest_stream = getenv("VG_NO_INGEST_STREAM") == nullptr;
	for (Slot &sl : ix->slot) {
		int rc = sl.h_ctr.reserve(16, "batch counters");
		if (rc) return rc;
		for (SlotEvent *ev : {&sl.pack_begin, &sl.pack_end, &sl.wave_begin, &sl.wave_end, &sl.deep_end, &sl.batch_done}) HIP_TRY(hipEventCreate(&ev->e));
		for (SlotEvent *ev : {&sl.e_fq, &sl.e_in}) HIP_TRY(hipEventCreateWithFlags(&ev->e, hipEventDisableTiming));
	}
	hipDeviceProp_t prop;
	HIP_TRY(hipGetDeviceProperties(&prop, device));
	ix->cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
	ix->lane_grid_blocks = ix->cus * 8;                          // 2048 lanes per CU = every wave slot
	int wpc = 16;                                                // waves per CU of the wave-tier grid: 128 VGPRs -> 4 waves per SIMD
	if (const char *e = getenv("VG_WAVES_PER_CU")) wpc = std::max(1, atoi(e));
	ix->wave_grid = ix->cus * wpc;
	if (const char *e = getenv("VG_FORCE_GENERIC")) ix->force_generic = atoi(e) != 0;
	if (const char *e = getenv("VG_WORK_CHUNK")) ix->work_chunk = (uint32_t)std::max(1, atoi(e));
	if (const char *e = getenv("VG_HOLD_PAIRS")) ix->hold_pairs = (uint32_t)std::min<long long>(std::max<long long>(0, atoll(e)), (long long)PCAP);
	if (const char *e = getenv("VG_WAVE_WGS")) ix->wave_wgs = (uint32_t)std::max(0, atoi(e));
	if (const char *e = getenv("VG_W2_CHUNK")) ix->w2_chunk = (uint32_t)std::max(1, atoi(e));
	if (const char *e = getenv("VG_W2_WPC")) ix->w2_wpc = (uint32_t)std::max(1, atoi(e));
	ix->w2_full_grid = getenv("VG_W2_FULL_GRID") != nullptr;
	return VG_OK;
}

// Which optional views a replica gets is decided BEFORE anything is built, from the dictionaries' sizes and a byte budget alone
// (vg_index_open_ex; without one: the device's total memory less 12 GiB) -- never from what happens to be free at that moment, so
// the same files and the same budget always give the same views (r03 asked hipMemGetInfo while building: a caller that shared
// the device got the slower layout without being told).  Views are taken in a fixed order while the planned total stays within
// the budget; vg_index_plan() says what was kept, what was left out and what that costs.
struct ViewPlan {
	bool mx = false, dx = false, sec = false, sig = false, probe = false, hx = false, jg32 = false, ssec = false;
	uint64_t base = 0, total = 0, budget = 0;
	uint64_t arena = 0;                    // bytes of the handle's one block (vg_arena.h): the finished index less what lives outside it
	bool limited = false;                  // views were left out for the budget
	uint32_t dx_bits = 32, ref_jg_bits = 32;   // buckets of the direct table / of the reference dictionary's jump table (DevIndex)
	std::string text;
	bool same_views(const ViewPlan &o) const { return mx == o.mx && dx == o.dx && sec == o.sec && sig == o.sig && probe == o.probe && hx == o.hx && jg32 == o.jg32 && ssec == o.ssec && dx_bits == o.dx_bits && ref_jg_bits == o.ref_jg_bits; }
};
// Tables that scale with the index AND the budget (r06).  The reference's jump table has 2^32 entries whatever the genome
// (qv.cc:539-584), and so had this library's direct table: a chr22-scale index (1 GB of files) took 92 GB of HBM, 99 % of it empty
// buckets.  A table over the top b bits of the same word finds the same entries as long as what the bucket leaves undecided is
// compared (ref_bounds, DevIndex::dx_bits), so the width is now a planning decision.  The NATURAL width of a table is the power of
// two at or above its entry count (0.5-1 entry per bucket, like hg38's 0.75 in 2^32; from 2^31 entries on that is 2^32 itself).
// Measured at chr22 scale (profiles/ab_chr22_table_bits_r06.txt): sparser is FASTER -- 2^32 buckets 0.333 ms per 1 M reads, 2^28
// 0.389, 2^27 (natural) 0.401, 2^26 0.437 -- because a bucket with two or more entries costs a second line and an empty or
// single-entry one is settled by its record; a table that would fit the 256 MB Infinity Cache is not faster for it (the L2-miss
// path is the limit).  So the plan takes the WIDEST table the budget holds, 2^32 first, then natural + 2 down to
// natural - 4: a whole device still gives the small index its 2^32 buckets, a budget of 8 GB gives it 2^27 and the same results.
// VG_DX_BITS / VG_REF_JG_BITS force a width (tests, A/B runs).
static uint32_t table_bits_for(uint64_t entries, const char *env)
{
	if (const char *e = getenv(env)) { const int b = atoi(e); if (b >= 16 && b <= 32) return (uint32_t)b; }
	uint32_t b = 16;
	while (b < 32 && (1ull << b) < entries) b++;
	return b >= 31 ? 32u : b;
}
static ViewPlan plan_views(const DevCols &c, uint64_t maxp, uint64_t ref_bf_bits, uint64_t snp_bf_bits, uint64_t budget_arg, uint64_t device_total, int cus)
{
	ViewPlan p;
	const uint64_t GiB = 1ull << 30, n = c.n_ref, m = c.n_snp, J32 = ((1ull << 32) + 1) * 4;
	p.budget = budget_arg ? budget_arg : (device_total > 12 * GiB ? device_total - 12 * GiB : device_total);
	const uint64_t plen = maxp + 64, sites = m / 32 + 1;                       // (an SNP seeds at most one site; ~32 k-mers per SNP)
	// lane-tier scratch: the deep one (a few lanes x 16384 contexts) always; the wide shallow one (every lane x 64 contexts) only for
	// the lane machine as the WHOLE path (VG_FORCE_GENERIC=1: tests compare the tiers) -- it was 0.74 GB that no other run touched
	const bool lane_only = getenv("VG_FORCE_GENERIC") && atoi(getenv("VG_FORCE_GENERIC")) != 0;
	const uint64_t scratch = (lane_only ? (uint64_t)cus * 8 * 256 * (64 * 16 + 32 * 12) : 0ull) + 4096ull * (16384 * 16 + 2048 * 12);
	p.ref_jg_bits = table_bits_for(n, "VG_REF_JG_BITS");         // (the mandatory part holds the natural width; 2^32 entries are an upgrade, below)
	const uint64_t Jref = ((1ull << p.ref_jg_bits) + 1) * 4;
	// what every layout holds: both dictionaries in file order with their jump tables, auxiliary rows, bit vectors, pile-up
	// sites and counters, lane-tier scratch, and room for three batch slots of a few million reads
	p.base = Jref + 16 * n + 40 * c.n_ref_aux + ((1ull << 24) + 1) * 4 + 16 * m + 50 * c.n_snp_aux + std::min<uint64_t>(ref_bf_bits, 1ull << 32) / 8 + snp_bf_bits / 8
	       + plen + plen / 4 + sites * 32 + scratch + 2 * GiB;
	p.total = p.base;
	const bool can_mx = !getenv("VG_NO_MX") && n + m < (1ull << 32);
	uint32_t bits = 14;
	while (bits < 30 && (1ull << bits) < n) bits++;
	char line[512];
	std::string kept, dropped;
	auto take = [&](bool allowed, uint64_t bytes, const char *name, const char *cost, bool &flag) {
		if (!allowed) return;
		if (p.total + bytes <= p.budget) { flag = true; p.total += bytes; snprintf(line, sizeof line, "%s%s %.1f GB", kept.empty() ? "" : ", ", name, bytes / 1e9); kept += line; }
		else { snprintf(line, sizeof line, "%s%s (%.1f GB; %s)", dropped.empty() ? "" : "; ", name, bytes / 1e9, cost); dropped += line; }
	};
	const bool want_probe = !getenv("VG_NO_PROBE_VIEW");
	take(want_probe && !getenv("VG_NO_SIG_VIEW"), (m + 16) * 2, "signature view of the strided SNP scan", "the scan reads the dictionary entries themselves: 11 lines per 8 entries instead of 1", p.sig);
	take(want_probe && getenv("VG_NO_SIG_VIEW") != nullptr, (m + 1) * 8, "probe view of the strided SNP scan", "the scan reads the dictionary entries themselves", p.probe);
	take(!getenv("VG_NO_SEC"), 12 * n + 16 + ((1ull << bits) + 1) * 4, "LO32-ordered view", "the 48 high-half neighbour queries of a gate-open chunk are made one by one: ~2 x the stage-B time", p.sec);
	if (can_mx) {
		// merged view + direct table together, the table as wide as the index wants it; under a budget that does not hold that, with
		// half and a quarter of the buckets (two and four entries' worth of key per bucket: more look-ups read a second line) before
		// the table is given up for the jump-table form (2^32 entries: the form the look-up without a direct table is written for)
		const uint32_t nat = table_bits_for(n + m, "VG_DX_BITS");
		const bool forced = getenv("VG_DX_BITS") != nullptr;
		uint32_t cand[8]; int nc = 0;
		if (forced) cand[nc++] = nat;
		else { cand[nc++] = 32u; for (int k = 2; k >= -4; k--) { const int b = (int)nat + k; if (b >= 16 && b < 32) cand[nc++] = (uint32_t)b; } }
		if (!getenv("VG_NO_DIRECT")) for (int ci = 0; ci < nc && !p.dx; ci++) {
			const uint32_t b = cand[ci];
			const uint64_t bytes = 16 * (n + m) + (1ull << b) * 16;
			if (p.total + bytes <= p.budget) {
				p.mx = p.dx = true; p.dx_bits = b; p.total += bytes;
				snprintf(line, sizeof line, "%smerged exact-match view %.1f GB, direct table of 2^%u buckets %.1f GB%s", kept.empty() ? "" : ", ", 16 * (n + m) / 1e9, b, (double)((1ull << b) * 16) / 1e9,
				         b + 1 == nat ? " (HALF the buckets the index wants: the budget)" : b + 2 == nat ? " (A QUARTER of the buckets the index wants: the budget)" : b + 2 < nat ? " (AN EIGHTH OR LESS of the buckets the index wants: the budget)" : b < 32u && ci > 0 ? " (the widest the budget holds; 2^32 is faster)" : "");
				kept += line;
			}
		}
		if (!p.dx) {
			take(true, 16 * (n + m) + J32, "merged exact-match view", "two look-ups per chunk instead of one, no both-strands shortcut: ~+45 % kernel time (r03 A/B)", p.mx);
			if (!getenv("VG_NO_DIRECT")) { snprintf(line, sizeof line, "%sdirect table (%.1f GB at 2^%u buckets; a jump-table gather in front of every exact look-up: ~+15 %% kernel time, r02 A/B)", dropped.empty() ? "" : "; ", (double)((1ull << (nat >= 18u ? nat - 2u : 16u)) * 16) / 1e9, nat >= 18u ? nat - 2u : 16u); dropped += line; }
		}
	} else {
		const bool want32 = !getenv("VG_NO_SNP_JG32");
		take(want32 && !getenv("VG_NO_HX"), ((1ull << 32) + 1) * 16 - (p.ref_jg_bits == 32u ? J32 : 0), "paired HI32 table", "separate jump tables, no absence filters: +25 % kernel time (r03: 6.34 vs 5.03 ms)", p.hx);
		take(want32 && !p.hx, J32, "HI32 jump table of the SNP dictionary", "SNP look-ups bisect HI24 buckets of ~190 entries: 8 dependent probes", p.jg32);
	}
	{
		uint32_t sb = 14;
		while (sb < 30 && (1ull << sb) < m) sb++;
		take(!getenv("VG_NO_SSEC") && m > 0, 12 * m + 16 + ((1ull << sb) + 1) * 4, "LO32-ordered view of the SNP dictionary", "the high-half SNP neighbour queries of a chunk whose SNP bit-vector probe is positive are made one by one: up to 36 bisections of a HI24 bucket, in stage B1's rounds", p.ssec);
	}
	if (p.ref_jg_bits < 32u && !getenv("VG_REF_JG_BITS") && !p.hx && p.total + (J32 - Jref) <= p.budget) {
		// the reference's own table, one entry per HI32 value: a gate-open chunk's bucket bounds in one gather (the coarse table reads
		// the bucket's entries to tell HI32 values apart: +7 % kernel time at chr22 scale)
		p.total += J32 - Jref; p.base += J32 - Jref; p.ref_jg_bits = 32u;
	}
	snprintf(line, sizeof line, "budget %.1f GB (%s): %.1f GB planned = %.1f GB of dictionaries, tables (reference jump table: 2^%u entries), sites and scratch", p.budget / 1e9,
	         budget_arg ? "the caller's, vg_index_open_ex" : "the device's memory less 12 GiB", p.total / 1e9, p.base / 1e9, p.ref_jg_bits);
	p.text = line;
	if (!kept.empty()) p.text += " + " + kept;
	p.text += dropped.empty() ? "; nothing left out" : "; LEFT OUT for the budget: " + dropped;
	if (p.base > p.budget) p.text += "; THE BUDGET IS BELOW THE SMALLEST LAYOUT";
	// the block holds everything but the batch slots (2 GiB reserved above, allocated with the first batches), the counters that
	// RCCL reduces in place and the clamped copy the host fetches (10 bytes per site); 64 MiB for the alignment of ~40 arrays
	p.arena = p.total - 2 * GiB - std::min<uint64_t>(sites * 10, p.total / 2) + (64ull << 20);
	// with views left out the finished index is smaller than what construction has alive at its peak (the columns beside the
	// entries, the sorts' buffers): the block then holds the permanent arrays only (vg_arena.h, set_temp_floor)
	p.limited = !dropped.empty() || (p.dx && p.dx_bits < table_bits_for(n + m, "VG_DX_BITS")) || (!getenv("VG_REF_JG_BITS") && !p.hx && p.ref_jg_bits < 32u && table_bits_for(n, "VG_REF_JG_BITS") < 32u);
	return p;
}

// From the columns (device) + the two bit vectors (host words) to the resident index.
// Device memory comes out of the handle's arena (vg_arena.h): permanent arrays with dev_alloc, temporaries as TempDev; one
// stream (ix->stream) carries every kernel, and a temporary is only given back after the stream has drained.  The ORDER below
// keeps what is alive at any moment -- permanent arrays so far + the temporaries of the step -- within the size of the finished
// index, which is the size of the arena: every column goes as soon as its last reader is done (the dictionaries' 16-byte entries
// are built early and serve the later steps in the columns' place), the radix sorts ping-pong between two buffer pairs, and
// neither wide table needs a jump table beside it (the entries carry their buckets).
static int build_on_device(vg_index *ix, DevCols &c, const ViewPlan &plan, uint64_t ref_bf_bits, const uint64_t *ref_bf_words, uint64_t snp_bf_bits, const uint64_t *snp_bf_words, PhaseClock &pc)
{
	int rc;
	DevIndex &d = ix->d;
	d.n_ref = c.n_ref; d.n_snp = c.n_snp;
	d.dx_bits = 32u; d.ref_jg_bits = 32u;
	d.ref_aux = c.ref_aux; d.snp_aux_pos = c.snp_aux_pos; d.snp_aux_info = c.snp_aux_info;
	hipStream_t st = ix->stream;
	// ---- largest position any entry names, and what a file that `vargeno index` did not write could get wrong: one wait for both
	unsigned long long maxp = 0;
	{
		TempDev<unsigned long long> dchk;                  // [0] max position, [1] k-mers out of order, [2] wild row indices, [3] rows that repeat a position
		if ((rc = dchk.alloc(4))) return rc;
		HIP_TRY(hipMemsetAsync(dchk.p, 0, 32, st));
		if (c.n_ref) vg_max_pos<<<2048, 256, 0, st>>>(c.ref_pos.p, c.ref_amb.p, c.n_ref, dchk.p);
		if (c.n_ref_aux) vg_max_pos<<<1024, 256, 0, st>>>(c.ref_aux, nullptr, c.n_ref_aux * AUX_COLS, dchk.p);
		if (c.n_snp) vg_max_pos<<<2048, 256, 0, st>>>(c.snp_pos.p, c.snp_amb.p, c.n_snp, dchk.p);
		if (c.n_snp_aux) vg_max_pos<<<1024, 256, 0, st>>>(c.snp_aux_pos, nullptr, c.n_snp_aux * AUX_COLS, dchk.p);
		if (c.n_ref) vg_check_columns<<<2048, 256, 0, st>>>(c.ref_kmer.p, c.ref_pos.p, c.ref_amb.p, c.n_ref, c.n_ref_aux, dchk.p + 1);
		if (c.n_snp) vg_check_columns<<<2048, 256, 0, st>>>(c.snp_kmer.p, c.snp_pos.p, c.snp_amb.p, c.n_snp, c.n_snp_aux, dchk.p + 1);
		if (c.n_ref_aux) vg_check_aux_rows<<<1024, 256, 0, st>>>(c.ref_aux, c.n_ref_aux, dchk.p + 3);
		if (c.n_snp_aux) vg_check_aux_rows<<<1024, 256, 0, st>>>(c.snp_aux_pos, c.n_snp_aux, dchk.p + 3);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipStreamSynchronize(st));
		unsigned long long chk[4] = {0, 0, 0, 0};
		HIP_TRY(hipMemcpy(chk, dchk.p, 32, hipMemcpyDeviceToHost));
		maxp = chk[0];
		d.aux_dups = chk[3] || getenv("VG_FORCE_AUX_DUPS") ? 1u : 0u;       // (the knob: tests drive the careful path on ordinary indexes)
		if (chk[3]) {
			char msg[200];
			snprintf(msg, sizeof msg, "%llu auxiliary rows repeat a position (the SNP list holds a record several times): rows are expanded column by column", chk[3]);
			ix->aux_note = msg;
		}
		if (chk[1] || chk[2]) {
			char msg[200];
			snprintf(msg, sizeof msg, "k-mers out of order in %llu places, %llu entries naming auxiliary rows the file does not have", chk[1], chk[2]);
			return fail(VG_EIO, "not an index `vargeno index` wrote: %s", msg);
		}
	}
	// ---- bit vectors: the reference addresses bit (hash % bits); hash32 is 32 bits wide, so only the first
	//      2^32 bits of the 9.6 Gbit reference vector can ever be read (src/generate_bf.h:112-128)
	{
		const uint64_t rbits = std::min<uint64_t>(ref_bf_bits, 1ull << 32);
		uint64_t *r = nullptr, *s2 = nullptr;
		if ((rc = dev_upload(ix, &r, ref_bf_words, (rbits + 63) / 64))) return rc;
		if ((rc = dev_upload(ix, &s2, snp_bf_words, (snp_bf_bits + 63) / 64))) return rc;
		d.ref_bf = r; d.ref_bf_bits = ref_bf_bits; d.snp_bf = s2; d.snp_bf_bits = snp_bf_bits;
	}
	{
		// the plan was made before anything was allocated, with the genome length <prefix>.chrlens gives (0 without it); what the
		// dictionaries really name decides the text -- and must still fit the budget
		size_t fr = 0, tot = 0;
		if (hipMemGetInfo(&fr, &tot) != hipSuccess) { (void)hipGetLastError(); tot = 0; }
		const ViewPlan real = plan_views(c, maxp, ref_bf_bits, snp_bf_bits, ix->max_device_bytes, (uint64_t)tot, ix->cus);
		ix->plan_text = real.same_views(plan) ? real.text : plan.text + "; (planned with the genome length of the .chrlens file: the dictionaries name positions beyond it)";
		if (!ix->aux_note.empty()) ix->plan_text += "; " + ix->aux_note;
		if (getenv("VG_VERBOSE")) fprintf(stderr, "[vargeno_hip] %s\n", ix->plan_text.c_str());
		if (real.base > real.budget) return fail(VG_ENOMEM, "the device-memory budget is below the smallest layout of this index: %s", real.text.c_str());
	}
	const bool want_mx = plan.mx;
	// sorted pairs end up in the FIRST buffer pair, the one allocated first and therefore higher in the arena: the pair that is
	// given back is the one next to the permanent arrays
	auto sort_into_a = [&](TempDev<uint64_t> &ka, TempDev<uint64_t> &kb, TempDev<uint32_t> &va, TempDev<uint32_t> &vb, uint64_t n) -> int {
		// (the sorts' own scratch is a few MB -- they ping-pong between the two buffer pairs, vg_sort.hip -- and lives only this long: a
		// temporary that outlives its step sits in a permanent array's way)
		TempDev<uint8_t> sort_tmp;
		const size_t sort_tmp_bytes = vg_dev_sort_pairs_temp_bytes((size_t)n);
		int rc2 = sort_tmp.alloc(sort_tmp_bytes);
		if (rc2) return rc2;
		bool in_b = false;
		const int se = vg_dev_sort_pairs_u64_u32(ka.p, kb.p, va.p, vb.p, n, st, sort_tmp.p, sort_tmp_bytes, &in_b);
		if (se != 0) return fail(VG_ENODEV, "device radix sort failed: %s", hipGetErrorString((hipError_t)se));
		if (in_b && n) {
			HIP_TRY(hipMemcpyAsync(ka.p, kb.p, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
			HIP_TRY(hipMemcpyAsync(va.p, vb.p, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
		}
		kb.release(); vb.release();
		return VG_OK;
	};
	pc.lap("checks, bit vectors");
	// ---- pile-up sites (src/qv.cc:602-603, 637-659): first, while little else is resident (their position-wide scratch is 4 bytes
	//      per genome position), and the SNP dictionary's frequency columns go right after
	{
		const uint64_t plen = maxp + 64, nblk = plen / 64 + 1;
		TempDev<uint32_t> winner; TempDev<uint64_t> blk; TempDev<uint8_t> tmp;
		if ((rc = winner.alloc(plen)) || (rc = blk.alloc(nblk + 1))) return rc;
		HIP_TRY(hipMemsetAsync(winner.p, 0, plen * 4, st));
		uint8_t *dp = nullptr; ulonglong2 *dr = nullptr;
		if ((rc = dev_alloc(ix, &dp, plen))) return rc;
		if ((rc = dev_alloc(ix, &dr, nblk))) return rc;
		if (c.n_snp) vg_site_winner<<<2048, 256, 0, st>>>(c.snp_pos.p, c.snp_info.p, c.snp_amb.p, c.n_snp, winner.p);
		vg_site_blocks<<<ix->cus * 16, 256, 0, st>>>(winner.p, c.snp_kmer.p, c.snp_info.p, plen, dp, dr, blk.p);
		HIP_TRY(hipMemsetAsync(blk.p + nblk, 0, 8, st));
		HIP_TRY(hipGetLastError());
		{
			const size_t need = vg_dev_scan_temp_bytes(1, nblk + 1);
			if ((rc = tmp.alloc(need))) return rc;
			const int se = vg_dev_exclusive_scan_u64(blk.p, blk.p, nblk + 1, st, tmp.p, need);
			if (se != 0) return fail(VG_ENODEV, "device scan failed: %s", hipGetErrorString((hipError_t)se));
		}
		HIP_TRY(hipStreamSynchronize(st));
		uint64_t nsites = 0;
		HIP_TRY(hipMemcpy(&nsites, blk.p + nblk, 8, hipMemcpyDeviceToHost));
		if (nsites >= (1ull << 31)) return fail(VG_ETOOBIG, "more than 2^31 SNP sites");
		ix->n_sites = nsites;
		TempDev<uint32_t> s_pos; TempDev<uint8_t> s_ref, s_alt, s_rf, s_af;
		uint8_t *dba = nullptr;
		if ((rc = s_pos.alloc(nsites)) || (rc = s_ref.alloc(nsites)) || (rc = s_alt.alloc(nsites)) || (rc = s_rf.alloc(nsites)) || (rc = s_af.alloc(nsites))) return rc;
		if ((rc = dev_alloc(ix, &dba, nsites + 1, true))) return rc;
		vg_site_tables<<<ix->cus * 16, 256, 0, st>>>(winner.p, dp, c.snp_rf.p, c.snp_af.p, plen, dr, blk.p, s_pos.p, s_ref.p, s_alt.p, s_rf.p, s_af.p, dba);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipStreamSynchronize(st));
		ix->site_pos.resize(nsites); ix->site_ref.resize(nsites); ix->site_alt.resize(nsites); ix->site_rf.resize(nsites); ix->site_af.resize(nsites);
		if (nsites) {
			HIP_TRY(hipMemcpy(ix->site_pos.data(), s_pos.p, nsites * 4, hipMemcpyDeviceToHost));
			HIP_TRY(hipMemcpy(ix->site_ref.data(), s_ref.p, nsites, hipMemcpyDeviceToHost));
			HIP_TRY(hipMemcpy(ix->site_alt.data(), s_alt.p, nsites, hipMemcpyDeviceToHost));
			HIP_TRY(hipMemcpy(ix->site_rf.data(), s_rf.p, nsites, hipMemcpyDeviceToHost));
			HIP_TRY(hipMemcpy(ix->site_af.data(), s_af.p, nsites, hipMemcpyDeviceToHost));
		}
		uint32_t *dc = nullptr, *dc4 = nullptr;
		if ((rc = dev_alloc(ix, &dc, 2 * nsites + 2, true, true))) return rc;       // (plain hipMalloc: RCCL reduces these in place)
		if ((rc = dev_alloc(ix, &dc4, 4 * nsites + 4, true))) return rc;
		d.srank = dr; d.pile = dp; d.pile_len = plen; d.cnt = dc; d.site_ba = dba; d.cnt4 = dc4;
		c.snp_rf.release(); c.snp_af.release();
	}
	pc.lap("pile-up sites");
	// ---- SNP dictionary: jump table over HI24, 16-byte entries, the strided scan's view; then its columns go (the k-mers stay for
	//      the merged view's keys, or -- an index without one -- for the HI32 jump table, if that is what the plan holds)
	{
		uint32_t *jg = nullptr; SnpEnt *ent = nullptr;
		if ((rc = dev_alloc(ix, &jg, (1ull << 24) + 1))) return rc;
		if ((rc = dev_alloc(ix, &ent, c.n_snp))) return rc;
		vg_build_jumpgate<<<(unsigned)((1ull << 24) / JG_SPAN), 256, 0, st>>>(c.snp_kmer.p, c.n_snp, jg, 1ull << 24, 40);
		vg_make_snp_entries<<<2048, 256, 0, st>>>(c.snp_kmer.p, c.snp_pos.p, c.snp_info.p, c.snp_amb.p, c.n_snp, ent);
		HIP_TRY(hipGetLastError());
		d.snp_jg = jg; d.snp = ent;
		c.snp_pos.release(); c.snp_info.release(); c.snp_amb.release();
		// the strided scan's view of the SNP dictionary: signatures (2 bytes per entry) by default, the probed values themselves
		// (8 bytes per entry) under VG_NO_SIG_VIEW, neither under VG_NO_PROBE_VIEW
		if (plan.sig) {
			uint16_t *sv = nullptr;
			if ((rc = dev_alloc(ix, &sv, c.n_snp + 16))) return rc;
			vg_make_snp_sig<<<2048, 256, 0, st>>>(c.snp_kmer.p, jg, c.n_snp, sv);
			HIP_TRY(hipGetLastError());
			d.snp_sig = sv;
		} else if (plan.probe) {
			uint64_t *pv = nullptr;
			if ((rc = dev_alloc(ix, &pv, c.n_snp + 1))) return rc;
			vg_make_snp_probe<<<2048, 256, 0, st>>>(c.snp_kmer.p, jg, c.n_snp, pv);
			HIP_TRY(hipGetLastError());
			d.snp_probe = pv;
		}
		// an index too large for the merged view and without the paired table gets a HI32 jump table of the SNP dictionary (17 GB):
		// its HI24 buckets hold ~190 entries there, 8 dependent bisection probes per look-up
		if (plan.jg32) {
			uint32_t *j32 = nullptr;
			if ((rc = dev_alloc(ix, &j32, (1ull << 32) + 1))) return rc;
			vg_build_jumpgate<<<(unsigned)((1ull << 32) / JG_SPAN), 256, 0, st>>>(c.snp_kmer.p, c.n_snp, j32, 1ull << 32, 32);
			HIP_TRY(hipGetLastError());
			d.snp_jg32 = j32;
		}
		// LO32-ordered view of the SNP dictionary: device radix sort of the swapped k-mers + a jump table over LO32's top bits
		if (plan.ssec && c.n_snp) {
			uint32_t sb = 14;
			while (sb < 30 && (1ull << sb) < c.n_snp) sb++;
			TempDev<uint64_t> ka, kb; TempDev<uint32_t> va, vb;
			if ((rc = ka.alloc(c.n_snp)) || (rc = va.alloc(c.n_snp))) return rc;
			vg_make_sec_keys<<<2048, 256, 0, st>>>(c.snp_kmer.p, c.n_snp, ka.p, va.p);
			HIP_TRY(hipGetLastError());
			if ((rc = kb.alloc(c.n_snp)) || (rc = vb.alloc(c.n_snp))) return rc;
			if ((rc = sort_into_a(ka, kb, va, vb, c.n_snp))) return rc;
			uint32_t *sjg = nullptr, *s3 = nullptr;
			if ((rc = dev_alloc(ix, &sjg, (1ull << sb) + 1))) return rc;
			if ((rc = dev_alloc(ix, &s3, 3 * c.n_snp + 4))) return rc;
			vg_build_jumpgate<<<(unsigned)((1ull << sb) / JG_SPAN), 256, 0, st>>>(ka.p, c.n_snp, sjg, 1ull << sb, (int)(64 - sb));
			vg_make_ssec3<<<2048, 256, 0, st>>>(ka.p, va.p, ent, c.n_snp, s3);
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipStreamSynchronize(st));
			d.ssec3 = s3; d.ssec_jg = sjg; d.ssec_bits = sb;
		}
		if (!want_mx) c.snp_kmer.release();
	}
	pc.lap("SNP dictionary, scan view, LO32-ordered view");
	// ---- reference dictionary: 16-byte entries, and -- unless the paired HI32 table will stand in for it -- the jump table over HI32
	{
		uint32_t *jg = nullptr; RefEnt *ent = nullptr;
		if (!plan.hx) {
			// (2^32 entries -- the reference's table, qv.cc:539-584 -- for an hg38-scale dictionary; a coarse table over the top bits of
			// HI32 for a small one: DevIndex::ref_jg_bits, ref_bounds)
			const uint32_t rb = plan.ref_jg_bits;
			if ((rc = dev_alloc(ix, &jg, (1ull << rb) + 1))) return rc;
			vg_build_jumpgate<<<(unsigned)(((1ull << rb) + JG_SPAN - 1) / JG_SPAN), 256, 0, st>>>(c.ref_kmer.p, c.n_ref, jg, 1ull << rb, (int)(64 - rb));
		}
		if ((rc = dev_alloc(ix, &ent, c.n_ref))) return rc;
		vg_make_ref_entries<<<2048, 256, 0, st>>>(c.ref_kmer.p, c.ref_pos.p, c.ref_amb.p, c.n_ref, ent);
		HIP_TRY(hipGetLastError());
		d.ref_jg = jg; d.ref = ent; d.ref_jg_bits = plan.hx ? 32u : plan.ref_jg_bits;
		c.ref_pos.release(); c.ref_amb.release();
		// secondary view ordered by (LO32, HI32): device radix sort of the swapped k-mers + a jump table over LO32's top bits
		if (plan.sec) {
			uint32_t bits = 14;
			while (bits < 30 && (1ull << bits) < c.n_ref) bits++;          // ~1-3 entries per bucket
			TempDev<uint64_t> ka, kb; TempDev<uint32_t> va, vb;
			if ((rc = ka.alloc(c.n_ref)) || (rc = va.alloc(c.n_ref))) return rc;
			vg_make_sec_keys<<<2048, 256, 0, st>>>(c.ref_kmer.p, c.n_ref, ka.p, va.p);
			HIP_TRY(hipGetLastError());
			if (!want_mx) c.ref_kmer.release();                    // (the merged view's keys are its last reader otherwise)
			if ((rc = kb.alloc(c.n_ref)) || (rc = vb.alloc(c.n_ref))) return rc;
			if ((rc = sort_into_a(ka, kb, va, vb, c.n_ref))) return rc;
			uint32_t *sjg = nullptr, *sec3 = nullptr;
			if ((rc = dev_alloc(ix, &sjg, (1ull << bits) + 1))) return rc;
			if ((rc = dev_alloc(ix, &sec3, 3 * c.n_ref + 4))) return rc;
			vg_build_jumpgate<<<(unsigned)((1ull << bits) / JG_SPAN), 256, 0, st>>>(ka.p, c.n_ref, sjg, 1ull << bits, (int)(64 - bits));
			vg_make_sec3<<<2048, 256, 0, st>>>(ka.p, va.p, ent, c.n_ref, sec3);
			// the reference bit vector against the dictionary: when they name the same LO32 values, the view answers qv.cc:955 too
			unsigned long long chk[3] = {1, 0, 0};
			if (ref_bf_bits >= (1ull << 32) && !getenv("VG_NO_BF_FROM_SEC")) {
				TempDev<unsigned long long> dchk;
				if ((rc = dchk.alloc(3))) return rc;
				HIP_TRY(hipMemsetAsync(dchk.p, 0, 24, st));
				vg_sec_bf_check<<<2048, 256, 0, st>>>(ka.p, c.n_ref, d.ref_bf, dchk.p);
				vg_popcount_words<<<2048, 256, 0, st>>>(d.ref_bf, (1ull << 32) / 64, dchk.p + 2);
				HIP_TRY(hipGetLastError());
				HIP_TRY(hipStreamSynchronize(st));
				HIP_TRY(hipMemcpy(chk, dchk.p, 24, hipMemcpyDeviceToHost));
			}
			HIP_TRY(hipGetLastError());
			d.sec3 = sec3; d.sec_jg = sjg; d.sec_bits = bits;
			d.sec_is_bf = (chk[0] == 0 && chk[1] == chk[2]) ? 1u : 0u;
		}
		if (!want_mx) c.ref_kmer.release();
	}
	pc.lap("reference dictionary + LO32-ordered view");
	// ---- paired HI32 table in place of the two HI32 jump tables (an index without merged view), from the entries' bucket words
	if (plan.hx) {
		uint4 *hx = nullptr;
		if ((rc = dev_alloc(ix, &hx, (1ull << 32) + 1))) return fail(VG_ENOMEM, "no room for the paired HI32 table although the plan had it -- is the device shared?  Pass a budget (vg_index_open_ex): %s", plan.text.c_str());
		HIP_TRY(hipMemsetAsync(hx, 0, ((1ull << 32) + 1) * 16, st));
		vg_hx_sentinel<<<1, 1, 0, st>>>(hx, (uint32_t)c.n_ref, (uint32_t)c.n_snp);
		if (c.n_ref) vg_hx_fill_ref<<<ix->cus * 32, 256, 0, st>>>(d.ref, c.n_ref, hx);
		if (c.n_snp) vg_hx_fill_snp<<<ix->cus * 32, 256, 0, st>>>(d.snp, c.n_snp, hx);
		if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return fail(VG_ENODEV, "building the paired HI32 table failed");
		d.hx = hx;
		pc.lap("paired HI32 table");
	}
	// ---- merged exact-match view (both dictionaries behind one HI32 table); its indices are 32 bits wide
	const uint64_t nm = c.n_ref + c.n_snp;
	unsigned long long quiet_cnt[3] = {0, 0, 0};
	if (want_mx) {
		TempDev<uint64_t> ka, kb; TempDev<uint32_t> va, vb;
		if ((rc = ka.alloc(nm))) return rc;
		if (c.n_ref) HIP_TRY(hipMemcpyAsync(ka.p, c.ref_kmer.p, (size_t)c.n_ref * 8, hipMemcpyDeviceToDevice, st));
		if (c.n_snp) HIP_TRY(hipMemcpyAsync(ka.p + c.n_ref, c.snp_kmer.p, (size_t)c.n_snp * 8, hipMemcpyDeviceToDevice, st));
		c.ref_kmer.release(); c.snp_kmer.release();            // 26 GB at hg38 scale: the sort's other buffers take their place
		TempDev<uint32_t> strand_bits;
		if ((rc = va.alloc(nm)) || (rc = strand_bits.alloc(nm / 32 + 2))) return rc;
		vg_iota_u32<<<2048, 256, 0, st>>>(va.p, nm);
		HIP_TRY(hipMemsetAsync(strand_bits.p, 0, (nm / 32 + 2) * 4, st));
		vg_canon_keys<<<2048, 256, 0, st>>>(ka.p, nm, strand_bits.p);
		HIP_TRY(hipGetLastError());
		if ((rc = kb.alloc(nm)) || (rc = vb.alloc(nm))) return rc;
		if ((rc = sort_into_a(ka, kb, va, vb, nm))) return rc;     // stable: ref before snp on equal k-mers
		uint32_t *mjg = nullptr; uint4 *mx = nullptr;
		if (!plan.dx) {
			if ((rc = dev_alloc(ix, &mjg, (1ull << 32) + 1))) return rc;
			vg_build_jumpgate<<<(unsigned)((1ull << 32) / JG_SPAN), 256, 0, st>>>(ka.p, nm, mjg, 1ull << 32, 32);
		}
		if ((rc = dev_alloc(ix, &mx, nm))) return rc;
		const uint32_t dxb = plan.dx ? plan.dx_bits : 32u;
		// quiet bits (vg_quiet.h): only the direct-table look-up reads them; VG_NO_QUIET=1 leaves every bit clear (A/B runs, parity tests)
		const bool want_quiet = plan.dx && !getenv("VG_NO_QUIET");
		TempDev<unsigned long long> qcnt;
		if (want_quiet) { if ((rc = qcnt.alloc(3))) return rc; HIP_TRY(hipMemsetAsync(qcnt.p, 0, 24, st)); }
		vg_make_mx_entries<<<2048, 256, 0, st>>>(ka.p, va.p, nm, c.n_ref, d.ref, d.snp, mx, strand_bits.p, dxb,
		                                         want_quiet ? reinterpret_cast<const unsigned long long *>(d.srank) : nullptr, d.pile_len, want_quiet ? qcnt.p : nullptr);
		HIP_TRY(hipGetLastError());
		if (want_quiet) {
			HIP_TRY(hipStreamSynchronize(st));
			HIP_TRY(hipMemcpy(quiet_cnt, qcnt.p, 24, hipMemcpyDeviceToHost));
		}
		ka.release(); va.release(); strand_bits.release();
		d.mx_jg = mjg; d.mx = mx;
		// direct table (64 GiB) in place of the merged jump table (16 GiB) when the plan has the room, from the entries' bucket
		// words; no bucket may exceed the 24-bit count field (it would be a >16 M-fold repeated 16-mer)
		if (plan.dx) {
			uint4 *dx = nullptr;
			TempDev<uint32_t> big;
			if ((rc = big.alloc(1))) return rc;
			HIP_TRY(hipMemsetAsync(big.p, 0, 4, st));
			uint32_t too_big = 0;
			if ((rc = dev_alloc(ix, &dx, 1ull << dxb))) return fail(VG_ENOMEM, "no room for the direct table although the plan had it -- is the device shared?  Pass a budget (vg_index_open_ex): %s", plan.text.c_str());
			HIP_TRY(hipMemsetAsync(dx, 0, (1ull << dxb) * 16, st));
			vg_make_direct<<<ix->cus * 32, 256, 0, st>>>(mx, nm, dx, d.ref_aux, d.snp_aux_pos, big.p, dxb);
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipStreamSynchronize(st));
			HIP_TRY(hipMemcpy(&too_big, big.p, 4, hipMemcpyDeviceToHost));
			if (too_big && dxb < 32u) {
				// a bucket of more than 255 entries in a table of fewer than 2^32 buckets (the mixed keys spread evenly: not seen): the entries
				// carry that table's field F, so the merged view goes with it -- the look-up takes both dictionaries' own tables instead
				dev_release(ix, dx); dx = nullptr;
				dev_release(ix, mx); mx = nullptr;
				d.mx = nullptr; d.mx_jg = nullptr;
				ix->plan_text += "; merged view + direct table not kept: a bucket of more than 255 entries";
			} else if (too_big) {
				// jump-table form after all: the 64 GiB go back, the jump table is made from the same bucket words
				dev_release(ix, dx); dx = nullptr;
				if ((rc = dev_alloc(ix, &mjg, (1ull << 32) + 1))) return rc;
				vg_jumpgate_from_buckets<<<ix->cus * 32, 256, 0, st>>>(mx, nm, mjg);
				HIP_TRY(hipGetLastError());
				d.mx_jg = mjg;
				ix->plan_text += "; direct table not kept: a bucket of more than 2^24 - 1 entries";
			} else { d.dx = dx; d.dx_bits = dxb; }
		}
		// (after the table: it reads the row form and the bucket words.  Without the table the entries keep the row form -- the
		// jump-table look-up expands rows itself -- and their bucket words, which nothing reads)
		if (d.dx) vg_inline_pairs<<<2048, 256, 0, st>>>(mx, nm, d.ref_aux, d.snp_aux_pos);
		HIP_TRY(hipGetLastError());
		if (d.dx) {
			// how many entries can vouch for a site-free window (tests read this to know that the bits were really set)
			char line[160];
			snprintf(line, sizeof line, "; quiet bits: A %llu, B %llu, both %llu of %llu mx entries", quiet_cnt[0], quiet_cnt[1], quiet_cnt[2], (unsigned long long)nm);
			ix->plan_text += line;
			if (getenv("VG_VERBOSE")) fprintf(stderr, "[vargeno_hip] %s\n", line + 2);
		}
		pc.lap("merged view, direct table");
	}
	// ---- scratch of the lane tier, overflow counters, stats
	// VG_SCRATCH_CAP / VG_SCRATCH_KCAP shrink the per-lane scratch so tests can drive every tier
	uint32_t cap = 64, kcap = 32;
	if (const char *e = getenv("VG_SCRATCH_CAP")) cap = (uint32_t)std::max(1, atoi(e));
	if (const char *e = getenv("VG_SCRATCH_KCAP")) kcap = (uint32_t)std::max(1, atoi(e));
	if (ix->force_generic && (rc = alloc_scratch(ix, ix->mid, (uint32_t)ix->lane_grid_blocks * 256u, cap, kcap))) return rc;
	if ((rc = alloc_scratch(ix, ix->big, 64u * 64u, 16384, 2048))) return rc;
	if (!getenv("VG_NO_LATE_STORE")) {
		// the late store (vg_late_collect): 65 536 reads / 2^20 chunks between two synchronisations (VG_LATE_READS: tests fill it up)
		LateStore &ls = ix->late;
		ls.cap_reads = 1u << 16; ls.cap_chunks = 1u << 20;
		if (const char *e = getenv("VG_LATE_READS")) { ls.cap_reads = (uint32_t)std::max(1, atoi(e)); ls.cap_chunks = std::min<uint32_t>(ls.cap_chunks, 32u * ls.cap_reads); }
		if ((rc = dev_alloc(ix, &ls.kmers, (uint64_t)ls.cap_chunks + 2, false, true)) || (rc = dev_alloc(ix, &ls.meta, ls.cap_reads, false, true)) || (rc = dev_alloc(ix, &ls.offsets, (uint64_t)ls.cap_reads + 1, false, true)) ||
		    (rc = dev_alloc(ix, &ls.lost, ls.cap_reads, false, true)) || (rc = dev_alloc(ix, &ls.lost_n, 1, true, true)) || (rc = dev_alloc(ix, &ls.state, 2, true, true)) ||
		    (rc = dev_alloc(ix, &ls.tag, ls.cap_reads, true, true))) return rc;
	}
	// sample planes: plane 0 is the counters above; the table and the fold's list have their full width from the start (1.25 MiB),
	// so that vg_samples_reserve adds the planes' own bytes and nothing else
	if ((rc = dev_alloc(ix, &ix->d_planes, VG_MAX_SAMPLES, false, true)) || (rc = dev_alloc(ix, &ix->d_dirty, VG_MAX_SAMPLES, true, true))) return rc;
	ix->planes.assign(1, Plane());
	ix->planes[0].p = PlanePtr{ix->d.cnt, ix->d.cnt4};
	ix->dirty_up.assign(1, 0u);
	HIP_TRY(hipMemcpy(ix->d_planes, &ix->planes[0].p, sizeof(PlanePtr), hipMemcpyHostToDevice));
	for (Slot &sl : ix->slot) if ((rc = dev_alloc(ix, &sl.ctr, 16, true, true))) return rc;       // sixteen words a batch; the layout: vg_wave.h, CTR_WORK_MAIN
	if ((rc = dev_alloc(ix, &ix->d_clamped, 2 * ix->n_sites + 2, false, true))) return rc;
	if ((rc = dev_alloc(ix, &ix->d_fq, 1, true, true))) return rc;
	if ((rc = dev_alloc(ix, &ix->bz.d_key, 1, true, true))) return rc;
	if ((rc = dev_alloc(ix, &ix->d_stats, S_COUNT, true, true))) return rc;
	HIP_TRY(hipStreamSynchronize(st));
#ifdef VG_VIEW_COUNTERS
	{
		VcRange r[24]; int nr = 0;
		auto add = [&](const void *p, uint64_t bytes, int id) { if (p && nr < 24) { r[nr].lo = (unsigned long long)p; r[nr].hi = r[nr].lo + bytes; r[nr].id = id; r[nr].pad = 0; nr++; } };
		add(d.dx, (1ull << d.dx_bits) * 16, VC_DX); add(d.mx, nm * 16, VC_MX); add(d.ref_jg, ((1ull << d.ref_jg_bits) + 1) * 4, VC_REF_JG); add(d.ref, c.n_ref * 16, VC_REF);
		add(d.snp_jg, ((1ull << 24) + 1) * 4, VC_SNP_JG); add(d.snp, c.n_snp * 16, VC_SNP); add(d.sec_jg, ((1ull << d.sec_bits) + 1) * 4, VC_SEC_JG); add(d.sec3, c.n_ref * 12 + 16, VC_SEC3);
		add(d.snp_sig, (c.n_snp + 16) * 2, VC_SIG); add(d.ref_bf, 1ull << 29, VC_REF_BF); add(d.snp_bf, (d.snp_bf_bits + 7) / 8, VC_SNP_BF);
		add(d.ref_aux, c.n_ref_aux * 40, VC_AUX_ANY); add(d.snp_aux_pos, c.n_snp_aux * 40, VC_AUX_ANY); add(d.snp_aux_info, c.n_snp_aux * 10, VC_AUX_ANY);
		add(d.pile, d.pile_len, VC_PILE_ANY); add(d.srank, (d.pile_len / 64 + 1) * 16, VC_SRANK); add(d.cnt4, (4 * ix->n_sites + 4) * 4, VC_CNT4);
		HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(vg_vc_ranges), r, sizeof r));
		HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(vg_vc_nranges), &nr, sizeof nr));
	}
#endif
	return VG_OK;
}

// Before anything is allocated: the plan (which views the budget buys) and the handle's one block of device memory, sized for the
// finished index.  maxp_est: the largest genome position, as far as it is known up front (0: unknown -- the arrays that are one
// byte or so per position then find no room in the block and are hipMalloc'ed beside it).
static int plan_and_arena(vg_index *ix, const DevCols &c, uint64_t maxp_est, uint64_t ref_bf_bits, uint64_t snp_bf_bits, ViewPlan &plan)
{
	if (c.n_ref >= 0xFFFFFFFFull || c.n_snp >= 0xFFFFFFFFull) return fail(VG_ETOOBIG, "dictionary too large (limit: 2^32 32-mers)");
	if (ref_bf_bits == 0 || snp_bf_bits == 0) return fail(VG_EINVAL, "empty bit vector");
	size_t fr = 0, tot = 0;
	if (hipMemGetInfo(&fr, &tot) != hipSuccess) { (void)hipGetLastError(); tot = 0; }
	if (tot == 0 && ix->max_device_bytes == 0) return fail(VG_ENODEV, "hipMemGetInfo failed and no device-memory budget was given (vg_index_open_ex): the views cannot be planned");
	plan = plan_views(c, maxp_est, ref_bf_bits, snp_bf_bits, ix->max_device_bytes, (uint64_t)tot, ix->cus);
	if (plan.base > plan.budget) return fail(VG_ENOMEM, "the device-memory budget is below the smallest layout of this index: %s", plan.text.c_str());
	// VG_NO_ARENA=1: every buffer its own hipMalloc / hipFree, as through round 4 (A/B runs).  A block that cannot be had (somebody
	// else holds the memory) is not an error here: the individual allocations will say so if they fail too.
	if (!getenv("VG_NO_ARENA")) {
		const double t0 = now_s();
		bool use_block = true;
		if (plan.limited) {
			// A plan with views left out: the block holds the permanent arrays only and the construction's temporaries (the columns
			// beside their entries, a sort's two buffer pairs) are taken from the device BESIDE it and given back -- that keeps the
			// finished handle within its budget, but needs the room: block + temporaries at their peak.  When the plan is limited by
			// the DEVICE itself (the default budget on a part smaller than the full layout) that room does not exist, and the open
			// used to fail in its staging allocations instead of building the smaller layout it had planned (round 5's advisor): then
			// no block at all -- every buffer its own allocation, so that what is alive at any moment is only what construction needs
			// at that moment (slower: memory that has just been freed is cleared at allocation, vg_arena.h).
			const uint64_t nm = plan.mx ? c.n_ref + c.n_snp : c.n_ref;
			const uint64_t temps = 13 * c.n_ref + 16 * c.n_snp + 24 * nm + (1ull << 30);
			if ((uint64_t)fr < plan.arena + temps) {
				use_block = false;
				if (getenv("VG_VERBOSE")) fprintf(stderr, "[vargeno_hip] %.1f GB free, block %.1f GB + temporaries %.1f GB would not fit: no block, one allocation per buffer\n", fr / 1e9, plan.arena / 1e9, temps / 1e9);
			}
		}
		if (use_block) {
			(void)ix->arena.init(plan.arena);
			if (plan.limited) ix->arena.set_temp_floor(UINT64_MAX);
		}
		g_alloc_s += now_s() - t0;
	}
	return VG_OK;
}

// while a handle is under construction on this thread its temporaries come out of its arena
struct Building {
	explicit Building(vg_index *ix) { g_building = ix; }
	~Building() { g_building = nullptr; }
};
// construction is over (every temporary has been given back): the handle's size is final
static void finish_construction(vg_index *ix)
{
	uint64_t plain = 0;
	for (const auto &kv : ix->owned_bytes) plain += kv.second;
	ix->dev_bytes = plain + ix->arena.size();
	char line[400];
	if (ix->arena.ready())
		snprintf(line, sizeof line, "; memory: one block of %.1f GB (%.1f GB of it in use now, at most %.1f GB during construction; %llu requests = %.1f GB did not fit and went to hipMalloc) + %.1f GB of hipMalloc'ed buffers",
		         ix->arena.size() / 1e9, ix->arena.in_use() / 1e9, ix->arena.peak() / 1e9, (unsigned long long)ix->arena_misses, ix->arena_miss_bytes / 1e9, plain / 1e9);
	else snprintf(line, sizeof line, "; memory: no arena (hipMalloc / hipFree per buffer), %.1f GB", plain / 1e9);
	ix->open_report += line;
	if (getenv("VG_VERBOSE")) fprintf(stderr, "[vargeno_hip] %s\n", line + 2);
}

// $VG_MAX_DEVICE_BYTES: the budget of vg_index_open / vg_index_create (vg_index_open_ex takes it as an argument)
static uint64_t env_budget()
{
	const char *e = getenv("VG_MAX_DEVICE_BYTES");
	return e && *e ? strtoull(e, nullptr, 10) : 0ull;
}

static int create_impl(const vg_index_arrays *a, int device, vg_index *ix)
{
	int rc = init_handle(ix, device);
	if (rc) return rc;
	Building guard(ix);
	PhaseClock pc(ix);
	DevCols c;
	c.n_ref = a->n_ref; c.n_ref_aux = a->n_ref_aux; c.n_snp = a->n_snp; c.n_snp_aux = a->n_snp_aux;
	// the largest position the arrays name (the loader's own rule, vg_max_pos): it sizes the arrays that are per genome position
	uint64_t maxp_est = 0;
	{
		auto scan = [&](const uint32_t *pos, const uint8_t *amb, uint64_t n) { for (uint64_t i = 0; i < n; i++) if ((!amb || amb[i] == 0) && pos[i] != POS_AMBIGUOUS && pos[i] > maxp_est) maxp_est = pos[i]; };
		scan(a->ref_pos, a->ref_amb, a->n_ref); scan(a->ref_aux, nullptr, a->n_ref_aux * AUX_COLS);
		scan(a->snp_pos, a->snp_amb, a->n_snp); scan(a->snp_aux_pos, nullptr, a->n_snp_aux * AUX_COLS);
	}
	ViewPlan plan;
	if ((rc = plan_and_arena(ix, c, maxp_est, a->ref_bf_bits, a->snp_bf_bits, plan))) return rc;
	if ((rc = c.ref_kmer.upload(a->ref_kmer, a->n_ref)) || (rc = c.ref_pos.upload(a->ref_pos, a->n_ref)) || (rc = c.ref_amb.upload(a->ref_amb, a->n_ref))) return rc;
	if ((rc = c.snp_kmer.upload(a->snp_kmer, a->n_snp)) || (rc = c.snp_pos.upload(a->snp_pos, a->n_snp)) || (rc = c.snp_info.upload(a->snp_info, a->n_snp)) ||
	    (rc = c.snp_amb.upload(a->snp_amb, a->n_snp)) || (rc = c.snp_rf.upload(a->snp_rf, a->n_snp)) || (rc = c.snp_af.upload(a->snp_af, a->n_snp))) return rc;
	if ((rc = dev_upload(ix, &c.ref_aux, a->ref_aux, a->n_ref_aux * AUX_COLS))) return rc;
	if ((rc = dev_upload(ix, &c.snp_aux_pos, a->snp_aux_pos, a->n_snp_aux * AUX_COLS))) return rc;
	if ((rc = dev_upload(ix, &c.snp_aux_info, a->snp_aux_info, a->n_snp_aux * AUX_COLS))) return rc;
	pc.lap("block allocated, columns copied to the device");
	return build_on_device(ix, c, plan, a->ref_bf_bits, a->ref_bf_words, a->snp_bf_bits, a->snp_bf_words, pc);
}

extern "C" int vg_index_create(const vg_index_arrays *a, int device, vg_index **out)
{
	if (!a || !out) return fail(VG_EINVAL, "null argument");
	*out = nullptr;
	vg_index *ix = new (std::nothrow) vg_index();
	if (!ix) return fail(VG_ENOMEM, "host allocation failed");
	ix->max_device_bytes = env_budget();
	int rc = guarded([&] { return create_impl(a, device, ix); });
	if (rc) { vg_index_close(ix); return rc; }
	finish_construction(ix);
	*out = ix;
	return VG_OK;
}

// ---- index files (formats: SURVEY.md §8f-1; writers src/dictgen.c:63-275, sdsl int_vector.hpp:1563-1595)
// A byte range of a file -> device memory: reader threads pread() pieces into a ring of pinned buffers, each piece is copied up
// as soon as it is complete (the page cache / an NVMe array serve the threads concurrently; one fread of the 43 GB hg38
// dictionary is a single memcpy stream, and a copy from pageable memory is staged a second time by the runtime).
// the page-locked staging of the file reads: made once per vg_index_open (eight 64 MiB buffers take 0.12 s to pin and 0.08 s to
// release, tools/alloc_probe), shared by both dictionary files
struct FileRing {
	static constexpr uint64_t PIECE = 64ull << 20;
	static constexpr int NBUF = 8;
	uint8_t *buf[NBUF] = {};
	hipEvent_t copied[NBUF] = {};
	hipStream_t cs = nullptr;
	int init()
	{
		for (int i = 0; i < NBUF; i++) {
			if (hipHostMalloc((void **)&buf[i], PIECE, hipHostMallocDefault) != hipSuccess) return fail(VG_ENOMEM, "hipHostMalloc(staging) failed");
			if (hipEventCreateWithFlags(&copied[i], hipEventDisableTiming) != hipSuccess) return fail(VG_ENODEV, "hipEventCreate failed");
		}
		if (hipStreamCreateWithFlags(&cs, hipStreamNonBlocking) != hipSuccess) return fail(VG_ENODEV, "hipStreamCreate failed");
		return VG_OK;
	}
	~FileRing()
	{
		for (auto p : buf) if (p) (void)hipHostFree(p);
		for (auto e : copied) if (e) (void)hipEventDestroy(e);
		if (cs) (void)hipStreamDestroy(cs);
	}
};
static int file_to_device(FileRing &R, int fd, uint64_t off, uint64_t bytes, uint8_t *dst, const std::string &path)
{
	if (bytes == 0) return VG_OK;
	constexpr uint64_t PIECE = FileRing::PIECE;
	constexpr int NBUF = FileRing::NBUF;
	const uint64_t n_pieces = (bytes + PIECE - 1) / PIECE;
	int rc = VG_OK;
	std::mutex mu; std::condition_variable cv;
	std::vector<uint8_t> state(n_pieces, 0);                    // 1 = read into its ring slot
	uint64_t issued = 0;                                        // pieces whose copy has been enqueued AND whose slot is free again once copied[slot] fires
	uint64_t freed = 0;                                         // pieces known to have left their ring slot
	std::atomic<uint64_t> next{0};
	bool io_error = false;
	const unsigned nt = std::min<unsigned>(host_threads(), 16u);
	std::vector<std::thread> readers;
	for (unsigned t = 0; t < nt; t++) readers.emplace_back([&] {
		for (;;) {
			const uint64_t p = next.fetch_add(1);
			if (p >= n_pieces) return;
			{ std::unique_lock<std::mutex> g(mu); cv.wait(g, [&] { return p < freed + (uint64_t)NBUF || io_error; }); if (io_error) return; }
			const uint64_t o = p * PIECE, n = std::min(PIECE, bytes - o);
			uint64_t done = 0;
			while (done < n) {
				const ssize_t g = pread(fd, R.buf[p % NBUF] + done, (size_t)(n - done), (off_t)(off + o + done));
				if (g <= 0) break;
				done += (uint64_t)g;
			}
			std::lock_guard<std::mutex> g(mu);
			if (done < n) io_error = true;
			state[p] = 1;
			cv.notify_all();
		}
	});
	for (uint64_t p = 0; p < n_pieces; p++) {
		{ std::unique_lock<std::mutex> g(mu); cv.wait(g, [&] { return state[p] != 0 || io_error; }); if (io_error) break; }
		const uint64_t o = p * PIECE, n = std::min(PIECE, bytes - o);
		if (hipMemcpyAsync(dst + o, R.buf[p % NBUF], n, hipMemcpyHostToDevice, R.cs) != hipSuccess || hipEventRecord(R.copied[p % NBUF], R.cs) != hipSuccess) {
			std::lock_guard<std::mutex> g(mu); io_error = true; rc = fail(VG_ENODEV, "host-to-device copy failed"); cv.notify_all(); break;
		}
		issued = p + 1;
		// the slot of piece p - NBUF + 1 .. is reusable once its copy has finished: wait for the oldest outstanding one when the ring is full
		if (issued - freed >= (uint64_t)NBUF - 1) {
			(void)hipEventSynchronize(R.copied[freed % NBUF]);
			std::lock_guard<std::mutex> g(mu); freed++; cv.notify_all();
		}
	}
	(void)hipStreamSynchronize(R.cs);
	{ std::lock_guard<std::mutex> g(mu); freed = n_pieces + NBUF; cv.notify_all(); }
	for (auto &t : readers) t.join();
	if (rc) return rc;
	if (io_error) return fail(VG_EIO, "short read on %s", path.c_str());
	return VG_OK;
}

static int read_bf(const std::string &path, uint64_t cap_bits, uint64_t &bits, std::vector<uint64_t> &words)
{
	FILE *f = fopen(path.c_str(), "rb");
	if (!f) return fail(VG_EIO, "cannot open %s", path.c_str());
	if (fread(&bits, 8, 1, f) != 1) { fclose(f); return fail(VG_EIO, "short read on %s", path.c_str()); }
	// sdsl int_vector<1> (int_vector.hpp:1563-1595): u64 bit count, then ceil(bits / 64) words.  A header that does not match the
	// file's size is a corrupt file: the kernels index the words with (hash % bits) >> 6
	{
		struct stat sb;
		const uint64_t words_all = bits / 64 + (bits % 64 != 0);
		if (fstat(fileno(f), &sb) != 0 || bits == 0 || words_all > ((uint64_t)sb.st_size - 8) / 8 || (uint64_t)sb.st_size != 8 + 8 * words_all) {
			fclose(f);
			return fail(VG_EIO, "%s: size does not match its header", path.c_str());
		}
	}
	const uint64_t capped = std::min(bits, cap_bits);
	const uint64_t nw = capped / 64 + (capped % 64 != 0);
	words.resize(nw);
	const size_t got = nw ? fread(words.data(), 8, nw, f) : 0;
	fclose(f);
	if (got != nw) return fail(VG_EIO, "short read on %s", path.c_str());
	return VG_OK;
}

struct Fd { int fd = -1; ~Fd() { if (fd >= 0) close(fd); } };

static int open_impl(const char *prefix, int device, vg_index *ix)
{
	const std::string pre(prefix);
	int rc;
	Fd rf, sf;
	rf.fd = open((pre + ".ref.dict").c_str(), O_RDONLY);
	if (rf.fd < 0) return fail(VG_EIO, "cannot open %s.ref.dict", prefix);
	sf.fd = open((pre + ".snp.dict").c_str(), O_RDONLY);
	if (sf.fd < 0) return fail(VG_EIO, "cannot open %s.snp.dict", prefix);
	struct stat rs, ss;
	if (fstat(rf.fd, &rs) != 0 || fstat(sf.fd, &ss) != 0) return fail(VG_EIO, "cannot stat the dictionary files of %s", prefix);
	const uint64_t rsize = (uint64_t)rs.st_size, ssize = (uint64_t)ss.st_size;
	if (rsize < 16 || ssize < 16) return fail(VG_EIO, "dictionary file too short: %s", prefix);
	uint64_t rh[2], sh[2];
	if (pread(rf.fd, rh, 16, 0) != 16 || pread(sf.fd, sh, 16, 0) != 16) return fail(VG_EIO, "short read on the dictionary files of %s", prefix);
	const uint64_t n_ref = rh[0], n_ref_aux = rh[1], n_snp = sh[0], n_snp_aux = sh[1];
	if (n_ref > (1ull << 32) || n_snp > (1ull << 32)) return fail(VG_ETOOBIG, "dictionary too large (limit: 2^32 32-mers)");
	// every count is bounded by the file it came from before it is multiplied (a corrupt header must not wrap the size check)
	if (n_ref > rsize / 13 || n_ref_aux > rsize / 40 || rsize != 16 + 13 * n_ref + 40 * n_ref_aux) return fail(VG_EIO, "%s.ref.dict: size does not match its header", prefix);
	if (n_snp > ssize / 16 || n_snp_aux > ssize / 78 || ssize != 16 + 16 * n_snp + 78 * n_snp_aux) return fail(VG_EIO, "%s.snp.dict: size does not match its header", prefix);
	uint64_t rbits = 0, sbits = 0;
	std::vector<uint64_t> rw, sw;
	const double t_bf0 = now_s();
	if ((rc = read_bf(pre + ".ref.bf", 1ull << 32, rbits, rw))) return rc;
	if ((rc = read_bf(pre + ".snp.bf", ~0ull, sbits, sw))) return rc;
	const double t_bf1 = now_s();
	if ((rc = init_handle(ix, device))) return rc;
	Building guard(ix);
	PhaseClock pc(ix);
	{
		char line[160];
		snprintf(line, sizeof line, "bit-vector files read %.2f s; device, streams, events %.2f s", t_bf1 - t_bf0, now_s() - t_bf1);
		ix->open_report = line;
		if (pc.on) fprintf(stderr, "[vargeno_hip] %s\n", line);
	}
	DevCols c;
	c.n_ref = n_ref; c.n_ref_aux = n_ref_aux; c.n_snp = n_snp; c.n_snp_aux = n_snp_aux;
	// the genome's length, from <prefix>.chrlens when `vargeno index` left one ("name length" per line): positions are 1-based over
	// the concatenated sequences, so their sum bounds every position the dictionaries name
	uint64_t maxp_est = 0;
	if (FILE *f = fopen((pre + ".chrlens").c_str(), "r")) {
		char name[256]; unsigned long long len = 0;
		while (fscanf(f, "%255s %llu", name, &len) == 2) maxp_est += len;
		fclose(f);
		if (maxp_est > (1ull << 32)) maxp_est = 0;
	}
	ViewPlan plan;
	if ((rc = plan_and_arena(ix, c, maxp_est, rbits, sbits, plan))) return rc;
	if ((rc = c.alloc())) return rc;
	if ((rc = dev_alloc(ix, &c.ref_aux, n_ref_aux * AUX_COLS))) return rc;
	if ((rc = dev_alloc(ix, &c.snp_aux_pos, n_snp_aux * AUX_COLS))) return rc;
	if ((rc = dev_alloc(ix, &c.snp_aux_info, n_snp_aux * AUX_COLS))) return rc;
	{
	FileRing ring;
	if ((rc = ring.init())) return rc;
	{
		// the files' bytes, as they are, next to the columns they unpack into (the larger one first; freed right after)
		TempDev<uint8_t> raw;
		if ((rc = raw.alloc(rsize - 16 + 64))) return rc;
		if ((rc = file_to_device(ring, rf.fd, 16, rsize - 16, raw.p, pre + ".ref.dict"))) return rc;
		vg_unpack_ref<<<4096, 256, 0, ix->stream>>>(raw.p, n_ref, c.ref_kmer.p, c.ref_pos.p, c.ref_amb.p);
		if (n_ref_aux) vg_unpack_ref_aux<<<1024, 256, 0, ix->stream>>>(raw.p + 13 * n_ref, n_ref_aux * AUX_COLS, c.ref_aux);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipStreamSynchronize(ix->stream));
	}
	{
		TempDev<uint8_t> raw;
		if ((rc = raw.alloc(ssize - 16 + 64))) return rc;
		if ((rc = file_to_device(ring, sf.fd, 16, ssize - 16, raw.p, pre + ".snp.dict"))) return rc;
		vg_unpack_snp<<<4096, 256, 0, ix->stream>>>(raw.p, n_snp, c.snp_kmer.p, c.snp_pos.p, c.snp_info.p, c.snp_amb.p, c.snp_rf.p, c.snp_af.p);
		if (n_snp_aux) vg_unpack_snp_aux<<<1024, 256, 0, ix->stream>>>(raw.p + 16 * n_snp, n_snp_aux, c.snp_aux_pos, c.snp_aux_info);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipStreamSynchronize(ix->stream));
	}
	}
	pc.lap("block allocated, dictionary files read, copied up, unpacked");
	return build_on_device(ix, c, plan, rbits, rw.data(), sbits, sw.data(), pc);
}

extern "C" int vg_index_open_ex(const char *prefix, int device, uint64_t max_device_bytes, vg_index **out)
{
	if (!prefix || !out) return fail(VG_EINVAL, "null argument");
	*out = nullptr;
	vg_index *ix = new (std::nothrow) vg_index();
	if (!ix) return fail(VG_ENOMEM, "host allocation failed");
	ix->max_device_bytes = max_device_bytes;
	const double t0 = now_s();
	int rc = guarded([&] { return open_impl(prefix, device, ix); });
	if (rc) { vg_index_close(ix); return rc; }
	finish_construction(ix);
	char line[80];
	snprintf(line, sizeof line, "; vg_index_open %.2f s in all", now_s() - t0);
	ix->open_report += line;
	*out = ix;
	return VG_OK;
}

extern "C" const char *vg_index_plan(const vg_index *ix) { return ix ? ix->plan_text.c_str() : ""; }
extern "C" const char *vg_index_open_report(const vg_index *ix) { return ix ? ix->open_report.c_str() : ""; }

extern "C" int vg_index_open(const char *prefix, int device, vg_index **out)
{
	return vg_index_open_ex(prefix, device, env_budget(), out);
}
extern "C" uint64_t vg_index_device_bytes(const vg_index *ix) { return ix ? ix->dev_bytes : 0; }
extern "C" uint64_t vg_num_sites(const vg_index *ix) { return ix ? ix->n_sites : 0; }
extern "C" uint64_t vg_held_passes(const vg_index *ix) { return ix ? ix->held_passes : 0; }
extern "C" uint32_t vg_index_views(const vg_index *ix)
{
	if (!ix) return 0;
	const DevIndex &d = ix->d;
	return (d.sec3 ? VG_VIEW_SEC : 0u) | (d.sec_is_bf ? VG_VIEW_SEC_IS_BF : 0u) | (d.mx ? VG_VIEW_MX : 0u) | (d.dx ? VG_VIEW_DX : 0u) | (d.snp_probe ? VG_VIEW_SNP_PROBE : 0u) | (d.snp_jg32 ? VG_VIEW_SNP_JG32 : 0u) | (d.hx ? VG_VIEW_HX : 0u) | (d.snp_sig ? VG_VIEW_SNP_SIG : 0u) | (d.ssec3 ? VG_VIEW_SSEC : 0u);
}

// ------------------------------------------------------------------------------------------------
// read batches
// ------------------------------------------------------------------------------------------------
// vg_lane_kernel, the counting build (stats) or the plain one
template <class... A>
static void launch_lane(bool stats, unsigned grid, unsigned block, hipStream_t st, const A &...a)
{
	if (stats) vg_lane_kernel<true><<<grid, block, 0, st>>>(a...);
	else vg_lane_kernel<false><<<grid, block, 0, st>>>(a...);
}

// the index as the kernels of a batch of sample `plane` see it: the shared tables, that plane's counters
static DevIndex plane_view(const vg_index *ix, uint32_t plane)
{
	DevIndex v = ix->d;
	v.cnt = ix->planes[plane].p.cnt; v.cnt4 = ix->planes[plane].p.cnt4;
	return v;
}

static int harvest(vg_index *ix, Slot &sl)
{
	if (!sl.busy) return VG_OK;
	HIP_TRY(hipEventSynchronize(sl.batch_done));
	// reads left for the per-batch lane tier: what the late store did not take (ctr[6]), or -- VG_FORCE_GENERIC, VG_NO_LATE_STORE -- all of listB
	const uint32_t resid = sl.lt_late ? sl.h_ctr.p[6] : sl.h_ctr.p[1];
	uint32_t *const r_list = sl.lt_late ? sl.listA.p : sl.listB.p, *const r_cnt = sl.lt_late ? &sl.ctr[6] : &sl.ctr[1];
	if (resid) ix->lane_tier_seen = true;
	if (resid && !sl.lt_enqueued) {
		// the lane machine with its lists in HBM finishes them now, into the batch's plane
		launch_lane(sl.lt_stats, ix->big.s.nlanes / 64, 64, ix->tail2, plane_view(ix, sl.plane), ix->big.s, sl.lt_bases, sl.lt_quals, sl.lt_offsets, 0, r_list, r_cnt, sl.listC.p, &sl.ctr[2], ix->d_stats, nullptr, sl.lt_gate, sl.pk_kmer.p, sl.pk_meta.p, sl.lt_packed, nullptr, nullptr);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(sl.h_ctr.p, sl.ctr, 32, hipMemcpyDeviceToHost, ix->tail2));
		HIP_TRY(hipStreamSynchronize(ix->tail2));
	}
	for (int i = 0; i < 4; i++) ix->cum[i] += sl.h_ctr.p[i];
	ix->held_passes += sl.h_ctr.p[CTR_HELD];
	ix->planes[sl.plane].invalid += sl.h_ctr.p[3];
	// the deep tier's grid follows the lists it has been getting (enqueue_batch): the larger of this batch's and half the hint before
	ix->spill_hint = std::max<uint32_t>(sl.h_ctr.p[0], ix->spill_hint / 2);
	ix->spill_known = true;
	float pack = 0, wave = 0, tail = 0, total = 0, w2 = 0;
	HIP_TRY(hipEventElapsedTime(&pack, sl.pack_begin, sl.pack_end)); HIP_TRY(hipEventElapsedTime(&wave, sl.wave_begin, sl.wave_end));
	HIP_TRY(hipEventElapsedTime(&tail, sl.wave_end, sl.batch_done)); HIP_TRY(hipEventElapsedTime(&total, sl.pack_begin, sl.batch_done)); HIP_TRY(hipEventElapsedTime(&w2, sl.wave_end, sl.deep_end));
	ix->t_pack += pack; ix->t_main += wave; ix->t_tail += tail; ix->t_total += total; ix->t_w2 += w2; ix->t_batches++;
	sl.busy = false;
	return VG_OK;
}

// The late store's one lane-machine run (see vg_late_collect): every stream of the handle is idle when this is called.
static int run_late_store(vg_index *ix)
{
	if (!ix->late_dirty || !ix->late.state) return VG_OK;
	unsigned long long st[2] = {0, 0};
	HIP_TRY(hipMemcpy(st, ix->late.state, 16, hipMemcpyDeviceToHost));
	ix->late_dirty = false;
	const uint64_t n = st[1];
	if (st[0] == 0) return VG_OK;
	if (n) {
		launch_lane(ix->late_stats, ix->big.s.nlanes / 64, 64, ix->tail, ix->d, ix->big.s, nullptr, nullptr, ix->late.offsets, n, nullptr, nullptr, ix->late.lost, ix->late.lost_n, ix->d_stats, nullptr, nullptr, ix->late.kmers, ix->late.meta, true, ix->d_planes, ix->late.tag);
		HIP_TRY(hipGetLastError());
	}
	uint32_t lost = 0;
	HIP_TRY(hipMemcpyAsync(&lost, ix->late.lost_n, 4, hipMemcpyDeviceToHost, ix->tail));
	HIP_TRY(hipMemsetAsync(ix->late.state, 0, 16, ix->tail));
	HIP_TRY(hipMemsetAsync(ix->late.lost_n, 0, 4, ix->tail));
	HIP_TRY(hipStreamSynchronize(ix->tail));
	ix->cum[2] += lost;
	ix->late_reads_run += n;
	return VG_OK;
}

// Drain both streams and turn "a read outgrew even the deep scratch" into an error code.
static int finish_pending(vg_index *ix)
{
	HIP_TRY(hipSetDevice(ix->device));
	HIP_TRY(hipStreamSynchronize(ix->stream));
	HIP_TRY(hipStreamSynchronize(ix->tail));
	HIP_TRY(hipStreamSynchronize(ix->tail2));
	// (the FASTQ stream's own work -- vg_fastq_stream_begin's reset of the stream state included -- is otherwise only ordered
	// before the batches it produced: an empty stream has none)
	if (ix->ingest) HIP_TRY(hipStreamSynchronize(ix->ingest));
	for (Slot &sl : ix->slot) { int rc = harvest(ix, sl); if (rc) return rc; }
	{ int rc = run_late_store(ix); if (rc) return rc; }
	// every plane that took increments, in ONE launch
	std::vector<uint32_t> dirty;
	for (uint32_t s = 0; s < (uint32_t)ix->planes.size(); s++) if (ix->planes[s].dirty) { dirty.push_back(s); ix->planes[s].dirty = false; }
	if (!dirty.empty() && ix->n_sites) {
		if (dirty != ix->dirty_up) {
			HIP_TRY(hipMemcpy(ix->d_dirty, dirty.data(), dirty.size() * 4, hipMemcpyHostToDevice));
			ix->dirty_up = dirty;
		}
		vg_fold_counters<<<dim3((unsigned)std::min<uint64_t>((ix->n_sites + 255) / 256, 4096), (unsigned)dirty.size()), 256, 0, ix->stream>>>(ix->d_planes, ix->d_dirty, ix->d.site_ba, ix->n_sites);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipStreamSynchronize(ix->stream));
	}
	if (ix->cum[2]) return fail(VG_ENOMEM, "a read produced more hit contexts than the deep scratch holds (the reference overruns MAX_HITS=2000 long before, qv.cc:709)");
	return VG_OK;
}

// The pack kernel goes in front of the wave tier on the main stream, or onto the ingest stream, where batch k+1's runs while
// batch k's wave kernel does.  What was measured (profiles/ab_hg38_r07_pack_corun.txt has the runs, DESIGN.md §4 the table):
//  * batches of a million reads: the launch gaps between the dependent kernels of one stream weigh most; chr22-scale, 1 M reads per
//    step, 0.384 -> 0.352 ms with the pack kernel, full grid, on the ingest stream (profiles/ab_chr22_pack_overlap_r05.txt);
//  * 8 M-read batches, full grid (16 workgroups per CU): no gain with today's kernels (2.742 against 2.750 / 2.764 ms per step), a
//    loss with round 3's (2.779 -> 2.865).  A pack workgroup fits beside three main-tier workgroups of a CU, not beside four: where
//    one is placed, a main-tier workgroup is not, and a full grid takes every CU in turn with the wave kernel;
//  * 8 M-read batches, ONE pack workgroup per CU: it stays beside three main-tier workgroups per CU for about the wave kernel's
//    whole duration (pack 0.53 -> 2.3 ms, wave kernel 2.12 -> 2.51 ms as its events see it: 5 % of that is the fourth workgroup
//    it lacks on a CU, the rest is shared memory bandwidth) and the step gets shorter, 2.69-2.71 -> 2.60 ms; two per CU: 2.63.
// So a large batch takes the ingest stream with the small grid -- when the wave kernel of the batch before is still running or
// waiting on the main stream.  When it is not (a handle's first batch, a caller that synchronises after every batch) there is
// nothing to run beside, and a pack kernel of one workgroup per CU would take 2.3 ms instead of 0.53: main stream, full grid.
// Not measured, hence left as they were: the instantiations for an index without the merged view and for a direct table of
// fewer than 2^32 buckets with large batches, and the counting build.
struct PackPlan { hipStream_t stream; bool corun; };
// packed: no pack kernel, the copies of the packed form take its place.  headline: the wave kernel is the headline instantiation.
static PackPlan plan_pack(const vg_index *ix, uint64_t n_reads, bool packed, bool headline)
{
	if (!ix->ingest) return {ix->stream, false};
	const bool small = n_reads <= ix->pack_small_reads;
	if (ix->pack_overlap == 1 || (ix->pack_overlap < 0 && small)) return {ix->ingest, !small};
	if (ix->pack_overlap < 0 && !packed && headline && ix->last_wave_end && hipEventQuery(ix->last_wave_end) == hipErrorNotReady) return {ix->ingest, true};
	return {ix->stream, false};
}

// A batch's first step, on the stream its first kernel goes to: wait for the stream that produced its buffers (a batch gathered by the
// FASTQ framing, or copied up, on the ingest stream), zero its counters, mark its start.
static int begin_batch(Slot &sl, hipStream_t on, hipStream_t produced_on)
{
	if (produced_on && produced_on != on) {
		HIP_TRY(hipEventRecord(sl.e_in, produced_on));
		HIP_TRY(hipStreamWaitEvent(on, sl.e_in, 0));
	}
	HIP_TRY(hipMemsetAsync(sl.ctr, 0, 64, on));
	HIP_TRY(hipEventRecord(sl.pack_begin, on));
	return VG_OK;
}

// One tier of the wave machine (<W1_*>: the main tier, <W3_*, 1>: the deep tier): the kernel built for an index without the merged
// view (big), the instantiation that compares (F, lo32) (sdx), or the general one, as the counting build (stats) or the plain one.
// hold (it matters to the main tier's two timed instantiations only): gate-open pairs may wait (vg_wave.h, "held pairs"); without it
// those two run as vg_wave_kernel_plain.
template <int ECAP, int NCAP, int WPB, class... A>
static void launch_wave(bool big, bool sdx, bool stats, bool hold, unsigned grid, hipStream_t st, const A &...a)
{
	if constexpr (WPB > 1) if (!hold && !big && !stats) {
		if (sdx) vg_wave_kernel_plain<ECAP, NCAP, WPB, true><<<grid, 64 * WPB, 0, st>>>(a...);
		else vg_wave_kernel_plain<ECAP, NCAP, WPB, false><<<grid, 64 * WPB, 0, st>>>(a...);
		return;
	}
	if (big) vg_wave_kernel_big<ECAP, NCAP, WPB><<<grid, 64 * WPB, 0, st>>>(a...);
	else if (sdx) vg_wave_kernel<false, ECAP, NCAP, WPB, true><<<grid, 64 * WPB, 0, st>>>(a...);
	else if (stats) vg_wave_kernel<true, ECAP, NCAP, WPB><<<grid, 64 * WPB, 0, st>>>(a...);
	else vg_wave_kernel<false, ECAP, NCAP, WPB><<<grid, 64 * WPB, 0, st>>>(a...);
}

// One batch = pack -> wave tier on the main stream, then lane tier (mid scratch) -> lane tier (deep scratch)
// on the tail stream; the list launches size themselves from device counters, so nothing waits for the host.
// n_reads: the batch's size, or (d_n_reads given) an upper bound of the size the device holds at d_n_reads
// packed: the batch is already packed (sl.pk_kmer / sl.pk_meta hold it, d_offsets = 32 x chunks before each read): no pack kernel
static int enqueue_batch(vg_index *ix, Slot &sl, const bool stats, const uint8_t *d_bases, const uint8_t *d_quals, const uint32_t *d_gate, const uint64_t *d_offsets, uint64_t n_reads, hipStream_t produced_on, const uint32_t *d_n_reads, const bool packed, const uint64_t total_bases)
{
	uint32_t *ctr = sl.ctr;
	int rc;
	const DevIndex dv = plane_view(ix, sl.plane);                    // the batch's sample: its counters, the shared tables
	if (!ix->force_generic) {
		const bool big = !stats && ix->d.mx == nullptr;                // an index without the merged view: the kernel built for it
		const bool sdx = !stats && !big && ix->d.dx != nullptr && ix->d.dx_bits < 32u;      // a direct table of fewer than 2^32 buckets: the instantiation that compares (F, lo32)
		const PackPlan pp = plan_pack(ix, n_reads, packed, !stats && !big && !sdx);
		hipStream_t ps = pp.stream;
		if ((rc = begin_batch(sl, ps, produced_on))) return rc;
		// reads per tile of the pack kernel: as many as the mean read length lets fit its LDS stream (64 up to 160 bases)
		const uint64_t mean_len = n_reads ? (total_bases + n_reads - 1) / n_reads : 1;
		const uint32_t pack_tr = (uint32_t)std::max<uint64_t>(4, std::min<uint64_t>(PACK_T, (uint64_t)PACK_T * PACK_MAXLEN / std::max<uint64_t>(mean_len, 1)));
		const unsigned pgrid = (unsigned)std::min<uint64_t>((n_reads + (uint64_t)pack_tr * PACK_WPB - 1) / ((uint64_t)pack_tr * PACK_WPB), pp.corun ? (uint64_t)(ix->pack_corun_wgs ? ix->pack_corun_wgs : ix->cus) : (uint64_t)ix->cus * ix->pack_bpc);
		const bool fused = ix->fuse_pack && !packed;                 // the main tier encodes the reads itself (experiment)
		const FuseIn fin{fused ? d_bases : nullptr, d_quals, d_gate, &ctr[3]}, nofuse{nullptr, nullptr, nullptr, nullptr};
		if (!packed && !fused) vg_pack_kernel<<<pgrid, PACK_T * PACK_WPB, 0, ps>>>(d_bases, d_quals, d_offsets, n_reads, sl.pk_kmer.p, sl.pk_meta.p, &ctr[3], d_n_reads, d_gate, pack_tr);
		HIP_TRY(hipEventRecord(sl.pack_end, ps));
		if (ps != ix->stream) HIP_TRY(hipStreamWaitEvent(ix->stream, sl.pack_end, 0));
		// The previous batch's deep-list tier (tail stream) runs under this batch's pack kernel and, for what is left of it,
		// under the head of this batch's wave kernel: its few single-wave workgroups drain while the main tier pulls its work
		// dynamically, which costs less than holding the wave kernel back for them (0.71 -> 0.66 ms per 1 M-read step).
		HIP_TRY(hipEventRecord(sl.wave_begin, ix->stream));       // the wave kernel's own start
		ix->planes[sl.plane].dirty = true;
		unsigned wgrid = (unsigned)std::min<uint64_t>((n_reads + 64 * W1_WPB - 1) / (64 * W1_WPB), (uint64_t)ix->wave_grid / W1_WPB);
		if (ix->wave_wgs) wgrid = std::min<unsigned>(wgrid, ix->wave_wgs);
		// Held pairs pay where the prune has left a wave few pairs per iteration: reads of at most four chunks.  Longer reads are not
		// pruned and meet the threshold in nearly every iteration, so a batch whose reads average five chunks or more runs the plain
		// kernel, as does every batch under a threshold of 0.  A batch whose length is not known here (total_bases 0: packed on the host,
		// or framed on the device) has a mean of 0 and is held.  The mean decides for the whole batch: a mixed batch below 160 is held
		// with its long reads in it, which is exact like every schedule and has not been measured.
		const bool hold = ix->hold_pairs > 0 && mean_len < 5 * 32;
		launch_wave<W1_ECAP, W1_NCAP, W1_WPB>(big, sdx, stats, hold, wgrid, ix->stream, dv, sl.pk_kmer.p, sl.pk_meta.p, d_offsets, n_reads, nullptr, d_n_reads, sl.listA.p, &ctr[0], &ctr[CTR_WORK_MAIN], ix->work_chunk, ix->hold_pairs, ix->d_stats, fin);
		HIP_TRY(hipEventRecord(sl.wave_end, ix->stream));
		ix->last_wave_end = sl.wave_end;
		// tail stream, the deep tier: the same kernel with deeper tables over the spill list (single-wave workgroups of 42 KB of LDS).
		// ONE deep tier (r04; r03 had a 40 + 16 tier in front of it): it starts the moment the main tier's workgroups retire, while
		// the CUs are free.  A tier enqueued behind another one found the NEXT batch's main-tier kernel on every CU and was only placed
		// when that kernel's workgroups retired, 2.2 ms later -- the tail stream was busy for a whole step, the handle's batch slots
		// waited for it and the main stream idled 0.2 ms per step (profiles/timeline_hg38_r04_three_tiers.txt).  With vote keys instead
		// of context lists the deep tier has 0.005-0.3 % of the reads to do, not 10 %.
		HIP_TRY(hipStreamWaitEvent(ix->tail, sl.wave_end, 0));
		// The deep tier's grid: single-wave workgroups of 42 KB of LDS that can only be PLACED where a main-tier workgroup has retired --
		// by then the next batch's kernels want the same CUs.  A full grid (3 per CU) for a list of 20 reads took 0.30 ms beside a
		// 0.32 ms main kernel at chr22 scale (profiles/rocprof_summary_r05_chr22.txt).  The list's size is only known on the device, but
		// lists of consecutive batches of one workload are alike: the grid follows the last harvested batches' lists (two reads per
		// wave's pull, and a floor), the full grid until a batch has been harvested.  A list longer than expected is still finished --
		// the waves pull their work from a counter and their pulls grow with the list -- just by fewer waves.
		unsigned w2grid = (unsigned)std::min<uint64_t>((n_reads + 63) / 64, (uint64_t)ix->cus * ix->w2_wpc);
		if (ix->spill_known && !ix->w2_full_grid) w2grid = std::min<unsigned>(w2grid, std::max<unsigned>(32u, (2u * ix->spill_hint + ix->w2_chunk - 1) / ix->w2_chunk + 16u));
		launch_wave<W3_ECAP, W3_NCAP, 1>(big, sdx, stats, false, w2grid, ix->tail, dv, sl.pk_kmer.p, sl.pk_meta.p, d_offsets, 0, sl.listA.p, &ctr[0], sl.listB.p, &ctr[1], &ctr[5], ix->w2_chunk, 0u, ix->d_stats, nofuse);
		// what the deep tier leaves behind goes to the handle's late store (the lane machine runs over it once, at the next
		// synchronisation); the slot only keeps what the store cannot take (listA is free again: the deep tier has consumed it)
		sl.lt_late = ix->late.state != nullptr;
		if (sl.lt_late) {
			vg_late_collect<<<4, 256, 0, ix->tail>>>(ix->late, sl.pk_kmer.p, sl.pk_meta.p, d_offsets, sl.listB.p, &ctr[1], sl.listA.p, &ctr[6], sl.plane);
			ix->late_dirty = true; ix->late_stats = stats;
		}
	} else {
		sl.lt_late = false;
		const unsigned g1 = (unsigned)std::min<uint64_t>((n_reads + 255) / 256, (uint64_t)ix->lane_grid_blocks);
		if ((rc = begin_batch(sl, ix->stream, produced_on))) return rc;
		HIP_TRY(hipEventRecord(sl.pack_end, ix->stream));
		HIP_TRY(hipEventRecord(sl.wave_begin, ix->stream));
		launch_lane(stats, g1, 256, ix->stream, dv, ix->mid.s, d_bases, d_quals, d_offsets, n_reads, nullptr, d_n_reads, sl.listB.p, &ctr[1], ix->d_stats, packed ? nullptr : &ctr[3], d_gate, sl.pk_kmer.p, sl.pk_meta.p, packed, nullptr, nullptr);
		HIP_TRY(hipEventRecord(sl.wave_end, ix->stream));
		HIP_TRY(hipStreamWaitEvent(ix->tail, sl.wave_end, 0));
	}
	HIP_TRY(hipEventRecord(sl.deep_end, ix->tail));
	// ... and the generic lane machine with the deep HBM scratch for whatever is left -- LATER, and only if anything is (r05): the
	// batch's counters come to the host behind its tiers, and harvest() launches the lane tier when they say that the deep tier left
	// reads behind (0-5 reads per 8 M at hg38 scale, mostly none).  Through r04 the kernel was enqueued unconditionally: 64 workgroups
	// that exit at once, but can only be PLACED when workgroups of the next batch's main tier retire -- 1.7-3.7 ms during which the
	// batch's slot stayed busy, and 2-4 ms at the end of every job.
	// (a workload whose batches DO leave reads for the lane tier -- long reads, tiny list capacities in the tests -- gets the kernel
	// enqueued behind the deep tier as before, from the first batch that showed it on: a launch at harvest time would stall the host
	// and the tail stream once per batch)
	sl.lt_bases = d_bases; sl.lt_quals = d_quals; sl.lt_offsets = d_offsets; sl.lt_gate = d_gate; sl.lt_packed = packed; sl.lt_stats = stats;
	sl.lt_enqueued = ix->lane_tier_seen;
	// (the lane tiers, once a workload needs them, and the counter copies behind them go to `tail2`; a workload that never does keeps
	// to the one tail stream -- chr22-scale steps are 3 % slower with the fourth stream in use: profiles/ab_tail_streams_r05.txt)
	hipStream_t lt = ix->tail;
	if (sl.lt_enqueued) {
		lt = ix->tail2;
		HIP_TRY(hipStreamWaitEvent(lt, sl.deep_end, 0));
		launch_lane(stats, ix->big.s.nlanes / 64, 64, lt, dv, ix->big.s, d_bases, d_quals, d_offsets, 0, sl.lt_late ? sl.listA.p : sl.listB.p, sl.lt_late ? &ctr[6] : &ctr[1], sl.listC.p, &ctr[2], ix->d_stats, nullptr, d_gate, sl.pk_kmer.p, sl.pk_meta.p, packed, nullptr, nullptr);
	}
	HIP_TRY(hipMemcpyAsync(sl.h_ctr.p, ctr, 32, hipMemcpyDeviceToHost, lt));
	HIP_TRY(hipEventRecord(sl.batch_done, lt));
	HIP_TRY(hipGetLastError());
	sl.busy = true;
	return VG_OK;
}

// sample: the plane the slot's next batch counts into -- the selected sample, or the open FASTQ stream's
static int acquire_slot(vg_index *ix, Slot **out, uint32_t sample)
{
	Slot &sl = ix->slot[ix->next_slot];
	ix->next_slot = (ix->next_slot + 1) % NSLOT;
	int rc = harvest(ix, sl);                             // blocks only when NSLOT batches are already in flight
	if (rc) return rc;
	sl.plane = sample;
	*out = &sl;
	return VG_OK;
}

// The slot's packed-read buffers and spill lists for a batch of n_reads reads in n_chunks 32-base chunks.  The slot is idle
// (acquire_slot harvested it), so its buffers may be replaced.
static int size_slot(Slot &sl, uint64_t n_reads, uint64_t n_chunks)
{
	int rc;
	if ((rc = sl.pk_kmer.reserve(n_chunks + 2, "packed reads"))) return rc;
	if ((rc = sl.pk_meta.reserve(n_reads + 1, "packed reads' flag words"))) return rc;
	return reserve_together({&sl.listA, &sl.listB, &sl.listC}, n_reads, "spill lists");
}

// produced_on: the stream whose earlier work fills the batch buffers (nullptr: they are complete already).
// d_n_reads: the batch was framed on the device and only the device knows its size; n_reads and total_bases are then upper bounds.
static int launch_batch(vg_index *ix, Slot &sl, const uint8_t *d_bases, const uint8_t *d_quals, const uint64_t *d_offsets, uint64_t n_reads, hipStream_t produced_on = nullptr,
                        const uint32_t *d_n_reads = nullptr, uint64_t total_bases = 0, const uint32_t *d_gate = nullptr)
{
	if (n_reads >= (1ull << 32) - (1ull << 24)) return fail(VG_EINVAL, "more than 2^32 - 2^24 reads in one batch");
	// packed-read buffers are sized from the batch's total length (8 bytes from the device; the handle's streams are
	// non-blocking, so this copy does not wait for kernels in flight)
	uint64_t total = total_bases;
	if (!d_n_reads) HIP_TRY(hipMemcpy(&total, d_offsets + n_reads, 8, hipMemcpyDeviceToHost));
	if (total >= (1ull << 37)) return fail(VG_ETOOBIG, "a batch of 2^37 bases or more (the kernels address a batch's 32-base slots with 32 bits)");
	if (total && (!d_bases || (!d_quals && !d_gate))) return fail(VG_EINVAL, "null argument: a batch with bases needs the base text and its quality strings or gate words");
	int rc = size_slot(sl, n_reads, total >> 5);
	if (rc) return rc;
	const uint64_t tb = d_n_reads ? 0ull : total;                // (a batch framed on the device: sizes are upper bounds, the mean length is unknown here)
	return enqueue_batch(ix, sl, ix->stats_enabled, d_bases, d_quals, d_gate, d_offsets, n_reads, produced_on, d_n_reads, false, tb);
}

extern "C" int vg_reads_process_device(vg_index *ix, const uint8_t *d_bases, const uint8_t *d_quals, const uint64_t *d_offsets, uint64_t n_reads)
{
	if (!ix || (!d_offsets && n_reads)) return fail(VG_EINVAL, "null argument");
	if (n_reads == 0) return VG_OK;
	HIP_TRY(hipSetDevice(ix->device));
	Slot *sl = nullptr;
	int rc = acquire_slot(ix, &sl, ix->cur_sample);
	if (rc) return rc;
	return launch_batch(ix, *sl, d_bases, d_quals, d_offsets, n_reads);
}

extern "C" int vg_reads_process_device_gated(vg_index *ix, const uint8_t *d_bases, const uint32_t *d_gate_words, const uint64_t *d_offsets, uint64_t n_reads)
{
	if (!ix || ((!d_offsets || !d_gate_words) && n_reads)) return fail(VG_EINVAL, "null argument");
	if (n_reads == 0) return VG_OK;
	HIP_TRY(hipSetDevice(ix->device));
	Slot *sl = nullptr;
	int rc = acquire_slot(ix, &sl, ix->cur_sample);
	if (rc) return rc;
	return launch_batch(ix, *sl, d_bases, nullptr, d_offsets, n_reads, nullptr, nullptr, 0, d_gate_words);
}

// A batch that is already 2-bit packed, in HOST memory ("pre-packed 2-bit + the <= 31 quality chars the gate can
// see", the latter reduced to the comparison's result): the slot's packed-read buffers are filled by copies instead of by the
// pack kernel.  copy_on: the stream the (asynchronous, page-locked source) copies go to, or nullptr for blocking copies.
static int launch_packed(vg_index *ix, Slot &sl, const uint64_t *kmers, const uint64_t *meta, const uint64_t *offsets, uint64_t n_reads, uint64_t n_chunks, hipStream_t copy_on)
{
	if (n_reads >= (1ull << 32) - (1ull << 24)) return fail(VG_EINVAL, "more than 2^32 - 2^24 reads in one batch");
	if (n_chunks >= (1ull << 32)) return fail(VG_ETOOBIG, "a batch of 2^32 chunks or more");
	int rc;
	if ((rc = size_slot(sl, n_reads, n_chunks)) || (rc = sl.st_offsets.reserve(n_reads + 1, "read offsets"))) return rc;
	if (copy_on) {
		// (hipMemcpyDefault: the source is page-locked host memory, or -- a read store's batch -- device memory)
		if (n_chunks) HIP_TRY(hipMemcpyAsync(sl.pk_kmer.p, kmers, n_chunks * 8, hipMemcpyDefault, copy_on));
		HIP_TRY(hipMemcpyAsync(sl.pk_meta.p, meta, n_reads * 8, hipMemcpyDefault, copy_on));
		HIP_TRY(hipMemcpyAsync(sl.st_offsets.p, offsets, (n_reads + 1) * 8, hipMemcpyDefault, copy_on));
	} else {
		if (n_chunks) HIP_TRY(hipMemcpy(sl.pk_kmer.p, kmers, n_chunks * 8, hipMemcpyHostToDevice));
		HIP_TRY(hipMemcpy(sl.pk_meta.p, meta, n_reads * 8, hipMemcpyHostToDevice));
		HIP_TRY(hipMemcpy(sl.st_offsets.p, offsets, (n_reads + 1) * 8, hipMemcpyHostToDevice));
	}
	return enqueue_batch(ix, sl, ix->stats_enabled, nullptr, nullptr, nullptr, sl.st_offsets.p, n_reads, copy_on, nullptr, true, 0);
}

// The check of a packed batch that a caller hands in (vg_reads_submit_packed*, vg_read_store_push): monotone chunk offsets from 0,
// at most 31 chunks per read, no reserved bit in a flag word.  Gives the batch's chunk count and its reads with a character other
// than ACGTN.
static int check_packed(const uint64_t *kmers, const uint64_t *meta, const uint64_t *chunk_offsets, uint64_t n_reads, uint64_t &n_chunks, uint64_t &invalid)
{
	if (chunk_offsets[0] != 0) return fail(VG_EINVAL, "chunk_offsets[0] must be 0");
	uint64_t n_invalid = 0, bad = 0;
	for (uint64_t i = 0; i < n_reads; i++) {                     // (branch-free: one pass over three arrays, the compiler vectorises it)
		const uint64_t d = chunk_offsets[i + 1] - chunk_offsets[i];
		bad |= (chunk_offsets[i + 1] < chunk_offsets[i] ? 1ull : 0ull) | (d > 31 ? 2ull : 0ull) | ((meta[i] & 0x3FFFFFFF00000000ull) ? 4ull : 0ull);
		n_invalid += meta[i] >> 63;
	}
	if (bad & 1ull) return fail(VG_EINVAL, "chunk offsets not monotone");
	if (bad & 2ull) return fail(VG_EBADREAD, "a packed read of more than 31 chunks (a FASTQ line the reference can read holds at most 1022 bases, qv.cc:700)");
	if (bad & 4ull) return fail(VG_EINVAL, "a packed read's flag word has reserved bits set (bits 0-31: gate bits, 62: N inside the read, 63: another character; nothing else)");
	n_chunks = chunk_offsets[n_reads];
	invalid = n_invalid;
	if (n_chunks && !kmers) return fail(VG_EINVAL, "null argument");
	return VG_OK;
}

// pinned: the caller's arrays are page-locked and stay untouched until vg_sync -- the copies are asynchronous (ingest stream) and
// the call returns as soon as the batch is enqueued (vg_reads_submit_packed_async: a caller that packed a whole file ahead of the
// index hands over hundreds of batches; with blocking copies each cost ~10 ms of the host's time)
static int submit_packed_impl(vg_index *ix, const uint64_t *kmers, const uint64_t *meta, const uint64_t *chunk_offsets, uint64_t n_reads, bool pinned)
{
	HIP_TRY(hipSetDevice(ix->device));
	uint64_t n_chunks = 0, invalid = 0;
	int rc = check_packed(kmers, meta, chunk_offsets, n_reads, n_chunks, invalid);
	if (rc) return rc;
	Slot *sl = nullptr;
	if ((rc = acquire_slot(ix, &sl, ix->cur_sample))) return rc;
	// the flat-batch offsets of the trimmed reads (32 x chunks before each), in the slot's page-locked staging
	if (n_reads + 1 > sl->hp_offsets.cap && (rc = reserve_together({&sl->hp_meta, &sl->hp_offsets}, (n_reads + 1) * 5 / 4, "packed staging"))) return rc;
	for (uint64_t i = 0; i <= n_reads; i++) sl->hp_offsets.p[i] = 32 * chunk_offsets[i];
	hipStream_t is = ix->ingest_or_main();
	rc = launch_packed(ix, *sl, kmers, meta, sl->hp_offsets.p, n_reads, n_chunks, is);
	if (rc == VG_OK && !pinned) HIP_TRY(hipStreamSynchronize(is));          // the caller's arrays are free again
	if (rc == VG_OK) { ix->host_invalid += invalid; ix->planes[sl->plane].invalid += invalid; }
	return rc;
}
extern "C" int vg_reads_submit_packed(vg_index *ix, const uint64_t *kmers, const uint64_t *meta, const uint64_t *chunk_offsets, uint64_t n_reads)
{
	if (!ix || !chunk_offsets || (n_reads && !meta)) return fail(VG_EINVAL, "null argument");
	if (n_reads == 0) return VG_OK;
	return guarded([&]() -> int { return submit_packed_impl(ix, kmers, meta, chunk_offsets, n_reads, false); });
}
extern "C" int vg_reads_submit_packed_async(vg_index *ix, const uint64_t *kmers, const uint64_t *meta, const uint64_t *chunk_offsets, uint64_t n_reads)
{
	if (!ix || !chunk_offsets || (n_reads && !meta)) return fail(VG_EINVAL, "null argument");
	if (n_reads == 0) return VG_OK;
	return guarded([&]() -> int { return submit_packed_impl(ix, kmers, meta, chunk_offsets, n_reads, true); });
}

// ---- a read store: packed batches parked in device memory before (or beside) an index handle -------------------------------
// The command line packs the FASTQ file while vg_index_open runs.  Keeping what it packs in page-locked HOST memory until the
// handle exists cost 0.15 s per GB to lock and 0.1 s per GB to give back when the process ends (11 GB for 200 M reads: more
// than the whole read loop), and the copies up only started after the open.  The device has ~45 GB to spare beside an hg38
// index and the link is idle two thirds of the open's time: the batches go up as they are packed, out of two small staging
// buffers, and the open handle takes them from device memory.
struct StoredBatch { const uint64_t *kmers, *meta, *offsets; uint64_t n_reads, n_chunks; };
struct vg_read_store {
	int device = 0;
	uint8_t *block = nullptr;
	uint64_t bytes = 0, used = 0, reads = 0, invalid = 0;
	hipStream_t stream = nullptr;
	std::vector<StoredBatch> batches;
};
__global__ void vg_chunk_to_flat_offsets(uint64_t *__restrict__ o, const uint64_t n)
{
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) o[i] <<= 5;
}
extern "C" int vg_read_store_create(int device, uint64_t max_bytes, vg_read_store **out)
{
	if (!out || max_bytes == 0) return fail(VG_EINVAL, "null argument / a store of no bytes");
	*out = nullptr;
	return guarded([&]() -> int {
		HIP_TRY(hipSetDevice(device));
		std::unique_ptr<vg_read_store> rs(new vg_read_store);
		rs->device = device;
		max_bytes = (max_bytes + 4095) & ~4095ull;
		hipError_t e = vg_malloc_patient((void **)&rs->block, max_bytes);
		if (e != hipSuccess) { char t[64]; snprintf(t, sizeof t, "%.1f GB", max_bytes / 1e9); return fail(VG_ENOMEM, "hipMalloc(read store, %s): %s", t, hipGetErrorString(e)); }
		rs->bytes = max_bytes;
		if (hipStreamCreateWithFlags(&rs->stream, hipStreamNonBlocking) != hipSuccess) { (void)hipFree(rs->block); return fail(VG_ENODEV, "hipStreamCreate(read store) failed"); }
		*out = rs.release();
		return VG_OK;
	});
}
extern "C" void vg_read_store_destroy(vg_read_store *rs)
{
	if (!rs) return;
	(void)hipSetDevice(rs->device);
	if (rs->stream) { (void)hipStreamSynchronize(rs->stream); (void)hipStreamDestroy(rs->stream); }
	if (rs->block) (void)hipFree(rs->block);
	delete rs;
}
extern "C" uint64_t vg_read_store_reads(const vg_read_store *rs) { return rs ? rs->reads : 0; }
extern "C" uint64_t vg_read_store_bytes_used(const vg_read_store *rs) { return rs ? rs->used : 0; }
extern "C" int vg_read_store_flush(vg_read_store *rs)
{
	if (!rs) return fail(VG_EINVAL, "null argument");
	HIP_TRY(hipSetDevice(rs->device));
	HIP_TRY(hipStreamSynchronize(rs->stream));
	return VG_OK;
}
extern "C" int vg_read_store_push(vg_read_store *rs, const uint64_t *kmers, const uint64_t *meta, const uint64_t *chunk_offsets, uint64_t n_reads)
{
	if (!rs || !chunk_offsets || (n_reads && !meta)) return fail(VG_EINVAL, "null argument");
	return guarded([&]() -> int {
		HIP_TRY(hipSetDevice(rs->device));
		HIP_TRY(hipStreamSynchronize(rs->stream));               // the arrays of the push before this one are free again
		if (n_reads == 0) return VG_OK;
		uint64_t n_chunks = 0, invalid = 0;
		const int rc = check_packed(kmers, meta, chunk_offsets, n_reads, n_chunks, invalid);
		if (rc) return rc;
		if (n_reads >= (1ull << 32) - (1ull << 24) || n_chunks >= (1ull << 32)) return fail(VG_ETOOBIG, "a batch of 2^32 chunks or more");
		auto up = [](uint64_t b) { return (b + 255) & ~255ull; };
		const uint64_t need = up((n_chunks + 2) * 8) + up(n_reads * 8) + up((n_reads + 1) * 8);
		if (rs->used + need > rs->bytes) { char t[96]; snprintf(t, sizeof t, "%.2f of %.2f GB used, this batch needs %.3f GB", rs->used / 1e9, rs->bytes / 1e9, need / 1e9); return fail(VG_ENOMEM, "the read store is full (%s)", t); }
		StoredBatch b;
		uint8_t *at = rs->block + rs->used;
		b.kmers = (uint64_t *)at; at += up((n_chunks + 2) * 8);
		b.meta = (uint64_t *)at; at += up(n_reads * 8);
		b.offsets = (uint64_t *)at;
		b.n_reads = n_reads; b.n_chunks = n_chunks;
		if (n_chunks) HIP_TRY(hipMemcpyAsync((void *)b.kmers, kmers, n_chunks * 8, hipMemcpyHostToDevice, rs->stream));
		HIP_TRY(hipMemcpyAsync((void *)b.meta, meta, n_reads * 8, hipMemcpyHostToDevice, rs->stream));
		HIP_TRY(hipMemcpyAsync((void *)b.offsets, chunk_offsets, (n_reads + 1) * 8, hipMemcpyHostToDevice, rs->stream));
		vg_chunk_to_flat_offsets<<<(unsigned)((n_reads + 1 + 255) / 256), 256, 0, rs->stream>>>((uint64_t *)b.offsets, n_reads + 1);
		HIP_TRY(hipGetLastError());
		rs->used += need; rs->reads += n_reads; rs->invalid += invalid;
		rs->batches.push_back(b);
		return VG_OK;
	});
}
extern "C" int vg_reads_submit_store(vg_index *ix, vg_read_store *rs)
{
	if (!ix || !rs) return fail(VG_EINVAL, "null argument");
	if (ix->device != rs->device) return fail(VG_EINVAL, "the read store and the index handle live on different devices");
	return guarded([&]() -> int {
		HIP_TRY(hipSetDevice(ix->device));
		HIP_TRY(hipStreamSynchronize(rs->stream));               // everything pushed is in device memory
		hipStream_t is = ix->ingest_or_main();
		for (const StoredBatch &b : rs->batches) {
			Slot *sl = nullptr;
			int rc = acquire_slot(ix, &sl, ix->cur_sample);
			if (rc) return rc;
			rc = launch_packed(ix, *sl, b.kmers, b.meta, b.offsets, b.n_reads, b.n_chunks, is);
			if (rc) return rc;
		}
		ix->host_invalid += rs->invalid; ix->planes[ix->cur_sample].invalid += rs->invalid;
		return VG_OK;
	});
}

static int submit_impl(vg_index *ix, const uint8_t *bases, const uint8_t *quals, const uint64_t *offsets, uint64_t n_reads);
extern "C" int vg_reads_submit(vg_index *ix, const uint8_t *bases, const uint8_t *quals, const uint64_t *offsets, uint64_t n_reads)
{
	if (!ix || !offsets) return fail(VG_EINVAL, "null argument");
	if (n_reads == 0) return VG_OK;
	return guarded([&] { return submit_impl(ix, bases, quals, offsets, n_reads); });
}
static int submit_impl(vg_index *ix, const uint8_t *bases, const uint8_t *quals, const uint64_t *offsets, uint64_t n_reads)
{
	HIP_TRY(hipSetDevice(ix->device));
	const uint64_t base0 = offsets[0];
	const uint64_t total = offsets[n_reads] - base0;
	for (uint64_t i = 0; i < n_reads; i++) {
		if (offsets[i + 1] < offsets[i]) return fail(VG_EINVAL, "offsets not monotone");
		if (offsets[i + 1] - offsets[i] > 1022) return fail(VG_EBADREAD, "read longer than 1022 bases (reference BUF_SIZE 1024, qv.cc:700)");
	}
	Slot *slp = nullptr;
	int rc = acquire_slot(ix, &slp, ix->cur_sample);
	if (rc) return rc;
	Slot &sl = *slp;
	if ((rc = sl.st_bases.reserve(total + 64, "base text")) || (rc = sl.st_quals.reserve(total + 64, "quality strings")) || (rc = sl.st_offsets.reserve(n_reads + 1, "read offsets"))) return rc;
	std::vector<uint64_t> rel;
	const uint64_t *off = offsets;
	if (base0) { rel.resize(n_reads + 1); for (uint64_t i = 0; i <= n_reads; i++) rel[i] = offsets[i] - base0; off = rel.data(); }
	// plain (blocking) copies: when they return the caller's buffers are free again; kernels of earlier batches keep running
	HIP_TRY(hipMemcpy(sl.st_bases.p, bases + base0, total, hipMemcpyHostToDevice));
	HIP_TRY(hipMemcpy(sl.st_quals.p, quals + base0, total, hipMemcpyHostToDevice));
	HIP_TRY(hipMemcpy(sl.st_offsets.p, off, (n_reads + 1) * 8, hipMemcpyHostToDevice));
	return launch_batch(ix, sl, sl.st_bases.p, sl.st_quals.p, sl.st_offsets.p, n_reads);
}

// ---- FASTQ text in, framed and processed on the device (replaces the four fgets() + strlen of qv.cc:760-784) ---------------
// CPUs this process may actually use: the hardware threads, capped by a cgroup CPU quota (cpu.max: "<quota> <period>" -- the GPU
// boxes of this pool give a container 16 CPUs' worth of time on a 256-thread host; threads beyond the quota only take time from
// each other, and a spinning one takes it from the working ones)
static unsigned usable_cpus()
{
	unsigned h = std::thread::hardware_concurrency();
	if (h == 0) h = 1;
	for (const char *path : {"/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"}) {
		FILE *f = fopen(path, "r");
		if (!f) continue;
		long long q = -1, per = 100000;
		char a[64] = "";
		if (fscanf(f, "%63s %lld", a, &per) >= 1 && strcmp(a, "max") != 0) q = atoll(a);
		fclose(f);
		if (q > 0 && per > 0) { const unsigned c = (unsigned)((q + per - 1) / per); if (c && c < h) h = c; }
		break;
	}
	return h;
}
static int host_pack_threads_default()
{
	if (const char *e = getenv("VG_PACK_THREADS")) return std::max(0, atoi(e));
	const unsigned c = usable_cpus();
	// Host packing pays when the process has CPUs to spare BESIDE whoever reads the file and feeds the device: from 32 usable CPUs on,
	// half of them (at most 96).  Below that the device-side framing is the dependable route: on this pool's boxes (a 16-CPU quota)
	// 13 packing threads reach 2.3 x 10^8 reads/s when nothing else runs and 0.9 x 10^8 when two more processes do -- a process that
	// asks for more CPU time than its quota is stopped for the rest of the 100 ms period -- against a steady 1.65 x 10^8 for the
	// device framing.
	return c >= 32 ? (int)std::min(c / 2, 96u) : 0;
}

extern "C" int vg_fastq_stream_begin_packed(vg_index *ix, int host_threads)
{
	if (!ix) return fail(VG_EINVAL, "null argument");
	if (host_threads < 0) host_threads = host_pack_threads_default();
	if (host_threads == 0) return vg_fastq_stream_begin(ix);
	if (host_threads > 256) host_threads = 256;               // (threads beyond the CPUs there are only spin)
	return guarded([&]() -> int {
		HIP_TRY(hipSetDevice(ix->device));
		if (!ix->packer || ix->packer->threads() != host_threads) { delete ix->packer; ix->packer = nullptr; ix->packer = new vgp::Packer(host_threads); }
		ix->packer->begin();
		ix->fq_open = true; ix->fq_packed = true; ix->fq_bgzf = false; ix->fq_gzip = false; ix->fq_prev_slot = -1;
		ix->fq_sample = ix->cur_sample;                          // the stream stays with the sample selected now
		return VG_OK;
	});
}

// one chunk of a host-packed stream: frame + pack into the slot's page-locked staging (host threads; the caller's buffer is free
// when this returns), then asynchronous copies of the packed form on the ingest stream and the read loop behind them
static int push_packed(vg_index *ix, const uint8_t *text, uint64_t nbytes)
{
	HIP_TRY(hipSetDevice(ix->device));
	if (ix->packer->poisoned()) return VG_OK;                 // refused earlier: the rest of the stream is the host reader's
	Slot *slp = nullptr;
	int rc = acquire_slot(ix, &slp, ix->fq_sample);            // (its previous batch has finished: the staging is free)
	if (rc) return rc;
	Slot &sl = *slp;
	const uint64_t need_r = vgp::Packer::reads_cap(nbytes) + 1, need_k = vgp::Packer::kmers_cap(nbytes);
	if ((rc = sl.hp_kmers.reserve(need_k, "packed staging")) || (rc = reserve_together({&sl.hp_meta, &sl.hp_offsets}, need_r, "packed staging"))) return rc;
	vgp::Staging st;
	st.kmers = sl.hp_kmers.p; st.kmers_cap = sl.hp_kmers.cap; st.meta = sl.hp_meta.p; st.offsets = sl.hp_offsets.p; st.reads_cap = sl.hp_offsets.cap;
	const vgp::ChunkResult r = ix->packer->push(text, nbytes, st);
	if (r.n_reads == 0) return VG_OK;                            // (a refused block poisons the stream; the records framed before it are still this batch)
	rc = launch_packed(ix, sl, sl.hp_kmers.p, sl.hp_meta.p, sl.hp_offsets.p, r.n_reads, r.n_chunks, ix->ingest_or_main());
	if (rc == VG_OK) { ix->host_invalid += r.n_invalid; ix->planes[sl.plane].invalid += r.n_invalid; }
	return rc;
}

extern "C" int vg_fastq_stream_begin(vg_index *ix)
{
	if (!ix) return fail(VG_EINVAL, "null argument");
	ix->fq_packed = false; ix->fq_bgzf = false; ix->fq_gzip = false;
	HIP_TRY(hipSetDevice(ix->device));
	HIP_TRY(hipMemsetAsync(ix->d_fq, 0, sizeof(FqStream), ix->ingest_or_main()));
	ix->fq_open = true; ix->fq_prev_slot = -1;
	ix->fq_sample = ix->cur_sample;                              // the stream stays with the sample selected now
	return VG_OK;
}

// What a chunk of `nbytes` of text needs in its slot.  Capacities follow from the chunk's size alone: lines average at least 8 bytes
// (or the chunk is refused), a record has four.
static int fq_reserve(Slot &sl, uint64_t nbytes)
{
	int rc;
	const uint64_t span = (uint64_t)FQ_CARRY + nbytes;
	const uint64_t n_tiles = (span + FQ_TILE - 1) / FQ_TILE;
	const uint64_t cap_lines = span / 8 + 16, cap_rec = cap_lines / 4 + 1;
	// the chunk after this slot's last one copied the tail of its text on the ingest stream: that must have happened before
	// the text is overwritten (the slot's own batch being finished does not imply it)
	if (sl.fq_tail_wanted) { HIP_TRY(hipEventSynchronize(sl.e_fq)); sl.fq_tail_wanted = false; }
	if ((rc = sl.fq_text.reserve(n_tiles * FQ_TILE + 64, "FASTQ text"))) return rc;
	if ((rc = sl.fq_tiles.reserve(n_tiles + 2, "FASTQ tiles"))) return rc;
	if ((rc = sl.fq_lines.reserve(cap_lines + 2, "FASTQ lines"))) return rc;
	if ((rc = sl.fq_chunk.reserve(1, "FASTQ chunk"))) return rc;
	if ((rc = sl.st_offsets.reserve(cap_rec + 2, "read offsets"))) return rc;
	if ((rc = sl.st_bases.reserve(span + 64, "base text"))) return rc;              // the bases of a chunk are shorter than its text
	if ((rc = sl.st_gate.reserve(cap_rec + 2, "gate words"))) return rc;
	if ((rc = sl.fq_tmp.reserve(vg_dev_scan_temp_bytes(n_tiles + 1, cap_rec + 1), "scan scratch"))) return rc;
	return VG_OK;
}

// The framing sequence of one chunk whose `nbytes` of text are (or will be, by work already enqueued on the ingest stream) at
// sl.fq_text.p + FQ_CARRY: carry, newline counts, line starts, record lengths, verdict, gather -- and the read loop behind them.
// Text chunks and inflated BGZF chunks (bad_key: see vg_fqs_prepare) both come through here.
static int fq_frame_and_launch(vg_index *ix, Slot &sl, int slot_no, uint64_t nbytes, const unsigned long long *bad_key)
{
	hipStream_t is = ix->ingest_or_main();
	const uint64_t span = (uint64_t)FQ_CARRY + nbytes;
	const uint64_t n_tiles = (span + FQ_TILE - 1) / FQ_TILE;
	const uint64_t cap_lines = span / 8 + 16, cap_rec = cap_lines / 4 + 1;
	sl.fq_text_len = nbytes;
	const uint8_t *prev_end = nullptr;
	if (ix->fq_prev_slot >= 0) { const Slot &pv = ix->slot[ix->fq_prev_slot]; prev_end = pv.fq_text.p + FQ_CARRY + pv.fq_text_len; }
	vg_fqs_prepare<<<1, 256, 0, is>>>(ix->d_fq, sl.fq_chunk.p, prev_end, sl.fq_text.p, (uint32_t)nbytes, bad_key);
	if (ix->fq_prev_slot >= 0) { Slot &pv = ix->slot[ix->fq_prev_slot]; HIP_TRY(hipEventRecord(pv.e_fq, is)); pv.fq_tail_wanted = true; }
	vg_fq_count_newlines<<<(unsigned)n_tiles, 256, 0, is>>>(sl.fq_text.p, sl.fq_chunk.p, sl.fq_tiles.p);
	HIP_TRY(hipMemsetAsync(sl.fq_tiles.p + n_tiles, 0, 4, is));
	HIP_TRY(hipGetLastError());
	int se = vg_dev_exclusive_scan_u32(sl.fq_tiles.p, sl.fq_tiles.p, n_tiles + 1, is, sl.fq_tmp.p, sl.fq_tmp.cap);
	if (se != 0) return fail(VG_ENODEV, "device scan failed: %s", hipGetErrorString((hipError_t)se));
	const uint32_t *d_n_lines = sl.fq_tiles.p + n_tiles;
	vg_fq_line_starts<<<(unsigned)n_tiles, 256, 0, is>>>(sl.fq_text.p, sl.fq_chunk.p, sl.fq_tiles.p, sl.fq_lines.p, (uint32_t)cap_lines);
	vg_fq_record_lengths<<<1024, 256, 0, is>>>(sl.fq_lines.p, d_n_lines, sl.fq_chunk.p, sl.st_offsets.p, (uint32_t)cap_rec, (uint32_t)cap_lines);
	HIP_TRY(hipGetLastError());
	se = vg_dev_exclusive_scan_u64(sl.st_offsets.p, sl.st_offsets.p, cap_rec + 1, is, sl.fq_tmp.p, sl.fq_tmp.cap);
	if (se != 0) return fail(VG_ENODEV, "device scan failed: %s", hipGetErrorString((hipError_t)se));
	vg_fqs_finish<<<1, 1, 0, is>>>(ix->d_fq, sl.fq_chunk.p, d_n_lines, sl.fq_lines.p, sl.st_offsets.p, (uint32_t)cap_rec);
	vg_fq_gather<<<(unsigned)std::min<uint64_t>((cap_rec + 3) / 4, (uint64_t)ix->cus * 32), 256, 0, is>>>(sl.fq_text.p, sl.fq_lines.p, sl.st_offsets.p, sl.fq_chunk.p, sl.st_bases.p, sl.st_gate.p);
	HIP_TRY(hipGetLastError());
	ix->fq_prev_slot = slot_no;
	return launch_batch(ix, sl, sl.st_bases.p, nullptr, sl.st_offsets.p, cap_rec, is, &sl.fq_chunk.p->n_reads, span, sl.st_gate.p);
}

static int push_bgzf(vg_index *ix, const uint8_t *data, uint64_t nbytes);
static int push_gzip(vg_index *ix, const uint8_t *data, uint64_t nbytes);
static int end_gzip(vg_index *ix);

// One chunk of the stream: a blocking host-to-device copy (the caller's buffer is free when the call returns), then framing
// and the read loop are only ENQUEUED -- record counts stay on the device until vg_fastq_stream_end.
extern "C" int vg_fastq_stream_push(vg_index *ix, const uint8_t *text, uint64_t nbytes)
{
	if (!ix || (!text && nbytes)) return fail(VG_EINVAL, "null argument");
	if (!ix->fq_open) return fail(VG_EINVAL, "vg_fastq_stream_push without vg_fastq_stream_begin");
	if (nbytes == 0) return VG_OK;
	if (nbytes >= (1ull << 31)) return fail(VG_EINVAL, "FASTQ chunk of 2 GiB or more");
	if (ix->fq_packed) return guarded([&] { return push_packed(ix, text, nbytes); });
	if (ix->fq_bgzf) return guarded([&] { return push_bgzf(ix, text, nbytes); });
	if (ix->fq_gzip) return guarded([&] { return push_gzip(ix, text, nbytes); });
	HIP_TRY(hipSetDevice(ix->device));
	const int slot_no = ix->next_slot;
	Slot *slp = nullptr;
	int rc = acquire_slot(ix, &slp, ix->fq_sample);
	if (rc) return rc;
	Slot &sl = *slp;
	if ((rc = fq_reserve(sl, nbytes))) return rc;
	HIP_TRY(hipMemcpy(sl.fq_text.p + FQ_CARRY, text, nbytes, hipMemcpyHostToDevice));
	return fq_frame_and_launch(ix, sl, slot_no, nbytes, nullptr);
}

// ---- BGZF streams: compressed bytes cross the link, the inflate kernel writes the slot's text, the framing above takes it from there
constexpr uint64_t BZ_SLOT_TEXT_MAX = (1ull << 31) - 1;               // the text chunks' own limit

static std::string bz_describe(unsigned long long key)
{
	return "BGZF block at compressed offset " + std::to_string(key >> 4) + ": " + vg_inflate_strerror((int)(key & 15u));
}

extern "C" int vg_fastq_stream_begin_bgzf(vg_index *ix)
{
	if (!ix) return fail(VG_EINVAL, "null argument");
	return guarded([&]() -> int {
		int rc = vg_fastq_stream_begin(ix);
		if (rc) return rc;
		BgzfStream &bz = ix->bz;
		HIP_TRY(hipMemsetAsync(bz.d_key, 0xff, sizeof *bz.d_key, ix->ingest_or_main()));
		bz.carry.clear(); bz.index.clear();
		bz.comp_pos = 0; bz.text_pos = 0; bz.host_key = ~0ull; bz.header_bad = false;
		bz.bam = false; bz.bam_hdr_done = false; bz.bam_not_bam = false; bz.bam_hdr.clear(); bz.bam_hdr_end = 0; bz.bam_n_ref = 0;
		bz.slot_text = BZ_SLOT_TEXT_MAX;
		if (const char *e = getenv("VG_BGZF_SLOT_TEXT")) bz.slot_text = std::min<uint64_t>(BZ_SLOT_TEXT_MAX, std::max<uint64_t>(VG_BGZF_MAX_ISIZE, strtoull(e, nullptr, 10)));   // (tests: the split path with small inputs)
		ix->fq_bgzf = true;
		return VG_OK;
	});
}

// blocks [i0, i1) of a push (bz.blocks; their bytes are in p, in_off relative to it) -> one slot: copy the compressed bytes and the
// table up, inflate into the slot's text, frame
static int bam_slot_frame(vg_index *ix, Slot &sl, int slot_no, uint64_t text_n, uint64_t text_off);
static int bam_reserve(Slot &sl, uint64_t nbytes);
static int bgzf_slot(vg_index *ix, const uint8_t *p, size_t i0, size_t i1, uint64_t text_n)
{
	BgzfStream &bz = ix->bz;
	const vg_bgzf_block &first = bz.blocks[i0], &last = bz.blocks[i1 - 1];
	const uint64_t c0 = first.comp_off - bz.comp_pos, c1 = (uint64_t)last.in_off + last.in_len + 8;
	bz.tab.assign(bz.blocks.begin() + (long)i0, bz.blocks.begin() + (long)i1);
	for (vg_bgzf_block &b : bz.tab) { b.in_off -= (uint32_t)c0; b.text_off -= first.text_off; }
	if (text_n == 0) {
		// nothing to frame (empty blocks, the end-of-file marker): their payloads and CRCs are checked here
		for (const vg_bgzf_block &b : bz.tab) {
			uint8_t none;
			const int rc = vg_inflate_block_host(p + c0 + b.in_off, b.in_len, &none, 0, b.crc);
			if (rc) bz.host_key = std::min(bz.host_key, (unsigned long long)b.comp_off << 4 | (unsigned)rc);
		}
		return VG_OK;
	}
	HIP_TRY(hipSetDevice(ix->device));
	const int slot_no = ix->next_slot;
	Slot *slp = nullptr;
	int rc = acquire_slot(ix, &slp, ix->fq_sample);
	if (rc) return rc;
	Slot &sl = *slp;
	if ((rc = bz.bam ? bam_reserve(sl, text_n) : fq_reserve(sl, text_n))) return rc;
	if ((rc = sl.bz_comp.reserve(c1 - c0 + 64, "BGZF bytes"))) return rc;   // (the kernel loads whole aligned 16-byte vectors around a payload)
	if ((rc = sl.bz_tab.reserve(bz.tab.size(), "BGZF block table"))) return rc;
	if ((rc = sl.bz_status.reserve(bz.tab.size(), "BGZF block results"))) return rc;
	HIP_TRY(hipMemcpy(sl.bz_comp.p, p + c0, c1 - c0, hipMemcpyHostToDevice));
	HIP_TRY(hipMemcpy(sl.bz_tab.p, bz.tab.data(), bz.tab.size() * sizeof(vg_bgzf_block), hipMemcpyHostToDevice));
	vg_bgzf_inflate_kernel<<<(unsigned)bz.tab.size(), 64, 0, ix->ingest_or_main()>>>(sl.bz_comp.p, sl.bz_tab.p, (uint32_t)bz.tab.size(), bz.bam ? sl.bam_raw.p + BAM_CARRY : sl.fq_text.p + FQ_CARRY, sl.bz_status.p, bz.d_key);
	HIP_TRY(hipGetLastError());
	if (bz.bam) return bam_slot_frame(ix, sl, slot_no, text_n, first.text_off);
	return fq_frame_and_launch(ix, sl, slot_no, text_n, bz.d_key);
}

static int push_bgzf(vg_index *ix, const uint8_t *data, uint64_t nbytes)
{
	BgzfStream &bz = ix->bz;
	if (bz.header_bad) return fail(VG_EIO, "the BGZF stream ended at bytes that are no BGZF block (an earlier push said where)");
	const uint8_t *p = data;
	uint64_t len = nbytes;
	if (!bz.carry.empty()) { bz.carry.insert(bz.carry.end(), data, data + nbytes); p = bz.carry.data(); len = bz.carry.size(); }
	bz.blocks.clear();
	uint64_t tail = 0, bad_off = 0;
	const int hdr_rc = vg_bgzf_scan(p, len, bz.comp_pos, bz.text_pos, bz.blocks, &tail, &bad_off);
	size_t first_send = 0;
	if (bz.bam && !bz.bam_hdr_done) {
		// the leading blocks are inflated here until the BAM header parses; blocks wholly inside it never go to the device
		first_send = bz.blocks.size();
		for (size_t i = 0; i < bz.blocks.size() && bz.host_key == ~0ull; i++) {
			const vg_bgzf_block &b = bz.blocks[i];
			const size_t o = bz.bam_hdr.size();
			bz.bam_hdr.resize(o + b.isize + 1);
			const int brc = vg_inflate_block_host(p + b.in_off, b.in_len, bz.bam_hdr.data() + o, b.isize, b.crc);
			bz.bam_hdr.resize(o + b.isize);
			if (brc) { bz.host_key = std::min(bz.host_key, (unsigned long long)b.comp_off << 4 | (unsigned)brc); break; }   // (vg_fastq_stream_end names it; nothing behind it is framed)
			const int rc = vg_bam_header(bz.bam_hdr.data(), bz.bam_hdr.size(), &bz.bam_hdr_end, &bz.bam_n_ref);
			if (rc == VG_BAM_BAD) { bz.bam_not_bam = true; bz.header_bad = true; return fail(VG_EIO, "the BGZF stream does not hold BAM: its inflated bytes do not start with the magic BAM\\1 and a header"); }
			if (rc == VG_BAM_OK) {
				bz.bam_hdr_done = true;
				first_send = bz.bam_hdr_end < b.text_off + b.isize ? i : i + 1;
				std::vector<uint8_t>().swap(bz.bam_hdr);
				break;
			}
		}
	}
	if (bz.bam && bz.host_key != ~0ull) first_send = bz.blocks.size();   // a bad block among those checked here: the stream is over
	for (size_t i0 = first_send; i0 < bz.blocks.size();) {            // slots of at most slot_text bytes of text, cut at block boundaries
		size_t i1 = i0;
		uint64_t text_n = 0;
		while (i1 < bz.blocks.size() && (i1 == i0 || text_n + bz.blocks[i1].isize <= bz.slot_text)) text_n += bz.blocks[i1++].isize;
		const int rc = bgzf_slot(ix, p, i0, i1, text_n);
		if (rc) return rc;
		i0 = i1;
	}
	uint64_t used = 0;                                                  // bytes of p that whole blocks took
	for (const vg_bgzf_block &b : bz.blocks) bz.index.emplace_back(b.text_off, b.comp_off);
	if (!bz.blocks.empty()) { const vg_bgzf_block &b = bz.blocks.back(); bz.text_pos = b.text_off + b.isize; used = (uint64_t)b.in_off + b.in_len + 8; }
	if (hdr_rc) {
		bz.header_bad = true;
		bz.comp_pos += used;
		bz.carry.clear();
		return fail(VG_EIO, "BGZF block at compressed offset %s: not a BGZF block header (1f 8b 08 04, a BC subfield, BSIZE and ISIZE in range)", std::to_string(bad_off).c_str());
	}
	std::vector<uint8_t> rest(p + used, p + len);                       // the incomplete block, if any, waits for the next push
	bz.carry.swap(rest);
	bz.comp_pos += used;
	return VG_OK;
}

extern "C" int vg_fastq_stream_bgzf_locate(vg_index *ix, uint64_t text_offset, uint64_t *block_offset, uint32_t *within)
{
	if (!ix || !block_offset || !within) return fail(VG_EINVAL, "null argument");
	const BgzfStream &bz = ix->bz;
	if (text_offset > bz.text_pos) return fail(VG_EINVAL, "text offset beyond what the BGZF stream has seen");
	// the last block that starts at or before the offset (empty blocks in front of it are passed over)
	auto it = std::upper_bound(bz.index.begin(), bz.index.end(), std::pair<uint64_t, uint64_t>(text_offset, UINT64_MAX));
	if (text_offset == bz.text_pos || it == bz.index.begin()) { *block_offset = bz.comp_pos; *within = 0; return VG_OK; }   // the end of the blocks seen: whatever comes next
	--it;
	*block_offset = it->second; *within = (uint32_t)(text_offset - it->first);
	return VG_OK;
}

// ---- BGZF without a handle: whole blocks of a buffer -> text in host memory (the tests see every inflated byte through these)
static int bz_buffer_args(const uint8_t *bgzf, uint64_t nbytes, uint8_t *text, uint64_t *text_len, uint64_t *consumed, uint64_t *bad_block_offset)
{
	if ((!bgzf && nbytes) || !text_len || !consumed || !bad_block_offset || !text) return fail(VG_EINVAL, "null argument");
	if (nbytes >= (1ull << 32)) return fail(VG_EINVAL, "BGZF buffer of 4 GiB or more");
	*text_len = 0; *consumed = 0; *bad_block_offset = UINT64_MAX;
	return VG_OK;
}

extern "C" int vg_bgzf_scan_host(const uint8_t *bgzf, uint64_t nbytes, uint64_t *blocks, uint64_t blocks_cap, uint64_t *n_blocks, uint64_t *consumed, uint64_t *bad_block_offset)
{
	if ((!bgzf && nbytes) || (!blocks && blocks_cap) || !n_blocks || !consumed || !bad_block_offset) return fail(VG_EINVAL, "null argument");
	if (nbytes >= (1ull << 32)) return fail(VG_EINVAL, "BGZF buffer of 4 GiB or more");
	return guarded([&]() -> int {
		std::vector<vg_bgzf_block> bl;
		uint64_t tail = 0, bad = UINT64_MAX;
		const int rc = vg_bgzf_scan(bgzf, nbytes, 0, 0, bl, &tail, &bad);
		*n_blocks = bl.size();
		*consumed = bl.empty() ? 0 : (uint64_t)bl.back().in_off + bl.back().in_len + 8;
		*bad_block_offset = rc ? bad : UINT64_MAX;
		if (bl.size() > blocks_cap) return fail(VG_ETOOBIG, "more BGZF blocks than the caller's table holds");
		for (size_t i = 0; i < bl.size(); i++) { const vg_bgzf_block &b = bl[i]; uint64_t *o = blocks + 6 * i; o[0] = b.comp_off; o[1] = b.text_off; o[2] = b.in_off; o[3] = b.in_len; o[4] = b.isize; o[5] = b.crc; }
		if (rc) (void)fail(VG_EIO, "BGZF block at compressed offset %s: not a BGZF block header", std::to_string(bad).c_str());
		return VG_OK;
	});
}

extern "C" int vg_bgzf_inflate_host(const uint8_t *bgzf, uint64_t nbytes, uint8_t *text, uint64_t text_cap, uint64_t *text_len, uint64_t *consumed, uint64_t *bad_block_offset)
{
	int rc = bz_buffer_args(bgzf, nbytes, text, text_len, consumed, bad_block_offset);
	if (rc) return rc;
	return guarded([&]() -> int {
		std::vector<vg_bgzf_block> bl;
		uint64_t tail = 0, bad = UINT64_MAX;
		const int hdr_rc = vg_bgzf_scan(bgzf, nbytes, 0, 0, bl, &tail, &bad);
		for (const vg_bgzf_block &b : bl) {
			if (b.text_off + b.isize > text_cap) return fail(VG_ETOOBIG, "the text of the BGZF blocks does not fit the caller's buffer");
			const int brc = vg_inflate_block_host(bgzf + b.in_off, b.in_len, text + b.text_off, b.isize, b.crc);
			if (brc) {
				*bad_block_offset = b.comp_off; *consumed = b.comp_off;
				(void)fail(VG_EIO, "%s", bz_describe((unsigned long long)b.comp_off << 4 | (unsigned)brc).c_str());
				return VG_OK;
			}
			*text_len = b.text_off + b.isize;
			*consumed = (uint64_t)b.in_off + b.in_len + 8;
		}
		if (hdr_rc) { *bad_block_offset = bad; (void)fail(VG_EIO, "BGZF block at compressed offset %s: not a BGZF block header", std::to_string(bad).c_str()); }
		return VG_OK;
	});
}

extern "C" int vg_bgzf_inflate_device(int device, const uint8_t *bgzf, uint64_t nbytes, uint8_t *text, uint64_t text_cap, uint64_t *text_len, uint64_t *consumed, uint64_t *bad_block_offset)
{
	int rc = bz_buffer_args(bgzf, nbytes, text, text_len, consumed, bad_block_offset);
	if (rc) return rc;
	return guarded([&]() -> int {
		std::vector<vg_bgzf_block> bl;
		uint64_t tail = 0, bad = UINT64_MAX;
		const int hdr_rc = vg_bgzf_scan(bgzf, nbytes, 0, 0, bl, &tail, &bad);
		const uint64_t comp_n = bl.empty() ? 0 : (uint64_t)bl.back().in_off + bl.back().in_len + 8;
		const uint64_t text_n = bl.empty() ? 0 : bl.back().text_off + bl.back().isize;
		if (text_n > text_cap) return fail(VG_ETOOBIG, "the text of the BGZF blocks does not fit the caller's buffer");
		unsigned long long key = ~0ull;
		if (!bl.empty()) {
			HIP_TRY(hipSetDevice(device));
			DevBuf<uint8_t> d_comp, d_text; DevBuf<vg_bgzf_block> d_tab; DevBuf<uint32_t> d_status; DevBuf<unsigned long long> d_key;
			if ((rc = d_comp.reserve(comp_n + 64, "BGZF bytes")) || (rc = d_text.reserve(text_n + 64, "inflated text")) || (rc = d_tab.reserve(bl.size(), "BGZF block table"))
			    || (rc = d_status.reserve(bl.size(), "BGZF block results")) || (rc = d_key.reserve(1, "BGZF verdict"))) return rc;
			HIP_TRY(hipMemcpy(d_comp.p, bgzf, comp_n, hipMemcpyHostToDevice));
			HIP_TRY(hipMemcpy(d_tab.p, bl.data(), bl.size() * sizeof(vg_bgzf_block), hipMemcpyHostToDevice));
			HIP_TRY(hipMemset(d_key.p, 0xff, sizeof key));
			const bool timed = getenv("VG_VERBOSE") != nullptr;
			const int rounds = timed ? 3 : 1;                          // (verbose: the kernel's own rate, warmed -- the same text is written again)
			hipEvent_t e0 = nullptr, e1 = nullptr;
			if (timed) { HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&e1)); }
			float ms = 0;
			for (int r = 0; r < rounds; r++) {
				if (timed) HIP_TRY(hipEventRecord(e0, nullptr));
				vg_bgzf_inflate_kernel<<<(unsigned)bl.size(), 64>>>(d_comp.p, d_tab.p, (uint32_t)bl.size(), d_text.p, d_status.p, d_key.p);
				HIP_TRY(hipGetLastError());
				if (timed) { HIP_TRY(hipEventRecord(e1, nullptr)); HIP_TRY(hipEventSynchronize(e1)); HIP_TRY(hipEventElapsedTime(&ms, e0, e1)); }
			}
			HIP_TRY(hipDeviceSynchronize());
			if (timed) {
				fprintf(stderr, "[vargeno_hip] bgzf inflate kernel: %zu blocks, %.3f ms, %.2f GB/s text, %.2f GB/s compressed\n", bl.size(), ms, text_n / 1e6 / ms, comp_n / 1e6 / ms);
				(void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
			}
			HIP_TRY(hipMemcpy(&key, d_key.p, sizeof key, hipMemcpyDeviceToHost));
			uint64_t good_text = text_n;
			if (key != ~0ull) for (const vg_bgzf_block &b : bl) if (b.comp_off == key >> 4) good_text = b.text_off;
			if (good_text) HIP_TRY(hipMemcpy(text, d_text.p, good_text, hipMemcpyDeviceToHost));
			*text_len = good_text;
		}
		*consumed = comp_n;
		if (key != ~0ull) { *bad_block_offset = key >> 4; *consumed = key >> 4; (void)fail(VG_EIO, "%s", bz_describe(key).c_str()); }
		else if (hdr_rc) { *bad_block_offset = bad; (void)fail(VG_EIO, "BGZF block at compressed offset %s: not a BGZF block header", std::to_string(bad).c_str()); }
		return VG_OK;
	});
}

// ---- text -> BGZF without a handle (vg_deflate.h: the same compressor on host threads and on the device; the same bytes) ----------
static int bz_deflate_args(const uint8_t *text, uint64_t nbytes, uint32_t block, int codes, const uint8_t *bgzf, const uint64_t *bgzf_len)
{
	if ((!text && nbytes) || !bgzf || !bgzf_len) return fail(VG_EINVAL, "null argument");
	if (codes != VG_DEFLATE_FIXED && codes != VG_DEFLATE_DYNAMIC) return fail(VG_EINVAL, "codes is VG_DEFLATE_FIXED or VG_DEFLATE_DYNAMIC");
	if (block > VG_BGZF_TEXT_BLOCK) return fail(VG_EINVAL, "a BGZF block holds at most 65280 bytes of text here");
	return VG_OK;
}
// The blocks are made in `work`: the caller's buffer when it holds the worst case, else a buffer of our own -- so that a capacity
// that turns out too small leaves the caller's bytes alone.
struct BzDeflateOut {
	uint8_t *bgzf; uint64_t cap, bound;
	std::vector<uint8_t> own;
	uint8_t *work = nullptr;
	BzDeflateOut(uint8_t *bgzf_, uint64_t cap_, uint64_t bound_) : bgzf(bgzf_), cap(cap_), bound(bound_)
	{
		if (cap >= bound) work = bgzf;
		else { own.resize((size_t)bound); work = own.data(); }
	}
	int deliver(uint64_t len, int eof, uint64_t *bgzf_len)
	{
		if (eof) { memcpy(work + len, vg_bgzf_eof_marker(), VG_BGZF_EOF_BYTES); len += VG_BGZF_EOF_BYTES; }
		if (work != bgzf) {
			if (len > cap) return fail(VG_ETOOBIG, "the BGZF blocks do not fit the caller's buffer (vg_bgzf_deflate_bound says what always does)");
			memcpy(bgzf, work, (size_t)len);
		}
		*bgzf_len = len;
		return VG_OK;
	}
};

extern "C" uint64_t vg_bgzf_deflate_bound(uint64_t nbytes, uint32_t block)
{
	return block > VG_BGZF_TEXT_BLOCK ? 0 : vg_bgzf_bound(nbytes, block ? block : VG_BGZF_TEXT_BLOCK);
}

extern "C" int vg_bgzf_deflate_host_coded(const uint8_t *text, uint64_t nbytes, uint32_t block, int eof, int threads, int codes, uint8_t *bgzf, uint64_t cap, uint64_t *bgzf_len)
{
	const int rc = bz_deflate_args(text, nbytes, block, codes, bgzf, bgzf_len);
	if (rc) return rc;
	return guarded([&]() -> int {
		const uint32_t B = block ? block : VG_BGZF_TEXT_BLOCK;
		const uint64_t nb = vg_bgzf_blocks_of(nbytes, B), stride = (uint64_t)B + 5 + VG_BGZF_HEADER + VG_BGZF_TRAILER;
		BzDeflateOut out(bgzf, cap, vg_bgzf_bound(nbytes, B));
		std::vector<uint32_t> size((size_t)nb);
		// every block at its worst-case place (they are independent: any thread, any order), then moved down into a file
		std::atomic<uint64_t> next{0};
		std::atomic<bool> no_memory{false};
		auto work = [&] {
			try {
				const bool dyn = codes == VG_DEFLATE_DYNAMIC;
				std::unique_ptr<VgDefShared> sh(dyn ? nullptr : new VgDefShared);
				std::unique_ptr<VgDefDynShared> shd(dyn ? new VgDefDynShared : nullptr);
				std::vector<uint32_t> slot((B + VG_DEF_SLACK) / 4 + 1), tok(dyn ? B : 0);
				for (;;) {                                                // 16 blocks per step
					const uint64_t b0 = next.fetch_add(16);
					if (b0 >= nb) break;
					for (uint64_t b = b0; b < std::min(nb, b0 + 16); b++) {
						const uint32_t n = (uint32_t)std::min<uint64_t>(B, nbytes - b * B);
						size[(size_t)b] = dyn ? vg_bgzf_deflate_block_host_dyn(text + b * B, n, out.work + b * stride, *shd, slot.data(), tok.data())
						                      : vg_bgzf_deflate_block_host(text + b * B, n, out.work + b * stride, *sh, slot.data());
					}
				}
			} catch (const std::bad_alloc &) { no_memory = true; }
		};
		const int nt = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(1, std::min(threads, 256)), (nb + 15) / 16));
		if (nt == 1) work();
		else {
			std::vector<std::thread> th;
			for (int t = 0; t < nt; t++) th.emplace_back(work);
			for (auto &x : th) x.join();
		}
		if (no_memory) return fail(VG_ENOMEM, "host allocation failed");
		uint64_t len = 0;
		for (uint64_t b = 0; b < nb; b++) { if (b) memmove(out.work + len, out.work + b * stride, size[(size_t)b]); len += size[(size_t)b]; }
		return out.deliver(len, eof, bgzf_len);
	});
}

extern "C" int vg_bgzf_deflate_host(const uint8_t *text, uint64_t nbytes, uint32_t block, int eof, int threads, uint8_t *bgzf, uint64_t cap, uint64_t *bgzf_len)
{
	return vg_bgzf_deflate_host_coded(text, nbytes, block, eof, threads, VG_DEFLATE_FIXED, bgzf, cap, bgzf_len);
}

// One chunk of blocks, from text that is ALREADY on the device (the call below uploads it; the joint text stream renders it there):
// d_text[0, tn) in k blocks of B bytes (the last one shorter) -> their BGZF bytes at dst in host memory, *sum of them.  The work
// buffers hold k blocks: slots k * slot_words words, tok k * tok_words words (dynamic codes only), meta / offs and their host
// mirrors k entries, out out_cap bytes.  Default stream, synchronous.
struct BzDeflateDev {
	uint32_t *slots, *tok; uint2 *meta; uint64_t *offs; uint8_t *out;
	uint2 *h_meta; uint64_t *h_offs;
	uint32_t slot_words, tok_words;
	uint64_t out_cap;
	bool timed; hipEvent_t e0, e1, e2;
};
static int bz_deflate_chunk(const BzDeflateDev &w, const uint8_t *d_text, uint64_t tn, uint32_t B, uint32_t k, bool dyn, uint8_t *dst, uint64_t *sum_out, float *ms_deflate, float *ms_frame)
{
	if (w.timed) HIP_TRY(hipEventRecord(w.e0, nullptr));
	if (dyn) vg_bgzf_deflate_dyn_kernel<<<k, 64>>>(d_text, tn, B, k, w.slots, w.slot_words, w.tok, w.tok_words, w.meta);
	else vg_bgzf_deflate_kernel<<<k, 64>>>(d_text, tn, B, k, w.slots, w.slot_words, w.meta);
	HIP_TRY(hipGetLastError());
	if (w.timed) HIP_TRY(hipEventRecord(w.e1, nullptr));
	HIP_TRY(hipMemcpy(w.h_meta, w.meta, (size_t)k * sizeof(uint2), hipMemcpyDeviceToHost));
	uint64_t sum = 0;
	bool sane = true;
	for (uint32_t i = 0; i < k; i++) {
		const uint32_t n = (uint32_t)std::min<uint64_t>(B, tn - (uint64_t)i * B);
		sane = sane && w.h_meta[i].x < n;                                  // (the core stores a block that would not shrink)
		w.h_offs[i] = sum;
		sum += VG_BGZF_HEADER + (w.h_meta[i].x ? w.h_meta[i].x : n + 5u) + VG_BGZF_TRAILER;
	}
	if (!sane || sum > w.out_cap) return fail(VG_EIO, "the deflate kernel reported a block that is not shorter than its text");
	HIP_TRY(hipMemcpy(w.offs, w.h_offs, (size_t)k * sizeof(uint64_t), hipMemcpyHostToDevice));
	vg_bgzf_frame_kernel<<<k, 64>>>(d_text, tn, B, k, w.slots, w.slot_words, w.meta, w.offs, w.out);
	HIP_TRY(hipGetLastError());
	if (w.timed) {
		HIP_TRY(hipEventRecord(w.e2, nullptr)); HIP_TRY(hipEventSynchronize(w.e2));
		float a = 0, c = 0;
		HIP_TRY(hipEventElapsedTime(&a, w.e0, w.e1)); HIP_TRY(hipEventElapsedTime(&c, w.e1, w.e2));
		*ms_deflate += a; *ms_frame += c;
	}
	HIP_TRY(hipMemcpy(dst, w.out, sum, hipMemcpyDeviceToHost));
	*sum_out = sum;
	return VG_OK;
}

// the index's side of the fused call (the tabix section at the end of this file): the chunk text[0, tn) that is resident at d_text,
// and the blocks made from it
static int vi_fused_chunk(vg_vcfidx *idx, const uint8_t *d_text, const uint8_t *text, uint64_t tn);
static int vi_fused_blocks(vg_vcfidx *idx, const uint8_t *bgzf, uint64_t n);

extern "C" int vg_bgzf_deflate_device_indexed(int device, const uint8_t *text, uint64_t nbytes, uint32_t block, int eof, int codes, vg_vcfidx *idx, uint8_t *bgzf, uint64_t cap, uint64_t *bgzf_len)
{
	int rc = bz_deflate_args(text, nbytes, block, codes, bgzf, bgzf_len);
	if (rc) return rc;
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(VG_ENODEV, "no HIP device available (vg_bgzf_deflate_host is the host's compressor)");
	return guarded([&]() -> int {
		const uint32_t B = block ? block : VG_BGZF_TEXT_BLOCK;
		const uint64_t nb = vg_bgzf_blocks_of(nbytes, B);
		HIP_TRY(hipSetDevice(device));
		// chunks of at most 64 MiB of text and 65 536 blocks: the device buffers are sized by a chunk, not by the text
		const uint64_t chunk_blocks = std::min<uint64_t>(std::max<uint64_t>(1, nb), std::min<uint64_t>(65536, std::max<uint64_t>(1, (64ull << 20) / B)));
		const uint32_t slot_words = ((B + VG_DEF_SLACK + 15u) & ~15u) / 4;
		const uint64_t chunk_out = vg_bgzf_bound(chunk_blocks * B, B);
		const bool dyn = codes == VG_DEFLATE_DYNAMIC;
		const uint32_t tok_words = (B + 15u) & ~15u;                           // the dynamic mode's tokens: a word per text byte at most
		DevBuf<uint8_t> d_text, d_out; DevBuf<uint32_t> d_slots, d_tok; DevBuf<uint2> d_meta; DevBuf<uint64_t> d_offs;
		if (nb && ((rc = d_text.reserve(chunk_blocks * B + 16, "text")) || (rc = d_slots.reserve(chunk_blocks * slot_words, "deflate slots")) || (rc = d_meta.reserve(chunk_blocks, "block results"))
		           || (rc = d_offs.reserve(chunk_blocks, "block offsets")) || (rc = d_out.reserve(chunk_out, "BGZF bytes")) || (dyn && (rc = d_tok.reserve(chunk_blocks * tok_words, "deflate tokens"))))) return rc;
		BzDeflateOut out(bgzf, cap, vg_bgzf_bound(nbytes, B));
		std::vector<uint2> meta((size_t)chunk_blocks);
		std::vector<uint64_t> offs((size_t)chunk_blocks);
		const bool timed = getenv("VG_VERBOSE") != nullptr;
		hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;
		if (timed) { HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&e1)); HIP_TRY(hipEventCreate(&e2)); }
		float ms_deflate = 0, ms_frame = 0;
		uint64_t len = 0;
		const BzDeflateDev dev{d_slots.p, d_tok.p, d_meta.p, d_offs.p, d_out.p, meta.data(), offs.data(), slot_words, tok_words, chunk_out, timed, e0, e1, e2};
		for (uint64_t b0 = 0; b0 < nb; b0 += chunk_blocks) {                   // one chunk per step
			const uint32_t k = (uint32_t)std::min(chunk_blocks, nb - b0);
			const uint64_t t0 = b0 * B, tn = std::min<uint64_t>((uint64_t)k * B, nbytes - t0);
			HIP_TRY(hipMemcpy(d_text.p, text + t0, tn, hipMemcpyHostToDevice));
			if (idx && (rc = vi_fused_chunk(idx, d_text.p, text + t0, tn))) return rc;
			uint64_t sum = 0;
			if ((rc = bz_deflate_chunk(dev, d_text.p, tn, B, k, dyn, out.work + len, &sum, &ms_deflate, &ms_frame))) return rc;
			if (idx && (rc = vi_fused_blocks(idx, out.work + len, sum))) return rc;
			len += sum;
		}
		if (timed) {
			fprintf(stderr, "[vargeno_hip] bgzf deflate: %llu blocks, %s codes, %.3f ms deflate kernel (%.2f GB/s text), %.3f ms framing (incl. the lengths' round trip), ratio %.3f\n", (unsigned long long)nb,
			        dyn ? "dynamic" : "fixed", ms_deflate, ms_deflate > 0 ? nbytes / 1e6 / ms_deflate : 0.0, ms_frame, nbytes ? (double)len / (double)nbytes : 0.0);
			(void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipEventDestroy(e2);
		}
		return out.deliver(len, eof, bgzf_len);
	});
}

extern "C" int vg_bgzf_deflate_device_coded(int device, const uint8_t *text, uint64_t nbytes, uint32_t block, int eof, int codes, uint8_t *bgzf, uint64_t cap, uint64_t *bgzf_len)
{
	return vg_bgzf_deflate_device_indexed(device, text, nbytes, block, eof, codes, nullptr, bgzf, cap, bgzf_len);
}

extern "C" int vg_bgzf_deflate_device(int device, const uint8_t *text, uint64_t nbytes, uint32_t block, int eof, uint8_t *bgzf, uint64_t cap, uint64_t *bgzf_len)
{
	return vg_bgzf_deflate_device_coded(device, text, nbytes, block, eof, VG_DEFLATE_FIXED, bgzf, cap, bgzf_len);
}

// ---- the dynamic mode's code-length builder alone (vg_def_code_lengths on the host, and one wave per histogram) ----
static int def_lengths_args(const uint32_t *freq, uint32_t n_sets, uint32_t n_sym, uint32_t limit, const uint8_t *lens)
{
	if ((!freq || !lens) && n_sets) return fail(VG_EINVAL, "null argument");
	if (n_sym < 2 || n_sym > VG_DEF_LL_TAB || limit < 1 || limit > 15 || n_sym > (1u << limit)) return fail(VG_EINVAL, "code lengths: 2 to 288 symbols, a limit of 1 to 15, and no more symbols than 2^limit");
	for (uint64_t i = 0; i < (uint64_t)n_sets; i++) {
		uint64_t sum = 0;
		for (uint32_t s = 0; s < n_sym; s++) sum += freq[i * n_sym + s];
		if (sum >> 32) return fail(VG_EINVAL, "code lengths: the counts of a histogram sum to 2^32 or more");
	}
	return VG_OK;
}

extern "C" int vg_deflate_code_lengths_host(const uint32_t *freq, uint32_t n_sets, uint32_t n_sym, uint32_t limit, uint8_t *lens)
{
	const int rc = def_lengths_args(freq, n_sets, n_sym, limit, lens);
	if (rc) return rc;
	return guarded([&]() -> int {
		std::unique_ptr<VgDefLenScratch> sc(new VgDefLenScratch);
		DefHostIO io;
		for (uint64_t i = 0; i < (uint64_t)n_sets; i++) vg_def_code_lengths(io, freq + i * n_sym, n_sym, limit, lens + i * n_sym, *sc);
		return VG_OK;
	});
}

extern "C" int vg_deflate_code_lengths_device(int device, const uint32_t *freq, uint32_t n_sets, uint32_t n_sym, uint32_t limit, uint8_t *lens)
{
	int rc = def_lengths_args(freq, n_sets, n_sym, limit, lens);
	if (rc) return rc;
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(VG_ENODEV, "no HIP device available (vg_deflate_code_lengths_host is the host's builder)");
	return guarded([&]() -> int {
		if (!n_sets) return VG_OK;
		HIP_TRY(hipSetDevice(device));
		const uint64_t cells = (uint64_t)n_sets * n_sym;
		DevBuf<uint32_t> d_freq; DevBuf<uint8_t> d_lens;
		if ((rc = d_freq.reserve(cells, "histograms")) || (rc = d_lens.reserve(cells, "code lengths"))) return rc;
		HIP_TRY(hipMemcpy(d_freq.p, freq, cells * sizeof(uint32_t), hipMemcpyHostToDevice));
		vg_def_code_lengths_kernel<<<n_sets, 64>>>(d_freq.p, n_sets, n_sym, limit, d_lens.p);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpy(lens, d_lens.p, cells, hipMemcpyDeviceToHost));
		return VG_OK;
	});
}

// ---- plain gzip without a handle (vg_gunzip.h: the reference decoder, the chunked stages on the host, and on the device) ----------
// the sizes of a call: the caller's, and for every field it left 0 (or with no opts at all) the environment's
static VgGzOpts gz_env_opts(uint64_t nbytes, const vg_gzip_opts *o = nullptr)
{
	auto num = [](uint64_t given, const char *name) -> uint64_t { if (given) return given; const char *e = getenv(name); return e && *e ? strtoull(e, nullptr, 10) : 0; };
	return vg_gz_opts_checked(VgGzOpts{num(o ? o->chunk_bytes : 0, "VG_GZ_CHUNK"), num(o ? o->slot_bytes : 0, "VG_GZ_SLOT"), num(o ? o->max_ratio : 0, "VG_GZ_MAX_RATIO"), num(o ? o->slot_max : 0, "VG_GZ_SLOT_MAX")}, nbytes);
}
static int gz_buffer_args(const uint8_t *gz, uint64_t nbytes, uint8_t *text, uint64_t *text_len, uint64_t *consumed, uint64_t *bad_offset)
{
	if ((!gz && nbytes) || !text_len || !consumed || !bad_offset || !text) return fail(VG_EINVAL, "null argument");
	*text_len = 0; *consumed = 0; *bad_offset = UINT64_MAX;
	return VG_OK;
}
// the result of a decoder as the C-ABI gives it: bad data is VG_EIO with the compressed offset and the VG_INF_* text
static int gz_finish(const VgGzResult &r, uint64_t *text_len, uint64_t *consumed, uint64_t *bad_offset, vg_gzip_stats *stats)
{
	static_assert(sizeof(vg_gzip_stats) == sizeof(VgGzStats), "vg_gzip_stats mirrors VgGzStats");
	*text_len = r.text_len; *consumed = r.consumed; *bad_offset = r.bad_offset;
	if (stats) memcpy(stats, &r.st, sizeof r.st);
	if (r.rc == VG_GZ_ECAP) return fail(VG_ETOOBIG, "the text of the gzip members does not fit the caller's buffer");
	if (r.rc) return fail(VG_EIO, "gzip stream at compressed offset %s: %s", std::to_string(r.bad_offset).c_str(), vg_gunzip_strerror(r.rc));
	return VG_OK;
}

extern "C" int vg_gunzip_host(const uint8_t *gz, uint64_t nbytes, uint8_t *text, uint64_t text_cap, uint64_t *text_len, uint64_t *consumed, uint64_t *bad_offset)
{
	const int rc = gz_buffer_args(gz, nbytes, text, text_len, consumed, bad_offset);
	if (rc) return rc;
	return guarded([&]() -> int {
		VgGzResult r;
		vg_gunzip_sequential(gz, nbytes, text, text_cap, &r);
		return gz_finish(r, text_len, consumed, bad_offset, nullptr);
	});
}

extern "C" int vg_gunzip_chunked_host(const uint8_t *gz, uint64_t nbytes, uint8_t *text, uint64_t text_cap, uint64_t *text_len, uint64_t *consumed, uint64_t *bad_offset, vg_gzip_stats *stats, const vg_gzip_opts *opts)
{
	const int rc = gz_buffer_args(gz, nbytes, text, text_len, consumed, bad_offset);
	if (rc) return rc;
	return guarded([&]() -> int {
		const VgGzOpts op = gz_env_opts(nbytes, opts);
		VgGzHostStages be(gz, text, op);
		VgGzResult r;
		const int brc = vg_gunzip_chunked(be, gz, nbytes, text_cap, op, &r);
		if (brc) return brc;
		return gz_finish(r, text_len, consumed, bad_offset, stats);
	});
}

// the stages of a slot as kernels; the host reads back one record per slot and one CRC
struct GzDeviceStages {
	VgGzOpts op;
	DevBuf<uint8_t> d_comp, d_text, d_tmp;
	DevBuf<VgGzChunkRec> d_ck; DevBuf<uint16_t> d_stag; DevBuf<uint64_t> d_lens, d_offs; DevBuf<VgGzSlotRec> d_rec; DevBuf<uint32_t> d_cnt; DevBuf<unsigned long long> d_bad;
	GzSlotDev d{};
	size_t tmp_bytes = 0;
	hipStream_t s = nullptr;                                             // where the stages run (a stream of a handle; null: the default stream)
	static constexpr uint64_t TEXT_PAD = 64;

	int prepare(const uint8_t *gz, uint64_t nbytes, uint64_t text_cap)
	{
		int rc;
		if ((rc = d_comp.reserve(nbytes + 64, "gzip bytes")) || (rc = d_text.reserve(text_cap + TEXT_PAD, "inflated text")) || (rc = d_rec.reserve(1, "gzip slot record"))
		    || (rc = d_cnt.reserve(4, "gzip counters")) || (rc = d_bad.reserve(1, "gzip verdict"))) return rc;
		HIP_TRY(hipMemcpy(d_comp.p, gz, nbytes, hipMemcpyHostToDevice));
		d.rec = d_rec.p; d.counters = d_cnt.p;
		d.chunk_bytes = (uint32_t)op.chunk_bytes; d.area = op.chunk_bytes * op.max_ratio;
		return slot_buffers((op.slot_bytes + op.chunk_bytes - 1) / op.chunk_bytes);
	}
	// the buffers that follow a slot's chunk count (grow-only: a slot is longer than slot_bytes only when a block did not fit it)
	int slot_buffers(uint64_t n_chunks)
	{
		int rc;
		tmp_bytes = std::max(tmp_bytes, vg_dev_scan_temp_bytes(1, n_chunks + 1));
		if ((rc = d_tmp.reserve(tmp_bytes, "scan scratch")) || (rc = d_ck.reserve(n_chunks, "gzip chunk records")) || (rc = d_stag.reserve(n_chunks * d.area, "gzip symbol staging"))
		    || (rc = d_lens.reserve(n_chunks + 1, "gzip chunk lengths")) || (rc = d_offs.reserve(n_chunks + 1, "gzip chunk offsets"))) return rc;
		d.ck = d_ck.p; d.stag = d_stag.p; d.lens = d_lens.p; d.offs = d_offs.p;
		return VG_OK;
	}
	int chain(uint64_t in_off, uint64_t in_len, uint32_t entry_bit, VgGzSlotRec *rec, uint64_t *text_len)
	{
		d.in = d_comp.p + in_off; d.in_len = (uint32_t)in_len; d.entry_bit = entry_bit;
		d.n_chunks = (uint32_t)((in_len + op.chunk_bytes - 1) / op.chunk_bytes);
		const int brc = slot_buffers(d.n_chunks);
		if (brc) return brc;
		HIP_TRY(hipMemsetAsync(d_cnt.p, 0, 4 * sizeof(uint32_t), s));
		vg_gz_find<<<d.n_chunks, 64, 0, s>>>(d);
		vg_gz_decode<<<d.n_chunks, 64, 0, s>>>(d);
		vg_gz_confirm<<<(d.n_chunks + 255) / 256, 256, 0, s>>>(d);
		vg_gz_repair<<<1, 64, 0, s>>>(d);
		HIP_TRY(hipGetLastError());
		const int se = vg_dev_exclusive_scan_u64(d.lens, d.offs, d.n_chunks + 1, s, d_tmp.p, tmp_bytes);
		if (se) return fail(VG_ENODEV, "scan of the gzip chunk lengths: %s", hipGetErrorString((hipError_t)se));
		HIP_TRY(hipMemcpyAsync(rec, d_rec.p, sizeof *rec, hipMemcpyDeviceToHost, s));
		HIP_TRY(hipMemcpyAsync(text_len, d.offs + d.n_chunks, sizeof *text_len, hipMemcpyDeviceToHost, s));
		HIP_TRY(hipStreamSynchronize(s));
		return VG_OK;
	}
	int resolve(uint64_t text_off, uint64_t before, uint64_t text_len, uint32_t *crc, uint64_t *bad_bit) { return resolve_at(d_text.p + text_off, before, text_len, crc, bad_bit); }
	// the slot's symbols -> tx[0, text_len); `before` bytes of the member's text lie in front of tx
	int resolve_at(uint8_t *tx, uint64_t before, uint64_t text_len, uint32_t *crc, uint64_t *bad_bit)
	{
		*crc = 0;
		if (text_len == 0) return VG_OK;
		HIP_TRY(hipMemsetAsync(d_bad.p, 0xff, sizeof(unsigned long long), s));
		HIP_TRY(hipMemsetAsync(d_cnt.p + 2, 0, sizeof(uint32_t), s));
		vg_gz_windows<<<1, GZ_WIN_T, 0, s>>>(d, tx, (uint32_t)before, d_bad.p);
		vg_gz_resolve<<<(unsigned)((text_len + GZ_RES_T * GZ_RES_PER - 1) / (GZ_RES_T * GZ_RES_PER)), GZ_RES_T, 0, s>>>(d, tx, (uint32_t)text_len, (uint32_t)before, d_bad.p);
		vg_gz_crc<<<(unsigned)((text_len + GZ_CRC_TILE - 1) / GZ_CRC_TILE), 256, 0, s>>>(tx, (uint32_t)text_len, d_cnt.p + 2);
		HIP_TRY(hipGetLastError());
		unsigned long long bad = ~0ull;
		HIP_TRY(hipMemcpyAsync(&bad, d_bad.p, sizeof bad, hipMemcpyDeviceToHost, s));
		HIP_TRY(hipMemcpyAsync(crc, d_cnt.p + 2, sizeof *crc, hipMemcpyDeviceToHost, s));
		HIP_TRY(hipStreamSynchronize(s));
		*bad_bit = bad;
		return VG_OK;
	}
};

extern "C" int vg_gunzip_device(int device, const uint8_t *gz, uint64_t nbytes, uint8_t *text, uint64_t text_cap, uint64_t *text_len, uint64_t *consumed, uint64_t *bad_offset, vg_gzip_stats *stats, const vg_gzip_opts *opts)
{
	int rc = gz_buffer_args(gz, nbytes, text, text_len, consumed, bad_offset);
	if (rc) return rc;
	return guarded([&]() -> int {
		VgGzResult r;
		if (nbytes) {
			HIP_TRY(hipSetDevice(device));
			GzDeviceStages be;
			be.op = gz_env_opts(nbytes, opts);
			if ((rc = be.prepare(gz, nbytes, text_cap))) return rc;
			const auto t0 = std::chrono::steady_clock::now();
			if ((rc = vg_gunzip_chunked(be, gz, nbytes, text_cap, be.op, &r))) return rc;
			HIP_TRY(hipDeviceSynchronize());
			if (getenv("VG_VERBOSE")) {                                 // the stages of all slots, without the copies of the whole file in and out
				const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
				fprintf(stderr, "[vargeno_hip] gzip inflate: chunk %lu slot %lu ratio %lu: %lu chunks, %lu guessed, %lu repaired, %.3f ms, %.2f GB/s text, %.2f GB/s compressed\n", (unsigned long)be.op.chunk_bytes,
				        (unsigned long)be.op.slot_bytes, (unsigned long)be.op.max_ratio, (unsigned long)r.st.chunks, (unsigned long)r.st.guessed, (unsigned long)r.st.repaired, ms, r.text_len / 1e6 / ms, r.consumed / 1e6 / ms);
			}
			if (r.text_len) HIP_TRY(hipMemcpy(text, be.d_text.p, r.text_len, hipMemcpyDeviceToHost));
		}
		return gz_finish(r, text_len, consumed, bad_offset, stats);
	});
}

// ---- plain gzip streams: compressed bytes cut anywhere cross the link slot by slot, the stages above write a slot's text, and the
// text route's framing takes it from there (fq_frame_and_launch, as it is).  VgGzPush (vg_gunzip.h) decides what a slot is and
// carries the incomplete tail block on the host; per slot the host reads back one record (text length, exit, verdict, counts) and
// one CRC.  The text of a slot is resolved into d_text behind a copy of the window -- the last 32 KiB of the member's text so far,
// kept in d_win (32 KiB device to device in, 32 KiB out: the slot's own text buffer has the carry of the framing in front of it) --
// and copied device to device into the batch slot's fq_text.  Everything is enqueued on the ingest stream, in order.
struct GzipStream {
	vg_index *ix;
	GzDeviceStages g;
	DevBuf<uint8_t> d_win;
	VgGzPush<GzipStream> drv;
	GzipStream(vg_index *ix_, const VgGzOpts &op) : ix(ix_), drv(*this, op) { g.op = op; }
	int init()
	{
		int rc;
		if ((rc = g.d_rec.reserve(1, "gzip slot record")) || (rc = g.d_cnt.reserve(4, "gzip counters")) || (rc = g.d_bad.reserve(1, "gzip verdict")) || (rc = d_win.reserve(VG_GZ_WINDOW, "gzip window"))) return rc;
		g.s = ix->ingest_or_main();
		g.d.rec = g.d_rec.p; g.d.counters = g.d_cnt.p;
		g.d.chunk_bytes = (uint32_t)g.op.chunk_bytes; g.d.area = g.op.chunk_bytes * g.op.max_ratio;
		return VG_OK;
	}
	int chain_at(const uint8_t *in, uint64_t in_len, uint32_t entry_bit, VgGzSlotRec *rec, uint64_t *text_len)
	{
		int rc;
		if ((rc = g.d_comp.reserve(in_len + 64, "gzip bytes"))) return rc;
		HIP_TRY(hipMemcpyAsync(g.d_comp.p, in, in_len, hipMemcpyHostToDevice, g.s));
		return g.chain(0, in_len, entry_bit, rec, text_len);
	}
	int resolve_next(uint64_t before, uint64_t text_len, uint32_t *crc, uint64_t *bad_bit)
	{
		*crc = 0;
		if (text_len == 0) return VG_OK;
		if (text_len >= (1ull << 31)) return fail(VG_ETOOBIG, "a gzip slot's text of 2 GiB or more");
		int rc;
		if ((rc = g.d_text.reserve(VG_GZ_WINDOW + text_len + GzDeviceStages::TEXT_PAD, "inflated text"))) return rc;
		uint8_t *tx = g.d_text.p + VG_GZ_WINDOW;
		if (before) HIP_TRY(hipMemcpyAsync(tx - before, d_win.p + VG_GZ_WINDOW - before, before, hipMemcpyDeviceToDevice, g.s));
		if ((rc = g.resolve_at(tx, before, text_len, crc, bad_bit)) || *bad_bit != VG_GZ_NONE) return rc;
		const uint64_t keep = std::min<uint64_t>(VG_GZ_WINDOW, before + text_len);   // the window of the next slot
		HIP_TRY(hipMemcpyAsync(d_win.p + VG_GZ_WINDOW - keep, tx + text_len - keep, keep, hipMemcpyDeviceToDevice, g.s));
		const int slot_no = ix->next_slot;
		Slot *slp = nullptr;
		if ((rc = acquire_slot(ix, &slp, ix->fq_sample))) return rc;
		Slot &sl = *slp;
		if ((rc = fq_reserve(sl, text_len))) return rc;
		HIP_TRY(hipMemcpyAsync(sl.fq_text.p + FQ_CARRY, tx, text_len, hipMemcpyDeviceToDevice, g.s));
		return fq_frame_and_launch(ix, sl, slot_no, text_len, nullptr);
	}
	// (enqueued only: the driver runs the slot's chain next, whose read-back waits for the stream; dst is a checkpoint's own heap
	// block, which stays where it is, and nobody reads it before vg_fastq_stream_end has returned)
	int window(uint8_t *dst, uint64_t before)
	{
		HIP_TRY(hipMemcpyAsync(dst, d_win.p + VG_GZ_WINDOW - before, before, hipMemcpyDeviceToHost, g.s));
		return VG_OK;
	}
};
static void gzip_stream_free(GzipStream *gs) { delete gs; }

extern "C" int vg_fastq_stream_begin_gzip(vg_index *ix)
{
	if (!ix) return fail(VG_EINVAL, "null argument");
	return guarded([&]() -> int {
		int rc = vg_fastq_stream_begin(ix);
		if (rc) return rc;
		ix->fq_open = false;                                              // (until the gzip side stands)
		delete ix->gz; ix->gz = nullptr;
		ix->gz = new GzipStream(ix, gz_env_opts(UINT64_MAX));
		if ((rc = ix->gz->init())) return rc;
		ix->fq_open = true; ix->fq_gzip = true;
		return VG_OK;
	});
}
static int push_gzip(vg_index *ix, const uint8_t *data, uint64_t nbytes)
{
	HIP_TRY(hipSetDevice(ix->device));
	return ix->gz->drv.push(data, nbytes);                                 // (bad data or a refused slot stops the decoder: vg_fastq_stream_end says which)
}
static int end_gzip(vg_index *ix)
{
	HIP_TRY(hipSetDevice(ix->device));
	return ix->gz->drv.end();
}
static int gzip_verdict(vg_index *ix, int *refused)
{
	const VgGzResult &r = ix->gz->drv.r;
	if (r.rc) return fail(VG_EIO, "gzip stream at compressed offset %s: %s", std::to_string(r.bad_offset).c_str(), vg_gunzip_strerror(r.rc));
	if (refused && r.st.slots_refused) *refused = 1;
	return VG_OK;
}
extern "C" int vg_gzip_stream_stats(vg_index *ix, vg_gzip_stats *stats)
{
	if (!ix || !stats) return fail(VG_EINVAL, "null argument");
	if (!ix->gz) return fail(VG_EINVAL, "vg_gzip_stream_stats without vg_fastq_stream_begin_gzip");
	memcpy(stats, &ix->gz->drv.r.st, sizeof *stats);
	return VG_OK;
}
extern "C" int vg_fastq_stream_gzip_checkpoint(vg_index *ix, uint64_t text_offset, uint64_t *comp_bit_offset, uint64_t *ckpt_text_offset, uint8_t *window, uint32_t *window_len)
{
	if (!ix || !comp_bit_offset || !ckpt_text_offset || !window || !window_len) return fail(VG_EINVAL, "null argument");
	if (!ix->gz) return fail(VG_EINVAL, "vg_fastq_stream_gzip_checkpoint without vg_fastq_stream_begin_gzip");
	*comp_bit_offset = 0; *ckpt_text_offset = 0; *window_len = 0;          // no slot was entered: the file's first byte
	if (const VgGzCheckpoint *c = ix->gz->drv.checkpoint(text_offset)) {
		*comp_bit_offset = c->comp_bit; *ckpt_text_offset = c->text_off; *window_len = (uint32_t)c->window.size();
		if (!c->window.empty()) memcpy(window, c->window.data(), c->window.size());
	}
	return VG_OK;
}

// the push driver over the host stages, `push_bytes` at a time: what a gzip stream decides, with no device (the CPU suite)
extern "C" int vg_gunzip_pushed_host(const uint8_t *gz, uint64_t nbytes, uint64_t push_bytes, uint8_t *text, uint64_t text_cap, uint64_t *text_len, uint64_t *consumed, uint64_t *bad_offset, vg_gzip_stats *stats, const vg_gzip_opts *opts)
{
	const int rc = gz_buffer_args(gz, nbytes, text, text_len, consumed, bad_offset);
	if (rc) return rc;
	if (!push_bytes) return fail(VG_EINVAL, "pushes of no bytes");
	return guarded([&]() -> int {
		VgGzHostPushStages be(gz_env_opts(UINT64_MAX, opts));
		VgGzPush<VgGzHostPushStages> drv(be, be.st.op);
		for (uint64_t at = 0; at < nbytes; at += push_bytes) (void)drv.push(gz + at, std::min(push_bytes, nbytes - at));
		(void)drv.end();
		if (drv.r.text_len > text_cap) return fail(VG_ETOOBIG, "the text of the gzip members does not fit the caller's buffer");
		if (drv.r.text_len) memcpy(text, be.out.data(), drv.r.text_len);
		return gz_finish(drv.r, text_len, consumed, bad_offset, stats);
	});
}

// ---- BAM streams: BGZF pushes as above; the blocks inflate into the slot's bam_raw and the records are framed there (vg_bam_*)
extern "C" int vg_fastq_stream_begin_bam(vg_index *ix)
{
	const int rc = vg_fastq_stream_begin_bgzf(ix);
	if (rc == VG_OK) ix->bz.bam = true;
	return rc;
}

// What the framing of `nbytes` inflated bytes needs: capacities follow from the byte count alone -- a record takes at least 37 bytes
// (records <= bytes / 36; + one per window for a refused chunk's speculation), and l bases take at least 3/2 l bytes of their record
// (bases <= 2/3 of the bytes)
struct BamCaps {
	uint64_t span, n_win, cap_rec, cap_bases, tmp_bytes;
	explicit BamCaps(uint64_t nbytes)
	{
		span = (uint64_t)BAM_CARRY + nbytes;
		n_win = (span + VG_BAM_WINDOW - 1) / VG_BAM_WINDOW;
		cap_rec = span / 36 + n_win + 2;
		cap_bases = span / 3 * 2 + 64;
		tmp_bytes = vg_dev_scan_temp_bytes(n_win + 1, cap_rec + 1);
	}
};
struct BamFrame {                                    // the buffers of one framing, all on the device
	uint8_t *raw; FqStream *st; FqChunk *ck; BamSlotInfo *info; BamWin *win; uint32_t *woff, *cnt, *rec; uint64_t *offsets; uint8_t *bases; uint32_t *gate; void *tmp;
};

// The framing sequence behind vg_bam_prepare, enqueued on `is`
static int bam_frame_enqueue(hipStream_t is, int cus, const BamFrame &f, const BamCaps &c, int32_t n_ref, uint32_t entry0, uint64_t text_off)
{
	const unsigned nw = (unsigned)c.n_win;
	vg_bam_walk_windows<<<nw, 64, 0, is>>>(f.raw, f.ck, f.win, f.woff, n_ref, entry0);
	vg_bam_confirm<<<(nw + 255) / 256, 256, 0, is>>>(f.ck, f.win, f.info);
	vg_bam_repair<<<1, 64, 0, is>>>(f.raw, f.ck, f.win, f.woff, f.info);
	vg_bam_counts<<<(nw + 1 + 255) / 256, 256, 0, is>>>(f.ck, f.win, nw, f.cnt);
	HIP_TRY(hipGetLastError());
	int se = vg_dev_exclusive_scan_u32(f.cnt, f.cnt, c.n_win + 1, is, f.tmp, c.tmp_bytes);
	if (se != 0) return fail(VG_ENODEV, "device scan failed: %s", hipGetErrorString((hipError_t)se));
	const unsigned lg = (unsigned)std::min<uint64_t>(std::max<uint64_t>((c.n_win + 3) / 4, 64), (uint64_t)cus * 16);
	vg_bam_lengths<<<lg, 256, 0, is>>>(f.raw, f.ck, f.win, f.woff, f.cnt, nw, f.info, f.rec, f.offsets, (uint32_t)c.cap_rec);
	HIP_TRY(hipGetLastError());
	se = vg_dev_exclusive_scan_u64(f.offsets, f.offsets, c.cap_rec + 1, is, f.tmp, c.tmp_bytes);
	if (se != 0) return fail(VG_ENODEV, "device scan failed: %s", hipGetErrorString((hipError_t)se));
	vg_bam_finish<<<1, 1, 0, is>>>(f.st, f.ck, f.win, f.info, f.cnt, nw, f.rec, f.offsets, (uint32_t)c.cap_rec, (unsigned long long)text_off);
	vg_bam_gather<<<(unsigned)std::min<uint64_t>((c.cap_rec + 3) / 4, (uint64_t)cus * 32), 256, 0, is>>>(f.raw, f.rec, f.offsets, f.ck, f.bases, f.gate);
	HIP_TRY(hipGetLastError());
	return VG_OK;
}

static int bam_reserve(Slot &sl, uint64_t nbytes)
{
	int rc;
	const BamCaps c(nbytes);
	// (the slot after this one's last chunk copied the tail of its bytes on the ingest stream: see fq_reserve)
	if (sl.fq_tail_wanted) { HIP_TRY(hipEventSynchronize(sl.e_fq)); sl.fq_tail_wanted = false; }
	if ((rc = sl.bam_raw.reserve(c.span + 64, "BAM bytes"))) return rc;
	if ((rc = sl.bam_win.reserve(c.n_win + 1, "BAM windows"))) return rc;
	if ((rc = sl.bam_woff.reserve(c.n_win * VG_BAM_WIN_RECS, "BAM window records"))) return rc;
	if ((rc = sl.bam_cnt.reserve(c.n_win + 2, "BAM window counts"))) return rc;
	if ((rc = sl.bam_rec.reserve(c.cap_rec + 2, "BAM record offsets"))) return rc;
	if ((rc = sl.bam_info.reserve(1, "BAM slot sums"))) return rc;
	if ((rc = sl.fq_chunk.reserve(1, "FASTQ chunk"))) return rc;
	if ((rc = sl.st_offsets.reserve(c.cap_rec + 2, "read offsets"))) return rc;
	if ((rc = sl.st_bases.reserve(c.cap_bases, "base text"))) return rc;
	if ((rc = sl.st_gate.reserve(c.cap_rec + 2, "gate words"))) return rc;
	if ((rc = sl.fq_tmp.reserve(c.tmp_bytes, "scan scratch"))) return rc;
	return VG_OK;
}

// One slot of a BAM stream whose text_n bytes are being inflated into sl.bam_raw.p + BAM_CARRY (text_off: their offset in the
// inflated stream): carry, framing, and the read loop behind them exactly as fq_frame_and_launch starts it
static int bam_slot_frame(vg_index *ix, Slot &sl, int slot_no, uint64_t text_n, uint64_t text_off)
{
	BgzfStream &bz = ix->bz;
	hipStream_t is = ix->ingest_or_main();
	const BamCaps c(text_n);
	sl.bam_raw_len = text_n;
	const uint8_t *prev_end = nullptr;
	uint32_t entry0 = 0;
	if (ix->fq_prev_slot >= 0) { const Slot &pv = ix->slot[ix->fq_prev_slot]; prev_end = pv.bam_raw.p + BAM_CARRY + pv.bam_raw_len; }
	else entry0 = (uint32_t)(bz.bam_hdr_end > text_off ? bz.bam_hdr_end - text_off : 0);      // the first slot: its first block holds the header's end
	vg_bam_prepare<<<1, 256, 0, is>>>(ix->d_fq, sl.fq_chunk.p, sl.bam_info.p, prev_end, sl.bam_raw.p, (uint32_t)text_n, bz.d_key, (unsigned long long)(text_off + entry0));
	if (ix->fq_prev_slot >= 0) { Slot &pv = ix->slot[ix->fq_prev_slot]; HIP_TRY(hipEventRecord(pv.e_fq, is)); pv.fq_tail_wanted = true; }
	const BamFrame f{sl.bam_raw.p, ix->d_fq, sl.fq_chunk.p, sl.bam_info.p, sl.bam_win.p, sl.bam_woff.p, sl.bam_cnt.p, sl.bam_rec.p, sl.st_offsets.p, sl.st_bases.p, sl.st_gate.p, sl.fq_tmp.p};
	const int rc = bam_frame_enqueue(is, ix->cus, f, c, bz.bam_n_ref, entry0, text_off);
	if (rc) return rc;
	ix->fq_prev_slot = slot_no;
	return launch_batch(ix, sl, sl.st_bases.p, nullptr, sl.st_offsets.p, c.cap_rec, is, &sl.fq_chunk.p->n_reads, c.cap_bases, sl.st_gate.p);
}

extern "C" int vg_bam_stream_stats(vg_index *ix, uint64_t *kept, uint64_t *skipped_flag, uint64_t *skipped_empty, uint64_t *repairs)
{
	if (!ix) return fail(VG_EINVAL, "null argument");
	HIP_TRY(hipSetDevice(ix->device));
	HIP_TRY(hipStreamSynchronize(ix->ingest_or_main()));
	FqStream h;
	HIP_TRY(hipMemcpy(&h, ix->d_fq, sizeof h, hipMemcpyDeviceToHost));
	if (kept) *kept = h.records;
	if (skipped_flag) *skipped_flag = h.skipped_flag;
	if (skipped_empty) *skipped_empty = h.skipped_empty;
	if (repairs) *repairs = h.repairs;
	return VG_OK;
}

// ---- BAM without a handle: a whole file in host memory
// the whole blocks of a buffer inflated on the host, and the BAM header in front of them parsed.  VG_OK: *hdr_rc is vg_bam_header's
// verdict on what was inflated; a bad block ends the text early (*bad_block: its compressed offset, UINT64_MAX: none)
static int bam_inflate_host(const uint8_t *bgzf, uint64_t nbytes, std::vector<vg_bgzf_block> &bl, std::vector<uint8_t> &raw, uint64_t *bad_block, std::string &why)
{
	uint64_t tail = 0, bad = UINT64_MAX;
	*bad_block = UINT64_MAX;
	const int scan_rc = vg_bgzf_scan(bgzf, nbytes, 0, 0, bl, &tail, &bad);
	raw.resize(bl.empty() ? 1 : (size_t)(bl.back().text_off + bl.back().isize) + 1);
	uint64_t n = 0;
	for (const vg_bgzf_block &b : bl) {
		const int brc = vg_inflate_block_host(bgzf + b.in_off, b.in_len, raw.data() + b.text_off, b.isize, b.crc);
		if (brc) { *bad_block = b.comp_off; why = bz_describe((unsigned long long)b.comp_off << 4 | (unsigned)brc); break; }
		n = b.text_off + b.isize;
	}
	raw.resize((size_t)n);
	if (*bad_block == UINT64_MAX && scan_rc) { *bad_block = bad; why = "BGZF block at compressed offset " + std::to_string(bad) + ": not a BGZF block header"; }
	else if (*bad_block == UINT64_MAX && tail) { *bad_block = nbytes - tail; why = "BGZF block at compressed offset " + std::to_string(nbytes - tail) + ": incomplete"; }
	return VG_OK;
}
static int bam_not_bam(const uint8_t *bgzf, uint64_t nbytes)
{
	if (nbytes >= 4 && !memcmp(bgzf, "CRAM", 4)) return fail(VG_EIO, "this is a CRAM file, not BAM: CRAM is not read here -- convert it, e.g. with samtools fastq through a FIFO");
	return fail(VG_EIO, "not a BAM file: the inflated bytes do not start with the magic BAM\\1 and a header");
}

extern "C" int vg_bam_to_fastq_host(const uint8_t *bgzf, uint64_t nbytes, uint8_t *text, uint64_t text_cap, uint64_t *text_len, uint64_t *n_records, uint64_t *bad_offset)
{
	if ((!bgzf && nbytes) || (!text && text_cap) || !text_len || !n_records || !bad_offset) return fail(VG_EINVAL, "null argument");
	if (nbytes >= (1ull << 32)) return fail(VG_EINVAL, "BAM buffer of 4 GiB or more");
	*text_len = 0; *n_records = 0; *bad_offset = UINT64_MAX;
	return guarded([&]() -> int {
		std::vector<vg_bgzf_block> bl;
		std::vector<uint8_t> raw;
		uint64_t bad_block = UINT64_MAX, hdr_end = 0, used = 0;
		std::string why, out;
		int32_t n_ref = 0;
		(void)bam_inflate_host(bgzf, nbytes, bl, raw, &bad_block, why);
		const int hrc = vg_bam_header(raw.data(), raw.size(), &hdr_end, &n_ref);
		if (hrc == VG_BAM_BAD || (raw.empty() && bl.empty())) return bam_not_bam(bgzf, nbytes);
		if (hrc == VG_BAM_MORE) {
			*bad_offset = raw.size();
			(void)fail(VG_EIO, "the BAM stream ends inside its header, at inflated offset %s%s", std::to_string(raw.size()).c_str(), why.empty() ? "" : (" (" + why + ")").c_str());
			return VG_OK;
		}
		VgBamCounts n;
		const int crc = vg_bam_convert(raw.data(), raw.size(), hdr_end, out, &used, n);
		if (out.size() > text_cap) return fail(VG_ETOOBIG, "the FASTQ text of the BAM records does not fit the caller's buffer");
		if (!out.empty()) memcpy(text, out.data(), out.size());
		*text_len = out.size(); *n_records = n.kept;
		if (crc == VG_BAM_BAD) { *bad_offset = used; (void)fail(VG_EIO, "BAM record at inflated offset %s: its block_size is smaller than its own fields announce", std::to_string(used).c_str()); }
		else if (used < raw.size() || bad_block != UINT64_MAX) {
			*bad_offset = used;
			(void)fail(VG_EIO, "the BAM stream ends inside a record, at inflated offset %s%s", std::to_string(used).c_str(), why.empty() ? "" : (" (" + why + ")").c_str());
		}
		return VG_OK;
	});
}

extern "C" int vg_bam_frame_device(int device, const uint8_t *bgzf, uint64_t nbytes, uint64_t *offsets, uint64_t cap_rec, uint8_t *bases, uint64_t cap_bases, uint32_t *gate,
                                   uint64_t *n_records, uint64_t stats[4], uint64_t *bad_offset)
{
	if ((!bgzf && nbytes) || !offsets || (!bases && cap_bases) || (!gate && cap_rec) || !n_records || !stats || !bad_offset) return fail(VG_EINVAL, "null argument");
	if (nbytes >= (1ull << 31)) return fail(VG_EINVAL, "BAM buffer of 2 GiB or more");
	*n_records = 0; *bad_offset = UINT64_MAX; offsets[0] = 0;
	for (int i = 0; i < 4; i++) stats[i] = 0;
	return guarded([&]() -> int {
		// the header on the host, as the stream does it: the leading blocks only
		std::vector<vg_bgzf_block> bl;
		uint64_t tail = 0, bad = UINT64_MAX, hdr_end = 0;
		const int scan_rc = vg_bgzf_scan(bgzf, nbytes, 0, 0, bl, &tail, &bad);
		std::vector<uint8_t> hdr;
		int32_t n_ref = 0;
		int hrc = VG_BAM_MORE;
		size_t first = bl.size();
		for (size_t i = 0; i < bl.size() && hrc == VG_BAM_MORE; i++) {
			const vg_bgzf_block &b = bl[i];
			const size_t o = hdr.size();
			hdr.resize(o + b.isize + 1);
			const int brc = vg_inflate_block_host(bgzf + b.in_off, b.in_len, hdr.data() + o, b.isize, b.crc);
			hdr.resize(o + b.isize);
			if (brc) { *bad_offset = o; return fail(VG_EIO, "%s", bz_describe((unsigned long long)b.comp_off << 4 | (unsigned)brc).c_str()); }
			hrc = vg_bam_header(hdr.data(), hdr.size(), &hdr_end, &n_ref);
			if (hrc == VG_BAM_OK) first = hdr_end < b.text_off + b.isize ? i : i + 1;
		}
		if (hrc == VG_BAM_BAD || bl.empty()) return bam_not_bam(bgzf, nbytes);
		if (hrc == VG_BAM_MORE) { *bad_offset = hdr.size(); (void)fail(VG_EIO, "the BAM stream ends inside its header, at inflated offset %s", std::to_string(hdr.size()).c_str()); return VG_OK; }
		const uint64_t text_end = bl.back().text_off + bl.back().isize;
		if (first == bl.size() || text_end == bl[first].text_off) {           // a header and no records
			if (scan_rc || tail) { *bad_offset = hdr_end; (void)fail(VG_EIO, "BGZF block at compressed offset %s: incomplete or not a BGZF block", std::to_string(scan_rc ? bad : nbytes - tail).c_str()); }
			return VG_OK;
		}
		const uint64_t text_off = bl[first].text_off, text_n = text_end - text_off;
		const uint64_t c0 = bl[first].comp_off, comp_n = (uint64_t)bl.back().in_off + bl.back().in_len + 8 - c0;
		std::vector<vg_bgzf_block> tab(bl.begin() + (long)first, bl.end());
		for (vg_bgzf_block &b : tab) { b.in_off -= (uint32_t)c0; b.text_off -= text_off; }
		const BamCaps c(text_n);
		HIP_TRY(hipSetDevice(device));
		hipDeviceProp_t prop;
		HIP_TRY(hipGetDeviceProperties(&prop, device));
		int rc;
		DevBuf<uint8_t> d_comp, d_raw, d_bases, d_tmp; DevBuf<vg_bgzf_block> d_tab; DevBuf<uint32_t> d_status, d_woff, d_cnt, d_rec, d_gate; DevBuf<unsigned long long> d_key;
		DevBuf<FqStream> d_st; DevBuf<FqChunk> d_ck; DevBuf<BamSlotInfo> d_info; DevBuf<BamWin> d_win; DevBuf<uint64_t> d_off;
		if ((rc = d_comp.reserve(comp_n + 64, "BGZF bytes")) || (rc = d_raw.reserve(c.span + 64, "BAM bytes")) || (rc = d_tab.reserve(tab.size(), "BGZF block table"))
		    || (rc = d_status.reserve(tab.size(), "BGZF block results")) || (rc = d_key.reserve(1, "BGZF verdict")) || (rc = d_st.reserve(1, "stream state")) || (rc = d_ck.reserve(1, "chunk"))
		    || (rc = d_info.reserve(1, "BAM slot sums")) || (rc = d_win.reserve(c.n_win + 1, "BAM windows")) || (rc = d_woff.reserve(c.n_win * VG_BAM_WIN_RECS, "BAM window records"))
		    || (rc = d_cnt.reserve(c.n_win + 2, "BAM window counts")) || (rc = d_rec.reserve(c.cap_rec + 2, "BAM record offsets")) || (rc = d_off.reserve(c.cap_rec + 2, "read offsets"))
		    || (rc = d_bases.reserve(c.cap_bases, "base text")) || (rc = d_gate.reserve(c.cap_rec + 2, "gate words")) || (rc = d_tmp.reserve(c.tmp_bytes, "scan scratch"))) return rc;
		HIP_TRY(hipMemcpy(d_comp.p, bgzf + c0, comp_n, hipMemcpyHostToDevice));
		HIP_TRY(hipMemcpy(d_tab.p, tab.data(), tab.size() * sizeof(vg_bgzf_block), hipMemcpyHostToDevice));
		HIP_TRY(hipMemset(d_key.p, 0xff, sizeof(unsigned long long)));
		HIP_TRY(hipMemset(d_st.p, 0, sizeof(FqStream)));
		const bool timed = getenv("VG_VERBOSE") != nullptr;
		hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
		if (timed) for (hipEvent_t &e : ev) HIP_TRY(hipEventCreate(&e));
		if (timed) HIP_TRY(hipEventRecord(ev[0], nullptr));
		vg_bgzf_inflate_kernel<<<(unsigned)tab.size(), 64>>>(d_comp.p, d_tab.p, (uint32_t)tab.size(), d_raw.p + BAM_CARRY, d_status.p, d_key.p);
		if (timed) HIP_TRY(hipEventRecord(ev[1], nullptr));
		const uint32_t entry0 = (uint32_t)(hdr_end > text_off ? hdr_end - text_off : 0);
		vg_bam_prepare<<<1, 256>>>(d_st.p, d_ck.p, d_info.p, nullptr, d_raw.p, (uint32_t)text_n, d_key.p, (unsigned long long)(text_off + entry0));
		HIP_TRY(hipGetLastError());
		const BamFrame f{d_raw.p, d_st.p, d_ck.p, d_info.p, d_win.p, d_woff.p, d_cnt.p, d_rec.p, d_off.p, d_bases.p, d_gate.p, d_tmp.p};
		if ((rc = bam_frame_enqueue(nullptr, prop.multiProcessorCount, f, c, n_ref, entry0, text_off))) return rc;
		if (timed) HIP_TRY(hipEventRecord(ev[2], nullptr));
		HIP_TRY(hipDeviceSynchronize());
		if (timed) {
			float ms_inf = 0, ms_frame = 0;
			HIP_TRY(hipEventElapsedTime(&ms_inf, ev[0], ev[1])); HIP_TRY(hipEventElapsedTime(&ms_frame, ev[1], ev[2]));
			fprintf(stderr, "[vargeno_hip] bam frame: %zu blocks, %llu inflated bytes, %llu windows: inflate %.3f ms, framing + gather %.3f ms\n", tab.size(), (unsigned long long)text_n, (unsigned long long)c.n_win, ms_inf, ms_frame);
			for (hipEvent_t &e : ev) (void)hipEventDestroy(e);
		}
		FqStream st; FqChunk ck; unsigned long long key = ~0ull;
		HIP_TRY(hipMemcpy(&st, d_st.p, sizeof st, hipMemcpyDeviceToHost));
		HIP_TRY(hipMemcpy(&ck, d_ck.p, sizeof ck, hipMemcpyDeviceToHost));
		HIP_TRY(hipMemcpy(&key, d_key.p, sizeof key, hipMemcpyDeviceToHost));
		stats[0] = st.records; stats[1] = st.skipped_flag; stats[2] = st.skipped_empty; stats[3] = st.repairs;
		if (ck.n_reads > cap_rec || ck.total > cap_bases) return fail(VG_ETOOBIG, "the BAM file's reads do not fit the caller's arrays");
		if (ck.n_reads) {
			HIP_TRY(hipMemcpy(offsets, d_off.p, ((size_t)ck.n_reads + 1) * 8, hipMemcpyDeviceToHost));
			HIP_TRY(hipMemcpy(gate, d_gate.p, (size_t)ck.n_reads * 4, hipMemcpyDeviceToHost));
			if (ck.total) HIP_TRY(hipMemcpy(bases, d_bases.p, ck.total, hipMemcpyDeviceToHost));
		}
		*n_records = ck.n_reads;
		if (key != ~0ull) { *bad_offset = st.consumed; (void)fail(VG_EIO, "%s", bz_describe(key).c_str()); }
		else if (st.poisoned) { *bad_offset = st.consumed; (void)fail(VG_EBADREAD, "the BAM records could not be framed on the device (a block_size out of range, a read of more than 1022 bases, or more than 64 repairs): frame from inflated offset %s on the host", std::to_string(st.consumed).c_str()); }
		else if (st.carry || scan_rc || tail) { *bad_offset = st.consumed; (void)fail(VG_EIO, "the BAM stream ends inside a record, at inflated offset %s", std::to_string(st.consumed).c_str()); }
		return VG_OK;
	});
}

static int fq_collect(vg_index *ix, bool drain, uint64_t *n_records, uint64_t *consumed, uint64_t *last_record_start, int *refused, FqStream *state = nullptr)
{
	HIP_TRY(hipSetDevice(ix->device));
	if (drain) { int rc = finish_pending(ix); if (rc) return rc; }
	else HIP_TRY(hipStreamSynchronize(ix->ingest_or_main()));       // framing only: the read loop runs on
	FqStream h;
	HIP_TRY(hipMemcpy(&h, ix->d_fq, sizeof h, hipMemcpyDeviceToHost));
	if (n_records) *n_records = h.records;
	if (consumed) *consumed = h.consumed;
	if (last_record_start) *last_record_start = h.last_record;
	if (refused) *refused = h.poisoned ? 1 : 0;
	if (state) *state = h;
	return VG_OK;
}

static int gzip_verdict(vg_index *ix, int *refused);
extern "C" int vg_fastq_stream_end(vg_index *ix, uint64_t *n_records, uint64_t *consumed, uint64_t *last_record_start, int *refused)
{
	if (!ix) return fail(VG_EINVAL, "null argument");
	if (!ix->fq_open) return fail(VG_EINVAL, "vg_fastq_stream_end without vg_fastq_stream_begin");
	ix->fq_open = false;
	if (ix->fq_packed) {
		ix->fq_packed = false;
		int rc = finish_pending(ix);
		if (rc) return rc;
		if (n_records) *n_records = ix->packer->records();
		if (consumed) *consumed = ix->packer->consumed();
		if (last_record_start) *last_record_start = ix->packer->last_record_start();
		if (refused) *refused = ix->packer->poisoned() ? 1 : 0;
		return VG_OK;
	}
	const bool gzip = ix->fq_gzip;
	ix->fq_gzip = false;
	if (gzip) {                                                          // what waits in the carry is decoded and framed first
		const int grc = guarded([&] { return end_gzip(ix); });
		if (grc) return grc;
	}
	FqStream h;
	int rc = fq_collect(ix, true, n_records, consumed, last_record_start, refused, &h);
	if (rc == VG_OK && gzip) return gzip_verdict(ix, refused);
	if (rc || !ix->fq_bgzf) return rc;
	ix->fq_bgzf = false;
	return guarded([&]() -> int {
		BgzfStream &bz = ix->bz;
		unsigned long long key = ~0ull;
		HIP_TRY(hipMemcpy(&key, bz.d_key, sizeof key, hipMemcpyDeviceToHost));
		key = std::min(key, bz.host_key);
		if (key != ~0ull) return fail(VG_EIO, "%s", bz_describe(key).c_str());
		if (bz.bam && !bz.header_bad) {
			// a BAM stream must end at a record boundary: say where it ends instead (and what the BGZF layer has to add)
			const std::string tail = bz.carry.empty() ? std::string() : " (BGZF block at compressed offset " + std::to_string(bz.comp_pos) + ": incomplete)";
			if (bz.bam_hdr_done && ix->fq_prev_slot < 0 && consumed) *consumed = bz.bam_hdr_end;   // (no slot was framed: nothing behind the header)
			if (!bz.bam_hdr_done) {
				if (consumed) *consumed = bz.text_pos;
				return fail(VG_EIO, "the BAM stream ends inside its header, at inflated offset %s%s", std::to_string(bz.text_pos).c_str(), tail.c_str());
			}
			if (!h.poisoned && (h.carry || !bz.carry.empty())) return fail(VG_EIO, "the BAM stream ends inside a record, at inflated offset %s%s", std::to_string(h.consumed).c_str(), tail.c_str());
		}
		if (bz.header_bad) return fail(VG_EIO, "BGZF block at compressed offset %s: not a BGZF block header", std::to_string(bz.comp_pos).c_str());
		if (!bz.carry.empty()) return fail(VG_EIO, "BGZF block at compressed offset %s: incomplete (the stream ends %s bytes into it)", std::to_string(bz.comp_pos).c_str(), std::to_string(bz.carry.size()).c_str());
		return VG_OK;
	});
}

// One self-contained chunk (a stream of one push): the older, synchronous form of the above -- the caller learns what was
// framed before it sends the next chunk (and resubmits the unconsumed tail itself).  Waits for the framing, not for the read loop.
extern "C" int vg_fastq_submit(vg_index *ix, const uint8_t *text, uint64_t nbytes, uint64_t *n_records, uint64_t *consumed, uint64_t *last_record_start)
{
	if (!ix || (!text && nbytes) || !n_records || !consumed) return fail(VG_EINVAL, "null argument");
	*n_records = 0; *consumed = 0;
	if (last_record_start) *last_record_start = 0;
	if (nbytes == 0) return VG_OK;
	if (ix->fq_open) return fail(VG_EINVAL, "vg_fastq_submit inside an open FASTQ stream");
	int rc = vg_fastq_stream_begin(ix);
	if (rc) return rc;
	rc = vg_fastq_stream_push(ix, text, nbytes);
	ix->fq_open = false;
	if (rc) return rc;
	int refused = 0;
	rc = fq_collect(ix, false, n_records, consumed, last_record_start, &refused);
	if (rc) return rc;
	if (refused) {
		*n_records = 0; *consumed = 0;
		return fail(VG_EBADREAD, "a FASTQ line longer than 1023 characters (reference BUF_SIZE 1024, qv.cc:700), a quality line shorter than the read's chunk count, or lines of fewer than 8 bytes on average: frame this chunk on the host");
	}
	return VG_OK;
}

// ---- host-side framing + packing alone: no device is touched (a caller that packs on its own threads and hands the batches to
// vg_reads_submit_packed; the CPU test-suite checks the framing rules through these)
struct vg_packer { vgp::Packer p; explicit vg_packer(int t) : p(t) {} };
extern "C" int vg_packer_create(int host_threads, vg_packer **out)
{
	if (!out) return fail(VG_EINVAL, "null argument");
	*out = nullptr;
	return guarded([&]() -> int {
		int t = host_threads;
		if (t <= 0) { t = host_pack_threads_default(); if (t <= 0) t = 1; }
		if (t > 256) t = 256;
		*out = new vg_packer(t);
		(*out)->p.begin();
		return VG_OK;
	});
}
extern "C" void vg_packer_destroy(vg_packer *pk) { delete pk; }
extern "C" int vg_packer_begin(vg_packer *pk)
{
	if (!pk) return fail(VG_EINVAL, "null argument");
	pk->p.begin();
	return VG_OK;
}
extern "C" uint64_t vg_packer_reads_cap(uint64_t nbytes) { return vgp::Packer::reads_cap(nbytes) + 1; }
extern "C" uint64_t vg_packer_kmers_cap(uint64_t nbytes) { return vgp::Packer::kmers_cap(nbytes); }
extern "C" int vg_packer_push(vg_packer *pk, const uint8_t *text, uint64_t nbytes, uint64_t *kmers, uint64_t kmers_cap, uint64_t *meta, uint64_t *chunk_offsets, uint64_t reads_cap,
                              uint64_t *n_reads, uint64_t *n_chunks, uint64_t *n_invalid)
{
	if (!pk || (!text && nbytes) || !kmers || !meta || !chunk_offsets || !n_reads || !n_chunks) return fail(VG_EINVAL, "null argument");
	return guarded([&]() -> int {
		vgp::Staging st;
		st.kmers = kmers; st.kmers_cap = kmers_cap; st.meta = meta; st.offsets = chunk_offsets; st.reads_cap = reads_cap;
		const vgp::ChunkResult r = pk->p.push(text, nbytes, st);
		*n_reads = r.n_reads; *n_chunks = r.n_chunks;
		if (n_invalid) *n_invalid = r.n_invalid;
		for (uint64_t i = 0; i <= r.n_reads && r.n_reads; i++) chunk_offsets[i] >>= 5;       // the packer writes flat-batch offsets (32 x chunks)
		return VG_OK;
	});
}
extern "C" int vg_packer_end(vg_packer *pk, uint64_t *n_records, uint64_t *consumed, uint64_t *last_record_start, int *refused)
{
	if (!pk) return fail(VG_EINVAL, "null argument");
	if (n_records) *n_records = pk->p.records();
	if (consumed) *consumed = pk->p.consumed();
	if (last_record_start) *last_record_start = pk->p.last_record_start();
	if (refused) *refused = pk->p.poisoned() ? 1 : 0;
	return VG_OK;
}

extern "C" int vg_sync(vg_index *ix)
{
	if (!ix) return fail(VG_EINVAL, "null argument");
	return finish_pending(ix);
}

extern "C" int vg_set_stats(vg_index *ix, int enable)
{
	if (!ix) return fail(VG_EINVAL, "null argument");
	if (ix->stats_enabled != (enable != 0)) { int rc = finish_pending(ix); if (rc) return rc; }
	ix->stats_enabled = enable != 0;
	return VG_OK;
}

extern "C" int vg_stats_get(vg_index *ix, vg_stats *out)
{
	if (!ix || !out) return fail(VG_EINVAL, "null argument");
	int rc = vg_sync(ix);
	if (rc) return rc;
	unsigned long long h[S_COUNT];
	HIP_TRY(hipMemcpy(h, ix->d_stats, sizeof h, hipMemcpyDeviceToHost));
	memset(out, 0, sizeof *out);
	out->reads = h[S_READS]; out->reads_n = h[S_READS_N]; out->reads_invalid = h[S_READS_INVALID];
	out->passes = h[S_PASSES]; out->passes_ok = h[S_PASSES_OK]; out->chunks = h[S_CHUNKS]; out->gate_open = h[S_GATE_OPEN];
	out->refbf_pos = h[S_REFBF_POS]; out->snpbf_pos = h[S_SNPBF_POS]; out->large_block = h[S_LARGE_BLOCK];
	out->ref_query = h[S_REF_QUERY]; out->snp_query = h[S_SNP_QUERY]; out->ref_probe = h[S_REF_PROBE]; out->snp_probe = h[S_SNP_PROBE];
	out->scan_ref = h[S_SCAN_REF]; out->scan_snp = h[S_SCAN_SNP]; out->scan_oob = h[S_SCAN_OOB];
	out->aux_ref = h[S_AUX_REF]; out->aux_snp = h[S_AUX_SNP]; out->site_test = h[S_SITE_TEST]; out->ctx = h[S_CTX];
	out->walks = h[S_WALKS]; out->incr = h[S_INCR]; out->ingest_bytes = h[S_INGEST];
	out->overflow_reads = ix->cum[0]; out->overflow_deep = ix->cum[1]; out->reads_invalid = ix->cum[3] + ix->host_invalid;
	const uint64_t scans = out->gate_open - out->large_block;
	out->alg_bytes = out->ingest_bytes + 8 * (out->ref_query + out->snp_query) + 9 * out->ref_probe + 11 * out->snp_probe
	               + 16 * out->gate_open + 16 * scans + 9 * out->scan_ref + 11 * out->scan_snp
	               + 40 * out->aux_ref + 50 * out->aux_snp + 4 * out->site_test + 128 * out->walks + 4 * out->incr;
	return VG_OK;
}

extern "C" int vg_timing_get(vg_index *ix, vg_timing *out)
{
	if (!ix || !out) return fail(VG_EINVAL, "null argument");
	memset(out, 0, sizeof *out);
	int rc = finish_pending(ix);
#ifdef VG_VIEW_COUNTERS
	{
		// the census since the last vg_timing_get (all launches of all tiers): loads and 128-byte lines asked for, per view
		static const char *names[VC_N] = {"other", "reads (k-mers, offsets, flag words)", "dx (direct table)", "mx (merged view)", "ref_jg", "ref entries", "snp_jg", "snp entries", "sec_jg", "sec3 (LO32-ordered view)",
		                                  "snp_sig", "ref_bf", "snp_bf", "aux rows, stage A", "aux rows, stage B (= any - A)", "-", "-", "srank (walk)", "cnt4 (atomics)", "aux rows, any stage", "pile (site bytes, stage B)"};
		unsigned long long ln[VC_N], ld[VC_N], zero[VC_N] = {0};
		if (hipMemcpyFromSymbol(ln, HIP_SYMBOL(vg_vc_lines), sizeof ln) == hipSuccess && hipMemcpyFromSymbol(ld, HIP_SYMBOL(vg_vc_loads), sizeof ld) == hipSuccess) {
			ln[VC_AUX_B] = ln[VC_AUX_ANY] - ln[VC_AUX_A]; ld[VC_AUX_B] = ld[VC_AUX_ANY] - ld[VC_AUX_A];
			unsigned long long tot = 0;
			for (int i = 0; i < VC_N; i++) if (i != VC_AUX_ANY) tot += ln[i];
			fprintf(stderr, "[view census] %llu batches; lines asked for (all lanes, before L1 / L2 merge anything): %llu\n", (unsigned long long)ix->t_batches, tot);
			for (int i = 0; i < VC_N; i++) if (ld[i] && i != VC_AUX_ANY) fprintf(stderr, "[view census]   %-38s loads %12llu  lines %12llu  (%.1f %%)\n", names[i], ld[i], ln[i], 100.0 * (double)ln[i] / (double)(tot ? tot : 1));
		}
		(void)hipMemcpyToSymbol(HIP_SYMBOL(vg_vc_lines), zero, sizeof zero);
		(void)hipMemcpyToSymbol(HIP_SYMBOL(vg_vc_loads), zero, sizeof zero);
	}
#endif
#ifdef VG_STAGE_CLOCKS
	{
		unsigned long long h[8];
		if (hipMemcpyFromSymbol(h, HIP_SYMBOL(vg_dbg_ovf), sizeof h) == hipSuccess)
			fprintf(stderr, "[dbg] list overflows (pass-level events) tier1: exact %llu neighbour %llu keys %llu | tier2: exact %llu neighbour %llu keys %llu\n", h[0], h[1], h[2], h[4], h[5], h[6]);
	}
#endif
	if (rc) return rc;
	if (!ix->t_batches) return fail(VG_EINVAL, "no batch has been processed since the last vg_timing_get");
	const double n = (double)ix->t_batches;
	out->ms_pack = (float)(ix->t_pack / n); out->ms_main = (float)(ix->t_main / n);
	out->ms_tail = (float)(ix->t_tail / n); out->ms_total = (float)(ix->t_total / n); out->ms_deep_lists = (float)(ix->t_w2 / n);
	out->batches = (uint32_t)ix->t_batches;
	ix->t_pack = ix->t_main = ix->t_tail = ix->t_total = ix->t_w2 = 0; ix->t_batches = 0;
	return VG_OK;
}

extern "C" int vg_sites_fetch(vg_index *ix, uint32_t *pos, uint8_t *ref_base, uint8_t *alt_base, uint8_t *ref_freq, uint8_t *alt_freq)
{
	if (!ix) return fail(VG_EINVAL, "null argument");
	const size_t n = ix->n_sites;
	if (pos) memcpy(pos, ix->site_pos.data(), n * 4);
	if (ref_base) memcpy(ref_base, ix->site_ref.data(), n);
	if (alt_base) memcpy(alt_base, ix->site_alt.data(), n);
	if (ref_freq) memcpy(ref_freq, ix->site_rf.data(), n);
	if (alt_freq) memcpy(alt_freq, ix->site_af.data(), n);
	return VG_OK;
}

// the exact sums of the selected sample (vg_sample_select): what fetch, device_ptr and the all-reduces act on
static uint32_t *sel_cnt(const vg_index *ix) { return ix->planes[ix->cur_sample].p.cnt; }

extern "C" int vg_counts_fetch(vg_index *ix, uint8_t *ref_cnt, uint8_t *alt_cnt)
{
	if (!ix || !ref_cnt || !alt_cnt) return fail(VG_EINVAL, "null argument");
	int rc = vg_sync(ix);
	if (rc) return rc;
	if (ix->n_sites == 0) return VG_OK;
	vg_clamp_counters<<<(unsigned)std::min<uint64_t>((ix->n_sites + 255) / 256, 4096), 256, 0, ix->stream>>>(sel_cnt(ix), ix->n_sites, ix->d_clamped, ix->d_clamped + ix->n_sites);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(ref_cnt, ix->d_clamped, ix->n_sites, hipMemcpyDeviceToHost, ix->stream));
	HIP_TRY(hipMemcpyAsync(alt_cnt, ix->d_clamped + ix->n_sites, ix->n_sites, hipMemcpyDeviceToHost, ix->stream));
	HIP_TRY(hipStreamSynchronize(ix->stream));
	return VG_OK;
}

// ---- the genotype caller on the device (vg_caller.h; reference qv.cc:1789-1848, GQ at :1681) ------------------------------------
// One lane per site: the exact sums clamped as vg_clamp_counters does, the site's two frequency bytes, the shared caller over the
// HOST's factor tables (staged in LDS once per block), one u16 out: gt << 14 | gq.  The device's log is not libm's, so a site
// whose -10 ln(confidence) is within `guard` of an integer -- or whose confidence is not inside (0, 1) at all -- gets the escape
// code and is counted: the host recomputes those.
constexpr unsigned VG_CALL_BLOCK = 256, VG_CALL_MAX_GRID = 4096;
__global__ __launch_bounds__(VG_CALL_BLOCK) void vg_call_kernel(const uint32_t *__restrict__ cnt, const uint8_t *__restrict__ ref_freq, const uint8_t *__restrict__ alt_freq,
                                                                const vg_caller_tables *__restrict__ tab, uint64_t n_sites, double guard,
                                                                uint16_t *__restrict__ calls, unsigned long long *__restrict__ n_escaped)
{
	__shared__ vg_caller_tables t;
	{
		constexpr unsigned words = sizeof(vg_caller_tables) / sizeof(double);
		const double *src = (const double *)tab;
		double *dst = (double *)&t;
		for (unsigned k = threadIdx.x; k < words; k += VG_CALL_BLOCK) dst[k] = src[k];
	}
	__syncthreads();
	uint32_t escaped = 0;
	for (uint64_t s = (uint64_t)blockIdx.x * VG_CALL_BLOCK + threadIdx.x; s < n_sites; s += (uint64_t)gridDim.x * VG_CALL_BLOCK) {
		const uint2 v = ((const uint2 *)cnt)[s];
		const vg_site_call c = vg_call_site(t, v.x < 63u ? v.x : 63u, v.y < 63u ? v.y : 63u, ref_freq[s], alt_freq[s]);
		uint32_t gq = 0;
		if (c.gt != VGC_NONE) {
			const double y = -10 * log(c.confidence);
			if (vg_gq_settled(c.confidence, y, guard)) gq = (uint32_t)(int)y;
			else { gq = VG_CALL_ESCAPE; escaped++; }
		}
		calls[s] = (uint16_t)((uint32_t)c.gt << 14 | gq);
	}
	for (int o = 32; o > 0; o >>= 1) escaped += __shfl_xor(escaped, o);
	if ((threadIdx.x & 63) == 0 && escaped) atomicAdd(n_escaped, (unsigned long long)escaped);
}

static unsigned call_grid(uint64_t n) { return (unsigned)std::min<uint64_t>((n + VG_CALL_BLOCK - 1) / VG_CALL_BLOCK, VG_CALL_MAX_GRID); }
static const vg_caller_tables &host_call_tables()
{
	static const vg_caller_tables t = [] { vg_caller_tables x; vg_caller_tables_fill(x); return x; }();
	return t;
}
// u16 codes -> final values; a site with the escape code is recomputed here, with libm's logarithm
static void resolve_calls(const uint16_t *code, const uint8_t *ref_cnt, const uint8_t *alt_cnt, const uint8_t *ref_freq, const uint8_t *alt_freq, uint64_t n, uint8_t *gt, int32_t *gq)
{
	const vg_caller_tables &t = host_call_tables();
	for (uint64_t s = 0; s < n; s++) {
		gt[s] = (uint8_t)(code[s] >> 14);
		gq[s] = code[s] & VG_CALL_ESCAPE;
		if (gq[s] == VG_CALL_ESCAPE) {
			const vg_site_call c = vg_call_site(t, ref_cnt[s], alt_cnt[s], ref_freq[s], alt_freq[s]);
			gt[s] = c.gt;
			gq[s] = c.gt == VGC_NONE ? 0 : vg_genotype_quality(c.confidence);
		}
	}
}

// the handle's caller buffers, at first use.  VG_ENOMEM leaves the handle as it was
static int call_buffers(vg_index *ix)
{
	if (ix->d_call_block) return VG_OK;
	const uint64_t n = ix->n_sites, col = (n + 255) & ~255ull;
	const size_t bytes = (size_t)(2 * col + ((2 * n + 255) & ~255ull) + ((sizeof(vg_caller_tables) + 255) & ~255ull) + 256);
	void *q = nullptr;
	if (vg_malloc_patient(&q, bytes) != hipSuccess) { (void)hipGetLastError(); return fail(VG_ENOMEM, "vg_sample_calls_fetch: no device memory for the caller's %s bytes", std::to_string(bytes).c_str()); }
	uint8_t *b = (uint8_t *)q;
	uint8_t *rf = b, *af = b + col;
	uint16_t *calls = (uint16_t *)(b + 2 * col);
	vg_caller_tables *tab = (vg_caller_tables *)(b + 2 * col + ((2 * n + 255) & ~255ull));
	unsigned long long *esc = (unsigned long long *)((uint8_t *)tab + ((sizeof(vg_caller_tables) + 255) & ~255ull));
	hipError_t e = hipSuccess;
	if (n) { e = hipMemcpy(rf, ix->site_rf.data(), n, hipMemcpyHostToDevice); if (e == hipSuccess) e = hipMemcpy(af, ix->site_af.data(), n, hipMemcpyHostToDevice); }
	if (e == hipSuccess) e = hipMemcpy(tab, &host_call_tables(), sizeof(vg_caller_tables), hipMemcpyHostToDevice);
	if (e != hipSuccess) { (void)hipFree(q); return fail(VG_ENODEV, "vg_sample_calls_fetch: %s", hipGetErrorString(e)); }
	ix->owned.push_back(q); ix->owned_bytes[q] = bytes; ix->dev_bytes += bytes;
	ix->d_call_block = q; ix->d_site_rf = rf; ix->d_site_af = af; ix->d_calls = calls; ix->d_call_tab = tab; ix->d_call_esc = esc;
	return VG_OK;
}

extern "C" int vg_sample_calls_fetch(vg_index *ix, uint8_t *gt, int32_t *gq, uint64_t *n_escaped)
{
	if (!ix || !gt || !gq) return fail(VG_EINVAL, "null argument");
	int rc = vg_sync(ix);
	if (rc) return rc;
	if (n_escaped) *n_escaped = 0;
	const uint64_t n = ix->n_sites;
	if (n == 0) return VG_OK;
	return guarded([&]() -> int {
		HIP_TRY(hipSetDevice(ix->device));
		std::vector<uint16_t> code((size_t)n);                    // (host memory first: bad_alloc is VG_ENOMEM too, before the device is asked)
		if ((rc = call_buffers(ix))) return rc;
		HIP_TRY(hipMemsetAsync(ix->d_call_esc, 0, sizeof(unsigned long long), ix->stream));
		vg_call_kernel<<<call_grid(n), VG_CALL_BLOCK, 0, ix->stream>>>(sel_cnt(ix), ix->d_site_rf, ix->d_site_af, ix->d_call_tab, n, VG_CALL_GUARD_DEFAULT, ix->d_calls, ix->d_call_esc);
		HIP_TRY(hipGetLastError());
		unsigned long long esc = 0;
		HIP_TRY(hipMemcpyAsync(code.data(), ix->d_calls, n * sizeof(uint16_t), hipMemcpyDeviceToHost, ix->stream));
		HIP_TRY(hipMemcpyAsync(&esc, ix->d_call_esc, sizeof esc, hipMemcpyDeviceToHost, ix->stream));
		HIP_TRY(hipStreamSynchronize(ix->stream));
		std::vector<uint8_t> cnt;
		if (esc) {                                                // the escaped sites' counters: the two clamped columns, as vg_counts_fetch takes them
			cnt.resize((size_t)(2 * n));
			vg_clamp_counters<<<(unsigned)std::min<uint64_t>((n + 255) / 256, 4096), 256, 0, ix->stream>>>(sel_cnt(ix), n, ix->d_clamped, ix->d_clamped + n);
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipMemcpyAsync(cnt.data(), ix->d_clamped, 2 * n, hipMemcpyDeviceToHost, ix->stream));
			HIP_TRY(hipStreamSynchronize(ix->stream));
		}
		resolve_calls(code.data(), cnt.data(), cnt.data() + (esc ? n : 0), ix->site_rf.data(), ix->site_af.data(), n, gt, gq);
		if (n_escaped) *n_escaped = esc;
		return VG_OK;
	});
}

extern "C" int vg_call_device(int device, const uint8_t *ref_cnt, const uint8_t *alt_cnt, const uint8_t *ref_freq, const uint8_t *alt_freq, uint64_t n, double guard, uint8_t *gt, int32_t *gq, uint64_t *n_escaped)
{
	if (n_escaped) *n_escaped = 0;
	if (n == 0) return VG_OK;
	if (!ref_cnt || !alt_cnt || !ref_freq || !alt_freq || !gt || !gq) return fail(VG_EINVAL, "null argument");
	if (!(guard > 0)) guard = VG_CALL_GUARD_DEFAULT;
	if (!(guard < 0.5)) return fail(VG_EINVAL, "vg_call_device: a guard of 0.5 or more settles nothing");
	return guarded([&]() -> int {
		HIP_TRY(hipSetDevice(device));
		std::vector<uint32_t> cnt((size_t)(2 * n));               // the kernel's input form: the counter array of a sample plane
		for (uint64_t s = 0; s < n; s++) { cnt[2 * s] = ref_cnt[s]; cnt[2 * s + 1] = alt_cnt[s]; }
		std::vector<uint16_t> code((size_t)n);
		DevBuf<uint32_t> d_cnt; DevBuf<uint8_t> d_rf, d_af; DevBuf<uint16_t> d_code; DevBuf<vg_caller_tables> d_tab; DevBuf<unsigned long long> d_esc;
		int rc;
		if ((rc = d_cnt.reserve(2 * n, "site counters")) || (rc = d_rf.reserve(n, "reference frequencies")) || (rc = d_af.reserve(n, "alternative frequencies"))
		    || (rc = d_code.reserve(n, "calls")) || (rc = d_tab.reserve(1, "caller tables")) || (rc = d_esc.reserve(1, "escape count"))) return rc;
		HIP_TRY(hipMemcpy(d_cnt.p, cnt.data(), 2 * n * sizeof(uint32_t), hipMemcpyHostToDevice));
		HIP_TRY(hipMemcpy(d_rf.p, ref_freq, n, hipMemcpyHostToDevice));
		HIP_TRY(hipMemcpy(d_af.p, alt_freq, n, hipMemcpyHostToDevice));
		HIP_TRY(hipMemcpy(d_tab.p, &host_call_tables(), sizeof(vg_caller_tables), hipMemcpyHostToDevice));
		HIP_TRY(hipMemset(d_esc.p, 0, sizeof(unsigned long long)));
		vg_call_kernel<<<call_grid(n), VG_CALL_BLOCK>>>(d_cnt.p, d_rf.p, d_af.p, d_tab.p, n, guard, d_code.p, d_esc.p);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipDeviceSynchronize());
		unsigned long long esc = 0;
		HIP_TRY(hipMemcpy(code.data(), d_code.p, n * sizeof(uint16_t), hipMemcpyDeviceToHost));
		HIP_TRY(hipMemcpy(&esc, d_esc.p, sizeof esc, hipMemcpyDeviceToHost));
		resolve_calls(code.data(), ref_cnt, alt_cnt, ref_freq, alt_freq, n, gt, gq);
		if (n_escaped) *n_escaped = esc;
		return VG_OK;
	});
}

extern "C" int vg_counts_reset(vg_index *ix)
{
	if (!ix) return fail(VG_EINVAL, "null argument");
	{ int rc = finish_pending(ix); if (rc) return rc; }
	HIP_TRY(hipMemsetAsync(ix->d.cnt, 0, (2 * ix->n_sites + 2) * 4, ix->stream));
	for (size_t s = 1; s < ix->planes.size(); s++) HIP_TRY(hipMemsetAsync(ix->planes[s].p.cnt, 0, 2 * ix->n_sites * 4, ix->stream));
	for (Plane &pl : ix->planes) pl.invalid = 0;
	HIP_TRY(hipMemsetAsync(ix->d_stats, 0, S_COUNT * sizeof(unsigned long long), ix->stream));
	for (auto &c : ix->cum) c = 0;
	ix->held_passes = 0;
	ix->host_invalid = 0;
	HIP_TRY(hipStreamSynchronize(ix->stream));
	return VG_OK;
}

extern "C" int vg_counts_device_ptr(vg_index *ix, void **d_counts, uint64_t *n_u32)
{
	if (!ix || !d_counts || !n_u32) return fail(VG_EINVAL, "null argument");
	{ int rc = finish_pending(ix); if (rc) return rc; }         // the sums are only meaningful once the batches in flight have landed
	*d_counts = sel_cnt(ix); *n_u32 = 2 * ix->n_sites;
	return VG_OK;
}

// ---- sample planes (include/vargeno_hip.h): several samples against one resident index --------------------------------------
extern "C" uint32_t vg_num_samples(const vg_index *ix) { return ix ? (uint32_t)ix->planes.size() : 0; }
extern "C" uint32_t vg_sample_selected(const vg_index *ix) { return ix ? ix->cur_sample : 0; }
extern "C" int vg_sample_select(vg_index *ix, uint32_t sample)
{
	if (!ix) return fail(VG_EINVAL, "null argument");
	if (sample >= ix->planes.size()) return fail(VG_EINVAL, "sample %s is out of range: the handle has %s plane(s) (vg_samples_reserve)", std::to_string(sample).c_str(), std::to_string(ix->planes.size()).c_str());
	ix->cur_sample = sample;
	return VG_OK;
}
extern "C" int vg_samples_reserve(vg_index *ix, uint32_t n_samples)
{
	if (!ix) return fail(VG_EINVAL, "null argument");
	if (n_samples < 1 || n_samples > VG_MAX_SAMPLES) return fail(VG_EINVAL, "vg_samples_reserve: 1 to 65535 samples");
	if (n_samples < ix->planes.size()) return fail(VG_EINVAL, "vg_samples_reserve: planes only grow (the handle has %s)", std::to_string(ix->planes.size()).c_str());
	{ int rc = finish_pending(ix); if (rc) return rc; }
	return guarded([&]() -> int {
		// all new planes first, the handle only changes when every one of them could be had
		const size_t have = ix->planes.size(), bytes = (size_t)(24 * ix->n_sites + 16);
		std::vector<void *> blk;
		for (size_t s = have; s < n_samples; s++) {
			void *q = nullptr;
			const hipError_t e = vg_malloc_patient(&q, bytes);
			if (e != hipSuccess || hipMemsetAsync(q, 0, bytes, ix->stream) != hipSuccess) {
				(void)hipGetLastError();
				(void)hipStreamSynchronize(ix->stream);
				if (e == hipSuccess) (void)hipFree(q);
				for (void *b : blk) (void)hipFree(b);
				return fail(VG_ENOMEM, "vg_samples_reserve: no device memory for plane %s of %s bytes", std::to_string(s).c_str(), std::to_string(bytes).c_str());
			}
			blk.push_back(q);
		}
		std::vector<PlanePtr> tab;
		for (void *q : blk) tab.push_back(PlanePtr{(uint32_t *)q + 4 * ix->n_sites + 4, (uint32_t *)q});
		if (!tab.empty()) {
			const hipError_t e = hipMemcpy(ix->d_planes + have, tab.data(), tab.size() * sizeof(PlanePtr), hipMemcpyHostToDevice);
			if (e != hipSuccess || hipStreamSynchronize(ix->stream) != hipSuccess) { for (void *b : blk) (void)hipFree(b); return fail(VG_ENODEV, "vg_samples_reserve: %s", hipGetErrorString(e)); }
		}
		for (size_t i = 0; i < blk.size(); i++) {
			ix->owned.push_back(blk[i]); ix->owned_bytes[blk[i]] = bytes; ix->dev_bytes += bytes;
			Plane pl; pl.p = tab[i];
			ix->planes.push_back(pl);
		}
		return VG_OK;
	});
}
extern "C" int vg_sample_reset(vg_index *ix, uint32_t sample)
{
	if (!ix) return fail(VG_EINVAL, "null argument");
	if (sample >= ix->planes.size()) return fail(VG_EINVAL, "sample %s is out of range", std::to_string(sample).c_str());
	{ int rc = finish_pending(ix); if (rc) return rc; }              // (the fold leaves cnt4 zeroed)
	HIP_TRY(hipMemsetAsync(ix->planes[sample].p.cnt, 0, 2 * ix->n_sites * 4, ix->stream));
	HIP_TRY(hipStreamSynchronize(ix->stream));
	ix->planes[sample].invalid = 0;
	return VG_OK;
}
extern "C" int vg_sample_invalid_reads(vg_index *ix, uint32_t sample, uint64_t *out)
{
	if (!ix || !out) return fail(VG_EINVAL, "null argument");
	if (sample >= ix->planes.size()) return fail(VG_EINVAL, "sample %s is out of range", std::to_string(sample).c_str());
	{ int rc = finish_pending(ix); if (rc) return rc; }
	*out = ix->planes[sample].invalid;
	return VG_OK;
}

// RCCL is resolved lazily (dlopen) so that the library loads, and the rest of the ABI works, on hosts without it; types,
// enumerators and prototypes come from its own header.
#include <rccl/rccl.h>
namespace {
struct Rccl {
	decltype(&ncclAllReduce) all_reduce = nullptr;
	decltype(&ncclCommInitAll) comm_init_all = nullptr;
	decltype(&ncclCommDestroy) comm_destroy = nullptr;
	decltype(&ncclGroupStart) group_start = nullptr;
	decltype(&ncclGroupEnd) group_end = nullptr;
	decltype(&ncclGetErrorString) error_string = nullptr;
	bool ok = false;
};
const Rccl &rccl()
{
	static const Rccl r = [] {
		Rccl x;
		void *h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
		if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
		if (!h) return x;
		x.all_reduce = (decltype(x.all_reduce))dlsym(h, "ncclAllReduce");
		x.comm_init_all = (decltype(x.comm_init_all))dlsym(h, "ncclCommInitAll");
		x.comm_destroy = (decltype(x.comm_destroy))dlsym(h, "ncclCommDestroy");
		x.group_start = (decltype(x.group_start))dlsym(h, "ncclGroupStart");
		x.group_end = (decltype(x.group_end))dlsym(h, "ncclGroupEnd");
		x.error_string = (decltype(x.error_string))dlsym(h, "ncclGetErrorString");
		x.ok = x.all_reduce && x.comm_init_all && x.comm_destroy && x.group_start && x.group_end && x.error_string;
		return x;
	}();
	return r;
}
}  // namespace

extern "C" int vg_counts_allreduce(vg_index *ix, void *nccl_comm)
{
	if (!ix || !nccl_comm) return fail(VG_EINVAL, "null argument");
	const Rccl &R = rccl();
	if (!R.ok) return fail(VG_ENODEV, "cannot load librccl (or it lacks the collective entry points)");
	{ int rc = finish_pending(ix); if (rc) return rc; }
	if (ix->n_sites == 0) return VG_OK;
	const ncclResult_t rc = R.all_reduce(sel_cnt(ix), sel_cnt(ix), (size_t)(2 * ix->n_sites), ncclUint32, ncclSum, (ncclComm_t)nccl_comm, ix->stream);
	if (rc != ncclSuccess) return fail(VG_ENODEV, "ncclAllReduce: %s", R.error_string(rc));
	HIP_TRY(hipStreamSynchronize(ix->stream));
	return VG_OK;
}

__global__ void vg_add_counters(uint32_t *__restrict__ dst, const uint32_t *__restrict__ src, uint64_t n)
{
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) dst[i] += src[i];
}

// One process driving n replicas (the CLI with VARGENO_GPUS=n): communicator over the replicas' devices, one grouped in-place
// all-reduce of the counters, communicator torn down.  n = 1 is the identity and still goes through RCCL.  Replicas that share
// a device (small indexes; the one-GPU test boxes) are summed on that device first -- RCCL wants one rank per device --, the
// first of them takes part in the all-reduce, and the others get its result.
extern "C" int vg_counts_allreduce_devices(vg_index **handles, int n)
{
	if (!handles || n <= 0) return fail(VG_EINVAL, "null argument");
	for (int i = 0; i < n; i++) {
		if (!handles[i]) return fail(VG_EINVAL, "null handle");
		if (handles[i]->n_sites != handles[0]->n_sites) return fail(VG_EINVAL, "the handles do not hold replicas of one index");
		if (handles[i]->cur_sample != handles[0]->cur_sample) return fail(VG_EINVAL, "the handles have different samples selected (vg_sample_select): the exchange sums ONE sample's counters");
		for (int j = 0; j < i; j++) if (handles[j] == handles[i]) return fail(VG_EINVAL, "the same handle twice");
	}
	const Rccl &R = rccl();
	if (!R.ok) return fail(VG_ENODEV, "cannot load librccl (or it lacks the collective entry points)");
	for (int i = 0; i < n; i++) { int rc = finish_pending(handles[i]); if (rc) return rc; }
	if (handles[0]->n_sites == 0) return VG_OK;
	return guarded([&]() -> int {
		// the order of operations lives in vg_allreduce_plan.h (so that it can be run against a mock); this is its HIP + RCCL backend
		struct Backend {
			vg_index **h; const Rccl &R; uint64_t words; std::vector<ncclComm_t> comms; ncclResult_t last = ncclSuccess;
			int device_of(int i) { return h[i]->device; }
			int add_into(int dst, int src)
			{
				if (hipSetDevice(h[dst]->device) != hipSuccess) return VG_ENODEV;
				vg_add_counters<<<(unsigned)std::min<uint64_t>((words + 255) / 256, 4096), 256, 0, h[dst]->stream>>>(sel_cnt(h[dst]), sel_cnt(h[src]), words);
				return hipGetLastError() == hipSuccess ? 0 : VG_ENODEV;
			}
			int comm_init(const int *devs, int nr) { comms.assign((size_t)nr, nullptr); last = R.comm_init_all(comms.data(), nr, devs); return last == ncclSuccess ? 0 : VG_ENODEV; }
			int group_start() { last = R.group_start(); return last == ncclSuccess ? 0 : VG_ENODEV; }
			int group_end() { const ncclResult_t r = R.group_end(); if (r != ncclSuccess) last = r; return r == ncclSuccess ? 0 : VG_ENODEV; }
			int all_reduce(int i, int rank)
			{
				if (hipSetDevice(h[i]->device) != hipSuccess) { last = ncclUnhandledCudaError; return VG_ENODEV; }
				last = R.all_reduce(sel_cnt(h[i]), sel_cnt(h[i]), (size_t)words, ncclUint32, ncclSum, comms[(size_t)rank], h[i]->stream);
				return last == ncclSuccess ? 0 : VG_ENODEV;
			}
			int copy_from(int dst, int src)
			{
				return hipSetDevice(h[src]->device) == hipSuccess && hipMemcpyAsync(sel_cnt(h[dst]), sel_cnt(h[src]), words * 4, hipMemcpyDeviceToDevice, h[src]->stream) == hipSuccess ? 0 : VG_ENODEV;
			}
			int sync(int i) { return hipSetDevice(h[i]->device) == hipSuccess && hipStreamSynchronize(h[i]->stream) == hipSuccess ? 0 : VG_ENODEV; }
			void comm_destroy() { for (ncclComm_t c : comms) if (c) (void)R.comm_destroy(c); comms.clear(); }
		} B{handles, R, 2 * handles[0]->n_sites, {}};
		const char *where = "";
		const int rc = run_allreduce(B, n, &where);
		if (rc) return fail(rc, "RCCL exchange of the site counters failed at: %s (%s)", where, B.last != ncclSuccess ? R.error_string(B.last) : "HIP error");
		return VG_OK;
	});
}

// ---- the genotype matrix and the pairwise sample table (vg_pairs.h; no reference counterpart) -----------------------------------
// A vg_gmatrix holds, on one device, the class planes of n_samples samples -- planes[(sample * 3 + plane) * n_words + word] -- and
// the n_samples x n_samples x 5 result.  It is no part of a vg_index.
//
// vg_pairs_pack_kernel: one wave per 64-site word, three ballots of the lanes' classes; a lane beyond n_sites votes for nothing, so
// the tail bits of the last word are zero.
//
// vg_pairs_kernel, the hot path: a workgroup -- one wave -- owns a VG_PAIR_TILE x VG_PAIR_TILE tile of sample pairs (tiles with
// tile_j >= tile_i; blockIdx.x) and words_per_block consecutive site words (blockIdx.y).  For VG_PAIR_RUN words at a time it stages
// the planes of the tile's row samples and of its column samples in LDS, image word (plane, w, s) at (plane * RUN + w) * PITCH + s:
// the samples of one word lie side by side.  64 lanes as 8 x 8; a lane owns rows {ty + 8a} x columns {tx + 8b}, a, b < 4: 16 pairs,
// 80 u32 term counters in registers (vg_pairs.h: five terms give the five counters of [i][j] and het_j for [j][i]).  Per word a
// lane reads 4 x 3 row words and 4 x 3 column words, 8 bytes each: among the 32 lanes of a read group (4 ty x 8 tx) the row reads
// are four adjacent words, each broadcast to eight lanes, and the column reads eight consecutive words, each read by four lanes --
// no bank is asked for two words.  The staging stores run over w fastest, 8 lanes PITCH words apart: PITCH is odd, so their 16
// dwords fall on 16 different banks.  At the end the counters go to the result with 64-bit vector atomics (the result is zeroed
// by a memset ahead of the launch): five to [i][j], and off the diagonal tiles het_j to [j][i][4]; a diagonal tile computes both
// (i, j) and (j, i) itself.  vg_pairs_mirror_kernel then copies the four symmetric counters of the off-diagonal tiles to [j][i].
constexpr unsigned VG_PAIR_TILE = 32, VG_PAIR_THREADS = 64, VG_PAIR_RUN = 8, VG_PAIR_PITCH = VG_PAIR_TILE + 1;
constexpr uint64_t VG_PAIR_WORDS_DEFAULT = 1024;              // site words per block: 65 536 sites, far inside a u32 counter
constexpr uint64_t VG_PAIR_WORDS_MAX = 1ull << 24;            // 2^30 sites per block: the u32 counters cannot wrap
constexpr uint32_t VG_GMATRIX_MAX_SAMPLES = 16384;

__global__ __launch_bounds__(256) void vg_pairs_pack_kernel(const uint8_t *__restrict__ gt, const int32_t *__restrict__ gq, uint64_t n_sites, uint64_t n_words, int32_t min_gq,
                                                            uint64_t *__restrict__ r, uint64_t *__restrict__ h, uint64_t *__restrict__ a)
{
	const unsigned lane = threadIdx.x & 63;
	const uint64_t n_waves = (uint64_t)gridDim.x * 4;
	for (uint64_t w = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6; w < n_words; w += n_waves) {      // (w is the same for a wave's lanes)
		const uint64_t s = w * 64 + lane;
		const int c = s < n_sites ? vg_pair_class(gt[s], gq[s], min_gq) : -1;
		const uint64_t br = __ballot(c == VGP_R), bh = __ballot(c == VGP_H), ba = __ballot(c == VGP_A);
		if (lane == 0) { r[w] = br; h[w] = bh; a[w] = ba; }
	}
}

__global__ __launch_bounds__(VG_PAIR_THREADS) void vg_pairs_kernel(const uint64_t *__restrict__ planes, uint64_t n_words, uint32_t n_samples, uint32_t n_tiles, uint64_t words_per_block,
                                                                   unsigned long long *__restrict__ counts)
{
	constexpr unsigned T = VG_PAIR_TILE, RUN = VG_PAIR_RUN, PITCH = VG_PAIR_PITCH;
	__shared__ uint64_t img[2][VGP_PLANES * RUN * PITCH];                 // [0] the row samples, [1] the column samples
	uint32_t ti = 0, rem = blockIdx.x;
	while (rem >= n_tiles - ti) { rem -= n_tiles - ti; ti++; }            // blockIdx.x counts the tiles (ti, tj >= ti) row by row
	const uint32_t tj = ti + rem;
	const uint64_t wbeg = (uint64_t)blockIdx.y * words_per_block, wend = wbeg + words_per_block < n_words ? wbeg + words_per_block : n_words;
	const unsigned tx = threadIdx.x & 7, ty = threadIdx.x >> 3;
	uint32_t acc[4][4][VGP_TERMS] = {};
	for (uint64_t w0 = wbeg; w0 < wend; w0 += RUN) {
		const uint64_t cnt = wend - w0;                                   // words of this run that exist (RUN or more: all)
		for (unsigned e = threadIdx.x; e < 2 * T * VGP_PLANES * RUN; e += VG_PAIR_THREADS) {
			const unsigned w = e % RUN, p = (e / RUN) % VGP_PLANES, s = (e / (RUN * VGP_PLANES)) % T, side = e / (RUN * VGP_PLANES * T);
			const uint32_t sample = (side ? tj : ti) * T + s;
			uint64_t v = 0;                                               // a sample beyond the matrix or a word beyond the block counts nothing
			if (sample < n_samples && w < cnt) v = planes[((uint64_t)sample * VGP_PLANES + p) * n_words + w0 + w];
			img[side][(p * RUN + w) * PITCH + s] = v;
		}
		__syncthreads();
#pragma unroll 1
		for (unsigned w = 0; w < RUN; w++) {
			uint64_t row[4][VGP_PLANES], col[4][VGP_PLANES];
#pragma unroll
			for (unsigned p = 0; p < VGP_PLANES; p++) {
#pragma unroll
				for (unsigned a = 0; a < 4; a++) { row[a][p] = img[0][(p * RUN + w) * PITCH + ty + 8 * a]; col[a][p] = img[1][(p * RUN + w) * PITCH + tx + 8 * a]; }
			}
#pragma unroll
			for (unsigned a = 0; a < 4; a++) {
#pragma unroll
				for (unsigned b = 0; b < 4; b++) {
					vg_pair_word_add(acc[a][b], row[a][VGP_R], row[a][VGP_H], row[a][VGP_A], col[b][VGP_R], col[b][VGP_H], col[b][VGP_A]);
					// one pair after the other: left alone the scheduler forms all 160 ANDs of the word first and needs 237 registers for them
					__builtin_amdgcn_sched_barrier(0);
				}
			}
		}
		__syncthreads();
	}
#pragma unroll
	for (unsigned a = 0; a < 4; a++) {
#pragma unroll
		for (unsigned b = 0; b < 4; b++) {
			const uint32_t i = ti * T + ty + 8 * a, j = tj * T + tx + 8 * b;
			if (i >= n_samples || j >= n_samples) continue;
			uint64_t c[VGP_COUNTERS];
			const uint64_t het_j = vg_pair_counters(acc[a][b], c);
			unsigned long long *ij = counts + ((uint64_t)i * n_samples + j) * VGP_COUNTERS;
#pragma unroll
			for (unsigned k = 0; k < VGP_COUNTERS; k++) if (c[k]) atomicAdd(ij + k, (unsigned long long)c[k]);
			if (ti != tj && het_j) atomicAdd(counts + ((uint64_t)j * n_samples + i) * VGP_COUNTERS + VGP_HET_I, (unsigned long long)het_j);
		}
	}
}

// [j][i][n, ibs0, ibs2, hethet] = [i][j][..] for the pairs of the off-diagonal tiles (tile of j above tile of i); [j][i][het_i] is
// already there.  One lane per (i, j): blockIdx.y = i
__global__ __launch_bounds__(256) void vg_pairs_mirror_kernel(unsigned long long *__restrict__ counts, uint32_t n_samples)
{
	const uint32_t i = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
	if (j >= n_samples || i / VG_PAIR_TILE >= j / VG_PAIR_TILE) return;
	const unsigned long long *ij = counts + ((uint64_t)i * n_samples + j) * VGP_COUNTERS;
	unsigned long long *ji = counts + ((uint64_t)j * n_samples + i) * VGP_COUNTERS;
	for (unsigned k = 0; k < VGP_HET_I; k++) ji[k] = ij[k];
}

struct vg_gmatrix {
	int device = 0;
	uint64_t n_sites = 0, n_words = 0, dev_bytes = 0;
	uint32_t n_samples = 0;
	uint64_t *d_planes = nullptr;                    // [n_samples][3][n_words]: zero = every call missing
	unsigned long long *d_counts = nullptr;          // [n_samples][n_samples][5]
	uint8_t *d_gt = nullptr;                         // one sample's columns on their way to the pack kernel
	int32_t *d_gq = nullptr;
	hipStream_t stream = nullptr;
	hipEvent_t ev0 = nullptr, ev1 = nullptr;         // around the pair kernels (VG_VERBOSE prints the time)
};

static void gmatrix_free(vg_gmatrix *gm)
{
	if (!gm) return;
	(void)hipSetDevice(gm->device);
	if (gm->ev0) (void)hipEventDestroy(gm->ev0);
	if (gm->ev1) (void)hipEventDestroy(gm->ev1);
	if (gm->stream) (void)hipStreamDestroy(gm->stream);
	for (void *p : {(void *)gm->d_planes, (void *)gm->d_counts, (void *)gm->d_gt, (void *)gm->d_gq}) if (p) (void)hipFree(p);
	(void)hipGetLastError();
	delete gm;
}

extern "C" int vg_gmatrix_create(int device, uint64_t n_sites, uint32_t n_samples, vg_gmatrix **out)
{
	if (!out) return fail(VG_EINVAL, "null argument");
	*out = nullptr;
	if (n_samples == 0) return fail(VG_EINVAL, "vg_gmatrix_create: no samples");
	if (n_sites >= (1ull << 32)) return fail(VG_EINVAL, "vg_gmatrix_create: 2^32 sites or more");
	if (n_samples > VG_GMATRIX_MAX_SAMPLES) return fail(VG_ETOOBIG, "vg_gmatrix_create: more than %s samples", std::to_string(VG_GMATRIX_MAX_SAMPLES).c_str());
	return guarded([&]() -> int {
		HIP_TRY(hipSetDevice(device));
		vg_gmatrix *gm = new vg_gmatrix;
		gm->device = device; gm->n_sites = n_sites; gm->n_words = (n_sites + 63) / 64; gm->n_samples = n_samples;
		const size_t plane_bytes = (size_t)n_samples * VGP_PLANES * gm->n_words * 8, count_bytes = (size_t)n_samples * n_samples * VGP_COUNTERS * 8;
		struct { void **p; size_t bytes; const char *what; } want[] = {
			{(void **)&gm->d_planes, plane_bytes, "the samples' planes"}, {(void **)&gm->d_counts, count_bytes, "the pair table"},
			{(void **)&gm->d_gt, (size_t)n_sites, "a gt column"}, {(void **)&gm->d_gq, (size_t)n_sites * 4, "a gq column"}};
		for (auto &w : want) {
			if (vg_malloc_patient(w.p, w.bytes ? w.bytes : 8) != hipSuccess) {
				(void)hipGetLastError();
				*w.p = nullptr;
				gmatrix_free(gm);
				return fail(VG_ENOMEM, "vg_gmatrix_create: no device memory for %s (%s bytes)", w.what, std::to_string(w.bytes).c_str());
			}
			gm->dev_bytes += w.bytes ? w.bytes : 8;
		}
		hipError_t e = hipStreamCreateWithFlags(&gm->stream, hipStreamNonBlocking);
		if (e == hipSuccess) e = hipEventCreate(&gm->ev0);
		if (e == hipSuccess) e = hipEventCreate(&gm->ev1);
		if (e == hipSuccess && plane_bytes) e = hipMemsetAsync(gm->d_planes, 0, plane_bytes, gm->stream);
		if (e == hipSuccess) e = hipStreamSynchronize(gm->stream);
		if (e != hipSuccess) { gmatrix_free(gm); return fail(VG_ENODEV, "vg_gmatrix_create: %s", hipGetErrorString(e)); }
		*out = gm;
		return VG_OK;
	});
}

extern "C" void vg_gmatrix_destroy(vg_gmatrix *gm) { gmatrix_free(gm); }
extern "C" uint64_t vg_gmatrix_device_bytes(const vg_gmatrix *gm) { return gm ? gm->dev_bytes : 0; }

extern "C" int vg_gmatrix_set(vg_gmatrix *gm, uint32_t sample, const uint8_t *gt, const int32_t *gq, int32_t min_gq)
{
	if (!gm || !gt || !gq) return fail(VG_EINVAL, "null argument");
	if (sample >= gm->n_samples) return fail(VG_EINVAL, "vg_gmatrix_set: sample %s is out of range", std::to_string(sample).c_str());
	if (gm->n_sites == 0) return VG_OK;
	HIP_TRY(hipSetDevice(gm->device));
	HIP_TRY(hipMemcpyAsync(gm->d_gt, gt, gm->n_sites, hipMemcpyHostToDevice, gm->stream));
	HIP_TRY(hipMemcpyAsync(gm->d_gq, gq, gm->n_sites * 4, hipMemcpyHostToDevice, gm->stream));
	uint64_t *r = gm->d_planes + (uint64_t)sample * VGP_PLANES * gm->n_words;
	const unsigned grid = (unsigned)std::min<uint64_t>((gm->n_words + 3) / 4, 4096);
	vg_pairs_pack_kernel<<<grid, 256, 0, gm->stream>>>(gm->d_gt, gm->d_gq, gm->n_sites, gm->n_words, min_gq, r + VGP_R * gm->n_words, r + VGP_H * gm->n_words, r + VGP_A * gm->n_words);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(gm->stream));                    // (the host arrays are the caller's again)
	return VG_OK;
}

extern "C" int vg_gmatrix_pairs(vg_gmatrix *gm, uint64_t words_per_block, uint64_t *counts)
{
	if (!gm || !counts) return fail(VG_EINVAL, "null argument");
	HIP_TRY(hipSetDevice(gm->device));
	const uint32_t N = gm->n_samples, n_tiles = (N + VG_PAIR_TILE - 1) / VG_PAIR_TILE;
	const size_t count_bytes = (size_t)N * N * VGP_COUNTERS * 8;
	uint64_t wpb = words_per_block ? words_per_block : VG_PAIR_WORDS_DEFAULT;
	if (wpb > VG_PAIR_WORDS_MAX) wpb = VG_PAIR_WORDS_MAX;
	if ((gm->n_words + wpb - 1) / wpb > 65535) wpb = (gm->n_words + 65534) / 65535;        // (a grid's second dimension ends there)
	const unsigned n_blocks = (unsigned)((gm->n_words + wpb - 1) / wpb);
	HIP_TRY(hipEventRecord(gm->ev0, gm->stream));
	HIP_TRY(hipMemsetAsync(gm->d_counts, 0, count_bytes, gm->stream));
	if (n_blocks) {
		vg_pairs_kernel<<<dim3(n_tiles * (n_tiles + 1) / 2, n_blocks), VG_PAIR_THREADS, 0, gm->stream>>>(gm->d_planes, gm->n_words, N, n_tiles, wpb, gm->d_counts);
		HIP_TRY(hipGetLastError());
		if (n_tiles > 1) {
			vg_pairs_mirror_kernel<<<dim3((N + 255) / 256, N), 256, 0, gm->stream>>>(gm->d_counts, N);
			HIP_TRY(hipGetLastError());
		}
	}
	HIP_TRY(hipEventRecord(gm->ev1, gm->stream));
	HIP_TRY(hipMemcpyAsync(counts, gm->d_counts, count_bytes, hipMemcpyDeviceToHost, gm->stream));
	HIP_TRY(hipStreamSynchronize(gm->stream));
	if (getenv("VG_VERBOSE")) {
		float ms = 0;
		HIP_TRY(hipEventElapsedTime(&ms, gm->ev0, gm->ev1));
		const double pw = (double)N * (N + 1) / 2 * (double)gm->n_words;
		fprintf(stderr, "[vargeno_hip] vg_gmatrix_pairs: %u samples, %lu site words in %u blocks of %lu: kernels %.3f ms, %.3e pair-words/s\n", N, (unsigned long)gm->n_words, n_blocks, (unsigned long)wpb, ms, ms > 0 ? pw / (ms * 1e-3) : 0.0);
	}
	return VG_OK;
}

extern "C" int vg_pairs_host(const uint8_t *gt, const int32_t *gq, uint64_t n_sites, uint32_t n_samples, int32_t min_gq, int threads, uint64_t *counts)
{
	if (!counts || ((!gt || !gq) && n_sites)) return fail(VG_EINVAL, "null argument");
	if (n_samples == 0) return fail(VG_EINVAL, "vg_pairs_host: no samples");
	if (n_sites >= (1ull << 32)) return fail(VG_EINVAL, "vg_pairs_host: 2^32 sites or more");
	return guarded([&]() -> int {
		vg_pairs_host_run(gt, gq, n_sites, n_samples, min_gq, threads, counts);
		return VG_OK;
	});
}

// ---- the cohort prior: every sample re-called with the cohort's own allele frequency (vg_cprior.h; no reference counterpart) ------
// A vg_cprior holds, on one device, the counter words of n_samples samples and their call words, both SAMPLE-MAJOR
// (word[sample * n_sites + site], 2 bytes each), the sites' final q, the two frequency columns of a run and one sample's columns of
// staging.  It is no part of a vg_index.
//
// vg_cprior_kernel: one lane per site (grid-stride).  The block stages the per-sample factors of the HOST's table -- keep, flip,
// half, depth, 3 056 bytes -- in LDS; the site's two freq[] entries come from the table in global memory, once.  The EM passes and
// the last pass walk the samples in index order inside the lane: the 64 lanes of a wave read 64 consecutive 2-byte words of one
// sample, one 128-byte line per wave and sample, and the passes after the first find the lines in L2 as far as it holds them.  The
// sum e is the lane's own, in sample order: no cross-lane sum, no atomic but the escape count's (a wave reduction, then one 64-bit
// add per wave).  Per sample and pass: five LDS reads (their banks are the counters' accident), about a dozen f64 multiplies and
// adds, one f64 division.  The last pass writes the call words sample-major, again a line per wave and sample.  A call whose
// -10 ln(confidence) the device's log cannot settle (vg_gq_settled) leaves with VG_CALL_ESCAPE, as in vg_call_kernel.
// 256 lanes per block: the kernel holds 3 KB of LDS per block and no barrier but the staging's, so the block size only decides how
// many lanes share one staging; nothing about its speed has been measured.
constexpr unsigned VG_CPRIOR_BLOCK = 256, VG_CPRIOR_MAX_GRID = 8192;
constexpr uint32_t VG_CPRIOR_MAX_SAMPLES = 16384;
__global__ __launch_bounds__(VG_CPRIOR_BLOCK) void vg_cprior_kernel(const uint16_t *__restrict__ cnt, const uint8_t *__restrict__ ref_freq, const uint8_t *__restrict__ alt_freq,
                                                                    const vg_caller_tables *__restrict__ tab, uint64_t n_sites, uint32_t n_samples, int iters, double pseudo, double guard,
                                                                    double *__restrict__ q_out, uint16_t *__restrict__ calls, unsigned long long *__restrict__ n_escaped)
{
	__shared__ vg_cprior_factors f;
	{
		constexpr unsigned words = sizeof(vg_cprior_factors) / sizeof(double);      // (the head of vg_caller_tables: vg_cprior.h)
		const double *src = (const double *)tab;
		double *dst = (double *)&f;
		for (unsigned k = threadIdx.x; k < words; k += VG_CPRIOR_BLOCK) dst[k] = src[k];
	}
	__syncthreads();
	uint32_t escaped = 0;
	for (uint64_t site = (uint64_t)blockIdx.x * VG_CPRIOR_BLOCK + threadIdx.x; site < n_sites; site += (uint64_t)gridDim.x * VG_CPRIOR_BLOCK) {
		const uint16_t *col = cnt + site;
		auto word = [&](uint32_t s) -> unsigned { return col[(uint64_t)s * n_sites]; };
		const double q = vg_cprior_site_q(f, word, n_samples, vg_cprior_qd(tab->freq[ref_freq[site]], tab->freq[alt_freq[site]]), iters, pseudo);
		q_out[site] = q;
		const vg_cprior_hw g = vg_cprior_hw_at(q);
		for (uint32_t s = 0; s < n_samples; s++) {
			const vg_site_call c = vg_cprior_call(f, g, word(s));
			uint32_t gq = 0;
			if (c.gt != VGC_NONE) {
				const double y = -10 * log(c.confidence);
				if (vg_gq_settled(c.confidence, y, guard)) gq = (uint32_t)(int)y;
				else { gq = VG_CALL_ESCAPE; escaped++; }
			}
			calls[(uint64_t)s * n_sites + site] = (uint16_t)((uint32_t)c.gt << 14 | gq);
		}
	}
	for (int o = 32; o > 0; o >>= 1) escaped += __shfl_xor(escaped, o);
	if ((threadIdx.x & 63) == 0 && escaped) atomicAdd(n_escaped, (unsigned long long)escaped);
}

// one sample's two counter columns (staging) -> its counter words, clamped
__global__ __launch_bounds__(256) void vg_cprior_pack_kernel(const uint8_t *__restrict__ ref_cnt, const uint8_t *__restrict__ alt_cnt, uint64_t n_sites, uint16_t *__restrict__ words)
{
	for (uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x; s < n_sites; s += (uint64_t)gridDim.x * 256) words[s] = vg_cprior_word(ref_cnt[s], alt_cnt[s]);
}

struct vg_cprior {
	int device = 0;
	uint64_t n_sites = 0, dev_bytes = 0;
	uint32_t n_samples = 0;
	uint16_t *d_cnt = nullptr, *d_calls = nullptr;   // [n_samples][n_sites]: r | a << 8 (zero: never set), gt << 14 | gq
	double *d_q = nullptr;                           // [n_sites]
	uint8_t *d_rf = nullptr, *d_af = nullptr;        // the frequency columns of a run
	uint8_t *d_stage = nullptr;                      // one sample's ref and alt columns on their way to the pack kernel
	vg_caller_tables *d_tab = nullptr;
	unsigned long long *d_esc = nullptr;
	hipStream_t stream = nullptr;
	hipEvent_t ev0 = nullptr, ev1 = nullptr;         // around the kernel (VG_VERBOSE prints the time)
	bool ran = false;                                // the call words are those of the counters as they are now
	std::vector<double> q;                           // the last run's q, for the entries that left it with the escape code
};

static void cprior_free(vg_cprior *cp)
{
	if (!cp) return;
	(void)hipSetDevice(cp->device);
	if (cp->ev0) (void)hipEventDestroy(cp->ev0);
	if (cp->ev1) (void)hipEventDestroy(cp->ev1);
	if (cp->stream) (void)hipStreamDestroy(cp->stream);
	for (void *p : {(void *)cp->d_cnt, (void *)cp->d_calls, (void *)cp->d_q, (void *)cp->d_rf, (void *)cp->d_af, (void *)cp->d_stage, (void *)cp->d_tab, (void *)cp->d_esc}) if (p) (void)hipFree(p);
	(void)hipGetLastError();
	delete cp;
}

static int cprior_check_rule(const char *who, int iters, double pseudo)
{
	if (iters < 1 || iters > VG_CPRIOR_ITERS_MAX) return fail(VG_EINVAL, "%s: iters is 1 .. 64", who);
	if (!(pseudo >= 0.0 && pseudo <= 1.7976931348623157e308)) return fail(VG_EINVAL, "%s: pseudo is finite and not negative", who);
	return VG_OK;
}

extern "C" int vg_cprior_create(int device, uint64_t n_sites, uint32_t n_samples, vg_cprior **out)
{
	if (!out) return fail(VG_EINVAL, "null argument");
	*out = nullptr;
	if (n_samples == 0) return fail(VG_EINVAL, "vg_cprior_create: no samples");
	if (n_sites >= (1ull << 32)) return fail(VG_EINVAL, "vg_cprior_create: 2^32 sites or more");
	if (n_samples > VG_CPRIOR_MAX_SAMPLES) return fail(VG_ETOOBIG, "vg_cprior_create: more than %s samples", std::to_string(VG_CPRIOR_MAX_SAMPLES).c_str());
	return guarded([&]() -> int {
		HIP_TRY(hipSetDevice(device));
		vg_cprior *cp = new vg_cprior;
		cp->device = device; cp->n_sites = n_sites; cp->n_samples = n_samples;
		try { cp->q.resize((size_t)n_sites); } catch (...) { delete cp; throw; }
		const size_t matrix_bytes = (size_t)n_samples * n_sites * 2;
		struct { void **p; size_t bytes; const char *what; } want[] = {
			{(void **)&cp->d_cnt, matrix_bytes, "the samples' counters"}, {(void **)&cp->d_calls, matrix_bytes, "the samples' calls"}, {(void **)&cp->d_q, (size_t)n_sites * 8, "the sites' q"},
			{(void **)&cp->d_rf, (size_t)n_sites, "a frequency column"}, {(void **)&cp->d_af, (size_t)n_sites, "a frequency column"}, {(void **)&cp->d_stage, (size_t)n_sites * 2, "a sample's counter columns"},
			{(void **)&cp->d_tab, sizeof(vg_caller_tables), "the caller tables"}, {(void **)&cp->d_esc, 8, "the escape count"}};
		for (auto &w : want) {
			if (vg_malloc_patient(w.p, w.bytes ? w.bytes : 8) != hipSuccess) {
				(void)hipGetLastError();
				*w.p = nullptr;
				cprior_free(cp);
				return fail(VG_ENOMEM, "vg_cprior_create: no device memory for %s (%s bytes)", w.what, std::to_string(w.bytes).c_str());
			}
			cp->dev_bytes += w.bytes ? w.bytes : 8;
		}
		hipError_t e = hipStreamCreateWithFlags(&cp->stream, hipStreamNonBlocking);
		if (e == hipSuccess) e = hipEventCreate(&cp->ev0);
		if (e == hipSuccess) e = hipEventCreate(&cp->ev1);
		if (e == hipSuccess && matrix_bytes) e = hipMemsetAsync(cp->d_cnt, 0, matrix_bytes, cp->stream);
		if (e == hipSuccess) e = hipMemcpyAsync(cp->d_tab, &host_call_tables(), sizeof(vg_caller_tables), hipMemcpyHostToDevice, cp->stream);
		if (e == hipSuccess) e = hipStreamSynchronize(cp->stream);
		if (e != hipSuccess) { cprior_free(cp); return fail(VG_ENODEV, "vg_cprior_create: %s", hipGetErrorString(e)); }
		*out = cp;
		return VG_OK;
	});
}

extern "C" void vg_cprior_destroy(vg_cprior *cp) { cprior_free(cp); }
extern "C" uint64_t vg_cprior_device_bytes(const vg_cprior *cp) { return cp ? cp->dev_bytes : 0; }

extern "C" int vg_cprior_set(vg_cprior *cp, uint32_t sample, const uint8_t *ref_cnt, const uint8_t *alt_cnt)
{
	if (!cp || !ref_cnt || !alt_cnt) return fail(VG_EINVAL, "null argument");
	if (sample >= cp->n_samples) return fail(VG_EINVAL, "vg_cprior_set: sample %s is out of range", std::to_string(sample).c_str());
	cp->ran = false;
	const uint64_t n = cp->n_sites;
	if (n == 0) return VG_OK;
	HIP_TRY(hipSetDevice(cp->device));
	HIP_TRY(hipMemcpyAsync(cp->d_stage, ref_cnt, n, hipMemcpyHostToDevice, cp->stream));
	HIP_TRY(hipMemcpyAsync(cp->d_stage + n, alt_cnt, n, hipMemcpyHostToDevice, cp->stream));
	vg_cprior_pack_kernel<<<(unsigned)std::min<uint64_t>((n + 255) / 256, 4096), 256, 0, cp->stream>>>(cp->d_stage, cp->d_stage + n, n, cp->d_cnt + (uint64_t)sample * n);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(cp->stream));                    // (the host arrays are the caller's again)
	return VG_OK;
}

extern "C" int vg_cprior_run(vg_cprior *cp, const uint8_t *ref_freq, const uint8_t *alt_freq, int iters, double pseudo, double guard, double *q_out, uint64_t *n_escaped)
{
	if (n_escaped) *n_escaped = 0;
	if (!cp || ((!ref_freq || !alt_freq) && cp->n_sites)) return fail(VG_EINVAL, "null argument");
	if (int rc = cprior_check_rule("vg_cprior_run", iters, pseudo)) return rc;
	if (!(guard > 0)) guard = VG_CALL_GUARD_DEFAULT;
	if (!(guard < 0.5)) return fail(VG_EINVAL, "vg_cprior_run: a guard of 0.5 or more settles nothing");
	const uint64_t n = cp->n_sites;
	if (n == 0) { cp->ran = true; return VG_OK; }
	HIP_TRY(hipSetDevice(cp->device));
	cp->ran = false;
	HIP_TRY(hipMemcpyAsync(cp->d_rf, ref_freq, n, hipMemcpyHostToDevice, cp->stream));
	HIP_TRY(hipMemcpyAsync(cp->d_af, alt_freq, n, hipMemcpyHostToDevice, cp->stream));
	HIP_TRY(hipMemsetAsync(cp->d_esc, 0, sizeof(unsigned long long), cp->stream));
	const unsigned grid = (unsigned)std::min<uint64_t>((n + VG_CPRIOR_BLOCK - 1) / VG_CPRIOR_BLOCK, VG_CPRIOR_MAX_GRID);
	HIP_TRY(hipEventRecord(cp->ev0, cp->stream));
	vg_cprior_kernel<<<grid, VG_CPRIOR_BLOCK, 0, cp->stream>>>(cp->d_cnt, cp->d_rf, cp->d_af, cp->d_tab, n, cp->n_samples, iters, pseudo, guard, cp->d_q, cp->d_calls, cp->d_esc);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipEventRecord(cp->ev1, cp->stream));
	unsigned long long esc = 0;
	HIP_TRY(hipMemcpyAsync(cp->q.data(), cp->d_q, n * sizeof(double), hipMemcpyDeviceToHost, cp->stream));
	HIP_TRY(hipMemcpyAsync(&esc, cp->d_esc, sizeof esc, hipMemcpyDeviceToHost, cp->stream));
	HIP_TRY(hipStreamSynchronize(cp->stream));
	cp->ran = true;
	if (q_out) memcpy(q_out, cp->q.data(), n * sizeof(double));
	if (n_escaped) *n_escaped = esc;
	if (getenv("VG_VERBOSE")) {
		float ms = 0;
		HIP_TRY(hipEventElapsedTime(&ms, cp->ev0, cp->ev1));
		fprintf(stderr, "[vargeno_hip] vg_cprior_run: %u samples, %lu sites, %d iterations in %u blocks: kernel %.3f ms, %lu entries left to the host\n", cp->n_samples, (unsigned long)n, iters, grid, ms, (unsigned long)esc);
	}
	return VG_OK;
}

extern "C" int vg_cprior_calls(vg_cprior *cp, uint32_t sample, uint8_t *gt, int32_t *gq)
{
	if (!cp || ((!gt || !gq) && cp->n_sites)) return fail(VG_EINVAL, "null argument");
	if (sample >= cp->n_samples) return fail(VG_EINVAL, "vg_cprior_calls: sample %s is out of range", std::to_string(sample).c_str());
	if (!cp->ran) return fail(VG_EINVAL, "vg_cprior_calls: no vg_cprior_run since the handle was made or a sample was set");
	const uint64_t n = cp->n_sites;
	if (n == 0) return VG_OK;
	return guarded([&]() -> int {
		HIP_TRY(hipSetDevice(cp->device));
		std::vector<uint16_t> code((size_t)n), cnt;
		HIP_TRY(hipMemcpyAsync(code.data(), cp->d_calls + (uint64_t)sample * n, n * sizeof(uint16_t), hipMemcpyDeviceToHost, cp->stream));
		HIP_TRY(hipStreamSynchronize(cp->stream));
		const vg_caller_tables &t = host_call_tables();
		for (uint64_t s = 0; s < n; s++) {
			gt[s] = (uint8_t)(code[s] >> 14);
			gq[s] = code[s] & VG_CALL_ESCAPE;
			if (gq[s] != VG_CALL_ESCAPE) continue;
			if (cnt.empty()) {                                        // the first escaped entry of the column: its counter words, once
				cnt.resize((size_t)n);
				HIP_TRY(hipMemcpyAsync(cnt.data(), cp->d_cnt + (uint64_t)sample * n, n * sizeof(uint16_t), hipMemcpyDeviceToHost, cp->stream));
				HIP_TRY(hipStreamSynchronize(cp->stream));
			}
			const vg_site_call c = vg_cprior_call(t, vg_cprior_hw_at(cp->q[s]), cnt[s]);      // the same function over the same q: the same bits up to the logarithm
			gt[s] = c.gt;
			gq[s] = c.gt == VGC_NONE ? 0 : vg_genotype_quality(c.confidence);
		}
		return VG_OK;
	});
}

extern "C" int vg_cprior_host(const uint8_t *ref_cnt, const uint8_t *alt_cnt, uint64_t n_sites, uint32_t n_samples, const uint8_t *ref_freq, const uint8_t *alt_freq, int iters, double pseudo, int threads,
                              uint8_t *gt, int32_t *gq, double *q_out)
{
	if ((!ref_cnt || !alt_cnt || !ref_freq || !alt_freq || !gt || !gq) && n_sites) return fail(VG_EINVAL, "null argument");
	if (n_samples == 0) return fail(VG_EINVAL, "vg_cprior_host: no samples");
	if (n_sites >= (1ull << 32)) return fail(VG_EINVAL, "vg_cprior_host: 2^32 sites or more");
	if (n_samples > VG_CPRIOR_MAX_SAMPLES) return fail(VG_ETOOBIG, "vg_cprior_host: more than %s samples", std::to_string(VG_CPRIOR_MAX_SAMPLES).c_str());
	if (int rc = cprior_check_rule("vg_cprior_host", iters, pseudo)) return rc;
	return guarded([&]() -> int {
		vg_cprior_host_run(ref_cnt, alt_cnt, n_sites, n_samples, ref_freq, alt_freq, iters, pseudo, threads, gt, gq, q_out);
		return VG_OK;
	});
}

// ---- the joint VCF's data lines rendered on the device (vg_jtext.h; no reference counterpart) -------------------------------------
// A vg_jtext holds, on one device, the calls of n_samples samples in SAMPLE-MAJOR columns and every buffer a span of records needs.
//   narrow[sample][site]   uint16: gt << 14 | gq, the word vg_sample_calls_fetch moves, when 0 <= gq <= 16382; gt << 14 | 16383 says
//                          "the gq is in the sample's wide column"; 0: no call.  2 bytes per site and sample
//   wide[slot][site]       int32 gq, one column per sample that has a gq outside 0 .. 16382 (wide_slot[sample], -1: none); create
//                          takes `wide_samples` of them
// Sample-major makes vg_jtext_set one stream (a column arrives, a column is written) and the render a gather: a wave reads 64
// samples' words of one site, 64 addresses n_sites * 2 bytes apart.  Site-major would make the render's reads one 128-byte line and
// set a scatter.  No measurement supports the choice yet.
//
// A span of R records is P = G + 1 PIECES per record, G = ceil(n_samples / 64): piece 0 is the head and "\tGT:GQ", piece 1 + g the
// cells of samples [64 g, 64 g + 64) -- the last one with the line's "\n".  Three steps:
//   vg_jt_len_kernel      one wave per (record, group), one lane per sample: the lane's call (vg_jt_pick over the record's sites),
//                         its cell's length, the wave's sum and -- ballot + popcount -- how many lanes show a call, a het, a hom; on a
//                         handle of the INFO mode group 0's wave also finds the head's splice kind
//   vg_jt_settle_kernel   one lane per record: sums the groups' counts into the record's NS, het, hom (12 bytes per record, also what
//                         vg_jtext_counts hands out); a record with NS 0 gets length 0 in every piece; the others their head piece's
//                         length -- the head, its splice (vg_jt_head_piece_len), "\tGT:GQ" -- and the newline; counts the lines
//   vg_jt_scan_*          exclusive scan of the R * P lengths to 64-bit byte offsets: per-block sums, one block over the sums, apply
//   vg_jt_write_kernel    TILED BY OUTPUT BYTES: a workgroup owns JT_TILE bytes of the output buffer at a dword-aligned address, finds
//                         the pieces that overlap them by bisection of the offsets, composes them in LDS -- a wave per piece: a head is
//                         a 64-byte-per-step copy, a group is one lane per sample, the cell's place a wave scan of the lengths -- and
//                         leaves as aligned dword stores.  A line or a head longer than a tile simply spans several workgroups.  The
//                         text may start at any byte of the buffer (the BGZF stream appends to pending text): the workgroup that owns
//                         the dword the text starts in loads that dword into LDS first, so the bytes in front are written back as
//                         they were; no other dword is shared.  The bytes after the end of the text in its last dword are unspecified
// ------------------------------------------------------------------------------------------------
constexpr uint32_t JT_TILE = 16384, JT_SCAN_ITEMS = 16, JT_SCAN_BLOCK = 256 * JT_SCAN_ITEMS;
constexpr uint32_t VG_JTEXT_MAX_SAMPLES = 16384;
constexpr uint64_t JT_CHUNK_TEXT = 16ull << 20, JT_CHUNK_BLOCKS = 16384;      // the stream's deflate work buffers: a chunk of blocks

struct JtStore {
	const uint16_t *narrow; const int32_t *wide; const int32_t *wide_slot;
	uint64_t n_sites; uint32_t n_samples;
};
// the call of `sample` at `site` as vg_jt_pick wants it: gt << 32 | (uint32_t)gq
__device__ __forceinline__ uint64_t jt_call(const JtStore &st, uint32_t sample, int32_t slot, uint32_t site)
{
	const uint32_t w = st.narrow[(uint64_t)sample * st.n_sites + site];
	uint32_t gq = w & 0x3fffu;
	if (gq == VG_JT_GQ_ESCAPE && slot >= 0) gq = (uint32_t)st.wide[(uint64_t)slot * st.n_sites + site];
	return (uint64_t)(w >> 14) << 32 | gq;
}
// *shown: the gt of the call the sample shows for the record (0: none, also for a lane beyond the samples)
__device__ __forceinline__ vg_jt_cell_t jt_lane_cell(const JtStore &st, uint32_t sample, const uint32_t *sites, uint32_t n, uint32_t *shown)
{
	uint64_t v = 0;
	if (sample < st.n_samples) {
		const int32_t slot = st.wide_slot[sample];
		v = vg_jt_pick(sites, n, [&](uint32_t site) { return jt_call(st, sample, slot, site); });
	}
	*shown = (uint32_t)(v >> 32);
	vg_jt_cell_t c = vg_jt_cell((uint32_t)(v >> 32), (int32_t)(uint32_t)v);
	if (sample >= st.n_samples) c.len = 0;
	return c;
}

// one sample's columns -> its narrow column, and its wide one if it has a slot (wide != nullptr)
__global__ __launch_bounds__(256) void vg_jt_pack_kernel(const uint8_t *__restrict__ gt, const int32_t *__restrict__ gq, uint64_t n_sites, uint16_t *__restrict__ narrow, int32_t *__restrict__ wide)
{
	for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n_sites; i += (uint64_t)gridDim.x * 256) {
		const uint32_t g = gt[i];
		const int32_t q = gq[i];
		const bool fits = q >= 0 && q < (int32_t)VG_JT_GQ_ESCAPE;
		narrow[i] = g ? (uint16_t)(g << 14 | (fits ? (uint32_t)q : VG_JT_GQ_ESCAPE)) : (uint16_t)0;
		if (wide) wide[i] = g ? q : 0;
	}
}

// A group's word between the length kernel and the settle kernel: the cells' length sum (at most 64 * 16: 11 bits) and, 7 bits each,
// how many of the 64 shown calls are called, het and hom.
constexpr uint32_t JT_SUM_BITS = 11, JT_CNT_BITS = 7, JT_CNT_MASK = (1u << JT_CNT_BITS) - 1;
static_assert(64 * VG_JT_CELL_MAX < (1u << JT_SUM_BITS) && JT_SUM_BITS + 3 * JT_CNT_BITS == 32, "the group word holds a length sum and three counts of up to 64");
constexpr uint32_t JT_KIND_SHIFT = 30;                                     // a record's splice kind rides on its NS word (NS <= 16 384) on the device

// info != 0: group 0's wave also reads the record's head, 64 bytes a step, for its splice kind (vg_jt_splice: the number of tabs and
// the last two bytes) and leaves it in the head piece's slot, which the settle kernel replaces by the piece's length.
__global__ __launch_bounds__(256) void vg_jt_len_kernel(JtStore st, const uint8_t *__restrict__ heads, const vg_jtext_record *__restrict__ recs, uint64_t n_records, const uint32_t *__restrict__ sites, uint32_t G, int info,
                                                        uint32_t *__restrict__ len)
{
	const uint32_t lane = threadIdx.x & 63;
	const uint64_t u = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);          // (the same for a wave's lanes)
	if (u >= n_records * G) return;
	const uint64_t r = u / G;
	const uint32_t g = (uint32_t)(u % G);
	const vg_jtext_record rec = recs[r];
	uint32_t shown;
	const vg_jt_cell_t c = jt_lane_cell(st, g * 64 + lane, sites + rec.site_at, rec.n_sites, &shown);
	uint32_t sum = c.len;
	for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
	const uint32_t called = (uint32_t)__popcll(__ballot(vg_jt_is_called(shown))), het = (uint32_t)__popcll(__ballot(vg_jt_is_het(shown))), hom = (uint32_t)__popcll(__ballot(vg_jt_is_hom(shown)));
	if (lane == 0) len[r * (G + 1) + 1 + g] = sum | called << JT_SUM_BITS | het << (JT_SUM_BITS + JT_CNT_BITS) | hom << (JT_SUM_BITS + 2 * JT_CNT_BITS);
	if (g != 0) return;
	uint32_t kind = VG_JT_SPLICE_NONE;
	if (info == VG_JT_INFO_COUNTS && rec.head_len) {
		const uint8_t *h = heads + rec.head_off;
		uint64_t tabs = 0;
		for (uint32_t base = 0; base < rec.head_len; base += 64) {          // (base is the wave's: every lane takes every step)
			const uint32_t j = base + lane;
			tabs += (uint64_t)__popcll(__ballot(j < rec.head_len && h[j] == '\t'));
		}
		kind = vg_jt_splice(tabs, rec.head_len, h[rec.head_len - 1], rec.head_len > 1 ? h[rec.head_len - 2] : 0u);
	}
	if (lane == 0) len[r * (G + 1)] = kind;
}

// counts[r]: the record's NS (with its splice kind above JT_KIND_SHIFT), het and hom; zeros for a record that produces no line
__global__ __launch_bounds__(256) void vg_jt_settle_kernel(const vg_jtext_record *__restrict__ recs, uint64_t n_records, uint32_t G, uint32_t *__restrict__ len, uint32_t *__restrict__ counts, unsigned long long *__restrict__ n_lines)
{
	const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	bool line = false;
	if (r < n_records) {
		uint32_t *p = len + r * (G + 1);
		uint32_t ns = 0, het = 0, hom = 0;
		for (uint32_t g = 0; g < G; g++) {
			const uint32_t w = p[1 + g];
			ns += w >> JT_SUM_BITS & JT_CNT_MASK; het += w >> (JT_SUM_BITS + JT_CNT_BITS) & JT_CNT_MASK; hom += w >> (JT_SUM_BITS + 2 * JT_CNT_BITS);
		}
		line = ns != 0;
		const uint32_t kind = p[0];
		p[0] = line ? vg_jt_head_piece_len(kind, recs[r].head_len, ns, het, hom) : 0u;
		for (uint32_t g = 0; g < G; g++) p[1 + g] = line ? (p[1 + g] & ((1u << JT_SUM_BITS) - 1)) + (g + 1 == G ? 1u : 0u) : 0u;
		counts[3 * r] = line ? ns | kind << JT_KIND_SHIFT : 0u; counts[3 * r + 1] = line ? het : 0u; counts[3 * r + 2] = line ? hom : 0u;
	}
	const unsigned long long votes = __ballot(line);
	if ((threadIdx.x & 63) == 0 && votes) atomicAdd(n_lines, (unsigned long long)__popcll(votes));
}

// exclusive scan of len[0, n) into off[0, n], off[n] = the total: a thread owns JT_SCAN_ITEMS consecutive items
__device__ __forceinline__ uint64_t jt_block_exclusive(uint64_t mine, uint64_t *lds /* 256 */, uint64_t *total)
{
	const unsigned t = threadIdx.x;
	lds[t] = mine;
	__syncthreads();
	for (unsigned o = 1; o < 256; o <<= 1) {
		const uint64_t y = t >= o ? lds[t - o] : 0;
		__syncthreads();
		lds[t] += y;
		__syncthreads();
	}
	const uint64_t incl = lds[t];
	*total = lds[255];
	__syncthreads();
	return incl - mine;
}
__global__ __launch_bounds__(256) void vg_jt_scan_sums_kernel(const uint32_t *__restrict__ len, uint64_t n, uint64_t *__restrict__ bsum)
{
	__shared__ uint64_t lds[256];
	const uint64_t base = (uint64_t)blockIdx.x * JT_SCAN_BLOCK + (uint64_t)threadIdx.x * JT_SCAN_ITEMS;
	uint64_t s = 0;
	for (uint32_t i = 0; i < JT_SCAN_ITEMS; i++) if (base + i < n) s += len[base + i];
	uint64_t total;
	(void)jt_block_exclusive(s, lds, &total);
	if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}
// one workgroup: bsum[0, nb) -> its exclusive scan in place, the total to bsum[nb] and off_total
__global__ __launch_bounds__(256) void vg_jt_scan_top_kernel(uint64_t *__restrict__ bsum, uint64_t nb, uint64_t *__restrict__ off_total)
{
	__shared__ uint64_t lds[256];
	uint64_t carry = 0;
	for (uint64_t c = 0; c < nb; c += 256) {
		const uint64_t i = c + threadIdx.x;
		const uint64_t v = i < nb ? bsum[i] : 0;
		uint64_t total;
		const uint64_t ex = jt_block_exclusive(v, lds, &total);
		if (i < nb) bsum[i] = carry + ex;
		carry += total;
	}
	if (threadIdx.x == 0) { bsum[nb] = carry; *off_total = carry; }
}
__global__ __launch_bounds__(256) void vg_jt_scan_apply_kernel(const uint32_t *__restrict__ len, uint64_t n, const uint64_t *__restrict__ bsum, uint64_t *__restrict__ off)
{
	__shared__ uint64_t lds[256];
	const uint64_t base = (uint64_t)blockIdx.x * JT_SCAN_BLOCK + (uint64_t)threadIdx.x * JT_SCAN_ITEMS;
	uint32_t v[JT_SCAN_ITEMS];
	uint64_t s = 0;
#pragma unroll
	for (uint32_t i = 0; i < JT_SCAN_ITEMS; i++) { v[i] = base + i < n ? len[base + i] : 0u; s += v[i]; }
	uint64_t total;
	uint64_t at = bsum[blockIdx.x] + jt_block_exclusive(s, lds, &total);
#pragma unroll
	for (uint32_t i = 0; i < JT_SCAN_ITEMS; i++) { if (base + i < n) off[base + i] = at; at += v[i]; }
}

// out: the dword-aligned output buffer; the span's text goes to out[start, start + off[n_items]).  grid: the tiles from the dword
// that holds byte `start` on (the host sizes it by the span's bound; a tile beyond the text returns)
__global__ __launch_bounds__(256) void vg_jt_write_kernel(JtStore st, const uint8_t *__restrict__ heads, const vg_jtext_record *__restrict__ recs, const uint32_t *__restrict__ sites, uint32_t G,
                                                          const uint32_t *__restrict__ len, const uint64_t *__restrict__ off, const uint32_t *__restrict__ counts, uint64_t n_items, uint8_t *out, uint64_t start)
{
	__shared__ uint32_t tile[JT_TILE / 4];
	uint8_t *const tb = (uint8_t *)tile;
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, P = G + 1;
	const uint64_t end_abs = start + off[n_items];
	const uint64_t A = (start & ~3ull) + (uint64_t)blockIdx.x * JT_TILE;       // the tile: bytes [A, A + JT_TILE) of out
	if (A >= end_abs) return;
	// the part of the text this tile holds, as text offsets [lo, hi); a text offset x lies at tile byte x - shift
	const uint64_t lo = (A > start ? A : start) - start, hi = (A + JT_TILE < end_abs ? A + JT_TILE : end_abs) - start;
	const int64_t shift = (int64_t)A - (int64_t)start;
	if (A < start && threadIdx.x == 0) tile[0] = *(const uint32_t *)(out + A);   // bytes of earlier text in the first dword stay as they are
	uint64_t a = 0, b = n_items;                                              // the first piece that ends behind lo
	while (a < b) { const uint64_t m = a + ((b - a) >> 1); if (off[m + 1] > lo) b = m; else a = m + 1; }
	__syncthreads();
	for (uint64_t p = a + wave; p < n_items; p += 4) {                          // a piece per wave and step
		const uint64_t o = off[p];
		if (o >= hi) break;
		const uint32_t n = len[p];
		if (!n) continue;
		const uint64_t r = p / P;
		const uint32_t k = (uint32_t)(p % P);
		const vg_jtext_record rec = recs[r];
		if (k == 0) {
			// the head piece: `keep` bytes of the head, the splice (";" if the INFO goes on, the tag), "\tGT:GQ" -- without a splice
			// keep = head_len and tag_at = fmt_at.  Bytes [j0, j1) of the piece are this tile's
			const uint64_t j0 = lo > o ? lo - o : 0, j1 = hi - o < n ? hi - o : n;
			const uint8_t *h = heads + rec.head_off;
			const uint32_t ns_word = counts[3 * r], kind = ns_word >> JT_KIND_SHIFT;
			const uint32_t keep = vg_jt_splice_keep(kind, rec.head_len), tag_at = keep + vg_jt_splice_sep(kind), fmt_at = n - 6;
			for (uint64_t j = j0 + lane; j < j1; j += 64) {
				if (j >= tag_at && j < fmt_at) continue;                        // the tag's bytes: below
				const uint32_t v = j < keep ? h[j] : j < tag_at ? (uint32_t)';' : (uint32_t)(0x51473a544709ull >> (8 * (j - fmt_at))) & 0xffu;
				tb[(int64_t)(o + j) - shift] = (uint8_t)v;
			}
			if (lane == 0 && tag_at < fmt_at && j0 < fmt_at && j1 > tag_at)   // one lane prints the tag, a byte at a time, where the tile holds it
				(void)vg_jt_tag(ns_word & ((1u << JT_KIND_SHIFT) - 1), counts[3 * r + 1], counts[3 * r + 2], [&](uint32_t i, uint32_t byte) {
					const uint64_t j = (uint64_t)tag_at + i;
					if (j >= j0 && j < j1) tb[(int64_t)(o + j) - shift] = (uint8_t)byte;
				});
		} else {
			const uint32_t g = k - 1;
			uint32_t shown;
			const vg_jt_cell_t c = jt_lane_cell(st, g * 64 + lane, sites + rec.site_at, rec.n_sites, &shown);
			uint32_t incl = c.len;
			for (int s = 1; s < 64; s <<= 1) { const uint32_t y = __shfl_up(incl, s); if ((int)lane >= s) incl += y; }
			const uint64_t at = o + incl - c.len;                               // the cell's text offset
			for (uint32_t i = 0; i < c.len; i++) {
				const uint64_t x = at + i;
				if (x >= lo && x < hi) tb[(int64_t)x - shift] = (uint8_t)vg_jt_byte(c, i);
			}
			if (g + 1 == G && lane == 0) { const uint64_t x = o + n - 1; if (x >= lo && x < hi) tb[(int64_t)x - shift] = '\n'; }
		}
	}
	__syncthreads();
	const uint32_t n_dw = (uint32_t)(((int64_t)hi - shift + 3) / 4);
	uint32_t *dst = (uint32_t *)(out + A);
	for (uint32_t i = threadIdx.x; i < n_dw; i += 256) dst[i] = tile[i];       // 1 KiB of the tile per step
}

// ------------------------------------------------------------------------------------------------
// The tabix index of a BGZF VCF (vg_vcfidx.h has the rules, the host scanner, the builder and the serialiser).  The kernels scan
// WHOLE LINES that are resident on the device, text[0, n) with text[n - 1] == '\n', into the header's records:
//   vg_vi_count_kernel    newlines per tile of VI_TILE bytes: a wave takes 64 bytes per step, ballot + popcount
//   (vg_jt_scan_*)        the counts' exclusive scan, 64-bit: where a tile's newlines go in the newline array
//   vg_vi_starts_kernel   nl[i] = offset of the i-th '\n': line i is text[nl[i - 1] + 1, nl[i])
//   vg_vi_parse_kernel    a lane per line: vg_vi_parse (a long REF is a long loop of one lane: slow, not wrong)
//   vg_vi_heads_kernel    a lane per line: does it open a record (flag), is its CHROM that of the line before it (same)
//   (vg_jt_scan_*)        the flags' exclusive scan: the record a line belongs to
//   vg_vi_emit_kernel     a record's first line writes its start and first facts, its last line the end: plain stores, no atomics
// What crosses the link is the records -- a run of lines in one 16 kb window is one -- and, on the joint text route, the CHROM
// bytes of the few records whose `same` bit is clear.
// ------------------------------------------------------------------------------------------------
constexpr uint32_t VI_TILE = 4096, VI_STEPS = VI_TILE / 256;             // 4 waves, 1 KiB each

// the newlines of this wave's KiB (wave-uniform), and in wsum[] those of the workgroup's four waves
__device__ __forceinline__ uint32_t vi_wave_count(const uint8_t *__restrict__ text, uint64_t n, uint64_t base, uint32_t lane, uint32_t wave, uint32_t *wsum)
{
	uint32_t c = 0;
	for (uint32_t s = 0; s < VI_STEPS; s++) {
		const uint64_t i = base + (uint64_t)s * 64 + lane;
		c += (uint32_t)__popcll(__ballot(i < n && text[i] == '\n'));
	}
	if (lane == 0) wsum[wave] = c;
	__syncthreads();
	return c;
}
__global__ __launch_bounds__(256) void vg_vi_count_kernel(const uint8_t *__restrict__ text, uint64_t n, uint32_t *__restrict__ cnt)
{
	__shared__ uint32_t wsum[4];
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	(void)vi_wave_count(text, n, (uint64_t)blockIdx.x * VI_TILE + (uint64_t)wave * (VI_TILE / 4), lane, wave, wsum);
	if (threadIdx.x == 0) cnt[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}
// off: the exclusive scan of cnt; nl holds off[tiles] entries
__global__ __launch_bounds__(256) void vg_vi_starts_kernel(const uint8_t *__restrict__ text, uint64_t n, const uint64_t *__restrict__ off, uint64_t n_lines, uint64_t *__restrict__ nl)
{
	__shared__ uint32_t wsum[4];
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint64_t base = (uint64_t)blockIdx.x * VI_TILE + (uint64_t)wave * (VI_TILE / 4);
	(void)vi_wave_count(text, n, base, lane, wave, wsum);
	uint64_t at = off[blockIdx.x];
	for (uint32_t w = 0; w < wave; w++) at += wsum[w];
	for (uint32_t s = 0; s < VI_STEPS; s++) {
		const uint64_t i = base + (uint64_t)s * 64 + lane;
		const bool is_nl = i < n && text[i] == '\n';
		const uint64_t m = __ballot(is_nl);
		const uint64_t slot = at + (uint64_t)__popcll(m & ((1ull << lane) - 1));
		if (is_nl && slot < n_lines) nl[slot] = i;
		at += (uint64_t)__popcll(m);
	}
}
__global__ __launch_bounds__(256) void vg_vi_parse_kernel(const uint8_t *__restrict__ text, const uint64_t *__restrict__ nl, uint64_t n_lines, vg_vi_line *__restrict__ lines)
{
	const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= n_lines) return;
	const uint64_t a = i ? nl[i - 1] + 1 : 0;
	lines[i] = vg_vi_parse(text + a, nl[i] - a);
}
__global__ __launch_bounds__(256) void vg_vi_heads_kernel(const uint8_t *__restrict__ text, const uint64_t *__restrict__ nl, uint64_t n_lines, const vg_vi_line *__restrict__ lines,
                                                          uint32_t *__restrict__ flag, uint32_t *__restrict__ same)
{
	const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= n_lines) return;
	const vg_vi_line cur = lines[i];
	uint32_t f = 0, sm = 0;
	if (cur.kind != VG_VI_SKIP) {
		f = 1;
		if (i && cur.kind == VG_VI_DATA) {
			const vg_vi_line prev = lines[i - 1];
			if (prev.kind == VG_VI_DATA && prev.clen == cur.clen) {
				const uint8_t *p = text + (i > 1 ? nl[i - 2] + 1 : 0), *q = text + nl[i - 1] + 1;
				uint32_t k = 0;
				while (k < cur.clen && p[k] == q[k]) k++;
				sm = k == cur.clen;
			}
			if (vg_vi_joins(prev, cur, sm != 0)) f = 0;
		}
	}
	flag[i] = f; same[i] = sm;
}
// roff: the exclusive scan of flag; recs holds roff[n_lines] records
__global__ __launch_bounds__(256) void vg_vi_emit_kernel(const uint64_t *__restrict__ nl, uint64_t n_lines, const vg_vi_line *__restrict__ lines, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ same,
                                                         const uint64_t *__restrict__ roff, uint64_t n_recs, uint64_t base, vg_vi_rec *__restrict__ recs)
{
	const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= n_lines) return;
	const vg_vi_line cur = lines[i];
	if (cur.kind == VG_VI_SKIP) return;
	const uint32_t f = flag[i];
	const uint64_t r = roff[i] + f - 1;                                      // (a line that joins has a record before it: roff[i] >= 1)
	if (r >= n_recs) return;
	if (f) {
		recs[r].start = base + (i ? nl[i - 1] + 1 : 0);
		recs[r].first_line = (uint32_t)i; recs[r].beg_first = cur.beg; recs[r].end_first = cur.end; recs[r].clen = cur.clen; recs[r].kind = cur.kind; recs[r].same = same[i];
	}
	const bool last = i + 1 == n_lines || lines[i + 1].kind == VG_VI_SKIP || flag[i + 1] != 0;
	if (last) { recs[r].end = base + nl[i] + 1; recs[r].last_line = (uint32_t)i; recs[r].beg_last = cur.beg; }
}

struct vg_vcfidx : VgVcfIdx {
	// the scan's device buffers: grow-only, on the device that scanned last
	int scratch_device = -1;
	DevBuf<uint8_t> d_text;
	DevBuf<uint32_t> d_cnt, d_flag, d_same;
	DevBuf<uint64_t> d_off, d_bsum, d_nl, d_roff;
	DevBuf<vg_vi_line> d_lines;
	DevBuf<vg_vi_rec> d_recs;
	hipEvent_t e0 = nullptr, e1 = nullptr;
	std::vector<uint8_t> name;                       // a record's CHROM bytes fetched from the device
	void release()
	{
		d_text.release(); d_cnt.release(); d_flag.release(); d_same.release(); d_off.release(); d_bsum.release(); d_nl.release(); d_roff.release(); d_lines.release(); d_recs.release();
		if (e0) (void)hipEventDestroy(e0);
		if (e1) (void)hipEventDestroy(e1);
		e0 = e1 = nullptr;
	}
};

// len[0, n) -> its exclusive scan off[0, n], 64-bit (the joint text's three scan kernels); bsum holds n / JT_SCAN_BLOCK + 2 entries
static int vi_exclusive(const uint32_t *len, uint64_t n, uint64_t *bsum, uint64_t *off)
{
	const uint64_t nb = (n + JT_SCAN_BLOCK - 1) / JT_SCAN_BLOCK;
	vg_jt_scan_sums_kernel<<<(unsigned)nb, 256>>>(len, n, bsum);
	HIP_TRY(hipGetLastError());
	vg_jt_scan_top_kernel<<<1, 256>>>(bsum, nb, off + n);
	HIP_TRY(hipGetLastError());
	vg_jt_scan_apply_kernel<<<(unsigned)nb, 256>>>(len, n, bsum, off);
	HIP_TRY(hipGetLastError());
	return VG_OK;
}

// The records of the whole lines d[0, n) (device memory of the current device; n == 0 or d[n - 1] == '\n'), text offset `base`,
// appended to out.  Nothing of the handle but its scratch buffers changes.  Default stream, synchronous.
static int vi_scan_resident(vg_vcfidx *ix, int device, const uint8_t *d, uint64_t n, uint64_t base, std::vector<vg_vi_rec> &out)
{
	if (!n) return VG_OK;
	if (ix->scratch_device != device) { ix->release(); ix->scratch_device = device; }
	const uint64_t tiles = (n + VI_TILE - 1) / VI_TILE;
	if (tiles >= (1ull << 31)) return fail(VG_ETOOBIG, "the index scan takes less than 8 TiB of text per piece");
	int rc;
	if ((rc = ix->d_cnt.reserve(tiles, "newline counts")) || (rc = ix->d_off.reserve(tiles + 1, "newline offsets")) || (rc = ix->d_bsum.reserve(tiles / JT_SCAN_BLOCK + 2, "the scan's sums"))) return rc;
	const bool timed = getenv("VG_VERBOSE") != nullptr;
	if (timed && !ix->e0) { HIP_TRY(hipEventCreate(&ix->e0)); HIP_TRY(hipEventCreate(&ix->e1)); }
	if (timed) HIP_TRY(hipEventRecord(ix->e0, nullptr));
	vg_vi_count_kernel<<<(unsigned)tiles, 256>>>(d, n, ix->d_cnt.p);
	HIP_TRY(hipGetLastError());
	if ((rc = vi_exclusive(ix->d_cnt.p, tiles, ix->d_bsum.p, ix->d_off.p))) return rc;
	uint64_t L = 0, R = 0;
	HIP_TRY(hipMemcpy(&L, ix->d_off.p + tiles, 8, hipMemcpyDeviceToHost));
	if (L > n) return fail(VG_EIO, "the index scan counted more lines than bytes");
	if (L >= (1ull << 32)) return fail(VG_ETOOBIG, "the index scan takes less than 2^32 lines per piece");
	if (L) {
		if ((rc = ix->d_nl.reserve(L, "line ends")) || (rc = ix->d_lines.reserve(L, "parsed lines")) || (rc = ix->d_flag.reserve(L, "record flags")) || (rc = ix->d_same.reserve(L, "chromosome bits"))
		    || (rc = ix->d_roff.reserve(L + 1, "record offsets")) || (rc = ix->d_bsum.reserve(L / JT_SCAN_BLOCK + 2, "the scan's sums"))) return rc;
		const unsigned grid = (unsigned)((L + 255) / 256);
		vg_vi_starts_kernel<<<(unsigned)tiles, 256>>>(d, n, ix->d_off.p, L, ix->d_nl.p);
		HIP_TRY(hipGetLastError());
		vg_vi_parse_kernel<<<grid, 256>>>(d, ix->d_nl.p, L, ix->d_lines.p);
		HIP_TRY(hipGetLastError());
		vg_vi_heads_kernel<<<grid, 256>>>(d, ix->d_nl.p, L, ix->d_lines.p, ix->d_flag.p, ix->d_same.p);
		HIP_TRY(hipGetLastError());
		if ((rc = vi_exclusive(ix->d_flag.p, L, ix->d_bsum.p, ix->d_roff.p))) return rc;
		HIP_TRY(hipMemcpy(&R, ix->d_roff.p + L, 8, hipMemcpyDeviceToHost));
		if (R > L) return fail(VG_EIO, "the index scan counted more records than lines");
		if (R) {
			if ((rc = ix->d_recs.reserve(R, "index records"))) return rc;
			vg_vi_emit_kernel<<<grid, 256>>>(ix->d_nl.p, L, ix->d_lines.p, ix->d_flag.p, ix->d_same.p, ix->d_roff.p, R, base, ix->d_recs.p);
			HIP_TRY(hipGetLastError());
		}
	}
	float ms = 0;
	if (timed) { HIP_TRY(hipEventRecord(ix->e1, nullptr)); HIP_TRY(hipEventSynchronize(ix->e1)); HIP_TRY(hipEventElapsedTime(&ms, ix->e0, ix->e1)); }
	if (R) {
		const size_t at = out.size();
		out.resize(at + (size_t)R);
		HIP_TRY(hipMemcpy(out.data() + at, ix->d_recs.p, (size_t)R * sizeof(vg_vi_rec), hipMemcpyDeviceToHost));
	} else HIP_TRY(hipDeviceSynchronize());
	if (timed) fprintf(stderr, "[vargeno_hip] vcf index scan: %lu bytes, %lu lines, %lu records, %.3f ms kernels (%.2f GB/s text, incl. two counts' round trips)\n", (unsigned long)n, (unsigned long)L, (unsigned long)R, ms, ms > 0 ? n / 1e6 / ms : 0.0);
	return VG_OK;
}

extern "C" int vg_vcfidx_create(uint32_t block, vg_vcfidx **out)
{
	if (!out) return fail(VG_EINVAL, "null argument");
	*out = nullptr;
	if (block > VG_BGZF_TEXT_BLOCK) return fail(VG_EINVAL, "a BGZF block holds at most 65280 bytes of text here");
	return guarded([&]() -> int {
		vg_vcfidx *ix = new vg_vcfidx;
		ix->B = block ? block : VG_BGZF_TEXT_BLOCK;
		*out = ix;
		return VG_OK;
	});
}
extern "C" void vg_vcfidx_destroy(vg_vcfidx *idx)
{
	if (!idx) return;
	idx->release();
	(void)hipGetLastError();
	delete idx;
}
extern "C" int vg_vcfidx_text_host(vg_vcfidx *idx, const uint8_t *text, uint64_t n, int threads)
{
	if (!idx || (!text && n)) return fail(VG_EINVAL, "null argument");
	return guarded([&]() -> int {
		const double t0 = now_s();
		(void)idx->feed_host(text, n, threads);
		idx->seconds += now_s() - t0;
		return VG_OK;
	});
}
extern "C" int vg_vcfidx_text_device(vg_vcfidx *idx, int device, const uint8_t *text, uint64_t n)
{
	if (!idx || (!text && n)) return fail(VG_EINVAL, "null argument");
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return fail(VG_ENODEV, "no HIP device available (vg_vcfidx_text_host is the host's scanner)"); }
	return guarded([&]() -> int {
		HIP_TRY(hipSetDevice(device));
		const double t0 = now_s();
		// whole lines go up in pieces of about 64 MiB that end behind a '\n'
		const int rc = idx->feed(text, n, [&](uint64_t off, uint64_t len, std::vector<vg_vi_rec> &out) -> int {
			const uint64_t piece = 64ull << 20, end = off + len;
			for (uint64_t a = off; a < end;) {
				uint64_t b = std::min(end, a + piece);
				if (b < end) {
					while (b > a && text[b - 1] != '\n') b--;
					if (b == a) { const uint8_t *q = (const uint8_t *)memchr(text + a + piece, '\n', (size_t)(end - a - piece)); b = q ? (uint64_t)(q - text) + 1 : end; }
				}
				if (idx->scratch_device != device) { idx->release(); idx->scratch_device = device; }
				int r = idx->d_text.reserve(b - a + 16, "text");
				if (r) return r;
				HIP_TRY(hipMemcpy(idx->d_text.p, text + a, b - a, hipMemcpyHostToDevice));
				if ((r = vi_scan_resident(idx, device, idx->d_text.p, b - a, idx->fed + a, out))) return r;
				a = b;
			}
			return VG_OK;
		});
		idx->seconds += now_s() - t0;
		return rc;
	});
}
extern "C" int vg_vcfidx_bgzf(vg_vcfidx *idx, const uint8_t *bgzf, uint64_t n)
{
	if (!idx || (!bgzf && n)) return fail(VG_EINVAL, "null argument");
	return guarded([&]() -> int {
		if (!idx->feed_bgzf(bgzf, n)) return fail(VG_EINVAL, "vg_vcfidx_bgzf: the bytes are not whole BGZF blocks");
		return VG_OK;
	});
}
static int vi_fused_chunk(vg_vcfidx *idx, const uint8_t *d_text, const uint8_t *text, uint64_t tn)
{
	int device = 0;
	HIP_TRY(hipGetDevice(&device));
	const double t0 = now_s();
	const int rc = idx->feed(text, tn, [&](uint64_t off, uint64_t len, std::vector<vg_vi_rec> &out) -> int {
		const int r = vi_scan_resident(idx, device, d_text + off, len, idx->fed + off, out);
		if (r != VG_ENOMEM) return r;
		// no device memory for the scan's buffers: the host has this chunk's text
		if (getenv("VG_VERBOSE")) fprintf(stderr, "[vargeno_hip] vcf index scan: no device memory (%s): this chunk is scanned on the host\n", vg_last_error());
		out.clear();
		vg_vi_scan_lines(text + off, len, idx->fed + off, out);
		return VG_OK;
	});
	idx->seconds += now_s() - t0;
	return rc;
}
static int vi_fused_blocks(vg_vcfidx *idx, const uint8_t *bgzf, uint64_t n)
{
	if (!idx->feed_bgzf(bgzf, n)) return fail(VG_EIO, "the index was handed bytes that are not whole BGZF blocks");
	return VG_OK;
}
extern "C" uint64_t vg_vcfidx_bound(const vg_vcfidx *idx) { return idx ? idx->raw_bytes() + (idx->carry.empty() ? 0 : idx->carry.size() + 1 + 8 * 4 + 2 * 24 + 32 + 8 * ((1u << 15) + 1)) : 0; }
extern "C" int vg_vcfidx_finish(vg_vcfidx *idx, uint8_t *tbi, uint64_t cap, uint64_t *len)
{
	if (!idx || !len || (!tbi && cap)) return fail(VG_EINVAL, "null argument");
	return guarded([&]() -> int {
		std::vector<uint8_t> raw;
		const int what = idx->serialise(raw);
		if (what == 1) return fail(VG_EINVAL, "the VCF cannot be indexed: %s (the line at text offset %s)", vg_vi_rule(idx->err), std::to_string(idx->err_at).c_str());
		if (what == 2) return fail(VG_EINVAL, "vg_vcfidx_finish: the BGZF blocks fed (%s) are not those of the text fed (%s)", std::to_string(idx->cstart.size()).c_str(), std::to_string(idx->blocks_of_text()).c_str());
		if (raw.size() > cap) return fail(VG_ETOOBIG, "the index does not fit the caller's buffer (vg_vcfidx_bound)");
		memcpy(tbi, raw.data(), raw.size());
		*len = raw.size();
		return VG_OK;
	});
}
extern "C" const char *vg_vcfidx_error(const vg_vcfidx *idx, uint64_t *offset)
{
	if (!idx || !idx->err) return nullptr;
	if (offset) *offset = idx->err_at;
	return vg_vi_rule(idx->err);
}
extern "C" int vg_vcfidx_stats(const vg_vcfidx *idx, uint64_t *out)
{
	if (!idx || !out) return fail(VG_EINVAL, "null argument");
	out[0] = idx->n_lines; out[1] = idx->tids.size(); out[2] = idx->n_bins; out[3] = idx->n_chunks; out[4] = (uint64_t)(idx->seconds * 1e6);
	return VG_OK;
}

struct vg_jtext {
	int device = 0;
	uint64_t n_sites = 0, rec_cap = 0, head_cap = 0, site_cap = 0, text_cap = 0, text_room = 0, dev_bytes = 0;
	uint32_t n_samples = 0, G = 0, wide_cap = 0;
	int info = VG_JT_INFO_NONE;                      // the mode of the handle's text (vg_jtext_create_info)
	uint16_t *d_narrow = nullptr;
	int32_t *d_wide = nullptr, *d_wide_slot = nullptr, *d_gq = nullptr;
	uint8_t *d_gt = nullptr, *d_heads = nullptr, *d_text = nullptr;
	vg_jtext_record *d_recs = nullptr;
	uint32_t *d_sites = nullptr, *d_len = nullptr, *d_counts = nullptr;
	uint64_t *d_off = nullptr, *d_bsum = nullptr;
	unsigned long long *d_lines = nullptr;
	std::vector<int32_t> wide_slot;                  // host mirror of d_wide_slot
	std::vector<uint8_t> slot_used;
	hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;
	// the BGZF stream
	bool with_bgzf = false, open = false, dyn = false;
	uint32_t B = 0;
	uint64_t pend = 0;                               // bytes of text in d_text that no block holds yet
	vg_vcfidx *idx = nullptr;                        // vg_jtext_bgzf_index: the index that follows the stream (not owned)
	uint32_t *d_slots = nullptr, *d_tok = nullptr;
	uint2 *d_meta = nullptr;
	uint64_t *d_boffs = nullptr;
	uint8_t *d_bout = nullptr;
	uint64_t bout_cap = 0;
	std::vector<uint2> h_meta;
	std::vector<uint64_t> h_boffs;
};

static void jtext_free(vg_jtext *jt)
{
	if (!jt) return;
	(void)hipSetDevice(jt->device);
	for (hipEvent_t e : {jt->ev0, jt->ev1, jt->ev2}) if (e) (void)hipEventDestroy(e);
	for (void *p : {(void *)jt->d_narrow, (void *)jt->d_wide, (void *)jt->d_wide_slot, (void *)jt->d_gq, (void *)jt->d_gt, (void *)jt->d_heads, (void *)jt->d_text, (void *)jt->d_recs, (void *)jt->d_sites,
	                (void *)jt->d_len, (void *)jt->d_counts, (void *)jt->d_off, (void *)jt->d_bsum, (void *)jt->d_lines, (void *)jt->d_slots, (void *)jt->d_tok, (void *)jt->d_meta, (void *)jt->d_boffs, (void *)jt->d_bout})
		if (p) (void)hipFree(p);
	(void)hipGetLastError();
	delete jt;
}

static bool jt_info_mode(int info) { return info == VG_JT_INFO_NONE || info == VG_JT_INFO_COUNTS; }
extern "C" uint64_t vg_jtext_text_bound(uint64_t head_bytes, uint64_t n_records, uint32_t n_samples) { return vg_jt_bound(head_bytes, n_records, n_samples); }
extern "C" uint64_t vg_jtext_text_bound_info(uint64_t head_bytes, uint64_t n_records, uint32_t n_samples, int info) { return jt_info_mode(info) ? vg_jt_bound_info(head_bytes, n_records, n_samples, info) : 0; }
extern "C" uint64_t vg_jtext_bgzf_bound(uint64_t text_bytes, uint32_t block)
{
	if (block > VG_BGZF_TEXT_BLOCK) return 0;
	const uint32_t B = block ? block : VG_BGZF_TEXT_BLOCK;
	return vg_bgzf_bound(text_bytes + B - 1, B);                              // (the pending text of earlier calls: less than a block)
}

extern "C" int vg_jtext_create_info(int device, uint64_t n_sites, uint32_t n_samples, uint32_t wide_samples, uint64_t max_records, uint64_t max_head_bytes, uint64_t max_site_refs, int with_bgzf, int info, vg_jtext **out)
{
	if (!out) return fail(VG_EINVAL, "null argument");
	*out = nullptr;
	if (!jt_info_mode(info)) return fail(VG_EINVAL, "vg_jtext_create_info: info is VG_JT_INFO_NONE or VG_JT_INFO_COUNTS");
	if (n_samples == 0) return fail(VG_EINVAL, "vg_jtext_create: no samples");
	if (n_sites >= (1ull << 32)) return fail(VG_EINVAL, "vg_jtext_create: 2^32 sites or more");
	if (n_samples > VG_JTEXT_MAX_SAMPLES) return fail(VG_ETOOBIG, "vg_jtext_create: more than %s samples", std::to_string(VG_JTEXT_MAX_SAMPLES).c_str());
	if (max_records == 0 || max_records >= (1ull << 32) || max_head_bytes >= (1ull << 40) || max_site_refs >= (1ull << 40)) return fail(VG_EINVAL, "vg_jtext_create: a span holds 1 to 2^32 - 1 records and less than 2^40 head bytes and site references");
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return fail(VG_ENODEV, "no HIP device available (vg_jtext_render_host is the host's loop)"); }
	return guarded([&]() -> int {
		HIP_TRY(hipSetDevice(device));
		vg_jtext *jt = new vg_jtext;
		jt->device = device; jt->n_sites = n_sites; jt->n_samples = n_samples; jt->G = (n_samples + 63) / 64; jt->wide_cap = std::min(wide_samples, n_samples);
		jt->rec_cap = max_records; jt->head_cap = max_head_bytes; jt->site_cap = max_site_refs; jt->with_bgzf = with_bgzf != 0; jt->info = info;
		jt->text_cap = vg_jt_bound_info(max_head_bytes, max_records, n_samples, info);
		jt->text_room = jt->text_cap + VG_BGZF_TEXT_BLOCK;
		const uint64_t items = max_records * (jt->G + 1);
		jt->bout_cap = JT_CHUNK_TEXT + JT_CHUNK_BLOCKS * 32 + 64;
		struct { void **p; uint64_t bytes; const char *what; bool stream; } want[] = {
			{(void **)&jt->d_narrow, (uint64_t)n_samples * n_sites * 2, "the samples' columns", false}, {(void **)&jt->d_wide, (uint64_t)jt->wide_cap * n_sites * 4, "the wide columns", false},
			{(void **)&jt->d_wide_slot, (uint64_t)n_samples * 4, "the wide column table", false}, {(void **)&jt->d_gt, n_sites, "a gt column", false}, {(void **)&jt->d_gq, n_sites * 4, "a gq column", false},
			{(void **)&jt->d_heads, max_head_bytes, "the heads", false}, {(void **)&jt->d_recs, max_records * sizeof(vg_jtext_record), "the records", false}, {(void **)&jt->d_sites, max_site_refs * 4, "the site references", false},
			{(void **)&jt->d_len, items * 4, "the piece lengths", false}, {(void **)&jt->d_counts, max_records * 12, "the records' counts", false}, {(void **)&jt->d_off, (items + 1) * 8, "the piece offsets", false}, {(void **)&jt->d_bsum, (items / JT_SCAN_BLOCK + 2) * 8, "the scan's sums", false},
			{(void **)&jt->d_lines, 8, "the line count", false}, {(void **)&jt->d_text, jt->text_room + JT_TILE + 64, "the text", false},
			{(void **)&jt->d_slots, JT_CHUNK_TEXT + JT_CHUNK_BLOCKS * (VG_DEF_SLACK + 32), "deflate slots", true}, {(void **)&jt->d_tok, (JT_CHUNK_TEXT + JT_CHUNK_BLOCKS * 16) * 4, "deflate tokens", true},
			{(void **)&jt->d_meta, JT_CHUNK_BLOCKS * sizeof(uint2), "block results", true}, {(void **)&jt->d_boffs, JT_CHUNK_BLOCKS * 8, "block offsets", true}, {(void **)&jt->d_bout, jt->bout_cap, "BGZF bytes", true}};
		for (auto &w : want) {
			if (w.stream && !jt->with_bgzf) continue;
			const uint64_t bytes = w.bytes ? w.bytes : 8;
			if (vg_malloc_patient(w.p, bytes) != hipSuccess) {
				(void)hipGetLastError();
				*w.p = nullptr;
				jtext_free(jt);
				return fail(VG_ENOMEM, "vg_jtext_create: no device memory for %s (%s bytes)", w.what, std::to_string(bytes).c_str());
			}
			jt->dev_bytes += bytes;
		}
		jt->wide_slot.assign(n_samples, -1);
		jt->slot_used.assign(jt->wide_cap, 0);
		if (jt->with_bgzf) { jt->h_meta.resize(JT_CHUNK_BLOCKS); jt->h_boffs.resize(JT_CHUNK_BLOCKS); }
		hipError_t e = hipEventCreate(&jt->ev0);
		if (e == hipSuccess) e = hipEventCreate(&jt->ev1);
		if (e == hipSuccess) e = hipEventCreate(&jt->ev2);
		if (e == hipSuccess) e = hipMemset(jt->d_narrow, 0, std::max<uint64_t>(8, (uint64_t)n_samples * n_sites * 2));
		if (e == hipSuccess) e = hipMemset(jt->d_wide_slot, 0xff, (uint64_t)n_samples * 4);
		if (e == hipSuccess) e = hipMemset(jt->d_text, 0, 64);
		if (e == hipSuccess) e = hipDeviceSynchronize();
		if (e != hipSuccess) { jtext_free(jt); return fail(VG_ENODEV, "vg_jtext_create: %s", hipGetErrorString(e)); }
		*out = jt;
		return VG_OK;
	});
}

extern "C" int vg_jtext_create(int device, uint64_t n_sites, uint32_t n_samples, uint32_t wide_samples, uint64_t max_records, uint64_t max_head_bytes, uint64_t max_site_refs, int with_bgzf, vg_jtext **out)
{
	return vg_jtext_create_info(device, n_sites, n_samples, wide_samples, max_records, max_head_bytes, max_site_refs, with_bgzf, VG_JT_INFO_NONE, out);
}

extern "C" void vg_jtext_destroy(vg_jtext *jt) { jtext_free(jt); }
extern "C" uint64_t vg_jtext_device_bytes(const vg_jtext *jt) { return jt ? jt->dev_bytes : 0; }

extern "C" int vg_jtext_set(vg_jtext *jt, uint32_t sample, const uint8_t *gt, const int32_t *gq)
{
	if (!jt || !gt || !gq) return fail(VG_EINVAL, "null argument");
	if (sample >= jt->n_samples) return fail(VG_EINVAL, "vg_jtext_set: sample %s is out of range", std::to_string(sample).c_str());
	bool wide = false;
	for (uint64_t i = 0; i < jt->n_sites; i++) {
		if (gt[i] > 3) return fail(VG_EINVAL, "vg_jtext_set: a gt above 3 (site %s)", std::to_string(i).c_str());
		wide = wide || (gt[i] && (gq[i] < 0 || gq[i] >= (int32_t)VG_JT_GQ_ESCAPE));
	}
	int32_t slot = jt->wide_slot[sample];
	if (wide && slot < 0) {
		for (uint32_t k = 0; k < jt->wide_cap && slot < 0; k++) if (!jt->slot_used[k]) slot = (int32_t)k;
		if (slot < 0) return fail(VG_ETOOBIG, "vg_jtext_set: sample %s has a gq outside 0 .. 16382 and every wide column is taken (vg_jtext_create's wide_samples)", std::to_string(sample).c_str());
	}
	if (jt->n_sites == 0) return VG_OK;
	HIP_TRY(hipSetDevice(jt->device));
	HIP_TRY(hipMemcpy(jt->d_gt, gt, jt->n_sites, hipMemcpyHostToDevice));
	HIP_TRY(hipMemcpy(jt->d_gq, gq, jt->n_sites * 4, hipMemcpyHostToDevice));
	const int32_t now = wide ? slot : -1;
	const unsigned grid = (unsigned)std::min<uint64_t>((jt->n_sites + 255) / 256, 4096);
	vg_jt_pack_kernel<<<grid, 256>>>(jt->d_gt, jt->d_gq, jt->n_sites, jt->d_narrow + (uint64_t)sample * jt->n_sites, wide ? jt->d_wide + (uint64_t)slot * jt->n_sites : nullptr);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpy(jt->d_wide_slot + sample, &now, 4, hipMemcpyHostToDevice));
	HIP_TRY(hipDeviceSynchronize());
	if (jt->wide_slot[sample] >= 0 && !wide) jt->slot_used[(size_t)jt->wide_slot[sample]] = 0;
	if (wide) jt->slot_used[(size_t)slot] = 1;
	jt->wide_slot[sample] = now;
	return VG_OK;
}

// what every call that takes a span checks before anything is written: null pointers and references outside their arrays are
// VG_EINVAL, a span beyond the handle's limits VG_ETOOBIG.  *head_sum: the sum of the records' head_len
// (with_heads false: a call that reads no head -- the counts alone -- does not look at head_off and head_len)
static int jt_span_args(const uint64_t n_sites, const uint8_t *heads, uint64_t heads_len, const vg_jtext_record *recs, uint64_t n_records, const uint32_t *sites, uint64_t n_site_refs, uint64_t *head_sum, bool with_heads = true)
{
	if ((!heads && heads_len) || (!recs && n_records) || (!sites && n_site_refs)) return fail(VG_EINVAL, "null argument");
	uint64_t sum = 0;
	for (uint64_t i = 0; i < n_records; i++) {
		const vg_jtext_record &r = recs[i];
		if (with_heads && (r.head_off > heads_len || r.head_len > heads_len - r.head_off)) return fail(VG_EINVAL, "record %s: its head lies outside the heads", std::to_string(i).c_str());
		if (r.site_at > n_site_refs || r.n_sites > n_site_refs - r.site_at) return fail(VG_EINVAL, "record %s: its site run lies outside the site references", std::to_string(i).c_str());
		sum += r.head_len;
	}
	for (uint64_t i = 0; i < n_site_refs; i++) if (sites[i] >= n_sites) return fail(VG_EINVAL, "site reference %s names a site the handle does not have", std::to_string(i).c_str());
	*head_sum = sum;
	return VG_OK;
}

// The first step of a span whose heads are on the device (info 0: no head is read): records and site references go up, the length
// kernel and the settle kernel leave the pieces' lengths in d_len, the records' counts in d_counts and the lines' number in d_lines
// (started: an event recorded in front of the kernels)
static int jt_lengths_dev(vg_jtext *jt, const JtStore &st, const vg_jtext_record *recs, uint64_t n_records, const uint32_t *sites, uint64_t n_site_refs, int info, hipEvent_t started = nullptr)
{
	HIP_TRY(hipMemcpy(jt->d_recs, recs, n_records * sizeof(vg_jtext_record), hipMemcpyHostToDevice));
	if (n_site_refs) HIP_TRY(hipMemcpy(jt->d_sites, sites, n_site_refs * 4, hipMemcpyHostToDevice));
	HIP_TRY(hipMemset(jt->d_lines, 0, 8));
	if (started) HIP_TRY(hipEventRecord(started, nullptr));
	vg_jt_len_kernel<<<(unsigned)((n_records * jt->G + 3) / 4), 256>>>(st, jt->d_heads, jt->d_recs, n_records, jt->d_sites, jt->G, info, jt->d_len);
	HIP_TRY(hipGetLastError());
	vg_jt_settle_kernel<<<(unsigned)((n_records + 255) / 256), 256>>>(jt->d_recs, n_records, jt->G, jt->d_len, jt->d_counts, jt->d_lines);
	HIP_TRY(hipGetLastError());
	return VG_OK;
}

// the three steps of a span (checked by jt_span_args and against the limits): its text to d_text[start, start + *total)
static int jt_render_dev(vg_jtext *jt, const uint8_t *heads, uint64_t heads_len, const vg_jtext_record *recs, uint64_t n_records, const uint32_t *sites, uint64_t n_site_refs, uint64_t head_sum, uint64_t start,
                         uint64_t *total, uint64_t *n_lines)
{
	*total = 0; *n_lines = 0;
	if (!n_records) return VG_OK;
	if (heads_len) HIP_TRY(hipMemcpy(jt->d_heads, heads, heads_len, hipMemcpyHostToDevice));
	const JtStore st{jt->d_narrow, jt->d_wide, jt->d_wide_slot, jt->n_sites, jt->n_samples};
	const uint32_t G = jt->G;
	const uint64_t items = n_records * (G + 1), nb = (items + JT_SCAN_BLOCK - 1) / JT_SCAN_BLOCK;
	const bool timed = getenv("VG_VERBOSE") != nullptr;
	const int rc = jt_lengths_dev(jt, st, recs, n_records, sites, n_site_refs, jt->info, timed ? jt->ev0 : nullptr);
	if (rc) return rc;
	vg_jt_scan_sums_kernel<<<(unsigned)nb, 256>>>(jt->d_len, items, jt->d_bsum);
	HIP_TRY(hipGetLastError());
	vg_jt_scan_top_kernel<<<1, 256>>>(jt->d_bsum, nb, jt->d_off + items);
	HIP_TRY(hipGetLastError());
	vg_jt_scan_apply_kernel<<<(unsigned)nb, 256>>>(jt->d_len, items, jt->d_bsum, jt->d_off);
	HIP_TRY(hipGetLastError());
	if (timed) HIP_TRY(hipEventRecord(jt->ev1, nullptr));
	// the tiles of the bound: one that lies beyond the text returns at once
	const uint64_t bound = vg_jt_bound_info(head_sum, n_records, jt->n_samples, jt->info);
	const uint64_t tiles = ((start & 3) + bound + JT_TILE - 1) / JT_TILE;
	vg_jt_write_kernel<<<(unsigned)tiles, 256>>>(st, jt->d_heads, jt->d_recs, jt->d_sites, G, jt->d_len, jt->d_off, jt->d_counts, items, jt->d_text, start);
	HIP_TRY(hipGetLastError());
	if (timed) HIP_TRY(hipEventRecord(jt->ev2, nullptr));
	unsigned long long lines = 0;
	HIP_TRY(hipMemcpy(total, jt->d_off + items, 8, hipMemcpyDeviceToHost));
	HIP_TRY(hipMemcpy(&lines, jt->d_lines, 8, hipMemcpyDeviceToHost));
	*n_lines = lines;
	if (*total > bound) return fail(VG_EIO, "the joint text kernels produced more bytes than the span's bound");
	if (timed) {
		float a = 0, c = 0;
		HIP_TRY(hipEventElapsedTime(&a, jt->ev0, jt->ev1)); HIP_TRY(hipEventElapsedTime(&c, jt->ev1, jt->ev2));
		fprintf(stderr, "[vargeno_hip] joint text: %lu records, %u samples, %lu lines, %lu bytes: lengths + scan %.3f ms, write %.3f ms (%.2f GB/s text)\n", (unsigned long)n_records, jt->n_samples, (unsigned long)lines,
		        (unsigned long)*total, a, c, c > 0 ? (double)*total / 1e6 / c : 0.0);
	}
	return VG_OK;
}

// a span against the handle's limits; the bound of its text must fit the text buffer behind `start` bytes
static int jt_span_limits(const vg_jtext *jt, uint64_t heads_len, uint64_t n_records, uint64_t n_site_refs, uint64_t head_sum)
{
	const uint64_t bound = vg_jt_bound_info(head_sum, n_records, jt->n_samples, jt->info);
	if (n_records > jt->rec_cap || heads_len > jt->head_cap || n_site_refs > jt->site_cap || bound > jt->text_cap || n_records * (jt->G + 1) >= (1ull << 32) || bound / JT_TILE >= (1ull << 31))      // (the last two: a grid's size)
		return fail(VG_ETOOBIG, "the span is beyond the limits the handle was created with (records, head bytes, site references)");
	return VG_OK;
}

extern "C" int vg_jtext_render(vg_jtext *jt, const uint8_t *heads, uint64_t heads_len, const vg_jtext_record *records, uint64_t n_records, const uint32_t *sites, uint64_t n_site_refs,
                               uint8_t *text, uint64_t cap, uint64_t *len, uint64_t *n_lines)
{
	if (!jt || !len || !n_lines || (!text && cap)) return fail(VG_EINVAL, "null argument");
	if (jt->open) return fail(VG_EINVAL, "vg_jtext_render: a BGZF stream is open on the handle (vg_jtext_bgzf_end closes it)");
	uint64_t head_sum = 0;
	int rc = jt_span_args(jt->n_sites, heads, heads_len, records, n_records, sites, n_site_refs, &head_sum);
	if (rc || (rc = jt_span_limits(jt, heads_len, n_records, n_site_refs, head_sum))) return rc;
	if (cap < vg_jt_bound_info(head_sum, n_records, jt->n_samples, jt->info)) return fail(VG_ETOOBIG, "the text buffer is smaller than the span's bound (vg_jtext_text_bound_info with the handle's mode)");
	HIP_TRY(hipSetDevice(jt->device));
	uint64_t total = 0, lines = 0;
	if ((rc = jt_render_dev(jt, heads, heads_len, records, n_records, sites, n_site_refs, head_sum, 0, &total, &lines))) return rc;
	if (total) HIP_TRY(hipMemcpy(text, jt->d_text, total, hipMemcpyDeviceToHost));
	*len = total; *n_lines = lines;
	return VG_OK;
}

extern "C" int vg_jtext_render_host_info(uint64_t n_sites, uint32_t n_samples, const uint8_t *const *gt, const int32_t *const *gq, const uint8_t *heads, uint64_t heads_len, const vg_jtext_record *records, uint64_t n_records,
                                         const uint32_t *sites, uint64_t n_site_refs, int info, int threads, uint8_t *text, uint64_t cap, uint64_t *len, uint64_t *n_lines)
{
	if (!gt || !gq || !len || !n_lines || (!text && cap)) return fail(VG_EINVAL, "null argument");
	if (!jt_info_mode(info)) return fail(VG_EINVAL, "vg_jtext_render_host_info: info is VG_JT_INFO_NONE or VG_JT_INFO_COUNTS");
	if (n_samples == 0) return fail(VG_EINVAL, "vg_jtext_render_host: no samples");
	if (n_samples > VG_JTEXT_MAX_SAMPLES) return fail(VG_ETOOBIG, "vg_jtext_render_host: more than %s samples", std::to_string(VG_JTEXT_MAX_SAMPLES).c_str());
	if (n_sites >= (1ull << 32)) return fail(VG_EINVAL, "vg_jtext_render_host: 2^32 sites or more");
	for (uint32_t s = 0; s < n_samples; s++) if (gt[s] && !gq[s]) return fail(VG_EINVAL, "null argument");
	uint64_t head_sum = 0;
	const int rc = jt_span_args(n_sites, heads, heads_len, records, n_records, sites, n_site_refs, &head_sum);
	if (rc) return rc;
	return guarded([&]() -> int {
		if (!vg_jtext_host_run_info(gt, gq, n_samples, heads, records, n_records, sites, info, threads, text, cap, len, n_lines)) return fail(VG_ETOOBIG, "the text buffer is smaller than the span's bound (vg_jtext_text_bound)");
		return VG_OK;
	});
}
extern "C" int vg_jtext_render_host(uint64_t n_sites, uint32_t n_samples, const uint8_t *const *gt, const int32_t *const *gq, const uint8_t *heads, uint64_t heads_len, const vg_jtext_record *records, uint64_t n_records,
                                    const uint32_t *sites, uint64_t n_site_refs, int threads, uint8_t *text, uint64_t cap, uint64_t *len, uint64_t *n_lines)
{
	return vg_jtext_render_host_info(n_sites, n_samples, gt, gq, heads, heads_len, records, n_records, sites, n_site_refs, VG_JT_INFO_NONE, threads, text, cap, len, n_lines);
}

// the records' NS, het, hom without their text: counts[n_records][3]
extern "C" int vg_jtext_counts(vg_jtext *jt, const vg_jtext_record *records, uint64_t n_records, const uint32_t *sites, uint64_t n_site_refs, uint32_t *counts)
{
	if (!jt || (!counts && n_records)) return fail(VG_EINVAL, "null argument");
	uint64_t head_sum = 0;
	const int rc = jt_span_args(jt->n_sites, nullptr, 0, records, n_records, sites, n_site_refs, &head_sum, false);
	if (rc) return rc;
	if (n_records > jt->rec_cap || n_site_refs > jt->site_cap || n_records * (jt->G + 1) >= (1ull << 32)) return fail(VG_ETOOBIG, "the span is beyond the limits the handle was created with (records, site references)");
	if (!n_records) return VG_OK;
	HIP_TRY(hipSetDevice(jt->device));
	const JtStore st{jt->d_narrow, jt->d_wide, jt->d_wide_slot, jt->n_sites, jt->n_samples};
	const int rc2 = jt_lengths_dev(jt, st, records, n_records, sites, n_site_refs, VG_JT_INFO_NONE);
	if (rc2) return rc2;
	HIP_TRY(hipMemcpy(counts, jt->d_counts, n_records * 12, hipMemcpyDeviceToHost));
	return VG_OK;
}
extern "C" int vg_jtext_counts_host(uint64_t n_sites, uint32_t n_samples, const uint8_t *const *gt, const int32_t *const *gq, const vg_jtext_record *records, uint64_t n_records, const uint32_t *sites, uint64_t n_site_refs,
                                    uint32_t *counts)
{
	if (!gt || !gq || (!counts && n_records)) return fail(VG_EINVAL, "null argument");
	if (n_samples == 0) return fail(VG_EINVAL, "vg_jtext_counts_host: no samples");
	if (n_samples > VG_JTEXT_MAX_SAMPLES) return fail(VG_ETOOBIG, "vg_jtext_counts_host: more than %s samples", std::to_string(VG_JTEXT_MAX_SAMPLES).c_str());
	if (n_sites >= (1ull << 32)) return fail(VG_EINVAL, "vg_jtext_counts_host: 2^32 sites or more");
	for (uint32_t s = 0; s < n_samples; s++) if (gt[s] && !gq[s]) return fail(VG_EINVAL, "null argument");
	uint64_t head_sum = 0;
	const int rc = jt_span_args(n_sites, nullptr, 0, records, n_records, sites, n_site_refs, &head_sum, false);
	if (rc) return rc;
	for (uint64_t i = 0; i < n_records; i++) {
		const vg_jt_counts_t c = vg_jt_counts_host(gt, gq, n_samples, records[i], sites);
		counts[3 * i] = c.ns; counts[3 * i + 1] = c.ns ? c.het : 0; counts[3 * i + 2] = c.ns ? c.hom : 0;
	}
	return VG_OK;
}

// ---- the BGZF stream of a vg_jtext: text gathers in d_text; every call compresses the whole blocks it completed ----
// d_text[0, have): its whole blocks (final: and the partial last one) -> bgzf + *len, chunk by chunk; the rest moves to the front
static int jt_stream_flush(vg_jtext *jt, uint64_t have, bool final, uint8_t *bgzf, uint64_t *len)
{
	const uint32_t B = jt->B;
	const uint64_t nb = final ? vg_bgzf_blocks_of(have, B) : have / B;
	const uint64_t chunk_blocks = std::min<uint64_t>(JT_CHUNK_BLOCKS, std::max<uint64_t>(1, JT_CHUNK_TEXT / B));
	const bool timed = getenv("VG_VERBOSE") != nullptr;
	const BzDeflateDev dev{jt->d_slots, jt->d_tok, jt->d_meta, jt->d_boffs, jt->d_bout, jt->h_meta.data(), jt->h_boffs.data(), ((B + VG_DEF_SLACK + 15u) & ~15u) / 4, (B + 15u) & ~15u, jt->bout_cap, timed, jt->ev0, jt->ev1, jt->ev2};
	float ms_deflate = 0, ms_frame = 0;
	const uint64_t len0 = *len;
	for (uint64_t b0 = 0; b0 < nb; b0 += chunk_blocks) {
		const uint32_t k = (uint32_t)std::min(chunk_blocks, nb - b0);
		const uint64_t t0 = b0 * B, tn = std::min<uint64_t>((uint64_t)k * B, have - t0);
		uint64_t sum = 0;
		const int rc = bz_deflate_chunk(dev, jt->d_text + t0, tn, B, k, jt->dyn, bgzf + *len, &sum, &ms_deflate, &ms_frame);
		if (rc) return rc;
		*len += sum;
	}
	const uint64_t done = std::min(have, nb * B);
	jt->pend = have - done;
	if (jt->pend && done) HIP_TRY(hipMemcpy(jt->d_text, jt->d_text + done, jt->pend, hipMemcpyDeviceToDevice));      // (less than a block behind at least one: no overlap)
	if (timed && nb) fprintf(stderr, "[vargeno_hip] joint text stream: %lu blocks, %s codes, %.3f ms deflate kernel, %.3f ms framing, %lu bytes of BGZF\n", (unsigned long)nb, jt->dyn ? "dynamic" : "fixed", ms_deflate, ms_frame, (unsigned long)(*len - len0));
	return VG_OK;
}

extern "C" int vg_jtext_bgzf_begin(vg_jtext *jt, uint32_t block, int codes)
{
	if (!jt) return fail(VG_EINVAL, "null argument");
	if (!jt->with_bgzf) return fail(VG_EINVAL, "vg_jtext_bgzf_begin: the handle was created without the stream's buffers (with_bgzf)");
	if (codes != VG_DEFLATE_FIXED && codes != VG_DEFLATE_DYNAMIC) return fail(VG_EINVAL, "codes is VG_DEFLATE_FIXED or VG_DEFLATE_DYNAMIC");
	if (block > VG_BGZF_TEXT_BLOCK) return fail(VG_EINVAL, "a BGZF block holds at most 65280 bytes of text here");
	jt->B = block ? block : VG_BGZF_TEXT_BLOCK; jt->dyn = codes == VG_DEFLATE_DYNAMIC; jt->pend = 0; jt->open = true; jt->idx = nullptr;
	return VG_OK;
}

extern "C" int vg_jtext_bgzf_index(vg_jtext *jt, vg_vcfidx *idx)
{
	if (!jt) return fail(VG_EINVAL, "null argument");
	if (!jt->open) return fail(VG_EINVAL, "no BGZF stream is open on the handle (vg_jtext_bgzf_begin)");
	if (idx && idx->B != jt->B) return fail(VG_EINVAL, "vg_jtext_bgzf_index: the index was created for another block size than the stream's");
	jt->idx = idx;
	return VG_OK;
}
// the index's side of the stream: the rendered lines d_text[pend, pend + total) -- whole lines, on the device alone
static int jt_index_lines(vg_jtext *jt, uint64_t total)
{
	vg_vcfidx *ix = jt->idx;
	return guarded([&]() -> int {
		const double t0 = now_s();
		if (!ix->carry.empty()) return fail(VG_EINVAL, "vg_jtext_bgzf_lines: the text joined before the span does not end with a line's end, the index cannot follow");
		std::vector<vg_vi_rec> recs;
		const uint64_t base = ix->fed;
		const int rc = vi_scan_resident(ix, jt->device, jt->d_text + jt->pend, total, base, recs);
		if (rc) return rc;
		bool copied = true;
		(void)ix->feed_records(total, recs, [&](const vg_vi_rec &r) -> const uint8_t * {
			ix->name.resize((size_t)r.clen + 1);
			if (r.clen && hipMemcpy(ix->name.data(), jt->d_text + jt->pend + (r.start - base), r.clen, hipMemcpyDeviceToHost) != hipSuccess) { copied = false; memset(ix->name.data(), 0, r.clen); }
			return ix->name.data();
		});
		ix->seconds += now_s() - t0;
		if (!copied) return fail(VG_ENODEV, "vg_jtext_bgzf_lines: a chromosome name could not be copied from the device");
		return VG_OK;
	});
}
// ... and the blocks a call hands back
static int jt_index_blocks(vg_jtext *jt, const uint8_t *bgzf, uint64_t len)
{
	if (!jt->idx || !len) return VG_OK;
	const int rc = vi_fused_blocks(jt->idx, bgzf, len);
	if (rc) jt->open = false;
	return rc;
}

extern "C" int vg_jtext_bgzf_text(vg_jtext *jt, const uint8_t *text, uint64_t nbytes, uint8_t *bgzf, uint64_t cap, uint64_t *bgzf_len)
{
	if (!jt || (!text && nbytes) || !bgzf || !bgzf_len) return fail(VG_EINVAL, "null argument");
	if (!jt->open) return fail(VG_EINVAL, "no BGZF stream is open on the handle (vg_jtext_bgzf_begin)");
	if (cap < vg_jtext_bgzf_bound(nbytes, jt->B)) return fail(VG_ETOOBIG, "the BGZF buffer is smaller than the call's bound (vg_jtext_bgzf_bound)");
	HIP_TRY(hipSetDevice(jt->device));
	uint64_t len = 0;
	for (uint64_t at = 0; at < nbytes;) {                                       // as much as the text buffer takes per step
		const uint64_t take = std::min(nbytes - at, jt->text_room - jt->pend);
		HIP_TRY(hipMemcpy(jt->d_text + jt->pend, text + at, take, hipMemcpyHostToDevice));
		at += take;
		const int rc = jt_stream_flush(jt, jt->pend + take, false, bgzf, &len);
		if (rc) { jt->open = false; return rc; }
	}
	if (jt->idx) {                                                            // header text: the host has it
		int rc = guarded([&]() -> int { const double t0 = now_s(); (void)jt->idx->feed_host(text, nbytes, 1); jt->idx->seconds += now_s() - t0; return VG_OK; });
		if (!rc) rc = jt_index_blocks(jt, bgzf, len);
		if (rc) { jt->open = false; return rc; }
	}
	*bgzf_len = len;
	return VG_OK;
}

extern "C" int vg_jtext_bgzf_lines(vg_jtext *jt, const uint8_t *heads, uint64_t heads_len, const vg_jtext_record *records, uint64_t n_records, const uint32_t *sites, uint64_t n_site_refs,
                                   uint8_t *bgzf, uint64_t cap, uint64_t *bgzf_len, uint64_t *text_len, uint64_t *n_lines)
{
	if (!jt || !bgzf || !bgzf_len || !text_len || !n_lines) return fail(VG_EINVAL, "null argument");
	if (!jt->open) return fail(VG_EINVAL, "no BGZF stream is open on the handle (vg_jtext_bgzf_begin)");
	uint64_t head_sum = 0;
	int rc = jt_span_args(jt->n_sites, heads, heads_len, records, n_records, sites, n_site_refs, &head_sum);
	if (rc || (rc = jt_span_limits(jt, heads_len, n_records, n_site_refs, head_sum))) return rc;
	if (cap < vg_jtext_bgzf_bound(vg_jt_bound_info(head_sum, n_records, jt->n_samples, jt->info), jt->B)) return fail(VG_ETOOBIG, "the BGZF buffer is smaller than the call's bound (vg_jtext_bgzf_bound of the span's text bound)");
	HIP_TRY(hipSetDevice(jt->device));
	uint64_t total = 0, lines = 0, len = 0;
	rc = jt_render_dev(jt, heads, heads_len, records, n_records, sites, n_site_refs, head_sum, jt->pend, &total, &lines);
	if (!rc && jt->idx && total) rc = jt_index_lines(jt, total);                // (before the flush moves the text)
	if (!rc) rc = jt_stream_flush(jt, jt->pend + total, false, bgzf, &len);
	if (!rc) rc = jt_index_blocks(jt, bgzf, len);
	if (rc) { jt->open = false; return rc; }
	*bgzf_len = len; *text_len = total; *n_lines = lines;
	return VG_OK;
}

extern "C" int vg_jtext_bgzf_end(vg_jtext *jt, uint8_t *bgzf, uint64_t cap, uint64_t *bgzf_len)
{
	if (!jt || !bgzf || !bgzf_len) return fail(VG_EINVAL, "null argument");
	if (!jt->open) return fail(VG_EINVAL, "no BGZF stream is open on the handle (vg_jtext_bgzf_begin)");
	if (cap < vg_jtext_bgzf_bound(0, jt->B)) return fail(VG_ETOOBIG, "the BGZF buffer is smaller than the call's bound (vg_jtext_bgzf_bound)");
	HIP_TRY(hipSetDevice(jt->device));
	uint64_t len = 0;
	int rc = jt_stream_flush(jt, jt->pend, true, bgzf, &len);
	if (!rc) rc = jt_index_blocks(jt, bgzf, len);
	jt->open = false;
	if (rc) return rc;
	memcpy(bgzf + len, vg_bgzf_eof_marker(), VG_BGZF_EOF_BYTES);
	*bgzf_len = len + VG_BGZF_EOF_BYTES;
	return VG_OK;
}

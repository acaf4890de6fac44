/* vargeno_hip.h -- C-ABI of the MI355X (gfx950) `vargeno geno` read-processing path.
 *
 * The reference has no plugin/FFI seam: the whole path is inlined in `static void genotype()`
 * (src/qv.cc:475-1787 of medvedevgroup/vargeno).  This header is the seam a maintainer would cut:
 * each entry point names the span of genotype() it replaces.  Plain pointers and sizes only; every
 * function returns 0 on success or a negative VG_E* code and never aborts (the reference asserts /
 * exit(EXIT_FAILURE)s instead: src/util.c:31-50, src/qv.cc:526-529).  One handle per GPU; a handle
 * is thread-compatible (one caller at a time).
 *
 * There is NO CPU fallback behind these calls: without a HIP device they fail with VG_ENODEV.
 */
#ifndef VARGENO_HIP_H
#define VARGENO_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define VG_OK        0
#define VG_EINVAL   -1   /* bad argument                                                     */
#define VG_EIO      -2   /* index file missing / short (reference: assert in util.c:31-50)   */
#define VG_ENOMEM   -3   /* host or device allocation failed                                 */
#define VG_ENODEV   -4   /* no HIP device / HIP runtime error (message via vg_last_error)    */
#define VG_ETOOBIG  -5   /* dictionary > 2^32 entries (reference: exit, qv.cc:526, 612)      */
#define VG_EBADREAD -6   /* a read longer than 1022 bases (reference BUF_SIZE, qv.cc:700)    */

typedef struct vg_index vg_index;        /* device-resident index + pile-up counters         */

/* The dictionaries and bit vectors exactly as the reference's files hold them, field by field
 * (dictgen.c:63-154 ref dict, :156-275 SNP dict; sdsl int_vector<1> payload words for the .bf
 * files).  Host pointers; copied, never retained. */
typedef struct {
	uint64_t n_ref;            const uint64_t *ref_kmer;  const uint32_t *ref_pos;  const uint8_t *ref_amb;
	uint64_t n_ref_aux;        const uint32_t *ref_aux;        /* [n_ref_aux][10]            */
	uint64_t n_snp;            const uint64_t *snp_kmer;  const uint32_t *snp_pos;
	const uint8_t *snp_info;   const uint8_t *snp_amb;    const uint8_t *snp_rf;    const uint8_t *snp_af;
	uint64_t n_snp_aux;        const uint32_t *snp_aux_pos;    /* [n_snp_aux][10]            */
	                           const uint8_t  *snp_aux_info;   /* [n_snp_aux][10]            */
	uint64_t ref_bf_bits;      const uint64_t *ref_bf_words;   /* >= ceil(min(bits,2^32)/64) */
	uint64_t snp_bf_bits;      const uint64_t *snp_bf_words;   /* >= ceil(bits/64)           */
} vg_index_arrays;

/* Counters mirroring the reference's `#if DEBUG` set (qv.cc:737-751) plus the event counts that
 * price algorithmic bytes.  All accumulate since open / vg_counts_reset. */
typedef struct {
	uint64_t reads, reads_n, reads_invalid, passes, passes_ok, chunks, gate_open,
	         refbf_pos, snpbf_pos, large_block, ref_query, snp_query, ref_probe, snp_probe,
	         scan_ref, scan_snp, scan_oob, aux_ref, aux_snp, site_test, ctx, walks, incr,
	         ingest_bytes;
	uint64_t overflow_reads;     /* reads that outgrew the main wave tier's LDS tables and were redone by
	                                the deep wave tier (same kernel, tables 3-7x deeper)       */
	uint64_t overflow_deep;      /* of those, reads that outgrew the deep lists too and went to the
	                                generic lane tier (one read per lane, lists in HBM scratch)   */
	uint64_t alg_bytes;          /* sum of unit cost x event count                            */
} vg_stats;

/* Kernel timing, averaged over the batches processed since the previous vg_timing_get, from HIP
 * events recorded on the handle's own streams. */
typedef struct {
	float ms_total;              /* first kernel start -> last kernel end of a batch           */
	float ms_pack;               /* vg_pack_kernel: ASCII -> 2-bit chunk k-mers + gate bits    */
	float ms_main;               /* vg_wave_kernel, the dominant kernel                        */
	float ms_tail;               /* the spill tiers (deep-list wave tier + generic lane tier) for the
	                                reads that outgrew the LDS lists: second stream, under the next
	                                batches' kernels                                             */
	uint32_t batches;
	float ms_deep_lists;         /* of ms_tail: the deep-list wave tier                        */
} vg_timing;

const char *vg_last_error(void);
/* sha256 prefix of the sources this library was compiled from (csrc/Makefile): lets a caller refuse a stale build */
const char *vg_build_id(void);
int  vg_device_count(void);
/* Total memory of a device in bytes (0 on failure): what a caller that puts SEVERAL replicas on one device divides into the
 * budgets it hands to vg_index_open_ex -- without a budget every replica plans for the whole device (less 12 GiB), and the
 * third or fourth one fails with VG_ENOMEM.  vg_share_budget() is that division as the CLI makes it:
 * (min(total, free at the time of the call) - 12 GiB) / replicas_on_the_device.  "Free at the time of the call" makes it ONE
 * number for all sharers only when it is asked for before any of them has opened: a process that opens its replicas itself calls
 * it once per device, before the first vg_index_open_ex, and hands every sharer that number (the command line; it also does so
 * for a single replica when it has taken a read store on the device).  Sharers in different processes must agree on a number
 * among themselves (bench.py: every rank calls before any opens, the minimum over the ranks is everybody's budget) -- a rank that
 * calls after a sibling has taken its block would get half a share. */
uint64_t vg_device_memory(int device);
uint64_t vg_share_budget(int device, int replicas_on_the_device);
/* Host -> device rate of page-locked memory over this device's link in bytes per second, measured now (three 64 MiB copies; 0 on
 * failure): what FASTQ text framed ON the device can arrive at -- the command line compares it with the rate its host threads
 * frame + pack at (vg_packer_*) and lets the faster route take the file (r05; r04 chose by the number of CPUs). */
double vg_link_rate(int device);

/* Page-locked host buffers for the batches / FASTQ chunks handed to vg_reads_submit / vg_fastq_submit
 * (optional: any host memory works, pinned memory copies at link speed).  NULL on failure. */
void *vg_host_alloc_pinned(size_t bytes);
void  vg_host_free_pinned(void *p);

/* Replaces the loader half of genotype(): qv.cc:519-695 (dict files -> jump tables, dict arrays,
 * aux tables, pile-up seeding) and main()'s BloomFilter::load (qv.cc:2140-2144).
 * vg_index_open reads <prefix>.ref.dict/.snp.dict/.ref.bf/.snp.bf; vg_index_create takes the same
 * content from memory. */
int  vg_index_open(const char *prefix, int device, vg_index **out);
/* The same with a device-memory budget for this replica (bytes; 0 = the device's whole memory less 12 GiB, which is what
 * vg_index_open assumes -- $VG_MAX_DEVICE_BYTES, when set, is its budget).  Which optional views are built is decided from the
 * dictionaries' sizes and the budget alone, in a fixed order, before anything is allocated -- never from what happens to be free at
 * that moment: the same files and the same budget always give the same vg_index_views().  A caller that shares the device must say
 * how much of it is its own; when an allocation the plan had room for fails all the same, the call fails with VG_ENOMEM instead of
 * silently building a slower layout.  VG_ENOMEM also when the budget is below the smallest layout.
 * The budget bounds what the FINISHED handle holds (vg_index_device_bytes <= budget; profiles/budget_sweep_r05.json).  With
 * every view planned, construction stays inside the handle's one block (vg_arena.h: the order of construction keeps the live set
 * within the finished size).  With views left out the finished handle is smaller than what construction has alive at its peak --
 * the dictionaries' columns beside their entries, the sorts' buffers -- and those temporaries are taken from the device beside the
 * block and given back: up to ~100 GB more than the budget for some hundred milliseconds at hg38 scale.  Replicas that SHARE a
 * device and open at the same time must leave that room (or open one after the other).  When the device does not have that room
 * free at the time of the call (a plan limited by the device's own size) the handle is built without the block, one allocation
 * per buffer: slower to open, same views, same results (r06).
 * Tables scale with the index (r06): the reference's jump table and the direct table have ~2 entries per k-mer instead of 2^32
 * (a chr22-scale index holds ~8 GB instead of 92); vg_index_plan() names the widths, and under a budget the direct table is
 * tried with half and a quarter of its buckets before it is given up. */
int  vg_index_open_ex(const char *prefix, int device, uint64_t max_device_bytes, vg_index **out);
/* What the budget bought, in words: planned bytes, views kept, views left out with what each costs ("" for a null handle).
 * The string lives as long as the handle. */
const char *vg_index_plan(const vg_index *ix);
/* Where the handle's start-up time went (the reference's loader, qv.cc:519-695, takes ~240 s at hg38 scale):
 * wall seconds of each phase of vg_index_open / vg_index_create with the part spent inside allocation calls, then the memory the
 * handle ended up with (r05: one block taken from the driver once and carved up, vg_arena.h).  "" for a null handle;
 * the string lives as long as the handle. */
const char *vg_index_open_report(const vg_index *ix);
int  vg_index_create(const vg_index_arrays *a, int device, vg_index **out);
void vg_index_close(vg_index *ix);               /* qv.cc:1775-1786 */

/* Device bytes held by the index (tables + pile-up + scratch). */
uint64_t vg_index_device_bytes(const vg_index *ix);

/* Which optional re-laid-out views of the dictionaries the handle holds (bit mask).  They change speed, never results: a
 * view is left out when the index is too large for it or the device had too little free memory while the handle was
 * built (or a VG_NO_* development switch said so) -- a caller that cares about throughput should look. */
#define VG_VIEW_SEC        1u   /* LO32-ordered view of the reference dictionary (high-half neighbours, qv.cc:1213-1296)   */
#define VG_VIEW_MX         2u   /* merged exact-match view of both dictionaries (qv.cc:840-841)                            */
#define VG_VIEW_DX         4u   /* direct table over HI32 in front of the merged view                                      */
#define VG_VIEW_SNP_PROBE  8u   /* strided-probe view of the SNP dictionary (iterate_snp_dict, qv.cc:413-464)              */
#define VG_VIEW_SNP_JG32  16u   /* HI32 jump table of the SNP dictionary (indexes too large for the merged view)           */
#define VG_VIEW_SNP_SIG   64u   /* ... its 16-bit signature form (the default; the probe view is built under VG_NO_SIG_VIEW)    */
#define VG_VIEW_SEC_IS_BF 128u  /* the reference bit vector was verified to be the LO32 set of the dictionary: the LO32-ordered
                                   view answers its probes too (false e.g. for an index built from a soft-masked FASTA)   */
#define VG_VIEW_HX        32u   /* paired HI32 table of both dictionaries (indexes too large for the merged view)          */
#define VG_VIEW_SSEC     256u   /* LO32-ordered view of the SNP dictionary (high-half SNP neighbours, qv.cc:1303-1352; r06) */
uint32_t vg_index_views(const vg_index *ix);

/* Replaces the FASTQ loop body, qv.cc:760-1558, for a batch of reads: flat ASCII bases and quality
 * characters (same offsets; offsets[n_reads] = total length) in HOST memory.  Copies to the
 * device and enqueues the kernels on the handle's stream; returns before they finish. */
int  vg_reads_submit(vg_index *ix, const uint8_t *bases, const uint8_t *quals,
                     const uint64_t *offsets, uint64_t n_reads);

/* Same, for a batch already resident in device memory (hipMalloc'd by the caller on ix's device):
 * what bench.py times.  The handle works on its own non-blocking streams: the buffers must be complete when the
 * call is made (synchronise the stream that produced them) and stay valid and unchanged until the next vg_sync. */
int  vg_reads_process_device(vg_index *ix, const uint8_t *d_bases, const uint8_t *d_quals,
                             const uint64_t *d_offsets, uint64_t n_reads);

/* The same batch with the quality strings reduced to what the path reads of them: ONE GATE WORD per read, bit c set iff quality
 * character c of the read is below '8' -- the only question qv.cc:836, 943 asks, with c the CHUNK number (a read of at most
 * 1022 bases has at most 31 chunks).  The reference's loop never looks at the other characters; handing the strings over makes
 * the device fetch every line of them for four characters per 150 bp read, as much traffic again as the bases.  This is the form
 * the device-side FASTQ framing (vg_fastq_stream_push) produces for itself, and what bench.py's resident batches use.
 * A read of more than 32 chunks (1055 bases: no FASTQ line the reference can read holds one) is counted in reads_invalid. */
int  vg_reads_process_device_gated(vg_index *ix, const uint8_t *d_bases, const uint32_t *d_gate_words,
                                   const uint64_t *d_offsets, uint64_t n_reads);

/* A batch that is already framed and 2-bit packed, in HOST memory -- SURVEY.md §8b's "pre-packed 2-bit + the <= 31 quality chars the
 * gate can see", the latter reduced to the comparison's result: kmers = the reads' chunk k-mers one read after the other
 * (encode_kmer, util.c:89-111: A0 C1 G2 T3, character k[0] in bits 0-1), chunk_offsets[r] = chunks before read r
 * (chunk_offsets[0] = 0, [n_reads] = total), meta[r] = gate bits of read r (bit c = quality character c < '8', qv.cc:836, 943) with
 * bit 62 set for a read the reference skips (an N in its trimmed part, qv.cc:815-828) and bit 63 for one it aborts on (another
 * character outside ACGTacgt, util.c:103) -- 48 bytes per 150 bp read where its FASTQ record has ~315.  Blocking copies: the
 * arrays are free when the call returns; the read loop is only enqueued.  VG_EBADREAD: a read of more than 31 chunks. */
int  vg_reads_submit_packed(vg_index *ix, const uint64_t *kmers, const uint64_t *meta, const uint64_t *chunk_offsets, uint64_t n_reads);
/* The same for arrays in PAGE-LOCKED memory (vg_host_alloc_pinned) that the caller leaves untouched until vg_sync: the copies are
 * asynchronous and the call returns as soon as the batch is enqueued (r05: the command line hands over the hundreds of batches it
 * packed while the index was being opened). */
int  vg_reads_submit_packed_async(vg_index *ix, const uint64_t *kmers, const uint64_t *meta, const uint64_t *chunk_offsets, uint64_t n_reads);

/* A read store: packed batches parked in DEVICE memory before an index handle exists on that device -- a job's FASTQ file is framed
 * and packed (vg_packer_*) while vg_index_open runs, and what is packed goes up the otherwise idle link at once instead of waiting
 * in page-locked host memory (which costs ~0.15 s per GB to lock and ~0.1 s per GB to give back at exit).  The reference has no
 * counterpart: it reads the file after load_dict_from_file has returned (qv.cc:1757-1767, then 760-784).
 *   vg_read_store_create   takes max_bytes of device memory at once (before the index is planned, so that the plan sees what is left)
 *   vg_read_store_push     validates one batch (the rules of vg_reads_submit_packed) and enqueues its copies; the arrays -- page-locked
 *                          memory copies at link speed -- must stay untouched until the NEXT vg_read_store_push / _flush on this
 *                          store returns (a caller alternates between two sets).  VG_ENOMEM: the store is full; the batch was not
 *                          taken and the caller sends it, and what follows, down another route
 *   vg_reads_submit_store  every batch of the store through the read loop of an open handle on the same device, in push order,
 *                          asynchronously (vg_sync); the store must live until then.  A store may be submitted more than once
 *   vg_read_store_destroy  gives the memory back */
typedef struct vg_read_store vg_read_store;
int      vg_read_store_create(int device, uint64_t max_bytes, vg_read_store **out);
int      vg_read_store_push(vg_read_store *rs, const uint64_t *kmers, const uint64_t *meta, const uint64_t *chunk_offsets, uint64_t n_reads);
int      vg_read_store_flush(vg_read_store *rs);
uint64_t vg_read_store_reads(const vg_read_store *rs);
uint64_t vg_read_store_bytes_used(const vg_read_store *rs);
int      vg_reads_submit_store(vg_index *ix, vg_read_store *rs);
void     vg_read_store_destroy(vg_read_store *rs);

/* Same again, starting from raw FASTQ text (host memory): replaces the four fgets() + strlen of qv.cc:760-784.
 *
 * Stream form -- the caller only moves bytes.  vg_fastq_stream_push takes the next chunk of the file, cut anywhere; the device
 * frames the complete 4-line records (carrying the unfinished last record of a chunk over to the next one by itself) and runs
 * them through the read loop.  The call returns when the chunk has been copied to the device (its buffer is free again; pinned
 * memory copies at link speed); framing and processing are only enqueued, and nothing is reported back until
 * vg_fastq_stream_end: records framed, bytes consumed (= offset of the first byte the device did not process: the incomplete tail
 * of the file, or everything from the first chunk it refused), offset of the last framed record (a host reader that must
 * reproduce the reference's stale-buffer behaviour on a truncated final record starts there), and whether a chunk was refused.
 * A chunk is refused -- and with it everything after it -- when it holds a line longer than fgets' 1023 characters, a quality
 * line shorter than the read's chunk count, or lines shorter than 8 bytes on average: frame the rest on the host
 * (vg_reads_submit).  One stream at a time per handle; chunks of less than 2 GiB. */
int  vg_fastq_stream_begin(vg_index *ix);
/* The same stream with the framing AND the 2-bit packing done by host threads inside the library (r04): the rules
 * are the device framing's (records = four lines counted from the start of the stream, lines of at most 1023 characters, a
 * quality character for every chunk; anything else refuses the chunk and the rest of the stream), but what crosses the link is
 * the packed form (8 bytes per chunk + 16 per read instead of the text: 6.5 x fewer bytes for 150 bp reads), so a host with cores
 * to spare ingests several times faster than the link can move text.  host_threads > 0: that many; 0: device framing after all
 * (same as vg_fastq_stream_begin); < 0: the library decides (half the CPUs the process may use -- a cgroup CPU quota counts --,
 * at most 96; device framing when that is fewer than 32; $VG_PACK_THREADS overrides).  At most 256 threads are started.  push / end are the calls above and report the same things. */
int  vg_fastq_stream_begin_packed(vg_index *ix, int host_threads);
int  vg_fastq_stream_push(vg_index *ix, const uint8_t *text, uint64_t nbytes);
int  vg_fastq_stream_end(vg_index *ix, uint64_t *n_records, uint64_t *consumed, uint64_t *last_record_start, int *refused);

/* The same device-framed stream over BGZF, the blocked gzip that bgzip / htslib write (gzip members of at most 64 KiB, each with
 * its compressed size in a `BC` extra subfield and CRC32 + ISIZE in its trailer; a BGZF file is also a valid .gz).  After
 * vg_fastq_stream_begin_bgzf, vg_fastq_stream_push takes BGZF bytes cut anywhere -- mid-header, mid-block, one byte at a time: the
 * library keeps an incomplete block (at most 64 KiB) for the next push, walks the block headers on the host, copies the COMPRESSED
 * bytes up and inflates them on the device, one wave per block, straight into the chunk's text buffer; framing and the read loop are
 * those of the text stream.  A push whose text would pass the text chunks' limit is split at block boundaries.
 * vg_fastq_stream_end reports records, consumed and last_record_start as offsets in the UNCOMPRESSED stream.  Bytes that are no
 * BGZF block header (1f 8b 08 04, XLEN subfields with BC of length 2, BSIZE + 1 >= header + 8, ISIZE <= 65536) make the push
 * return VG_EIO.  A block that fails on the device (deflate error / size / CRC), or an incomplete block left at the end, makes
 * vg_fastq_stream_end return VG_EIO: vg_last_error() names the compressed offset and the reason, the out-parameters hold what was
 * framed before it -- nothing of the chunk with the bad block or of later ones is -- and the handle stays usable.  A missing
 * end-of-file marker block is accepted; an empty block anywhere is a block of zero bytes. */
int  vg_fastq_stream_begin_bgzf(vg_index *ix);
/* Where an uncompressed offset of the handle's last BGZF stream lies: compressed offset of its block and the offset inside the
 * block's text (a host reader that takes over at last_record_start / consumed inflates from there).  The library keeps 16 bytes
 * per block, valid until the next vg_fastq_stream_begin*.  text_offset = the end of the text seen: the offset behind the last
 * whole block, 0. */
int  vg_fastq_stream_bgzf_locate(vg_index *ix, uint64_t text_offset, uint64_t *block_offset, uint32_t *within);

/* The same stream over BAM (a BGZF file whose inflated bytes are a header and binary records): after vg_fastq_stream_begin_bam,
 * vg_fastq_stream_push takes the BAM file's bytes cut anywhere.  The library inflates the leading blocks on the host until the BAM
 * header parses (blocks wholly inside it never go to the device; bytes that inflate to something else make the push return VG_EIO);
 * everything behind goes up compressed, is inflated on the device and FRAMED there: the chain of block_size fields is walked in
 * fixed 64 KiB windows, speculatively in parallel and then confirmed (csrc/vg_bam.h has the record rules, vargeno_hip.hip the
 * kernels); a record that straddles two slots is carried on the device.  No text exists on this route: bases are unpacked from
 * their nibbles into the batch, the qualities are reduced to the read's gate word.  What a record becomes is defined by the
 * equivalent FASTQ text (vg_bam_to_fastq_host): secondary / supplementary records (flag 0x900) and records without bases are
 * skipped; flag 0x10 reverse-complements.
 * vg_fastq_stream_end reports kept records, and consumed / last_record_start as offsets in the INFLATED BAM stream: consumed is the
 * first byte not framed (a record boundary), last_record_start the last kept record; vg_fastq_stream_bgzf_locate maps both.  A
 * chunk is refused (and everything behind it) when a record's block_size is smaller than its fields announce or above 65 532, or
 * a read is longer than 1022 bases: the caller converts from `consumed` on the host.  A stream that ends inside the header or inside
 * a record makes vg_fastq_stream_end return VG_EIO with the inflated offset in vg_last_error(); bad blocks as for BGZF.
 * vg_bam_stream_stats: the counters of the handle's last BAM stream (any pointer may be NULL): kept records, records skipped by flag,
 * skipped for l_seq == 0, and windows whose speculated entry was wrong and that were walked again.  Waits for the framing. */
int  vg_fastq_stream_begin_bam(vg_index *ix);
int  vg_bam_stream_stats(vg_index *ix, uint64_t *kept, uint64_t *skipped_flag, uint64_t *skipped_empty, uint64_t *repairs);

/* BAM without a handle.
 * vg_bam_frame_device: a whole BAM file in host memory through the stream's kernels as ONE slot, the flat batch layout back:
 * offsets[0 .. n] (offsets[n] = total bases), the bases as ASCII, one gate word per read (bit c: quality character c < '8', for
 * c < min(length / 32, 32)).  stats[4] = kept, skipped by flag, skipped empty, repairs.  *bad_offset = UINT64_MAX when the whole
 * stream was framed, else the inflated offset of the first byte that was not (a refusal: vg_last_error() says which; the stream ends
 * inside a record or the header; a bad block) -- the call still returns VG_OK and the arrays hold what was framed (nothing, after a
 * refusal).  VG_EIO: not BAM.  VG_ETOOBIG: the reads do not fit cap_rec / cap_bases.  Files of less than 2 GiB.
 * vg_bam_to_fastq_host: the equivalent FASTQ text, by the host build of the same record parser; no device is touched.  *n_records =
 * records converted; *bad_offset as above (UINT64_MAX, or the inflated offset where conversion stopped: the stream ends inside a
 * record or the header, a block_size too small for its record, a bad block); text of the records before it is there. */
int  vg_bam_frame_device(int device, const uint8_t *bgzf, uint64_t nbytes, uint64_t *offsets, uint64_t cap_rec, uint8_t *bases, uint64_t cap_bases, uint32_t *gate,
                         uint64_t *n_records, uint64_t stats[4], uint64_t *bad_offset);
int  vg_bam_to_fastq_host(const uint8_t *bgzf, uint64_t nbytes, uint8_t *text, uint64_t text_cap, uint64_t *text_len, uint64_t *n_records, uint64_t *bad_offset);

/* BGZF without a handle: the whole blocks of bgzf[0, nbytes) inflated into text[0, text_cap) in host memory -- on `device` by the
 * stream's kernel (compressed bytes up, text back), or on the host by the host build of the same decoder.  *text_len = bytes of text
 * written, *consumed = compressed bytes used (trailing bytes of an incomplete block are not), *bad_block_offset = compressed offset
 * of the first block that failed (header, deflate error, size or CRC; UINT64_MAX: none) -- the text of the blocks before it is
 * there, *consumed stops at it, vg_last_error() has the reason, and the call still returns VG_OK.  VG_ETOOBIG: the text does not
 * fit text_cap (nothing is written beyond it).  Buffers of less than 4 GiB.  With VG_VERBOSE set the device form prints the
 * kernel's own time and rate. */
int  vg_bgzf_inflate_device(int device, const uint8_t *bgzf, uint64_t nbytes, uint8_t *text, uint64_t text_cap, uint64_t *text_len, uint64_t *consumed, uint64_t *bad_block_offset);
int  vg_bgzf_inflate_host(const uint8_t *bgzf, uint64_t nbytes, uint8_t *text, uint64_t text_cap, uint64_t *text_len, uint64_t *consumed, uint64_t *bad_block_offset);
/* The header walk alone: every whole block of bgzf[0, nbytes) as six numbers in blocks[6 * i ..]: compressed offset, text offset,
 * payload offset, payload length, ISIZE, CRC32.  *consumed / *bad_block_offset as above (header errors only). */
int  vg_bgzf_scan_host(const uint8_t *bgzf, uint64_t nbytes, uint64_t *blocks, uint64_t blocks_cap, uint64_t *n_blocks, uint64_t *consumed, uint64_t *bad_block_offset);

/* The other direction: text[0, nbytes) in host memory written as BGZF into bgzf[0, cap), *bgzf_len = its bytes.  `block` = text bytes
 * per block: 0 means 65 280 (htslib's), 1 ... 65 280 are allowed, anything above is VG_EINVAL.  eof != 0 appends htslib's 28-byte
 * empty block (empty text with eof gives exactly that marker).  A block is fixed-Huffman DEFLATE with matches of 4 ... 258 bytes, or
 * stored when that would not be smaller than its text; its header is bgzip's (MTIME 0, XFL 0, OS ff, one BC subfield).  The bytes
 * are a function of the text and `block` alone: the same from the host form on any number of `threads` and from the device form,
 * and the concatenation of calls over pieces cut at multiples of `block` (all but the last with eof = 0) is the one call's output.
 * vg_bgzf_deflate_bound: what always fits (every block stored, plus the marker; 0 for a `block` that is refused).  VG_ETOOBIG: cap
 * is too small, nothing is written.  VG_EINVAL: a null pointer.  The device form never falls back: VG_ENODEV without a device,
 * VG_ENOMEM without device memory (nothing is left behind); with VG_VERBOSE set it prints the kernels' own time and rate. */
uint64_t vg_bgzf_deflate_bound(uint64_t nbytes, uint32_t block);
int  vg_bgzf_deflate_host(const uint8_t *text, uint64_t nbytes, uint32_t block, int eof, int threads, uint8_t *bgzf, uint64_t cap, uint64_t *bgzf_len);
int  vg_bgzf_deflate_device(int device, const uint8_t *text, uint64_t nbytes, uint32_t block, int eof, uint8_t *bgzf, uint64_t cap, uint64_t *bgzf_len);
/* The same with the coding mode named.  VG_DEFLATE_FIXED: the two calls above, byte for byte.  VG_DEFLATE_DYNAMIC: the same match
 * finder; every block is one DEFLATE block in the smallest of three forms -- stored, fixed codes, or dynamic codes (BTYPE 2) built
 * for the block from its own symbol counts, lengths limited to 15 (7 for the code-length code) -- so no block is larger than in
 * the fixed mode, and one that takes the stored or the fixed form is that mode's block.  Everything said above about the bytes
 * (host = device, threads, cuts at block boundaries), the bound and the errors holds in either mode.  Another `codes`: VG_EINVAL. */
enum { VG_DEFLATE_FIXED = 0, VG_DEFLATE_DYNAMIC = 1 };
int  vg_bgzf_deflate_host_coded(const uint8_t *text, uint64_t nbytes, uint32_t block, int eof, int threads, int codes, uint8_t *bgzf, uint64_t cap, uint64_t *bgzf_len);
int  vg_bgzf_deflate_device_coded(int device, const uint8_t *text, uint64_t nbytes, uint32_t block, int eof, int codes, uint8_t *bgzf, uint64_t cap, uint64_t *bgzf_len);
/* The code-length builder of the dynamic mode, for callers who build their own streams: n_sets independent histograms
 * freq[set * n_sym + symbol] of 2 <= n_sym <= 288 counters each -> lens[set * n_sym + symbol], a Huffman code's lengths, none above
 * `limit` (1 <= limit <= 15, n_sym <= 2^limit).  Integers only, ties broken by symbol number; a symbol with count 0 gets length 0,
 * except that a set with fewer than two symbols in use has its lowest unused symbols join them at length 1; the Kraft sum of every
 * set is exactly 1.  The device form runs one wave per histogram and returns the host form's bytes.  VG_EINVAL: a null pointer,
 * sizes outside the above, or a histogram whose counts sum to 2^32 or more. */
int  vg_deflate_code_lengths_host(const uint32_t *freq, uint32_t n_sets, uint32_t n_sym, uint32_t limit, uint8_t *lens);
int  vg_deflate_code_lengths_device(int device, const uint32_t *freq, uint32_t n_sets, uint32_t n_sym, uint32_t limit, uint8_t *lens);

/* Plain gzip (RFC 1952 members around one DEFLATE stream: what gzip, pigz and sequencers write; no block table) without a handle.
 * gz[0, nbytes) is inflated member after member into text[0, text_cap) in host memory; *text_len = bytes of text, *consumed =
 * compressed bytes used, both at the end of the last member that was decoded whole with its CRC32 and ISIZE (mod 2^32) verified.
 * Bad data -- a truncated member, a CRC32 or ISIZE mismatch, bytes after a member that are no gzip header, a broken DEFLATE block --
 * returns VG_EIO: *bad_offset is the compressed offset and vg_last_error() names it with the decoder's reason.  VG_ETOOBIG: the
 * text does not fit.
 *   vg_gunzip_host            the reference decoder: sequential, one thread
 *   vg_gunzip_device          the chunked route on `device`: the compressed bytes are cut into slots and the slots into chunks; a
 *                             wave per chunk guesses a block start and decodes from it into 16-bit symbols, the guesses are
 *                             confirmed against their predecessors' exits, the wrong ones repaired in order, and the symbols
 *                             resolved into text (DESIGN.md §4 "The plain-gzip kernels"; the routes are in §5).  The result is the reference decoder's whatever was guessed.
 *   vg_gunzip_chunked_host    the same stages run on the host, one after the other: what the kernels do, with no device
 * The chunked calls take their sizes from `opts` (a field that is 0, or opts NULL: from the environment, read at every call): VG_GZ_CHUNK (compressed bytes per chunk, default 16384),
 * VG_GZ_SLOT (compressed bytes per slot, default 16 MiB, at most 64 MiB), VG_GZ_MAX_RATIO (a slot's text capacity as a multiple of
 * its compressed bytes, default 8), VG_GZ_SLOT_MAX (a slot that holds no whole DEFLATE block is tried again twice as long, up to
 * this many bytes, default and at most 64 MiB; beyond it the call fails with VG_EIO, "deflate block larger than a slot").  A slot whose text would exceed that bound, or that needs more than 64 repairs, is REFUSED, never
 * overrun: the call returns VG_OK with stats->slots_refused = 1, *text_len / *consumed at that slot's entry -- a block boundary,
 * whose exact bit offset is stats->resume_bit (*consumed = resume_bit / 8) -- and the caller decodes on from there by other means. */
typedef struct vg_gzip_opts {
	uint64_t chunk_bytes;      /* VG_GZ_CHUNK */
	uint64_t slot_bytes;       /* VG_GZ_SLOT */
	uint64_t max_ratio;        /* VG_GZ_MAX_RATIO */
	uint64_t slot_max;         /* VG_GZ_SLOT_MAX */
} vg_gzip_opts;
typedef struct vg_gzip_stats {
	uint64_t members;          /* members decoded whole and verified */
	uint64_t chunks;           /* chunks of all slots */
	uint64_t guessed;          /* chunks with an entry: a slot's chunk 0, or a guess of the finder */
	uint64_t confirmed;        /* guesses that were their predecessor's exit */
	uint64_t repaired;         /* chunks decoded again from their predecessor's exit */
	uint64_t tested;           /* bit offsets that passed the prefilter and took the full header test */
	uint64_t slots_refused;
	uint64_t resume_bit;       /* compressed bit offset of the last block boundary reached (a member's end: its next byte) */
} vg_gzip_stats;
int  vg_gunzip_host(const uint8_t *gz, uint64_t nbytes, uint8_t *text, uint64_t text_cap, uint64_t *text_len, uint64_t *consumed, uint64_t *bad_offset);
int  vg_gunzip_device(int device, const uint8_t *gz, uint64_t nbytes, uint8_t *text, uint64_t text_cap, uint64_t *text_len, uint64_t *consumed, uint64_t *bad_offset, vg_gzip_stats *stats, const vg_gzip_opts *opts);
int  vg_gunzip_chunked_host(const uint8_t *gz, uint64_t nbytes, uint8_t *text, uint64_t text_cap, uint64_t *text_len, uint64_t *consumed, uint64_t *bad_offset, vg_gzip_stats *stats, const vg_gzip_opts *opts);
/* The same decisions over PUSHES of push_bytes, on the host: what a gzip stream (below) does with bytes cut anywhere -- the incomplete
 * tail block, a header or a trailer cut short wait for the next push.  Results as vg_gunzip_chunked_host's, byte for byte. */
int  vg_gunzip_pushed_host(const uint8_t *gz, uint64_t nbytes, uint64_t push_bytes, uint8_t *text, uint64_t text_cap, uint64_t *text_len, uint64_t *consumed, uint64_t *bad_offset, vg_gzip_stats *stats, const vg_gzip_opts *opts);

/* The device-framed FASTQ stream over plain gzip.  After vg_fastq_stream_begin_gzip, vg_fastq_stream_push takes gzip bytes cut
 * anywhere; whole slots of them (VG_GZ_SLOT, read at begin like the other VG_GZ_* sizes) are inflated on the device by the chunked
 * route above and their text is framed where it lies; the bytes of an incomplete block wait on the host for the next push.
 * vg_fastq_stream_end inflates what is left, and returns VG_OK only when every member's CRC32 and ISIZE were verified; bad data is
 * VG_EIO, vg_last_error() naming the compressed offset and the reason.  Offsets it reports (consumed, last_record_start) are TEXT
 * offsets.  A REFUSED slot (text beyond the ratio bound, more than 64 repairs) poisons the stream as a refused text chunk does:
 * nothing of it or after it is framed, *refused = 1, and the caller takes over on the host:
 *   vg_fastq_stream_gzip_checkpoint   the last slot entry at or before a text offset: its compressed BIT offset in the file (a
 *                                     DEFLATE block boundary inside a member), the text offset there, and the member's text in
 *                                     front of it (window[0, *window_len), at most 32768 bytes) -- enough to inflate on from there.
 *                                     The member's CRC32 cannot be checked by who starts there.  No slot entered: bit offset 0.
 *   vg_gzip_stream_stats              the counts of the stream so far (valid until the next vg_fastq_stream_begin_gzip) */
int  vg_fastq_stream_begin_gzip(vg_index *ix);
int  vg_gzip_stream_stats(vg_index *ix, vg_gzip_stats *stats);
int  vg_fastq_stream_gzip_checkpoint(vg_index *ix, uint64_t text_offset, uint64_t *comp_bit_offset, uint64_t *ckpt_text_offset, uint8_t *window, uint32_t *window_len);

/* One self-contained chunk, synchronously: *consumed = bytes used (the rest, an incomplete last record, is the caller's to
 * resubmit with the next chunk); waits for the framing, not for the read loop.  VG_EBADREAD: the chunk was refused (see above);
 * nothing was processed. */
int  vg_fastq_submit(vg_index *ix, const uint8_t *text, uint64_t nbytes,
                     uint64_t *n_records, uint64_t *consumed, uint64_t *last_record_start);

/* The host-side framing + packing on its own (no device is touched): for a caller that packs on its own threads and hands the
 * batches to vg_reads_submit_packed.  A packer is a stream like the one above: push chunks cut anywhere; each push returns the
 * complete records it framed (arrays sized with vg_packer_reads_cap / _kmers_cap of the chunk's length); vg_packer_end reports
 * records, bytes consumed, the start of the last framed record and whether a chunk was refused (nothing of a refused chunk or of
 * what follows it is returned). */
typedef struct vg_packer vg_packer;
int  vg_packer_create(int host_threads, vg_packer **out);
void vg_packer_destroy(vg_packer *pk);
int  vg_packer_begin(vg_packer *pk);
uint64_t vg_packer_reads_cap(uint64_t nbytes);
uint64_t vg_packer_kmers_cap(uint64_t nbytes);
int  vg_packer_push(vg_packer *pk, const uint8_t *text, uint64_t nbytes, uint64_t *kmers, uint64_t kmers_cap, uint64_t *meta,
                    uint64_t *chunk_offsets, uint64_t reads_cap, uint64_t *n_reads, uint64_t *n_chunks, uint64_t *n_invalid);
int  vg_packer_end(vg_packer *pk, uint64_t *n_records, uint64_t *consumed, uint64_t *last_record_start, int *refused);

int  vg_sync(vg_index *ix);                       /* drain the stream                          */
int  vg_stats_get(vg_index *ix, vg_stats *out);   /* implies vg_sync                           */
int  vg_set_stats(vg_index *ix, int enable);      /* event counting on (default) / off: the
                                                     counting build of the kernel carries ~50 extra
                                                     registers per lane, so timed runs switch it off */
int  vg_timing_get(vg_index *ix, vg_timing *out);
/* Passes whose gate-open pairs the main wave tier let wait for a later iteration's stage B ("held pairs", csrc/vg_wave.h), over
 * the batches harvested since open / vg_counts_reset (call vg_sync first).  A schedule figure, never a result: the counters are
 * the same for every setting of VG_HOLD_PAIRS, and 0 here when that is 0. */
uint64_t vg_held_passes(const vg_index *ix);

/* SNP sites = positions seeded with ref != alt (qv.cc:637-659, 1580), ascending.
 * Counters are exact sums; the reference's 6-bit saturation (vartype.h:27, qv.cc:1411, 1419) is
 * min(63, sum) and is applied by vg_counts_fetch. */
uint64_t vg_num_sites(const vg_index *ix);
int  vg_sites_fetch(vg_index *ix, uint32_t *pos, uint8_t *ref_base, uint8_t *alt_base,
                    uint8_t *ref_freq, uint8_t *alt_freq);
int  vg_counts_fetch(vg_index *ix, uint8_t *ref_cnt, uint8_t *alt_cnt);    /* clamped at 63     */
int  vg_counts_reset(vg_index *ix);

/* Replaces the caller, qv.cc:1789-1848 (posterior) and :1681 (the GQ column): the step that turns the counters into an answer.
 * Per site gt = 0 not called (no reads, or both counters saturated), 1 hom-ref, 2 hom-alt, 3 het -- the reference's GTYPE_*
 * numbering -- and gq = (int)(-10 ln(confidence)) exactly as the reference prints it (0 where gt is 0; -2147483648 where allele
 * frequencies whose squares sum above 1 make the confidence negative, as there).
 * A kernel computes the call where the counters live, one lane per site, and 2 bytes per site cross the link (gt << 14 | gq).  The
 * arithmetic up to the confidence is the host caller's own, bit for bit (csrc/vg_caller.h: one function for both, contraction
 * off, the per-count factor tables computed once on the host with libm and uploaded).  The logarithm is not: the kernel settles a
 * site only when its -10 ln(confidence) lies farther than a guard (1e-6) from the nearest integer, the confidence is inside (0, 1)
 * and the result is below 16383; every other site leaves the device with an escape code and is recomputed on the host with libm
 * before the call returns.  The values handed out are final.
 *   vg_sample_calls_fetch   the selected sample (vg_sample_select), like vg_counts_fetch: implies vg_sync; with several replicas
 *                           the all-reduce comes first.  gt, gq: vg_num_sites entries each.  *n_escaped (may be NULL): the sites
 *                           the host recomputed.  The first call takes 4 bytes of device memory per site (the sites' frequency
 *                           columns and the staging) plus ~5 KiB, outside the plan, counted by vg_index_device_bytes; VG_ENOMEM
 *                           for it leaves the handle usable (and the caller with vg_counts_fetch and a host loop)
 *   vg_call_device          the same kernel without a handle, over n quadruples in host memory (counters are clamped at 63 first):
 *                           what drives it over the caller's whole domain.  guard <= 0: the default; a guard must be below 0.5 */
int  vg_sample_calls_fetch(vg_index *ix, uint8_t *gt, int32_t *gq, uint64_t *n_escaped);
int  vg_call_device(int device, const uint8_t *ref_cnt, const uint8_t *alt_cnt, const uint8_t *ref_freq, const uint8_t *alt_freq,
                    uint64_t n, double guard, uint8_t *gt, int32_t *gq, uint64_t *n_escaped);

/* The genotype matrix of a cohort and its first consumer, the pairwise sample table: are two samples the same individual, swapped,
 * related?  No reference counterpart (the reference genotypes one sample per process).  The rules live in csrc/vg_pairs.h, one
 * statement for the host loop and the kernels: a call (gt, gq) of vg_sample_calls_fetch is COUNTED iff gt != 0 && gq >= min_gq; a
 * counted call is of class R (gt 1), A (gt 2) or H (gt 3), C = R | H | A; a sample is three bit planes of ceil(n_sites / 64) words.
 * The table is counts[i][j][5] for ALL i, j, in the order n = |Ci & Cj|, ibs0 = |Ri&Aj | Ai&Rj|, ibs2 = |Ri&Rj | Hi&Hj | Ai&Aj|,
 * hethet = |Hi & Hj|, het_i = |Hi & Cj| ([j][i][4] is "j het where i is counted"); the diagonal is the sample with itself:
 * n = its counted sites = ibs2, ibs0 = 0, hethet = het_i = its hets.  Integer sums: the result is exact whatever the launch.
 * A vg_gmatrix lives on one device and is tied to no vg_index; a handle is thread-compatible.
 *   vg_gmatrix_create        planes for n_samples samples (1 .. 16 384; 0: VG_EINVAL, more: VG_ETOOBIG) of n_sites sites (below 2^32,
 *                            else VG_EINVAL; 0 is allowed: every count is 0), the n_samples^2 x 40-byte result (10.7 GB at the cap)
 *                            and one sample's columns of staging (5 bytes per site).  VG_ENOMEM leaves nothing behind
 *   vg_gmatrix_set           one sample's final gt / gq columns (host arrays of n_sites entries, free again on return) packed into its
 *                            planes by a kernel.  A sample never set is all-missing; setting a sample again replaces it.  VG_EINVAL:
 *                            a null pointer, a sample out of range -- the matrix stays as it was
 *   vg_gmatrix_pairs         the table into counts[n_samples * n_samples * 5] (host memory).  Synchronous.  words_per_block: site
 *                            words one workgroup of the pair kernel counts (the site range is a grid dimension, so that a few
 *                            samples still make many workgroups); 0 = the default, 1024; made larger where the grid would pass
 *                            65 535 blocks, and at most 2^24.  With VG_VERBOSE set the call prints the kernels' own time and rate
 *   vg_gmatrix_device_bytes  device memory the matrix holds (0 for a null handle)
 *   vg_pairs_host            the same table by the same header on `threads` host threads (< 1: one), from gt / gq laid out
 *                            [n_samples][n_sites], sample-major.  Touches no device */
typedef struct vg_gmatrix vg_gmatrix;
int  vg_gmatrix_create(int device, uint64_t n_sites, uint32_t n_samples, vg_gmatrix **out);
int  vg_gmatrix_set(vg_gmatrix *gm, uint32_t sample, const uint8_t *gt, const int32_t *gq, int32_t min_gq);
int  vg_gmatrix_pairs(vg_gmatrix *gm, uint64_t words_per_block, uint64_t *counts);
uint64_t vg_gmatrix_device_bytes(const vg_gmatrix *gm);
void vg_gmatrix_destroy(vg_gmatrix *gm);
int  vg_pairs_host(const uint8_t *gt, const int32_t *gq, uint64_t n_sites, uint32_t n_samples, int32_t min_gq, int threads, uint64_t *counts);

/* The cohort prior: the samples of a cohort called again, with the alt allele frequency q of every site estimated from the cohort
 * itself in place of the dictionary's two frequencies.  No reference counterpart (the reference calls one sample per process).  The
 * rule lives in csrc/vg_cprior.h, one statement for the host loop and the kernel: a sample is informative at a site iff
 * vg_call_site would call it; q starts at the dictionary's alt_freq / (ref_freq + alt_freq) (0.5 where both are 0), and `iters` EM
 * passes (1 .. 64; 8 is the default of the command line) replace it by (expected alt alleles of the informative samples under
 * Hardy-Weinberg at q + pseudo * the dictionary's) / (2 * informative samples + pseudo), clamped to [1e-6, 1 - 1e-6]; `pseudo`
 * (finite, >= 0; 2.0 by default) is the dictionary's weight in alleles.  An informative sample's call is the caller's own choice
 * among hom-ref / het / hom-alt under Hardy-Weinberg at the final q, its confidence the posterior x the Poisson(7.1) mass of its
 * depth, gq = (int)(-10 ln(confidence)); any other sample has gt 0, gq 0.  gt / gq are the numbering and the columns of
 * vg_sample_calls_fetch.  The arithmetic up to the confidence is bit for bit the host loop's; the logarithm is not shared, as in the
 * caller: the kernel leaves an entry whose -10 ln(confidence) lies within `guard` of an integer with an escape code, and the host
 * recomputes such an entry with libm before it is handed out.  The values handed out are final.
 * A vg_cprior lives on one device and is tied to no vg_index; a handle is thread-compatible.
 *   vg_cprior_create        ALL device memory the handle will ever use: the samples' counters and their calls, sample-major, 2 bytes
 *                           per site and sample each; q, 8 bytes per site; the two frequency columns, 1 byte per site each; one
 *                           sample's two counter columns of staging, 2 bytes per site; the caller's factor tables (5 104 bytes) and
 *                           the escape count (8): 4 * n_samples * n_sites + 12 * n_sites + 5 112 bytes, an empty buffer counting 8.
 *                           The handle also keeps 8 bytes per site of host memory.  n_samples 1 .. 16 384 (0: VG_EINVAL, more:
 *                           VG_ETOOBIG), n_sites below 2^32 (else VG_EINVAL; 0 is allowed).  VG_ENOMEM leaves nothing behind
 *   vg_cprior_set           one sample's counter columns as vg_counts_fetch hands them out (host arrays of n_sites entries, free again
 *                           on return; clamped again at 63).  A sample never set is uninformative everywhere; setting a sample again
 *                           replaces it.  VG_EINVAL: a null pointer, a sample out of range -- the handle stays as it was
 *   vg_cprior_run           the kernel over the counters as they are, with the sites' frequency bytes (host arrays of n_sites
 *                           entries).  Synchronous.  q_out (may be NULL): n_sites doubles, the final q.  *n_escaped (may be NULL): the
 *                           entries the kernel left to the host; they are recomputed as vg_cprior_calls hands their column out.
 *                           guard <= 0: the default, 1e-6; a guard must be below 0.5.  VG_EINVAL: iters or pseudo outside their
 *                           ranges.  With VG_VERBOSE set the call prints the kernel's own time
 *   vg_cprior_calls         the final gt / gq columns of one sample (n_sites entries each) after a run; VG_EINVAL without one, or
 *                           when a sample was set since
 *   vg_cprior_device_bytes  device memory the handle holds (0 for a null handle)
 *   vg_cprior_host          the same q, gt and gq by the header's host loop on `threads` host threads (< 1: one), from counters laid
 *                           out [n_samples][n_sites], sample-major, into gt / gq of that layout and q_out (may be NULL).  Touches no
 *                           device */
#ifndef VG_CPRIOR_ITERS
#define VG_CPRIOR_ITERS     8      /* the defaults of the command line and the Python binding */
#define VG_CPRIOR_PSEUDO    2.0
#define VG_CPRIOR_ITERS_MAX 64
#endif
typedef struct vg_cprior vg_cprior;
int  vg_cprior_create(int device, uint64_t n_sites, uint32_t n_samples, vg_cprior **out);
int  vg_cprior_set(vg_cprior *cp, uint32_t sample, const uint8_t *ref_cnt, const uint8_t *alt_cnt);
int  vg_cprior_run(vg_cprior *cp, const uint8_t *ref_freq, const uint8_t *alt_freq, int iters, double pseudo, double guard, double *q_out, uint64_t *n_escaped);
int  vg_cprior_calls(vg_cprior *cp, uint32_t sample, uint8_t *gt, int32_t *gq);
uint64_t vg_cprior_device_bytes(const vg_cprior *cp);
void vg_cprior_destroy(vg_cprior *cp);
int  vg_cprior_host(const uint8_t *ref_cnt, const uint8_t *alt_cnt, uint64_t n_sites, uint32_t n_samples, const uint8_t *ref_freq, const uint8_t *alt_freq, int iters, double pseudo, int threads,
                    uint8_t *gt, int32_t *gq, double *q_out);

/* The data lines of the joint (multi-sample) VCF rendered on the device.  No reference counterpart.  The rules live in csrc/vg_jtext.h,
 * one statement for the host loop and the kernels.  A sample's CELL for a call (gt, gq) of vg_sample_calls_fetch is "\t" + "0/0" (gt 1),
 * "1/1" (gt 2) or "0/1" (gt 3) + ":" + gq as "%d" prints an int32 (any value: 6 to 16 bytes); a sample without a call shows "\t./.:.".
 * A RECORD is one data line of the SNP list whose key names sites of the index: its first eight fields heads[head_off, +head_len) and
 * the run sites[site_at, +n_sites) of site indices of that key in genome order (not necessarily consecutive).  Every sample shows the
 * call of the LAST site of the run at which its gt != 0.  If no sample has one the record produces no bytes; otherwise its LINE is
 * the head, "\tGT:GQ", the cells in sample order, "\n".  The text of a span of records is at most
 * vg_jtext_text_bound = the sum of head_len + n_records * (7 + 16 * n_samples) bytes.
 * A vg_jtext lives on one device and is tied to no vg_index; a handle is thread-compatible.
 *   vg_jtext_create        ALL device memory the handle will ever use (later calls never allocate): the samples' columns, sample-major,
 *                          2 bytes per site and sample (gt << 14 | gq); `wide_samples` wide columns of 4 bytes per site for samples
 *                          that have a gq outside 0 .. 16382; one sample's columns of staging (5 bytes per site); and the buffers of a
 *                          span of at most max_records records, max_head_bytes bytes of heads and max_site_refs site references: those,
 *                          ceil(n_samples / 64) + 1 lengths and offsets (12 bytes each) and 12 bytes of counts per record and the
 *                          span's text bound + 80 KiB.
 *                          with_bgzf != 0: also the work buffers of the BGZF stream below (about 110 MB).  n_samples 1 .. 16 384 (0:
 *                          VG_EINVAL, more: VG_ETOOBIG), n_sites below 2^32.  VG_ENOMEM leaves nothing behind; VG_ENODEV without a device
 *   vg_jtext_set           one sample's final gt / gq columns (host arrays of n_sites entries, free again on return).  A sample never
 *                          set is all-missing; setting a sample again replaces it.  VG_EINVAL: a null pointer, a sample out of range,
 *                          a gt above 3; VG_ETOOBIG: the sample needs a wide column and none is free -- the handle stays as it was
 *   vg_jtext_render        the text of a span into text[0, cap) in host memory: *len bytes, *n_lines records that produced a line.
 *                          Synchronous.  VG_ETOOBIG: cap below the span's bound, or a span beyond the limits of create; VG_EINVAL: a
 *                          null pointer, a head or a site run outside its array, a site index >= n_sites, an open stream -- nothing is
 *                          written.  With VG_VERBOSE set the call prints the kernels' own time and rate
 *   vg_jtext_render_host   the same bytes by the header's host loop on `threads` threads (< 1: one), from per-sample column pointers
 *                          gt[s], gq[s] (gt[s] NULL: never set).  Touches no device; no limits but the cap
 *   vg_jtext_device_bytes  device memory the handle holds (0 for a null handle)
 * The BGZF stream (with_bgzf): text is joined on the device and leaves it compressed.  After vg_jtext_bgzf_begin(block, codes) -- as
 * vg_bgzf_deflate_host_coded's -- vg_jtext_bgzf_text joins host bytes (header lines), vg_jtext_bgzf_lines the rendered text of a span
 * (*text_len bytes of it, *n_lines lines), vg_jtext_bgzf_end the last partial block and the end-of-file marker.  Each call hands
 * back, in bgzf[0, *bgzf_len), the blocks it completed; text short of a block stays pending on the device.  The concatenation of
 * everything handed back is vg_bgzf_deflate_host_coded(the whole text, block, eof 1, codes), byte for byte.  cap must be at least
 * vg_jtext_bgzf_bound(bytes of text the call may add, block) -- for _lines the span's text bound, for _end 0 -- else VG_ETOOBIG and
 * nothing happens.  A call without an open stream, or begin on a handle created without with_bgzf: VG_EINVAL.
 * The INFO mode (opt-in; the calls above are the _info calls with VG_JT_INFO_NONE and write the bytes they always wrote).  With
 * VG_JT_INFO_COUNTS a line's head carries the record's allele counts over the calls the line SHOWS: NS = samples whose shown call has
 * gt != 0, AN = 2 NS, AC = hets + 2 hom-alts, AF = AC / AN rounded half up to six decimals without trailing zeros ("0", "1", "0.5",
 * "0.333333"), as the tag "NS=<NS>;AN=<AN>;AC=<AC>;AF=<AF>" (at most 38 bytes).  A head with exactly seven tabs has eight fields: an
 * INFO of "." is replaced by the tag, an empty INFO gets the tag, any other gets ";" and the tag; a head with another number of tabs
 * is written unchanged.  A span's bound grows by VG_JT_INFO_MAX = 40 bytes per record.  Any other mode: VG_EINVAL (the bound: 0).
 *   vg_jtext_create_info        vg_jtext_create with the mode, which belongs to the handle: render, bgzf_lines and the index that
 *                               follows the stream write and scan the text of that mode (the text buffer is sized by that mode's bound)
 *   vg_jtext_text_bound_info    the bound of a span in a mode: what render's cap and bgzf_lines' bound take on such a handle
 *   vg_jtext_render_host_info   vg_jtext_render_host in a mode
 *   vg_jtext_counts             the numbers without the text, on a handle of either mode: counts[n_records][3] = NS, het, hom of every
 *                               record, zeros for a record that produces no line.  Reads no head (head_off, head_len are ignored).
 *                               Errors as render's; allowed while a stream is open
 *   vg_jtext_counts_host        the same from per-sample column pointers, on the host */
#ifndef VG_JT_INFO_NONE
#define VG_JT_INFO_NONE   0
#define VG_JT_INFO_COUNTS 1
#define VG_JT_INFO_MAX    40
#endif
#ifndef VG_JTEXT_RECORD_DEFINED
#define VG_JTEXT_RECORD_DEFINED
typedef struct vg_jtext_record {
	uint64_t head_off;     /* the first eight fields: heads[head_off, head_off + head_len) */
	uint64_t site_at;      /* the key's sites: sites[site_at, site_at + n_sites) */
	uint32_t head_len;
	uint32_t n_sites;
} vg_jtext_record;
#endif
typedef struct vg_jtext vg_jtext;
int  vg_jtext_create(int device, uint64_t n_sites, uint32_t n_samples, uint32_t wide_samples, uint64_t max_records, uint64_t max_head_bytes, uint64_t max_site_refs, int with_bgzf, vg_jtext **out);
void vg_jtext_destroy(vg_jtext *jt);
uint64_t vg_jtext_device_bytes(const vg_jtext *jt);
int  vg_jtext_set(vg_jtext *jt, uint32_t sample, const uint8_t *gt, const int32_t *gq);
uint64_t vg_jtext_text_bound(uint64_t head_bytes, uint64_t n_records, uint32_t n_samples);
uint64_t vg_jtext_bgzf_bound(uint64_t text_bytes, uint32_t block);
int  vg_jtext_render(vg_jtext *jt, const uint8_t *heads, uint64_t heads_len, const vg_jtext_record *records, uint64_t n_records, const uint32_t *sites, uint64_t n_site_refs,
                     uint8_t *text, uint64_t cap, uint64_t *len, uint64_t *n_lines);
int  vg_jtext_render_host(uint64_t n_sites, uint32_t n_samples, const uint8_t *const *gt, const int32_t *const *gq, const uint8_t *heads, uint64_t heads_len, const vg_jtext_record *records, uint64_t n_records,
                          const uint32_t *sites, uint64_t n_site_refs, int threads, uint8_t *text, uint64_t cap, uint64_t *len, uint64_t *n_lines);
int  vg_jtext_bgzf_begin(vg_jtext *jt, uint32_t block, int codes);
int  vg_jtext_bgzf_text(vg_jtext *jt, const uint8_t *text, uint64_t nbytes, uint8_t *bgzf, uint64_t cap, uint64_t *bgzf_len);
int  vg_jtext_bgzf_lines(vg_jtext *jt, const uint8_t *heads, uint64_t heads_len, const vg_jtext_record *records, uint64_t n_records, const uint32_t *sites, uint64_t n_site_refs,
                         uint8_t *bgzf, uint64_t cap, uint64_t *bgzf_len, uint64_t *text_len, uint64_t *n_lines);
int  vg_jtext_bgzf_end(vg_jtext *jt, uint8_t *bgzf, uint64_t cap, uint64_t *bgzf_len);
int  vg_jtext_create_info(int device, uint64_t n_sites, uint32_t n_samples, uint32_t wide_samples, uint64_t max_records, uint64_t max_head_bytes, uint64_t max_site_refs, int with_bgzf, int info, vg_jtext **out);
uint64_t vg_jtext_text_bound_info(uint64_t head_bytes, uint64_t n_records, uint32_t n_samples, int info);
int  vg_jtext_render_host_info(uint64_t n_sites, uint32_t n_samples, const uint8_t *const *gt, const int32_t *const *gq, const uint8_t *heads, uint64_t heads_len, const vg_jtext_record *records, uint64_t n_records,
                               const uint32_t *sites, uint64_t n_site_refs, int info, int threads, uint8_t *text, uint64_t cap, uint64_t *len, uint64_t *n_lines);
int  vg_jtext_counts(vg_jtext *jt, const vg_jtext_record *records, uint64_t n_records, const uint32_t *sites, uint64_t n_site_refs, uint32_t *counts);
int  vg_jtext_counts_host(uint64_t n_sites, uint32_t n_samples, const uint8_t *const *gt, const int32_t *const *gq, const vg_jtext_record *records, uint64_t n_records, const uint32_t *sites, uint64_t n_site_refs,
                          uint32_t *counts);

/* The tabix index (.tbi) of a BGZF VCF, made while the file is compressed.  No reference counterpart.  The rules -- which lines
 * count, coordinates, bins, chunks, the linear index, the file layout -- live in csrc/vg_vcfidx.h, stated once for the host scanner
 * and the scan kernels; small bins are not merged into their parents and INFO/END is not read (both differ from htslib, both are
 * valid), coordinates end at 2^29.  A vg_vcfidx is a streaming handle tied to no vg_index and no device; thread-compatible.
 *   vg_vcfidx_create       `block`: text bytes per BGZF block of the file (0: 65 280; above: VG_EINVAL)
 *   vg_vcfidx_text_host    the next n bytes of the VCF text, cut anywhere (mid-line, mid-field), scanned on `threads` host threads
 *   vg_vcfidx_text_device  the same state afterwards, by upload and the scan kernels on `device`.  It never falls back: VG_ENODEV or
 *                          VG_ENOMEM leaves the handle as it was, so the same bytes can go to the host form
 *   vg_vcfidx_bgzf         the file's BGZF bytes as they are produced: whole blocks, sizes read from BSIZE (else VG_EINVAL); the
 *                          end-of-file marker is ignored
 *   vg_vcfidx_finish       ends the text (a last line without '\n' is a line) and writes the raw index bytes to tbi[0, cap), *len of
 *                          them; vg_vcfidx_bound says what fits them.  VG_EINVAL: the index was refused, or the blocks fed are not
 *                          those of the text fed.  VG_ETOOBIG: cap is too small.  The .tbi FILE is these bytes through
 *                          vg_bgzf_deflate_host_coded(block 0, eof 1, VG_DEFLATE_FIXED)
 *   vg_vcfidx_error        after a data line broke a rule: the rule's words and *offset = the line's offset in the text; NULL while
 *                          the index stands.  A refusal is sticky: later text is counted and ignored, the compressor never sees it
 *   vg_vcfidx_stats        out[0 .. 5): data lines, chromosomes, bins, chunks, microseconds spent scanning
 * Two fused forms, so that text is uploaded once:
 *   vg_bgzf_deflate_device_indexed  vg_bgzf_deflate_device_coded that also scans each uploaded chunk while it is resident and feeds
 *                          the blocks it made (not the marker) to idx.  idx == NULL: the old call, byte for byte.  A chunk whose
 *                          scan finds no device memory is scanned by the host scanner (one line with VG_VERBOSE)
 *   vg_jtext_bgzf_index    after vg_jtext_bgzf_begin: from then on _text, _lines and _end scan what they join -- header text on the
 *                          host, which has it; the rendered region on the device, which alone has it -- and feed the blocks they
 *                          hand back.  The scan's buffers are the one thing these calls allocate.  idx == NULL detaches. */
typedef struct vg_vcfidx vg_vcfidx;
int  vg_vcfidx_create(uint32_t block, vg_vcfidx **out);
void vg_vcfidx_destroy(vg_vcfidx *idx);
int  vg_vcfidx_text_host(vg_vcfidx *idx, const uint8_t *text, uint64_t n, int threads);
int  vg_vcfidx_text_device(vg_vcfidx *idx, int device, const uint8_t *text, uint64_t n);
int  vg_vcfidx_bgzf(vg_vcfidx *idx, const uint8_t *bgzf, uint64_t n);
uint64_t vg_vcfidx_bound(const vg_vcfidx *idx);
int  vg_vcfidx_finish(vg_vcfidx *idx, uint8_t *tbi, uint64_t cap, uint64_t *len);
const char *vg_vcfidx_error(const vg_vcfidx *idx, uint64_t *offset);
int  vg_vcfidx_stats(const vg_vcfidx *idx, uint64_t *out);
int  vg_bgzf_deflate_device_indexed(int device, const uint8_t *text, uint64_t nbytes, uint32_t block, int eof, int codes, vg_vcfidx *idx, uint8_t *bgzf, uint64_t cap, uint64_t *bgzf_len);
int  vg_jtext_bgzf_index(vg_jtext *jt, vg_vcfidx *idx);

/* Sample planes: several samples against ONE resident index. The reference genotypes one sample per process: the counters it hands
 * to the caller (qv.cc:1573-1626) are the only per-sample state of its read loop, the dictionaries are read-only.  A PLANE is that
 * state for one sample on the device: the exact sums (8 bytes per SNP site) and the wave kernel's base-indexed counters (16 bytes
 * per site, + 16): 24 * vg_num_sites + 16 bytes of HBM per plane -- 240 MB at 10 M sites --, taken outside the handle's plan and
 * counted by vg_index_device_bytes.  Everything else (tables, views, scratch) is shared.  A handle is born with plane 0; a caller
 * that never reserves sees exactly the behaviour of a handle without planes.
 *   vg_samples_reserve      grows the handle to n_samples planes (1 .. 65 535; a smaller number than it has: VG_EINVAL).  Existing
 *                           planes keep their contents, new ones start at zero.  VG_ENOMEM leaves the handle as it was.  Implies vg_sync
 *   vg_num_samples          planes of the handle (1 for a fresh one)
 *   vg_sample_select        no synchronisation, no device work: may be called between any two submits (out of range: VG_EINVAL).
 *                           Every read-taking call -- vg_reads_submit*, vg_reads_process_device*, vg_reads_submit_store,
 *                           vg_fastq_submit -- counts its batches into the sample selected AT THE CALL, whatever is selected when
 *                           they run; batches of different samples are in flight together.  A FASTQ stream belongs to the sample
 *                           selected at vg_fastq_stream_begin*: selecting another one while it is open does not move it.
 *                           vg_counts_fetch, vg_counts_device_ptr, vg_counts_allreduce and vg_counts_allreduce_devices act on the
 *                           selected sample (the last one wants the same selection on all handles: VG_EINVAL otherwise)
 *   vg_sample_selected      the sample selected now (0 for a fresh handle)
 *   vg_sample_reset         zeroes ONE sample's counters and its invalid-read count (implies vg_sync).  vg_counts_reset stays what
 *                           it was: all counters -- now of all planes -- and the handle-wide event counts
 *   vg_sample_invalid_reads reads of the sample that the reference would have aborted on (a character outside ACGTNacgtn,
 *                           util.c:103), since open / vg_counts_reset / vg_sample_reset of it.  Implies vg_sync
 * vg_stats stays handle-wide: the sum over the samples since open / vg_counts_reset. */
int      vg_samples_reserve(vg_index *ix, uint32_t n_samples);
uint32_t vg_num_samples(const vg_index *ix);
int      vg_sample_select(vg_index *ix, uint32_t sample);
uint32_t vg_sample_selected(const vg_index *ix);
int      vg_sample_reset(vg_index *ix, uint32_t sample);
int      vg_sample_invalid_reads(vg_index *ix, uint32_t sample, uint64_t *out);

/* Device pointer to the raw u32 counter array, length 2 * vg_num_sites: [2*s] = ref, [2*s+1] = alt
 * (the call first drains the batches in flight).
 * This is the ONE buffer that crosses GPUs: sum it over ranks (RCCL all-reduce over xGMI) before
 * vg_counts_fetch.  Reads shard with no other exchange. */
int  vg_counts_device_ptr(vg_index *ix, void **d_counts, uint64_t *n_u32);

/* All-reduce (sum) the counters over the ranks of an RCCL communicator (ncclComm_t passed as
 * void*), on the handle's stream. */
int  vg_counts_allreduce(vg_index *ix, void *nccl_comm);

/* The same exchange for ONE process that drives n devices (one handle each, all replicas of one index): builds an RCCL
 * communicator over the handles' devices, all-reduces every replica's counters in place, tears the communicator down.
 * This is what `vargeno geno` calls with VARGENO_GPUS=n.  n = 1 is the identity (and still goes through RCCL).
 * Replicas that share a device are summed on that device first; one of them joins the all-reduce, all get the result. */
int  vg_counts_allreduce_devices(vg_index **handles, int n);

#ifdef __cplusplus
}
#endif
#endif

// vg_host.h -- host side of the vargeno drop-in (C++17): `vargeno index` (file producers of the hot
// path's inputs), FASTQ framing, genotype caller and VCF writer.  None of this is device code; it is
// what sits on either side of the C-ABI in include/vargeno_hip.h.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <memory>
#include <string>
#include <utility>
#include <vector>

namespace vgh {

// ---- errors: the reference asserts / exit()s; the host library throws, main() turns it into exit(1)
struct Error {
	std::string msg;
};

// ---- `vargeno index` (reference src/qv.cc:2239-2389) ------------------------------------------
struct IndexOptions {
	bool write_lite = true;      // <prefix>.ref.bf.lite.bf: written by the reference, read by nothing in `geno`
	int threads = 0;             // 0 = all
	bool quiet = false;
};
void build_index(const std::string &fasta, const std::string &vcf, const std::string &prefix, const IndexOptions &opt);

// ---- FASTQ framing (reference src/qv.cc:760-784) ----------------------------------------------
struct ReadBatch {
	std::vector<uint8_t> bases, quals;     // flat, same offsets
	std::vector<uint64_t> offsets;         // n + 1
	uint64_t n() const { return offsets.empty() ? 0 : offsets.size() - 1; }
	void clear() { bases.clear(); quals.clear(); offsets.assign(1, 0); }
};
class FastqReader {
public:
	explicit FastqReader(const std::string &path);
	// a stream that can be read only once (a pipe: the reference fopen()s whatever path it is given and fgets its way through,
	// qv.cc:2182, 760-763): bytes [base, base + the spans' lengths) of it are in the caller's memory (kept alive by the caller),
	// everything after them is read from fd.  seek() works inside those bytes only.
	FastqReader(int fd, uint64_t base, std::vector<std::pair<const uint8_t *, size_t>> spans);
	~FastqReader();
	// appends up to max_reads records; returns the number appended (0 at end of file)
	uint64_t next(ReadBatch &out, uint64_t max_reads);
	// continue from byte `off` of the file; the four line buffers keep their content (what a truncated record sees)
	void seek(uint64_t off);
private:
	struct Impl;
	Impl *p;
};

// ---- BGZF-compressed FASTQ on the host (bgzf.cpp; the decoder is ../vg_inflate.h, shared with the device kernel) ----
enum class FastqKind { Text, Bgzf, PlainGzip, Bam, Cram };
// what a regular file's first bytes say: BGZF (gzip magic with the `BC` subfield) -- BAM when its first inflated bytes are the magic
// BAM\1 --, some other gzip, CRAM (its magic), or anything else (text)
FastqKind sniff_fastq(int fd);
// VARGENO_BGZF_THREADS' default: min(usable CPUs, 8)
int bgzf_threads_default(int usable_cpus);
// A compressed reads file as a once-only descriptor of FASTQ text, produced by threads of its own.  read_fd() is an ordinary FASTQ
// descriptor (owned by the object: it must outlive its reader; < 0: no pipe could be made, error says so).  After the reader has met
// the end of the text, finish() and look at `error`: a bad or incomplete block (or record) ends the text early and is named there.
class TextPipe {
public:
	virtual ~TextPipe() {}
	virtual int read_fd() const = 0;
	virtual void finish() = 0;
	// after finish(), for VARGENO_VERBOSE: the stderr line that says what the pipe did, "" when there is nothing to say.  what: whom
	// it fed; takeover: it ran behind a device route, which has said its own line
	virtual std::string describe(const char *what, bool takeover) const = 0;
	std::string error;
	uint64_t comp_bytes = 0, text_bytes = 0;       // valid after finish()
	double seconds = 0.0;                          // from construction to the end of the text
};
// A BGZF file as a once-only text descriptor: from compressed offset comp_from (a block start) on, `threads` host threads inflate
// the blocks, in order, into a pipe; the first `skip` bytes of text are dropped.  read_fd() is an ordinary FASTQ descriptor (owned
// by the object: it must outlive its reader).  After the reader has met the end of the text, finish() and look at `error`: a bad or
// incomplete block ends the text early and is named there, with its compressed offset.
// read_fd() < 0: no pipe could be made (error says so).
class BgzfTextPipe : public TextPipe {
public:
	BgzfTextPipe(int fd, uint64_t comp_from, uint32_t skip, int threads);
	~BgzfTextPipe() override;
	BgzfTextPipe(const BgzfTextPipe &) = delete;
	BgzfTextPipe &operator=(const BgzfTextPipe &) = delete;
	int read_fd() const override;
	void finish() override;
	std::string describe(const char *what, bool takeover) const override;
private:
	struct Impl;
	Impl *p;
};
// The blocks from compressed offset comp_from on, inflated on this thread until they hold more than want_text bytes (or the file
// ends); *comp_next = offset of the block after them.  false: err says which block is bad.
bool bgzf_inflate_span(int fd, uint64_t comp_from, uint64_t want_text, std::vector<uint8_t> &text, uint64_t *comp_next, std::string &err);

// ---- plain gzip on the host (gzip.cpp; the decoder is ../vg_gunzip.h, shared with the device kernels) ----
// A plain gzip file (any number of members) as a once-only text descriptor: one thread runs the sequential decoder into a pipe.
// After finish(): error names the compressed offset of bad data -- a broken block, a CRC32 or ISIZE mismatch, a truncated member,
// bytes behind a member that are no gzip header.
class GzipTextPipe : public TextPipe {
public:
	explicit GzipTextPipe(int fd);
	// Behind a device stream (vg_fastq_stream_gzip_checkpoint): the decoder starts at compressed bit offset at_bit, a block boundary
	// inside a member whose text in front of it is win[0, win_len); the first span_len bytes of its text are decoded by the
	// constructor into `span`, the rest goes into the pipe.  The CRC32 of the member it starts in is not checked (the device checks
	// it when it inflates that member to its end).  read_fd() < 0: error says why.
	GzipTextPipe(int fd, uint64_t at_bit, const uint8_t *win, uint32_t win_len, uint64_t span_len, std::vector<uint8_t> &span);
	~GzipTextPipe() override;
	GzipTextPipe(const GzipTextPipe &) = delete;
	GzipTextPipe &operator=(const GzipTextPipe &) = delete;
	int read_fd() const override;
	void finish() override;
	std::string describe(const char *what, bool takeover) const override;
private:
	void start(int fd);
	struct Impl;
	Impl *p;
};
// the text of the gzip file at fd written to `to` by the same decoder on this thread; false: err says what is wrong, and where
bool gzip_cat(int fd, FILE *to, std::string &err);

// ---- BAM on the host (bam.cpp; the record parser is ../vg_bam.h, shared with the device kernels) ----
// The header of the BAM file at fd, from its leading blocks: offset of the first record in the inflated stream, and n_ref.
// false: err says why (not BAM, a bad block, a file that ends inside the header -- with the inflated offset)
bool bam_header_info(int fd, uint64_t *header_end, int32_t *n_ref, std::string &err);
// A BAM file as a once-only descriptor of its equivalent FASTQ text (../vg_bam.h has the conversion): a BgzfTextPipe(fd, comp_from,
// skip, threads) inflates, a converter thread writes the text into a pipe.  at_header: the inflated bytes start with the BAM header
// (comp_from = 0, skip = 0); else they start at a record boundary, which is inflated offset stream_from (error messages count from
// it).  The header's n_ref is not asked for: the conversion follows the block_size chain from a known record boundary and never
// has to judge whether a record is plausible.
// After finish(): error names the inflated offset when the stream ends inside the header or a record, or a record's block_size is
// too small for its fields; the counters say what became of the records.
class BamTextPipe : public TextPipe {
public:
	BamTextPipe(int fd, uint64_t comp_from, uint32_t skip, int threads, bool at_header, uint64_t stream_from);
	~BamTextPipe() override;
	BamTextPipe(const BamTextPipe &) = delete;
	BamTextPipe &operator=(const BamTextPipe &) = delete;
	int read_fd() const override;
	void finish() override;
	std::string describe(const char *what, bool takeover) const override;
	uint64_t kept = 0, skipped_flag = 0, skipped_empty = 0;
private:
	struct Impl;
	Impl *p;
};
// The kept record at inflated offset `within` of the block at compressed offset `block`, as FASTQ text (the device route's
// take-over primes the host reader's line buffers with the last record framed).  false: err says why
bool bam_record_text(int fd, uint64_t block, uint32_t within, std::string &text, std::string &err);

// ---- caller + VCF writer (behaviour of reference src/qv.cc:1573-1747, 1789-1848; the arithmetic is ../vg_caller.h) ----
enum : uint8_t { GT_NONE = 0, GT_HOM_REF = 1, GT_HOM_ALT = 2, GT_HET = 3 };     // numbering of the reference's GTYPE_* (vartype.h)
struct Genotype {
	uint8_t gt;            // GT_*
	double confidence;     // posterior of the winning genotype x Poisson(7.1) mass of the depth
};
// counts are the 6-bit saturated pile-up counters; frequencies are the dictionary's n/255 encodings
Genotype call_genotype(unsigned ref_cnt, unsigned alt_cnt, uint8_t ref_freq, uint8_t alt_freq);
int genotype_quality(double confidence);                                        // the GQ column: (int)(-10 ln c)

struct ChrLen { std::string name; uint64_t len; };
std::vector<ChrLen> read_chrlens(const std::string &path);

struct SiteCounts {
	std::vector<uint32_t> pos;                     // 1-based over the concatenated genome, ascending
	std::vector<uint8_t> ref_freq, alt_freq, ref_cnt, alt_cnt;
};
// ---- where VCF text goes: a plain file, or a BGZF file (VARGENO_VCF_BGZF) ----
// The BGZF file is vg_bgzf_deflate_host_coded(the whole text, block, eof 1, codes), byte for byte, on either route: the text is gathered into
// spans that are multiples of the block (the last one shorter), and a thread of the sink compresses one span -- on `device`
// (vg_bgzf_deflate_device_coded: upload, kernels, read-back) or on `threads` host threads -- and writes it while the next is being
// made; two spans wait at most.  A device without memory for a span (VG_ENOMEM) hands the rest of the file to the host loop, one
// line under `verbose`.
enum class VcfBgzf { Off, Host, Device };
struct VcfOutput {
	VcfBgzf bgzf = VcfBgzf::Off;
	int device = 0, threads = 1;
	uint32_t block = 0;                            // text bytes per BGZF block; 0: 65 280
	int codes = 0;                                 // VG_DEFLATE_FIXED or VG_DEFLATE_DYNAMIC (VARGENO_VCF_CODES)
	bool index = false;                            // VARGENO_VCF_INDEX=tbi: <path>.tbi beside a BGZF file (never beside plain text)
	bool verbose = false;
};
class VcfSink {
public:
	virtual ~VcfSink() {}                          // a sink that is destroyed unclosed leaves its file without the end-of-file marker
	virtual void write(const char *p, size_t n) = 0;
	virtual void close() = 0;                      // the last bytes (BGZF: and the marker) are in the file; throws Error when it could not be written
};
std::unique_ptr<VcfSink> open_vcf_sink(const std::string &path, const VcfOutput &how);      // throws Error when the file cannot be created
// The index of a BGZF file (VcfOutput::index) is made by the sink's worker as it compresses -- on the device route by the fused call
// (vg_bgzf_deflate_device_indexed), on the host route by the host scanner around the host compressor -- and written by close() after
// the VCF has closed cleanly; a sink destroyed unclosed writes none.  A VCF with a data line the index cannot hold is completed, gets
// no .tbi (one left by an earlier run is removed), one line on stderr, and counts here: a command that ends with a count above zero fails.
unsigned vcf_index_refusals();

// returns {ref calls, alt calls, het calls}
struct CallSummary { uint64_t ref = 0, alt = 0, het = 0; };
// one call per site: gt = GT_*, gq as the reference prints it (0 where gt is GT_NONE)
struct SiteCalls { std::vector<uint8_t> gt; std::vector<int32_t> gq; };
void call_sites(const SiteCounts &s, SiteCalls &out);                           // the host call loop
// vcf_text: the SNP list's bytes if the caller has read them already (the command line reads them while the index is being opened)
// calls: the sites' calls if the caller has them already (vg_sample_calls_fetch); the counters of `s` are not looked at then
CallSummary write_genotyped_vcf(const SiteCounts &s, const std::vector<ChrLen> &chrlens,
                                const std::string &vcf_in, const std::string &vcf_out, const std::string *vcf_text = nullptr, const SiteCalls *calls = nullptr,
                                const VcfOutput &how = VcfOutput());
// One multi-sample VCF: a line per record that at least one sample's own VCF would contain, a column per sample in the given order.
// Throws when the SNP list cannot be read or the file cannot be written.
struct JointSample { std::string name; SiteCalls calls; };
// Who makes the data lines (VARGENO_JOINT_TEXT).  Host: the writer's own loop, a line at a time on the VCF threads.  Planned and Device:
// the threads only build the PLAN of a run of data lines -- per line that names a key of the book its first eight fields and the key's
// sites (../vg_jtext.h) -- and the run is rendered in spans of at most `lines` records (0: a default that keeps a span's text near
// 128 MiB): Planned by the header's host loop (the plan builder's test on machines without a device), Device by the kernels of
// vg_jtext_render on `device`.  With Device and VcfBgzf::Device header text and lines go through the handle's BGZF stream and the
// rendered text never crosses the link; otherwise the text goes to the sink like the host loop's.  The handle is made before the
// output file: VG_ENOMEM hands the file to Host (one line under `verbose`), any other failure throws.  The bytes of the file are
// the same on every route.
// info_counts (VARGENO_JOINT_INFO=counts): every data line's INFO carries NS / AN / AC / AF over the calls the line shows -- the rule,
// the tag's text and where it is spliced into the eighth field are ../vg_jtext.h's, compiled by all three routes -- and the header
// declares the four keys in front of the #CHROM line.  A line with fewer than eight fields is written as without it.
// prior_line (VARGENO_JOINT_PRIOR=cohort): the samples' columns were called again with the cohort's own allele frequencies
// (../vg_cprior.h) before they came here; the writer only says so, in this one header line in front of the #CHROM line.  Empty: none.
enum class JointText { Host, Planned, Device };
struct JointTextRoute {
	JointText route = JointText::Host;
	uint64_t lines = 0;                            // VARGENO_JOINT_TEXT_LINES
	int device = 0;
	bool info_counts = false;                      // VARGENO_JOINT_INFO=counts
	std::string prior_line;                        // "##vargenoPrior=cohort,iters=8,pseudo=2\n" or empty
};
// The first of NS, AN, AC, AF that the SNP list's leading header lines declare as an INFO key ("##INFO=<ID=AF,"), or "" -- also when
// the list cannot be read, which the writer says in its own words.  Such a list would get the key declared twice under info_counts.
std::string joint_info_declared(const std::string &vcf_in);
void write_joint_vcf(const std::vector<uint32_t> &pos, const std::vector<ChrLen> &chrlens, const std::vector<JointSample> &samples,
                     const std::string &vcf_in, const std::string &vcf_out, const std::string *vcf_text = nullptr, const VcfOutput &how = VcfOutput(),
                     const JointTextRoute &text_route = JointTextRoute());
bool read_whole_file(const std::string &path, std::string &text);

}  // namespace vgh

// main.cpp -- the `vargeno` command line of the drop-in (reference front-end: src/qv.cc:1853-2395).
//   vargeno index <ref.fa> <snps.vcf> <prefix>
//   vargeno geno  <prefix> <reads.fq> <snps.vcf> <out.vcf>
//   vargeno cohort <prefix> <manifest> <snps.vcf>     many samples against ONE resident index (no reference counterpart; run_cohort)
//   vargeno joint  <prefix> <manifest> <snps.vcf> <joint.vcf>   the same cohort as ONE multi-sample VCF: a line per site, a column per sample
// Same positional arguments, file names, messages and exit codes as upstream.  `geno` drives the
// HIP library through the C-ABI of include/vargeno_hip.h only.  Extra knobs come from the
// environment so that the argument list stays the reference's:
//   VARGENO_GPUS=n        n index replicas, one per GPU of this node (default 1): each streams its own record-aligned range of
//                         the FASTQ file, counters summed with RCCL
//   VARGENO_SHARE_DEVICES=1  allow more replicas than GPUs (replica g on device g % GPUs): small indexes, one-GPU test boxes
//   VARGENO_BATCH=n       reads per batch of the host-framed path (default 4194304)
//   VARGENO_CHUNK_MB=n    FASTQ bytes per chunk handed to the library (default 64; 256 when the host packs)
//   VARGENO_PACK_THREADS=n  host threads (per replica) that frame and 2-bit pack the FASTQ text, so that 48 bytes per read cross the
//                         link instead of ~315 of text (default: the CPUs the process may use -- a cgroup quota counts -- less two,
//                         shared among the replicas, at most 96).  They start BEFORE the index is opened and pack beside it; when the
//                         index is ready their measured rate is compared with the link's (vg_link_rate) and the faster route --
//                         host packing, or the text framed on the device -- takes the rest of the file.  0: device framing only
//   VARGENO_PREPACK=0     do not pack ahead of the index (and do not measure: host packing if VARGENO_PACK_THREADS > 0, else device framing)
//   VARGENO_PREPACK_GB=n  device memory the packed-ahead reads may take per device (the read store; default 16, at most an eighth of the device)
//   VARGENO_PREPACK_BYTES=n  the read store's size in bytes, exactly (tests: a store that fills up in the middle of a small file)
//   VARGENO_PREPACK_MMAP=0  the pre-packer reads the file with pread into buffers of its own instead of mapping it
//   VARGENO_ORDERLY_EXIT=1  close the handles and let the runtime shut down before the process ends (default: it ends when the VCF is closed)
//   VARGENO_VCF_CLOCKS=1  stderr: the seconds of the caller / VCF pass, phase by phase
//   VARGENO_READERS=n     threads reading the FASTQ file into pinned chunk buffers (default: an eighth of the hardware threads, 8 to 32)
//   VARGENO_MAX_DEVICE_GB=x  device-memory budget per replica (vg_index_open_ex): which re-laid-out views the replica holds follows
//                         from the index and this number alone (default: the whole device); VARGENO_VERBOSE=1 prints the plan
//   VARGENO_DUMP_COUNTS=path  also write the per-site counters the caller is given (ref counts then alt counts, one byte per site, site order of the index)
//   VARGENO_HOST_FASTQ=1  frame the FASTQ on the host (the reference's four fgets per record) instead of on the device
//   VARGENO_PIPE_COPIERS=n  a FASTQ that is not a regular file: copier threads the one reader deals the pipe's pages to (default 4, at most 16;
//                         0: the plain read() loop; see PipeIngest)
//   VARGENO_COHORT_INFLIGHT=n  cohort: samples genotyped at the same time, each in a sample plane of its own (default 4)
//   VARGENO_CALLER=device|host  geno, cohort: where the genotypes are called -- `device`: by the caller kernel, where the counters live
//                         (vg_sample_calls_fetch: 2 bytes per site cross the link; no device memory for it: the host loop after all, one
//                         line under VARGENO_VERBOSE); `host` (the default): the host loop over the fetched counters.  `joint` always asks the device
//   VARGENO_JOINT_PAIRS=path  joint: after the joint VCF, and only if no sample failed, the pairwise sample table of the cohort (same individual?
//                         swapped? related?) goes to <path>: the samples' calls are packed into a genotype matrix on replica 0's device and
//                         counted pair by pair there (vg_gmatrix_*); no device memory for it: the host loop (vg_pairs_host) on
//                         VARGENO_THREADS threads, one line under VARGENO_VERBOSE.  The joint VCF is the same bytes with or without it.
//                         Tab-separated: ##sites, ##min_gq, one ##sample line each (called = counted sites, het = counted hets), then per
//                         pair a < b in manifest order n, ibs0, ibs2, hethet, het_a, het_b (csrc/vg_pairs.h), concordance = ibs2 / n and
//                         relatedness = (hethet - 2 ibs0) / min(het_a, het_b), `nan` over a zero denominator
//   VARGENO_VCF_BGZF=device|host  geno, cohort, joint: the VCF (every sample's, the joint one; not the pair table) is written as BGZF, the
//                         `.vcf.gz` that bcftools / tabix / htslib read: exactly vg_bgzf_deflate_host(the whole VCF text, blocks of 65 280
//                         bytes, the end-of-file marker) on either route.  `device`: spans of the text are deflated by the deflate kernel on
//                         replica 0's device while the next span is being made (no device memory for a span: the host loop takes the rest
//                         of the file, one line under VARGENO_VERBOSE); `host`: by VARGENO_BGZF_THREADS host threads.  Unset or empty:
//                         plain text, as the reference writes it.  Any other value is refused before a device is touched
//   VARGENO_VCF_CODES=fixed|dynamic  geno, cohort, joint: how the blocks of a BGZF VCF are coded (no effect on plain text).  `fixed`, also
//                         unset or empty: fixed Huffman codes.  `dynamic`: per block the smallest of stored, fixed codes and dynamic
//                         codes built for the block on the route that compresses it -- the same match finder, smaller files, exactly
//                         vg_bgzf_deflate_host_coded(..., VG_DEFLATE_DYNAMIC, ...) on either route.  Any other value is refused before
//                         a device is touched
//   VARGENO_VCF_INDEX=tbi   geno, cohort, joint: every BGZF VCF the command writes gets its tabix index <path>.tbi, made in the pass
//                         that compresses the file on the route that compresses it (csrc/vg_vcfidx.h has the rules; on the
//                         VARGENO_JOINT_TEXT=device + VARGENO_VCF_BGZF=device stream the scan kernels read the rendered text where it is).
//                         The pair table is never indexed.  A data line the index cannot hold (unsorted positions, a chromosome that
//                         comes back, POS 0 or not a number, an end beyond 2^29, ...): the VCF is completed as ever, no .tbi is left, one
//                         line on stderr names the rule and the line's byte offset in the text, and the command ends non-zero.
//                         VARGENO_VERBOSE prints "vcf index: <route>, data lines, chromosomes, bins, chunks, bytes, seconds".  Unset or
//                         empty: no index.  Any other value, or `tbi` without VARGENO_VCF_BGZF, is refused before a device is touched
//   VARGENO_JOINT_TEXT=host|planned|device  joint (and the hidden jointvcf): who makes the data lines of the joint VCF; the file is the same
//                         bytes on every route.  `host`, also unset or empty: the writer's loop, a line at a time on the VCF threads.
//                         `planned`: the threads only build the plan of the lines (first eight fields + the key's sites, csrc/vg_jtext.h) and
//                         spans of it are rendered by the header's host loop.  `device`: the spans are rendered by the joint text kernels
//                         on replica 0's device (vg_jtext_*); with VARGENO_VCF_BGZF=device the header and the lines are joined and
//                         deflated there, so the rendered text never crosses the link.  No device memory for it: `host` after all, one
//                         line under VARGENO_VERBOSE, which also prints "joint text: <route>, records, lines, spans, text bytes, seconds".
//                         Any other value is refused before an index or a device is looked at
//   VARGENO_JOINT_INFO=counts  joint (and the hidden jointvcf): every data line's INFO also carries NS=<samples with a call>;AN=<2 NS>;
//                         AC=<hets + 2 hom-alts>;AF=<AC / AN, six decimals at most>, counted over the calls the line shows (on the
//                         VARGENO_JOINT_TEXT=device route by the text kernels, a wave reduction per record; csrc/vg_jtext.h has the rule),
//                         and the header declares the four keys.  An INFO of "." is replaced, any other gets ";" and the tag; a line
//                         with fewer than eight fields stays as it is.  The bytes are the same on every text route, plain or BGZF.
//                         A SNP list whose header already declares one of the four keys is refused before a device is touched or a
//                         file created (a list that carries such keys undeclared is not noticed: its lines get them twice).  Unset or
//                         empty: the file as ever.  Any other value is refused before an index or a device is looked at
//   VARGENO_JOINT_PRIOR=cohort  joint (and the hidden jointvcf): after the last sample every column is called again with the alt allele
//                         frequency the cohort itself shows at each site in place of the dictionary's two frequencies (csrc/vg_cprior.h has
//                         the rule: 8 EM passes, the dictionary's frequency counting as 2 alleles).  joint keeps every finished sample's
//                         counters for it, 2 more bytes of host memory per site and sample.  The re-called columns are what the joint
//                         file, its INFO counts and the pair table see; the header gets "##vargenoPrior=cohort,iters=8,pseudo=2" in front of
//                         #CHROM.  Unset or empty: the file as ever.  Any other value is refused before an index or a device is looked at.
//                         geno and cohort do not read it
//   VARGENO_JOINT_PRIOR_ROUTE=device|host  who re-calls: `device`, also unset or empty, the prior kernel on replica 0's device (vg_cprior_*),
//                         the host loop where the device has no memory for the matrix (one line under VARGENO_VERBOSE); `host`: the
//                         header's host loop on VARGENO_THREADS threads.  jointvcf has no device and always takes `host`.  The columns
//                         are the same on both.  VARGENO_VERBOSE prints "cohort prior: <route>, sites, samples, entries recomputed on the host"
//   VARGENO_JOINT_TEXT_LINES=n  records per rendered span (default: what keeps a span's text near 128 MiB, at most 2^20)
//   VARGENO_PAIRS_MIN_GQ=n  the table counts a call iff it is called and its GQ is at least n (default 0)
//   VARGENO_VERBOSE=1     stderr: the index plan and start-up report, one "ingest, replica g:" line per route taken, the "reads:" line with
//                         the wall time phase by phase; index: the "cuts:" line
//   VARGENO_STATS=1       the kernel's counting build: events per read (vg_set_stats; off by default here, it carries ~50 more registers per lane)
//   VARGENO_FORCE_RCCL=1  send the counters of a single replica through the RCCL all-reduce too (the identity)
//   VARGENO_FQPIPE_QUIET=1  the hidden `fqpipe` command counts the reads and prints a rate instead of one line per record
//   VARGENO_NO_LITE=1     index: skip <prefix>.ref.bf.lite.bf (2.3 GB, read by nothing in geno)
//   VARGENO_THREADS=n     index: threads (default: all); joint: threads of the pair table's host loop
// Hidden commands of the BGZF routes (tests and measurements; main() has the others):
//   bgzfcat <in>         a BGZF file's text on stdout (the host threads of the BGZF input route)
//   bgzfzip <in> <out> [block]  <in> written as BGZF to <out>, `block` text bytes per block (default 65 280), by the route
//                         VARGENO_VCF_BGZF names (default `host`; `device` needs one) in the coding mode VARGENO_VCF_CODES names: the sink
//                         the three commands write their VCF through
// Where `index` cuts its work (host/index_build.cpp; numbers clamped to >= 1, defaults unchanged when unset -- tests make them
// tiny so that every boundary falls inside sequences, N runs and repeat copies; VARGENO_VERBOSE=1 prints one "cuts:" line
// with what the build actually did; every chunk costs 48 KiB of bucket counters, so tiny chunks are for small inputs):
//   VARGENO_PARSE_PIECE=n   bytes per piece of the SNP list, cut at line ends (default 4 MiB)
//   VARGENO_FASTA_PIECE=n   bytes per piece of a FASTA record's text, dictionary side (default 16 MiB)
//   VARGENO_BF_CHUNK=n      k-mer windows per chunk of the reference bit-vector pass (default 2^22)
//   VARGENO_KMER_CHUNK=n    k-mer windows per chunk of the reference-dictionary pass (default 2^22)
//   VARGENO_SNP_CHUNK=n     SNP records per chunk of the SNP-dictionary pass (default 2^15)
//   VARGENO_COUNTING_SORT_MIN=n  records from which a dictionary bucket is sorted with the counting pass first (default 4 x 2^12)
//   VARGENO_DENSE_BF=0|1    reference bit vectors populated up front (1) or lazily zeroed (0) (default: 1 for a FASTA > 256 MB)
//   VARGENO_WRITE_MODE=pwrite|stream|mmap  how the dictionary files are written (default pwrite)
//   VARGENO_STREAM_QUEUE=n  stream mode: bytes queued for the writer thread before producers wait (default 2 GiB)
#include <ctype.h>
#include <errno.h>
#include <fcntl.h>
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>
#include <sys/mman.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/vargeno_hip.h"
#include "vg_host.h"
#include "bgzf.cpp"       // the host side of the BGZF routes, in this translation unit (csrc/Makefile: builds that list the four host files get it)
#include "bam.cpp"        // the host side of the BAM routes, the same way; behind bgzf.cpp, whose helpers it uses
#include "gzip.cpp"       // the host side of the plain-gzip route, the same way

static void print_help()
{
	fprintf(stderr, "Usage: vargeno <option> [option parameters ...]\n");
	fprintf(stderr, "Option  Description                   Parameters\n");
	fprintf(stderr, "------  -----------                   ----------\n");
	fprintf(stderr, "index   Generate index            <input FASTA> <input SNPs in VCF> <index_prefix>\n");
	fprintf(stderr, "geno    Perform genotyping        <index_prefix> <input FASTQ> <input SNPs in VCF> <output file in VCF>\n");
	fprintf(stderr, "cohort  Genotype many samples     <index_prefix> <manifest: one <input FASTQ><TAB><output file in VCF> per line> <input SNPs in VCF>\n");
	fprintf(stderr, "joint   ... into one VCF          <index_prefix> <manifest: one <input FASTQ><TAB><sample name> per line> <input SNPs in VCF> <output file in VCF>\n");
}
static void arg_check(int argc, int expected)
{
	if (argc - 2 != expected) { print_help(); exit(EXIT_FAILURE); }
}
static int env_int(const char *name, int dflt) { const char *e = getenv(name); return e && *e ? atoi(e) : dflt; }
static const char *env_str(const char *name) { const char *e = getenv(name); return e ? e : ""; }
// VARGENO_GZIP, read once: what becomes of a plain gzip file (gzip magic, no BGZF block table).  Unset or empty: refused by name.
// `host`: inflated by one host thread into a pipe.  `device`: `geno` with one replica streams the compressed file to the device
// (gzip_device_route); every other job takes the host route.  Anything else is refused like unset.
enum class GzipRoute { Refuse, Host, Device };
static GzipRoute gzip_route()
{
	static const GzipRoute r = [] { const std::string v = env_str("VARGENO_GZIP"); return v == "host" ? GzipRoute::Host : v == "device" ? GzipRoute::Device : GzipRoute::Refuse; }();
	return r;
}
// VARGENO_VCF_BGZF, read once: Off (unset or empty), Host, Device.  false: another value -- said on stderr, in one line
static bool vcf_bgzf_route(vgh::VcfBgzf *route)
{
	const std::string v = env_str("VARGENO_VCF_BGZF");
	*route = v == "host" ? vgh::VcfBgzf::Host : v == "device" ? vgh::VcfBgzf::Device : vgh::VcfBgzf::Off;
	if (v.empty() || *route != vgh::VcfBgzf::Off) return true;
	fprintf(stderr, "vargeno: VARGENO_VCF_BGZF=%s is not understood: `device` or `host` writes the VCF as BGZF, unset writes plain text\n", v.c_str());
	return false;
}
// VARGENO_VCF_CODES, read once: VG_DEFLATE_FIXED (unset, empty or `fixed`) or VG_DEFLATE_DYNAMIC.  false: another value -- said on
// stderr, in one line
static bool vcf_bgzf_codes(int *codes)
{
	const std::string v = env_str("VARGENO_VCF_CODES");
	*codes = v == "dynamic" ? VG_DEFLATE_DYNAMIC : VG_DEFLATE_FIXED;
	if (v.empty() || v == "fixed" || v == "dynamic") return true;
	fprintf(stderr, "vargeno: VARGENO_VCF_CODES=%s is not understood: `fixed` or `dynamic` names the Huffman codes of a BGZF VCF, unset is `fixed`\n", v.c_str());
	return false;
}
// VARGENO_VCF_INDEX, read once: on (`tbi`) or off (unset or empty).  false: another value, or `tbi` while the VCF is plain text --
// said on stderr, in one line
static bool vcf_index_switch(bool *on, vgh::VcfBgzf route)
{
	const std::string v = env_str("VARGENO_VCF_INDEX");
	*on = v == "tbi";
	if (v.empty()) return true;
	if (!*on) { fprintf(stderr, "vargeno: VARGENO_VCF_INDEX=%s is not understood: `tbi` writes a tabix index beside every BGZF VCF, unset writes none\n", v.c_str()); return false; }
	if (route != vgh::VcfBgzf::Off) return true;
	fprintf(stderr, "vargeno: VARGENO_VCF_INDEX=tbi indexes BGZF output: set VARGENO_VCF_BGZF=device or VARGENO_VCF_BGZF=host as well\n");
	return false;
}
// VARGENO_JOINT_TEXT (and VARGENO_JOINT_TEXT_LINES), read once: who makes the data lines of the joint file -- `host` (unset or empty),
// `planned` or `device` (vg_host.h: JointText).  false: another value -- said on stderr, in one line
static bool joint_text_route(vgh::JointTextRoute *r)
{
	const std::string v = env_str("VARGENO_JOINT_TEXT");
	r->route = v == "planned" ? vgh::JointText::Planned : v == "device" ? vgh::JointText::Device : vgh::JointText::Host;
	r->lines = (uint64_t)std::max(0ll, atoll(env_str("VARGENO_JOINT_TEXT_LINES")));
	r->device = 0;                                                   // (replica 0 sits on device 0)
	if (v.empty() || v == "host" || r->route != vgh::JointText::Host) return true;
	fprintf(stderr, "vargeno: VARGENO_JOINT_TEXT=%s is not understood: `host`, `planned` or `device` names who makes the lines of the joint VCF, unset is `host`\n", v.c_str());
	return false;
}
// VARGENO_JOINT_INFO, read once: `counts` (NS / AN / AC / AF in every line's INFO) or off (unset or empty).  false: another value --
// said on stderr, in one line
static bool joint_info_switch(bool *counts)
{
	const std::string v = env_str("VARGENO_JOINT_INFO");
	*counts = v == "counts";
	if (v.empty() || *counts) return true;
	fprintf(stderr, "vargeno: VARGENO_JOINT_INFO=%s is not understood: `counts` adds NS, AN, AC and AF to the INFO of the joint VCF's lines, unset adds nothing\n", v.c_str());
	return false;
}
// VARGENO_JOINT_PRIOR and VARGENO_JOINT_PRIOR_ROUTE, read once.  false: a value that is none of their words -- said on stderr, in one line
struct JointPrior {
	bool cohort = false;                                             // VARGENO_JOINT_PRIOR=cohort
	bool device = true;                                              // VARGENO_JOINT_PRIOR_ROUTE (`device` unless `host`)
	int iters = VG_CPRIOR_ITERS;                                     // (the rule's defaults: no variable changes them)
	double pseudo = VG_CPRIOR_PSEUDO;
	std::string header_line() const
	{
		char b[96];
		snprintf(b, sizeof b, "##vargenoPrior=cohort,iters=%d,pseudo=%g\n", iters, pseudo);
		return cohort ? std::string(b) : std::string();
	}
};
static bool joint_prior_switch(JointPrior *jp)
{
	const std::string v = env_str("VARGENO_JOINT_PRIOR"), r = env_str("VARGENO_JOINT_PRIOR_ROUTE");
	jp->cohort = v == "cohort";
	jp->device = r != "host";
	if (!v.empty() && !jp->cohort) {
		fprintf(stderr, "vargeno: VARGENO_JOINT_PRIOR=%s is not understood: `cohort` calls the joint VCF's samples again with allele frequencies estimated from the cohort, unset leaves the calls as they are\n", v.c_str());
		return false;
	}
	if (r.empty() || r == "device" || r == "host") return true;
	fprintf(stderr, "vargeno: VARGENO_JOINT_PRIOR_ROUTE=%s is not understood: `device` or `host` names who computes the cohort prior, unset is `device`\n", r.c_str());
	return false;
}
// CPUs this process may use: the hardware threads, capped by a cgroup CPU quota (cpu.max: "<quota> <period>"; this pool's GPU boxes
// give a container 16 CPUs' worth of time on a 256-thread host)
static int usable_cpus()
{
	int h = (int)std::thread::hardware_concurrency();
	if (h <= 0) h = 1;
	if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
		char a[64] = ""; long long per = 100000;
		if (fscanf(f, "%63s %lld", a, &per) >= 1 && strcmp(a, "max") != 0 && per > 0) { const long long q = atoll(a); const int c = (int)((q + per - 1) / per); if (q > 0 && c > 0 && c < h) h = c; }
		fclose(f);
	}
	return h;
}

// Every VARGENO_* value `geno` and the hidden `fqpipe` use, read ONCE, here, before any thread exists, and handed down by const
// reference.  The constructor clamps, and resolves the defaults that depend on the machine (`have` devices, the usable CPUs).
struct GenoOptions {
	const int have;                                                  // devices of this node: replica g sits on device g % have
	int ngpu = env_int("VARGENO_GPUS", 1);                           // replicas
	const bool share = env_int("VARGENO_SHARE_DEVICES", 0) != 0;     // more replicas than devices
	const uint64_t batch = (uint64_t)env_int("VARGENO_BATCH", 1 << 22);
	const bool verbose = env_int("VARGENO_VERBOSE", 0) != 0;
	const bool host_framing = env_int("VARGENO_HOST_FASTQ", 0) != 0;
	const int hw = usable_cpus();
	// host threads that frame + pack (per replica); 0: the text is framed on the device, nothing is packed ahead
	int pack_threads = env_int("VARGENO_PACK_THREADS", -1);
	const bool pack_threads_given = pack_threads >= 0;
	const int n_readers = std::max(1, std::min(env_int("VARGENO_READERS", std::max(8, std::min(32, hw / 8))), 64));
	const bool prepack = env_int("VARGENO_PREPACK", 1) != 0, prepack_mmap = env_int("VARGENO_PREPACK_MMAP", 1) != 0;
	const uint64_t prepack_want = (uint64_t)std::max(1, env_int("VARGENO_PREPACK_GB", 16)) << 30;
	const uint64_t prepack_bytes = (uint64_t)std::max(0ll, atoll(env_str("VARGENO_PREPACK_BYTES")));    // 0: not given
	const int chunk_mb = env_int("VARGENO_CHUNK_MB", INT_MIN);       // INT_MIN: not given -- each of its three users has a default of its own
	const int pipe_copiers = std::min(16, std::max(0, env_int("VARGENO_PIPE_COPIERS", 4)));
	const uint64_t budget = (uint64_t)(atof(env_str("VARGENO_MAX_DEVICE_GB")) * 1e9);                   // 0: not given
	const int stats = env_int("VARGENO_STATS", 0);
	const int cohort_inflight = std::max(1, env_int("VARGENO_COHORT_INFLIGHT", 4));      // cohort: samples in flight together = sample planes per replica
	const bool force_rccl = env_int("VARGENO_FORCE_RCCL", 0) != 0, orderly_exit = env_int("VARGENO_ORDERLY_EXIT", 0) != 0, fqpipe_quiet = env_int("VARGENO_FQPIPE_QUIET", 0) != 0;
	const char *const dump_counts = getenv("VARGENO_DUMP_COUNTS");
	// BGZF input: host threads that inflate (BgzfTextPipe), and the route of one replica -- `device`: compressed bytes cross the link
	// and are inflated there; `host` (the default until profiles/bgzf_ingest.txt says otherwise): inflated here, then the once-only route
	const int bgzf_threads = std::max(1, std::min(env_int("VARGENO_BGZF_THREADS", vgh::bgzf_threads_default(hw)), 256));
	const bool bgzf_device = std::string(env_str("VARGENO_BGZF")) == "device";
	// plain gzip input (no block table): refused unless VARGENO_GZIP asks for it -- `host`: one thread inflates into a pipe (GzipTextPipe)
	// `device`: one replica streams the compressed file to the device, which inflates it slot by slot (vg_fastq_stream_begin_gzip);
	// several replicas and every `cohort` / `joint` sample take the host route, as BGZF does
	const bool gzip_host = gzip_route() != GzipRoute::Refuse;
	const bool gzip_device = gzip_route() == GzipRoute::Device;
	const bool caller_device = std::string(env_str("VARGENO_CALLER")) == "device";      // genotypes from the caller kernel (default: the host loop)
	// joint: the pairwise sample table (empty: none), the GQ from which a call counts in it, the threads of its host loop
	const std::string joint_pairs = env_str("VARGENO_JOINT_PAIRS");
	const int pairs_min_gq = env_int("VARGENO_PAIRS_MIN_GQ", 0);
	const int pairs_threads = std::max(1, env_int("VARGENO_THREADS", usable_cpus()));
	// how the VCF is written (VARGENO_VCF_BGZF and VARGENO_VCF_CODES; main() has refused a value that is neither of its two words): on replica 0's
	// device, which is device 0, or on the BGZF threads
	// joint: who makes the data lines (VARGENO_JOINT_TEXT; main() has refused a value that is none of its three words)
	// ... and whether their INFO carries the counts (VARGENO_JOINT_INFO; refused by main() likewise)
	// ... and whether the columns are called again with the cohort's own allele frequencies (VARGENO_JOINT_PRIOR; refused by main() likewise)
	const JointPrior joint_prior = [] { JointPrior jp; (void)joint_prior_switch(&jp); return jp; }();
	const vgh::JointTextRoute joint_text = [] { vgh::JointTextRoute r; JointPrior jp; (void)joint_text_route(&r); (void)joint_info_switch(&r.info_counts); (void)joint_prior_switch(&jp); r.prior_line = jp.header_line(); return r; }();
	const vgh::VcfOutput vcf_out = [this] { vgh::VcfOutput w; (void)vcf_bgzf_route(&w.bgzf); (void)vcf_bgzf_codes(&w.codes); (void)vcf_index_switch(&w.index, w.bgzf); w.device = 0; w.threads = bgzf_threads; w.verbose = verbose; return w; }();
	explicit GenoOptions(int devices) : have(devices)
	{
		if (ngpu > have && !share) ngpu = have;
		if (ngpu < 1) ngpu = 1;
		if (pack_threads < 0) pack_threads = std::max(2, std::min(hw - 2, 96) / ngpu);
	}
	uint64_t chunk(int dflt_mb) const { return (uint64_t)std::max(1, chunk_mb == INT_MIN ? dflt_mb : chunk_mb) << 20; }
	uint64_t pipe_chunk() const { return chunk(64); }                // the once-only route's ring
	uint64_t prepack_chunk() const { return chunk(256); }            // what a pre-packer frames + packs at a time
	uint64_t rest_chunk(bool host_packs) const { return chunk(host_packs ? 256 : 64); }      // the rest of a range
	int range_readers() const { return std::max(2, n_readers / ngpu); }
	int replicas_on_device(int g) const { int on = 0; for (int k = 0; k < ngpu; k++) on += k % have == g % have; return on; }
};

#define VG_CHECK(call)                                                                           \
	do {                                                                                         \
		int rc_ = (call);                                                                        \
		if (rc_ != VG_OK) { fprintf(stderr, "vargeno: %s failed (%d): %s\n", #call, rc_, vg_last_error()); exit(EXIT_FAILURE); } \
	} while (0)

// Bytes [lo, hi) of a descriptor, read ahead of ONE consumer that takes them chunk by chunk, in order: n_readers threads pread()
// the range piecewise (pieces of at most 8 MiB, claimed in file order) into the caller's ring of chunk buffers.  Chunk i lives in
// buf(i) from wait(i) to release(i); the readers run at most the ring's length ahead of the last release.
class RangeReader {
public:
	RangeReader(int fd, uint64_t lo, uint64_t hi, uint64_t chunk, int n_readers, std::vector<uint8_t *> ring)
		: fd_(fd), lo_(lo), fsize_(hi - lo), chunk_(chunk), piece_(std::min<uint64_t>(chunk, 8ull << 20)), ppc_((chunk + piece_ - 1) / piece_),
		  n_chunks_((fsize_ + chunk - 1) / chunk), ring_(std::move(ring)), left_((size_t)n_chunks_)
	{
		for (uint64_t i = 0; i < n_chunks_; i++) left_[(size_t)i] = (uint32_t)((chunk_len(i) + piece_ - 1) / piece_);
		for (int t = 0; t < n_readers; t++) readers_.emplace_back([this] { read_pieces(); });
	}
	~RangeReader() { stop(); }
	uint64_t n_chunks() const { return n_chunks_; }
	uint64_t chunk_len(uint64_t i) const { return std::min(chunk_, fsize_ - i * chunk_); }
	uint8_t *buf(uint64_t i) const { return ring_[(size_t)(i % ring_.size())]; }
	// chunk i is complete in buf(i) (true), or a pread failed somewhere (false)
	bool wait(uint64_t i) { std::unique_lock<std::mutex> g(mu_); cv_.wait(g, [&] { return left_[(size_t)i] == 0 || io_error_; }); return !io_error_; }
	// the consumer is done with chunk i: its buffer may be refilled
	void release(uint64_t i) { { std::lock_guard<std::mutex> g(mu_); released_ = i + 1; } cv_.notify_all(); }
	// no more chunks are wanted: the readers finish the pread they are in and are joined
	void stop() { { std::lock_guard<std::mutex> g(mu_); quit_ = true; } cv_.notify_all(); for (auto &t : readers_) if (t.joinable()) t.join(); }
	bool failed() { std::lock_guard<std::mutex> g(mu_); return io_error_; }
private:
	void read_pieces()
	{
		for (;;) {
			const uint64_t p = next_piece_.fetch_add(1);
			const uint64_t ci = p / ppc_, off = ci * chunk_ + (p % ppc_) * piece_;
			if (ci >= n_chunks_) return;
			if (off >= std::min(fsize_, (ci + 1) * chunk_)) continue;
			{ std::unique_lock<std::mutex> g(mu_); cv_.wait(g, [&] { return ci < released_ + (uint64_t)ring_.size() || io_error_ || quit_; }); if (io_error_ || quit_) return; }
			uint64_t n = std::min(piece_, std::min(fsize_, (ci + 1) * chunk_) - off), done = 0;
			uint8_t *dst = buf(ci) + (off - ci * chunk_);
			while (done < n) {
				const ssize_t g = pread(fd_, dst + done, (size_t)(n - done), (off_t)(lo_ + off + done));
				if (g <= 0) break;
				done += (uint64_t)g;
			}
			std::lock_guard<std::mutex> g(mu_);
			if (done < n) io_error_ = true;
			left_[(size_t)ci]--;
			cv_.notify_all();
		}
	}
	const int fd_; const uint64_t lo_, fsize_, chunk_, piece_, ppc_, n_chunks_;     // ppc_: pieces per (full) chunk
	const std::vector<uint8_t *> ring_;
	std::mutex mu_; std::condition_variable cv_;
	std::vector<uint32_t> left_;                                     // pieces of chunk i still to be read
	uint64_t released_ = 0;                                          // chunks the consumer is done with (their buffers are free again)
	std::atomic<uint64_t> next_piece_{0};
	bool io_error_ = false, quit_ = false;
	std::vector<std::thread> readers_;
};

// Bytes [lo, hi) of the FASTQ file as a stream to one replica: a RangeReader fills a ring of pinned chunk buffers; this thread
// pushes the chunks in order (vg_fastq_stream_push returns as soon as a chunk is on the device) and learns what was framed only
// at the end.  Offsets in the result are relative to lo.
struct StreamResult {
	uint64_t nrec = 0, used = 0, last = 0;
	int refused = 0;
	std::string error;                                               // empty: fine
};
// STREAM_BGZF: the bytes are BGZF (vg_fastq_stream_begin_bgzf) -- the same ring over the compressed file; the result's offsets are text
// offsets.  STREAM_BAM: a BAM file (vg_fastq_stream_begin_bam); the offsets are offsets in the inflated BAM stream.
// STREAM_GZIP: plain gzip (vg_fastq_stream_begin_gzip); text offsets too.
enum StreamBytes { STREAM_TEXT, STREAM_BGZF, STREAM_BAM, STREAM_GZIP };
static StreamResult stream_range(vg_index *ix, int fd, uint64_t lo, uint64_t hi, uint64_t chunk, int n_readers, int pack_threads, StreamBytes bytes = STREAM_TEXT)
{
	StreamResult res;
	const int NBUF = 4;
	std::vector<uint8_t *> ring((size_t)NBUF, nullptr);
	std::vector<std::vector<uint8_t>> pageable((size_t)NBUF);
	for (int i = 0; i < NBUF; i++) {
		ring[(size_t)i] = (uint8_t *)vg_host_alloc_pinned((size_t)chunk);
		if (!ring[(size_t)i]) { pageable[(size_t)i].resize((size_t)chunk); ring[(size_t)i] = pageable[(size_t)i].data(); }
	}
	RangeReader rr(fd, lo, hi, chunk, n_readers, ring);
	int rc = bytes == STREAM_GZIP ? vg_fastq_stream_begin_gzip(ix) : bytes == STREAM_BAM ? vg_fastq_stream_begin_bam(ix) : bytes == STREAM_BGZF ? vg_fastq_stream_begin_bgzf(ix) : pack_threads > 0 ? vg_fastq_stream_begin_packed(ix, pack_threads) : vg_fastq_stream_begin(ix);
	for (uint64_t i = 0; i < rr.n_chunks() && rc == VG_OK; i++) {
		if (!rr.wait(i)) break;
		rc = vg_fastq_stream_push(ix, rr.buf(i), rr.chunk_len(i));
		rr.release(i);
	}
	rr.stop();                                                       // (the readers are joined: the ring is ours again)
	if (rc != VG_OK) res.error = std::string("FASTQ stream failed: ") + vg_last_error();
	else if (rr.failed()) res.error = "error reading the FASTQ file";
	else {
		rc = vg_fastq_stream_end(ix, &res.nrec, &res.used, &res.last, &res.refused);
		if (rc != VG_OK) res.error = std::string("vg_fastq_stream_end failed: ") + vg_last_error();
	}
	for (int i = 0; i < NBUF; i++) if (pageable[(size_t)i].empty()) vg_host_free_pinned(ring[(size_t)i]);
	return res;
}

// ---- packing ahead of the index ------------------------------------------------------------------------------------------------
// Framing + 2-bit packing need no device (vg_packer_*), and vg_index_open takes seconds during which the host would otherwise
// idle: bytes [lo, hi) of the FASTQ file are read and packed WHILE the replica's index is being built (r05; the r04 command line
// started to pack only when the handle existed).  What is packed goes up to the device at once, into a read store
// (vg_read_store_*: device memory taken before the index is planned; the link is idle two thirds of the open's time), out of two
// page-locked staging sets -- a first version kept the batches in page-locked HOST memory until the handle existed: 11 GB for
// 200 M reads, 0.15 s per GB to lock and 0.1 s per GB for the operating system to take back at exit, more than the read loop
// itself takes (profiles/job_tail_r05.txt).  The packed form is ~56 bytes per 150 bp read, so a 30x file (620 M reads) is 35 GB:
// VARGENO_PREPACK_GB (default 16) bounds the store; what does not fit is framed after the open like the rest of the range.
// The pre-packer also MEASURES its rate (text bytes framed + packed per second with the threads it was given, on this host, now);
// when the index is ready the caller compares it with the link's rate -- what the device-side framing of the remaining text
// would run at -- and lets the faster one finish.
class PrePacker {
public:
	PrePacker(int fd, uint64_t lo, uint64_t hi, uint64_t chunk, int n_readers, int pack_threads, bool use_mmap, vg_read_store *store)
		: fd_(fd), lo_(lo), hi_(hi), chunk_(std::min(chunk, std::max<uint64_t>(hi - lo, 1))), n_readers_(n_readers), pack_threads_(pack_threads), use_mmap_(use_mmap), store_(store)
	{
		clock_gettime(CLOCK_MONOTONIC, &born_);
		th_ = std::thread([this] { run(); });
	}
	~PrePacker()
	{
		stop();
		if (th_.joinable()) th_.join();
	}
	void stop() { stop_.store(true); }
	bool done() const { return done_.load(); }
	void join() { if (th_.joinable()) th_.join(); }
	// valid after join(): what vg_fastq_stream_end would have said about the bytes [lo, lo + consumed) -- the batches in the store
	uint64_t records() const { return records_; }
	uint64_t consumed() const { return consumed_; }
	uint64_t last_record_start() const { return last_; }
	bool refused() const { return refused_; }
	bool store_full() const { return full_; }
	double text_bytes_per_s() const { const double t = pack_s_.load(); return t > 0 ? (double)packed_text_.load() / t : 0.0; }
	uint64_t text_bytes_done() const { return packed_text_.load(); }
	double finished_after_s() const { return finished_s_.load(); }           // seconds from construction to the last batch (0: still running)
	std::string error;
private:
	void run()
	{
		const uint64_t fsize = hi_ - lo_, n_chunks = (fsize + chunk_ - 1) / chunk_;
		vg_packer *pk = nullptr;
		if (vg_packer_create(pack_threads_, &pk) != VG_OK) { error = vg_last_error(); finish(); return; }
		// two page-locked staging sets of a chunk's worst case (a 256 MiB chunk: 3 x 67 MB each): the store copies out of one
		// while the packer fills the other
		const uint64_t rcap = vg_packer_reads_cap(chunk_), kcap = vg_packer_kmers_cap(chunk_);
		uint64_t *stage[2] = {nullptr, nullptr};
		for (int k = 0; k < 2; k++) {
			stage[k] = (uint64_t *)vg_host_alloc_pinned((size_t)(kcap + 2 * rcap + 2) * 8);
			if (!stage[k]) { error = "page-locked staging for the pre-packer: allocation failed"; if (stage[0]) vg_host_free_pinned(stage[0]); vg_packer_destroy(pk); finish(); return; }
		}
		// The text: the file mapped (the packer's threads read the page cache / tmpfs pages themselves: no copy into buffers of
		// ours, which cost as many CPU seconds as the packing itself -- and the job shares a CPU quota with the index's start-up),
		// the chunks after the current one asked for ahead (MADV_WILLNEED); VARGENO_PREPACK_MMAP=0 or a file that cannot be
		// mapped: a RangeReader fills three chunk buffers with pread, a chunk ahead of the packer
		const uint64_t page = (uint64_t)sysconf(_SC_PAGESIZE), map_lo = lo_ / page * page;
		const uint8_t *map = nullptr;
		if (use_mmap_) {
			void *m = mmap(nullptr, (size_t)(hi_ - map_lo), PROT_READ, MAP_SHARED, fd_, (off_t)map_lo);
			if (m != MAP_FAILED) { map = (const uint8_t *)m; (void)madvise(m, (size_t)(hi_ - map_lo), MADV_SEQUENTIAL); }
		}
		std::vector<std::vector<uint8_t>> text(map ? 0u : 3u);
		std::vector<uint8_t *> ring;
		for (auto &t : text) { t.resize((size_t)std::min(chunk_, fsize)); ring.push_back(t.data()); }
		std::unique_ptr<RangeReader> rr(map ? nullptr : new RangeReader(fd_, lo_, hi_, chunk_, n_readers_, ring));
		uint64_t n_pushes = 0;                                                   // batches handed to the store
		for (uint64_t i = 0; i < n_chunks && !stop_.load(); i++) {
			if (rr && !rr->wait(i)) break;
			const uint64_t len = std::min(chunk_, fsize - i * chunk_);
			// (the sets alternate on the number of PUSHES: the store waits for the copies of the push before at its next push, so a
			// chunk that framed nothing -- no push -- must not hand the set of a push still in flight to the chunk after it)
			uint64_t *sk = stage[n_pushes & 1], *sm = sk + kcap, *so = sm + rcap;
			uint64_t nr = 0, nc = 0, ninv = 0;
			struct timespec a, b; clock_gettime(CLOCK_MONOTONIC, &a);
			const uint8_t *src = map ? map + (lo_ - map_lo) + i * chunk_ : rr->buf(i);
			if (map && i + 1 < n_chunks) (void)madvise((void *)(map + ((lo_ - map_lo) + (i + 1) * chunk_) / page * page), (size_t)std::min(2 * chunk_, hi_ - lo_ - (i + 1) * chunk_), MADV_WILLNEED);
			const int rc = vg_packer_push(pk, src, len, sk, kcap, sm, so, rcap, &nr, &nc, &ninv);
			if (map && i > 0) (void)madvise((void *)(map + ((lo_ - map_lo) + (i - 1) * chunk_ + page - 1) / page * page), (size_t)(chunk_ / page * page - page), MADV_DONTNEED);      // (the mapping of the chunk before: its pages stay in the page cache, the page tables go)
			clock_gettime(CLOCK_MONOTONIC, &b);
			if (rc != VG_OK) { error = vg_last_error(); break; }
			pack_s_.store(pack_s_.load() + (double)(b.tv_sec - a.tv_sec) + 1e-9 * (double)(b.tv_nsec - a.tv_nsec));
			if (rr) rr->release(i);
			if (nr) {
				// (the push waits for the copies of the chunk before -- the other staging set -- and enqueues this chunk's)
				const int prc = vg_read_store_push(store_, sk, sm, so, nr);
				if (prc == VG_ENOMEM) { full_ = true; break; }                      // (this chunk's records are dropped with it: the stream is re-framed from the last batch that was kept)
				if (prc != VG_OK) { error = vg_last_error(); break; }
				n_pushes++;
				uint64_t rec = 0, cons = 0, last = 0; int ref = 0;
				(void)vg_packer_end(pk, &rec, &cons, &last, &ref);               // (a query: the stream's totals so far)
				records_ = rec; consumed_ = cons; last_ = last;
			}
			packed_text_.fetch_add(len);
			int ref = 0;
			(void)vg_packer_end(pk, nullptr, nullptr, nullptr, &ref);
			if (ref) { refused_ = true; break; }
		}
		if (rr) rr->stop();
		if (rr && rr->failed() && error.empty()) error = "error reading the FASTQ file";
		if (vg_read_store_flush(store_) != VG_OK && error.empty()) error = vg_last_error();      // the staging sets are free
		if (map) (void)munmap((void *)map, (size_t)(hi_ - map_lo));
		for (int k = 0; k < 2; k++) vg_host_free_pinned(stage[k]);
		vg_packer_destroy(pk);
		finish();
	}
	void finish()
	{
		struct timespec now; clock_gettime(CLOCK_MONOTONIC, &now);
		finished_s_.store((double)(now.tv_sec - born_.tv_sec) + 1e-9 * (double)(now.tv_nsec - born_.tv_nsec));
		done_.store(true);
	}
	const int fd_; const uint64_t lo_, hi_, chunk_; const int n_readers_, pack_threads_; const bool use_mmap_;
	vg_read_store *const store_;
	std::thread th_;
	std::atomic<bool> stop_{false}, done_{false};
	uint64_t records_ = 0, consumed_ = 0, last_ = 0;
	bool refused_ = false, full_ = false;
	std::atomic<double> pack_s_{0.0}; std::atomic<uint64_t> packed_text_{0};
	struct timespec born_; std::atomic<double> finished_s_{0.0};
};

// ---- a FASTQ "file" that can be read only once -------------------------------------------------------------------------------
// The reference fopen()s whatever path it is given and fgets its way through it (qv.cc:2182, 760-763): a FIFO, /dev/stdin, bash's
// <(zcat reads.fq.gz) all work there by construction.  Here the file routes above pread / mmap ranges of the file from many
// threads, cut it at record starts per replica, and re-open it for the host reader -- none of which a pipe allows: a FIFO
// loses its only reader between two open()s, a /dev/fd/N substitution has size 0.  So a path that is not a regular file takes THIS
// route: the one descriptor is drained by one thread (whole chunks into a small ring, from the moment the command line
// starts -- beside the index open; the pipe's pages are moved on to a few copier threads, see read_loop), the chunks are framed + packed by the host packer (vg_packer_*: bytes cut anywhere), and the
// packed batches go to the replicas round robin -- into their read stores while the index is still opening, straight into the
// read loop (vg_reads_submit_packed) afterwards.  No ranges, no seek.  What the packer refuses (a line beyond fgets' 1023
// characters ...) and the possibly truncated tail go through the host reader like on the file routes: it is given the bytes
// still in memory (from the start of the last framed record on, to prime the reference's stale line buffers) and the descriptor.
class PipeIngest {
public:
	// sink(replica, kmers, meta, chunk_offsets, n_reads): a packed batch for a replica's read loop, once attach() has been called;
	// blocking (the arrays are free when it returns); returns an error text or ""
	typedef std::function<std::string(size_t, const uint64_t *, const uint64_t *, const uint64_t *, uint64_t)> Sink;
	PipeIngest(int fd, uint64_t chunk, int pack_threads, int copiers, const std::vector<vg_read_store *> &stores, Sink sink)
		: fd_(fd), chunk_(chunk), pack_threads_(pack_threads < 1 ? 1 : pack_threads), want_copiers_(copiers), stores_(stores), sink_(std::move(sink))
	{
		clock_gettime(CLOCK_MONOTONIC, &born_);
		for (auto &b : ring_) b.data.resize((size_t)chunk_);
		reader_ = std::thread([this] { read_loop(); });
		worker_ = std::thread([this] { work_loop(); });
	}
	~PipeIngest() { finish(); }
	// the handles exist: the stores' batches are submitted by the caller; from now on batches go straight to the handles
	void attach() { { std::lock_guard<std::mutex> g(mu_); attached_ = true; } cv_.notify_all(); }
	void finish() { if (worker_.joinable()) worker_.join(); if (reader_.joinable()) reader_.join(); }
	// valid after finish(): the stream's totals, and what the host reader needs
	uint64_t records = 0, consumed = 0, last = 0, bytes_read = 0;
	bool refused = false;
	uint64_t to_store = 0, direct = 0;                       // reads that went through a read store / straight into the read loop
	double seconds = 0.0;                                    // from construction to the end of the stream
	int copiers = 0;                                         // copier threads the reader dealt the stream to (0: it read() the descriptor itself)
	std::string error;
	// bytes [span_base, span_base + the spans) of the stream are still in memory (every chunk from the one that holds `last` on);
	// the descriptor continues behind them
	uint64_t span_base = 0;
	std::vector<std::pair<const uint8_t *, size_t>> spans;
private:
	struct Buf { std::vector<uint8_t> data; uint64_t len = 0, off = 0; bool last = false; };
	static constexpr int NB = 4;                             // the chunk before the packer's (its tail may hold the last framed record), the packer's, two read ahead
	// A pipe is one copy stream per reader: read() copies page by page under the pipe's lock (~5 GB/s against a producer that
	// write()s, ~9 GB/s against one that lends its pages, profiles/pipe_ab_r06.jsonl).  splice() between two pipes MOVES page
	// references instead: the reader thread deals the stream in segments to a few private pipes, and a copier thread per private
	// pipe read()s its segments into their places in the chunk -- the copies run side by side ($VARGENO_PIPE_COPIERS, default 4;
	// 0: the plain read() loop).  Everything taken from the descriptor has reached the ring when a chunk is handed on, so the
	// host reader still continues at the descriptor.  A descriptor that cannot be spliced from (EINVAL on the first call): read().
	struct Copier {
		int r = -1, w = -1;
		std::thread th;
		std::mutex mu; std::condition_variable cv;
		std::vector<std::pair<uint8_t *, size_t>> q; size_t head = 0;      // segments of the current chunk, in order
		bool stop = false, failed = false;
		void run()
		{
			for (;;) {
				std::pair<uint8_t *, size_t> job;
				{ std::unique_lock<std::mutex> g(mu); cv.wait(g, [&] { return head < q.size() || stop; }); if (head >= q.size()) return; job = q[head]; }
				size_t at = 0;
				bool bad = false;
				while (at < job.second) {
					const ssize_t got = read(r, job.first + at, job.second - at);
					if (got < 0 && errno == EINTR) continue;
					if (got <= 0) { bad = true; break; }
					at += (size_t)got;
				}
				{ std::lock_guard<std::mutex> g(mu); head++; if (bad) failed = true; }
				cv.notify_all();
			}
		}
		void push(uint8_t *dest, size_t n) { { std::lock_guard<std::mutex> g(mu); q.emplace_back(dest, n); } cv.notify_all(); }
		bool drain() { std::unique_lock<std::mutex> g(mu); cv.wait(g, [&] { return head >= q.size(); }); q.clear(); head = 0; return !failed; }
	};
	void read_loop()
	{
		std::vector<std::unique_ptr<Copier>> cop;
		for (int k = 0; k < want_copiers_; k++) {
			int p[2];
			if (pipe(p) != 0) break;
			(void)fcntl(p[1], F_SETPIPE_SZ, 1 << 20);               // (fails harmlessly when the user's pipe pages are used up: 64 KiB then)
			cop.emplace_back(new Copier());
			cop.back()->r = p[0]; cop.back()->w = p[1];
			Copier *c = cop.back().get();
			c->th = std::thread([c] { c->run(); });
		}
		bool fan = !cop.empty();
		uint64_t seg = 0, spliced = 0;
		for (uint64_t i = 0;; i++) {
			{ std::unique_lock<std::mutex> g(mu_); cv_.wait(g, [&] { return i + 2 <= done_ + (uint64_t)NB || stop_reading_; }); if (stop_reading_) break; }
			Buf &b = ring_[i % NB];
			uint64_t got = 0;
			bool eof = false, bad = false;
			while (got < chunk_) {
				ssize_t g;
				if (fan) {
					Copier &c = *cop[(size_t)(seg % cop.size())];
					g = splice(fd_, nullptr, c.w, nullptr, (size_t)std::min<uint64_t>(chunk_ - got, 1u << 20), SPLICE_F_MOVE);
					if (g < 0 && errno == EINTR) continue;
					if (g < 0 && spliced == 0 && (errno == EINVAL || errno == ENOSYS || errno == EBADF)) { fan = false; continue; }
					if (g > 0) { c.push(b.data.data() + got, (size_t)g); seg++; spliced += (uint64_t)g; }
				} else {
					g = read(fd_, b.data.data() + got, (size_t)(chunk_ - got));
					if (g < 0 && errno == EINTR) continue;
				}
				if (g < 0) { bad = true; eof = true; break; }
				if (g == 0) { eof = true; break; }
				got += (uint64_t)g;
				// (a refusal: the packer will read no further -- hand over what has arrived, the host reader reads on from the descriptor)
				{ std::lock_guard<std::mutex> l(mu_); if (stop_reading_) break; }
			}
			for (auto &c : cop) if (!c->drain()) { bad = true; eof = true; }      // (every byte taken from the descriptor is in the chunk now)
			{ std::lock_guard<std::mutex> l(mu_); if (bad) io_error_ = true; b.len = got; b.off = total_read_; b.last = eof; total_read_ += got; filled_ = i + 1; if (eof) eof_ = true; }
			cv_.notify_all();
			if (eof) break;
		}
		for (auto &c : cop) {
			{ std::lock_guard<std::mutex> g(c->mu); c->stop = true; }
			c->cv.notify_all();
			c->th.join();
			close(c->r); close(c->w);
		}
		{ std::lock_guard<std::mutex> l(mu_); reader_done_ = true; copiers_ = fan ? (int)cop.size() : 0; }
		cv_.notify_all();
	}
	void work_loop()
	{
		vg_packer *pk = nullptr;
		const uint64_t rcap = vg_packer_reads_cap(chunk_), kcap = vg_packer_kmers_cap(chunk_);
		uint64_t *stage[2] = {nullptr, nullptr};
		int set_store[2] = {-1, -1};                         // the store whose copies may still read staging set k
		auto bail = [&](const std::string &e) { if (error.empty()) error = e; };
		if (vg_packer_create(pack_threads_, &pk) != VG_OK) bail(vg_last_error());
		bool pinned[2] = {true, true};                       // (page-locked when a device is there to lock it for; any memory works)
		for (int k = 0; k < 2 && error.empty(); k++) {
			stage[k] = (uint64_t *)vg_host_alloc_pinned((size_t)(kcap + 2 * rcap + 2) * 8);
			if (!stage[k]) { pinned[k] = false; stage[k] = (uint64_t *)malloc((size_t)(kcap + 2 * rcap + 2) * 8); }
			if (!stage[k]) bail("staging for the FASTQ stream: allocation failed");
		}
		const size_t nrep = stores_.size();
		size_t rr = 0;
		uint64_t n_sets = 0;
		uint64_t i = 0;
		for (; error.empty(); i++) {
			{ std::unique_lock<std::mutex> g(mu_); cv_.wait(g, [&] { return filled_ > i || reader_done_; }); if (filled_ <= i) break; }
			Buf &b = ring_[i % NB];
			if (b.len) {
				const int k = (int)(n_sets & 1);
				if (set_store[k] >= 0) { if (vg_read_store_flush(stores_[(size_t)set_store[k]]) != VG_OK) { bail(vg_last_error()); break; } set_store[k] = -1; }
				uint64_t *sk = stage[k], *sm = sk + kcap, *so = sm + rcap;
				uint64_t nr = 0, nc = 0, ninv = 0;
				if (vg_packer_push(pk, b.data.data(), b.len, sk, kcap, sm, so, rcap, &nr, &nc, &ninv) != VG_OK) { bail(vg_last_error()); break; }
				if (nr) {
					bool sent = false;
					bool att; { std::lock_guard<std::mutex> g(mu_); att = attached_; }
					if (!att && stores_[rr]) {
						const int prc = vg_read_store_push(stores_[rr], sk, sm, so, nr);
						if (prc == VG_OK) { sent = true; set_store[k] = (int)rr; n_sets++; to_store += nr; }
						else if (prc != VG_ENOMEM) { bail(vg_last_error()); break; }
					}
					if (!sent) {
						// the store is full (or there is none): this batch waits here for the handle -- the reader thread keeps filling the ring,
						// then the pipe's writer waits
						{ std::unique_lock<std::mutex> g(mu_); cv_.wait(g, [&] { return attached_; }); }
						const std::string e = sink_(rr, sk, sm, so, nr);
					if (!e.empty()) { bail(e); break; }
					direct += nr;
					}
					rr = (rr + 1) % nrep;
				}
				int ref = 0;
				(void)vg_packer_end(pk, &records, &consumed, &last, &ref);     // (a query: the stream's totals so far)
				if (ref) { refused = true; i++; break; }
			}
			{ std::lock_guard<std::mutex> g(mu_); done_ = i + 1; }           // (chunk i stays in the ring until chunk i + 1 is done with: the last framed record may begin in it)
			cv_.notify_all();
			if (b.last) { i++; break; }
		}
		// the end of the stream, a refusal or an error: the reader stops after the read() it is in; every chunk from the one before the
		// packer's last on is handed to the host reader
		{ std::lock_guard<std::mutex> g(mu_); stop_reading_ = true; }
		cv_.notify_all();
		if (reader_.joinable()) reader_.join();
		for (int k = 0; k < 2; k++) if (set_store[k] >= 0) (void)vg_read_store_flush(stores_[(size_t)set_store[k]]);
		{
			std::lock_guard<std::mutex> g(mu_);
			if (io_error_) bail("error reading the FASTQ stream");
			bytes_read = total_read_;
			copiers = copiers_;
			// chunks [first, filled_) are intact in the ring: first = the chunk before the last one the packer saw (or 0)
			const uint64_t seen = i;                                             // chunks the packer has been given
			const uint64_t first = seen >= 2 ? seen - 2 : 0;
			span_base = filled_ > first ? ring_[first % NB].off : total_read_;
			for (uint64_t c = first; c < filled_; c++) spans.emplace_back(ring_[c % NB].data.data(), (size_t)ring_[c % NB].len);
		}
		for (int k = 0; k < 2; k++) if (stage[k]) { if (pinned[k]) vg_host_free_pinned(stage[k]); else free(stage[k]); }
		if (pk) vg_packer_destroy(pk);
		struct timespec now; clock_gettime(CLOCK_MONOTONIC, &now);
		seconds = (double)(now.tv_sec - born_.tv_sec) + 1e-9 * (double)(now.tv_nsec - born_.tv_nsec);
	}
	const int fd_; const uint64_t chunk_; const int pack_threads_, want_copiers_;
	std::vector<vg_read_store *> stores_;
	Sink sink_;
	Buf ring_[NB];
	std::mutex mu_; std::condition_variable cv_;
	uint64_t filled_ = 0, done_ = 0, total_read_ = 0;
	bool eof_ = false, reader_done_ = false, stop_reading_ = false, io_error_ = false, attached_ = false;
	int copiers_ = 0;
	std::thread reader_, worker_;
	struct timespec born_;
};

// The first record start at or after `from`: the start of a line that begins with '@' whose next-but-one line begins with '+'
// (a quality line may begin with '@', but then the line two below it is a sequence line, and no sequence begins with '+').
// Returns fsize when there is none; UINT64_MAX on a line too long to be a FASTQ line of this tool (the caller falls back).
static uint64_t find_record_start(int fd, uint64_t from, uint64_t fsize)
{
	if (from == 0) return 0;
	const uint64_t WIN = 1 << 20;
	std::vector<char> buf((size_t)WIN);
	uint64_t base = from - 1;                                        // one byte back: is `from` itself the start of a line?
	const uint64_t n = std::min(WIN, fsize - base);
	uint64_t got = 0;
	while (got < n) { const ssize_t g = pread(fd, buf.data() + got, (size_t)(n - got), (off_t)(base + got)); if (g <= 0) break; got += (uint64_t)g; }
	std::vector<uint64_t> starts;                                    // line starts inside the window
	for (uint64_t i = 0; i + 1 < got; i++) if (buf[(size_t)i] == '\n') starts.push_back(i + 1);
	for (size_t k = 0; k + 2 < starts.size(); k++)
		if (buf[(size_t)starts[k]] == '@' && buf[(size_t)starts[k + 2]] == '+') return base + starts[k];
	// the window reaches the end of the file and holds no record start: the split point fell inside the last record (its header
	// line included) -- what is left belongs to the range before
	if (base + got >= fsize) return fsize;
	return UINT64_MAX;
}

// Where n replicas split the file: cut[0] = 0 <= cut[1] <= ... <= cut[n] = fsize, every inner cut a record start.  false: no
// record start where one should be (the caller frames the whole file on the host).
static bool range_cuts(int fd, uint64_t fsize, int n, std::vector<uint64_t> &cut)
{
	cut.assign((size_t)n + 1, fsize);
	cut[0] = 0;
	for (int g = 1; g < n; g++) {
		const uint64_t at = find_record_start(fd, std::max(cut[(size_t)g - 1], fsize / (uint64_t)n * (uint64_t)g), fsize);
		if (at == UINT64_MAX) return false;
		cut[(size_t)g] = at;
	}
	return true;
}

static double secs(const struct timespec &a, const struct timespec &b) { return (double)(b.tv_sec - a.tv_sec) + 1e-9 * (double)(b.tv_nsec - a.tv_nsec); }

// ---- `vargeno geno`, step by step (run_geno at the end puts the steps together) ------------------------------------------------
// The FASTQ as the command line was given it; what it is decides the ingest route
struct FastqInput {
	int fd = -1;                               // (-1 under VARGENO_HOST_FASTQ=1: the host reader opens the path itself)
	uint64_t fsize = 0;
	bool once_only = false;                    // a FIFO, /dev/stdin, <(...): one descriptor, read once, no ranges (PipeIngest)
	bool cuts_ok = false;                      // a regular file, and cut[] holds a record-aligned range per replica
	std::vector<uint64_t> cut;
	bool bgzf_device = false;                  // a BGZF file, one replica, VARGENO_BGZF=device: the compressed bytes are streamed to the device
	bool gzip_device = false;                  // a plain gzip file, one replica, VARGENO_GZIP=device: the same, through the chunked inflate
	bool bam = false;                          // ... the file is BAM: the device frames its records (bgzf_device), or the pipe below converts them to text
	std::unique_ptr<vgh::TextPipe> bz_pipe;    // a BGZF / BAM file on every other route: inflated (and converted) by host threads; fd is the pipe's read end
	int file_fd = -1;                          // ... and the file itself
};
// Bytes of a once-only stream that are still in memory, for the host reader: [base, base + the spans); the descriptor continues behind them
struct HostSpans {
	uint64_t base = 0;
	std::vector<std::pair<const uint8_t *, size_t>> spans;
};
// What an ingest route hands to the host reader that runs behind it
struct HostHandover {
	uint64_t total = 0;                        // reads the route framed
	uint64_t host_from = 0;                    // file offset the host reader takes over from
	uint64_t prime_from = UINT64_MAX;          // start of the last record the route framed (to prime the stale buffers)
	int next_gpu = 0;                          // the replica the host reader's first batch goes to
};

// The size of replica g's read store: VARGENO_PREPACK_GB per device, never more than an eighth of the device, shared among the
// replicas on it, at most `bound`; or VARGENO_PREPACK_BYTES exactly (tests: a store that fills up after a chunk or two)
static uint64_t read_store_bytes(const GenoOptions &o, int g, uint64_t bound)
{
	const uint64_t bytes = std::min<uint64_t>(std::min<uint64_t>(o.prepack_want, vg_device_memory(g % o.have) / 8) / (uint64_t)o.replicas_on_device(g), bound);
	return o.prepack_bytes ? o.prepack_bytes : bytes;
}

// false: the path cannot be opened (said on stderr)
static bool open_fastq(const std::string &fastq, const GenoOptions &o, FastqInput &in)
{
	struct stat sb;
	if (o.host_framing && (stat(fastq.c_str(), &sb) != 0 || !S_ISREG(sb.st_mode))) return true;     // (the host reader opens the path itself, once)
	in.fd = open(fastq.c_str(), O_RDONLY);
	if (in.fd < 0) { fprintf(stderr, "vargeno: cannot open %s\n", fastq.c_str()); return false; }
	if (fstat(in.fd, &sb) != 0) { close(in.fd); fprintf(stderr, "vargeno: cannot stat %s\n", fastq.c_str()); return false; }
	in.fsize = (uint64_t)sb.st_size;
	in.once_only = !S_ISREG(sb.st_mode);
	// a regular file says what it is (a FIFO or /dev/stdin cannot be looked at without taking its bytes: it is text, as before)
	const vgh::FastqKind kind = in.once_only ? vgh::FastqKind::Text : vgh::sniff_fastq(in.fd);
	if (kind == vgh::FastqKind::Bgzf || kind == vgh::FastqKind::Bam) {
		in.bam = kind == vgh::FastqKind::Bam;
		if (o.bgzf_device && o.ngpu == 1 && !o.host_framing) { in.bgzf_device = true; return true; }
		in.file_fd = in.fd;
		if (in.bam) in.bz_pipe.reset(new vgh::BamTextPipe(in.file_fd, 0, 0, o.bgzf_threads, true, 0));
		else in.bz_pipe.reset(new vgh::BgzfTextPipe(in.file_fd, 0, 0, o.bgzf_threads));
		if (in.bz_pipe->read_fd() < 0) { fprintf(stderr, "vargeno: %s\n", in.bz_pipe->error.c_str()); return false; }
		in.fd = in.bz_pipe->read_fd();
		in.once_only = true;
	} else if (kind == vgh::FastqKind::PlainGzip && o.gzip_host) {          // (VARGENO_GZIP unset: plain_gzip() has refused the file before)
		if (o.gzip_device && o.ngpu == 1 && !o.host_framing) { in.gzip_device = true; return true; }
		in.file_fd = in.fd;
		in.bz_pipe.reset(new vgh::GzipTextPipe(in.file_fd));
		if (in.bz_pipe->read_fd() < 0) { fprintf(stderr, "vargeno: %s\n", in.bz_pipe->error.c_str()); return false; }
		in.fd = in.bz_pipe->read_fd();
		in.once_only = true;
	}
	if (o.host_framing) { if (!in.bz_pipe) { close(in.fd); in.fd = -1; } return true; }
	if (in.once_only) (void)fcntl(in.fd, F_SETPIPE_SZ, 1 << 20);        // (a pipe: the largest buffer an unprivileged process may ask for; fails harmlessly on anything else)
	else in.cuts_ok = range_cuts(in.fd, in.fsize, o.ngpu, in.cut);
	return true;
}

// The once-only route starts NOW, beside the index open: a read store per replica (none: its batches wait for the handle), and
// the ingest whose sink submits to the handles in `ix` once they exist (PipeIngest::attach)
static std::unique_ptr<PipeIngest> start_pipe_ingest(const GenoOptions &o, int fd, std::vector<vg_read_store *> &store, const std::vector<vg_index *> &ix)
{
	if (o.prepack) for (int g = 0; g < o.ngpu; g++)
		if (vg_read_store_create(g % o.have, read_store_bytes(o, g, UINT64_MAX), &store[(size_t)g]) != VG_OK) store[(size_t)g] = nullptr;
	return std::unique_ptr<PipeIngest>(new PipeIngest(fd, o.pipe_chunk(), std::max(1, o.pack_threads * o.ngpu), o.pipe_copiers, store,
	                                                  [&ix](size_t g, const uint64_t *k, const uint64_t *m, const uint64_t *off, uint64_t n) -> std::string {
		                                                  return vg_reads_submit_packed(ix[g], k, m, off, n) == VG_OK ? std::string() : std::string("vg_reads_submit_packed failed: ") + vg_last_error();
	                                                  }));
}

// The ranged route packs ahead of the index: a read store per replica, on its device, taken NOW (the index is planned with what
// is left): as large as the range's packed form (~1/5.5 of its text, and room for a chunk's worst case is not needed: a push that
// does not fit ends the pre-packing), at most VARGENO_PREPACK_GB per device and never more than an eighth of the device
static std::vector<std::unique_ptr<PrePacker>> start_prepackers(const GenoOptions &o, const FastqInput &in, std::vector<vg_read_store *> &store)
{
	std::vector<std::unique_ptr<PrePacker>> pre((size_t)o.ngpu);
	if (!in.cuts_ok || o.pack_threads <= 0 || !o.prepack) return pre;
	for (int g = 0; g < o.ngpu; g++) {
		const uint64_t lo = in.cut[(size_t)g], hi = in.cut[(size_t)g + 1];
		if (lo >= hi) continue;
		if (vg_read_store_create(g % o.have, read_store_bytes(o, g, (hi - lo) / 5 + (8ull << 20)), &store[(size_t)g]) != VG_OK) { fprintf(stderr, "vargeno: no read store on device %d (%s): its range is framed after the index is open\n", g % o.have, vg_last_error()); continue; }
		pre[(size_t)g].reset(new PrePacker(in.fd, lo, hi, o.prepack_chunk(), o.range_readers(), o.pack_threads, o.prepack_mmap, store[(size_t)g]));
	}
	return pre;
}

// All replicas open their index at once, each under a budget computed HERE, before the first open.  false: said on stderr
static bool open_indexes(const std::string &prefix, const GenoOptions &o, const std::vector<vg_read_store *> &store, std::vector<vg_index *> &ix, bool pipe_running)
{
	const int ngpu = o.ngpu, have = o.have;
	std::vector<std::thread> th;
	std::vector<int> rcs((size_t)ngpu, 0);
	std::vector<std::string> errs((size_t)ngpu);
	// replicas that share a device (VARGENO_SHARE_DEVICES) share its memory too: without a budget of its own each of them gets
	// an equal part -- planned for the whole device, the third or fourth one would fail where it could have run on fewer views
	std::vector<uint64_t> budgets((size_t)ngpu, o.budget);
	if (!o.budget && ngpu > have) for (int g = 0; g < ngpu; g++) { const int on = o.replicas_on_device(g); if (on > 1) budgets[(size_t)g] = vg_share_budget(g % have, on); }
	// a read store was taken on the device before the index is planned: the plan must be told, or it plans for the device's TOTAL
	// less 12 GiB while the store (up to 16 GiB) already holds part of that -- an index whose views fill the budget would then
	// fail in its allocations where it could have run on fewer views.  vg_share_budget looks at what is free NOW (all budgets are
	// computed here, before any replica opens)
	if (!o.budget) for (int g = 0; g < ngpu; g++) if (!budgets[(size_t)g] && store[(size_t)g]) budgets[(size_t)g] = vg_share_budget(g % have, o.replicas_on_device(g));
	for (int g = 0; g < ngpu; g++) th.emplace_back([&, g] { rcs[(size_t)g] = vg_index_open_ex(prefix.c_str(), g % have, budgets[(size_t)g], &ix[(size_t)g]); if (rcs[(size_t)g]) errs[(size_t)g] = vg_last_error(); });
	for (auto &t : th) t.join();
	for (int g = 0; g < ngpu; g++) if (rcs[(size_t)g]) {
		fprintf(stderr, "vargeno: cannot load index %s on GPU %d (%d): %s\n", prefix.c_str(), g, rcs[(size_t)g], errs[(size_t)g].c_str());
		if (pipe_running) exit(EXIT_FAILURE);                           // (its threads hold the pipe: no unwinding)
		return false;
	}
	return true;
}

// Replica g's range [cut[g], cut[g + 1]) on the ranged route: what its pre-packer (if it has one) put into the read store is
// submitted first, then the rest of the range is streamed.  `route` says in words what was done (the verbose "ingest" line).
static StreamResult ingest_range(const GenoOptions &o, const FastqInput &in, int g, double link, vg_index *ix, vg_read_store *store, PrePacker *pre, std::string &route)
{
	StreamResult r;
	const uint64_t range_lo = in.cut[(size_t)g], range_hi = in.cut[(size_t)g + 1];
	uint64_t done_to = 0;                                  // bytes of the range framed so far
	// the rest of a range (what the pre-packer did not take -- it was stopped, its store filled up, or it never ran): host
	// packing or device framing, whichever is faster HERE.  With a pre-packer its measured rate decides, whether it is
	// still running or done (a 30x file overruns a 16 GB store: the larger part of the file is "the rest"); without one
	// (VARGENO_PREPACK=0, no store) the number of CPUs does, as in r04, unless VARGENO_PACK_THREADS says what is wanted
	bool pack_rest = o.pack_threads > 0 && (o.pack_threads_given || o.hw >= 32);
	if (pre) {
		PrePacker &pp = *pre;
		pack_rest = o.pack_threads > 0;
		// it keeps the rest of the range unless the device-side framing would finish it at least a second earlier
		// (changing horses costs about that much: a new stream, its readers starting cold)
		const double rp = pp.text_bytes_per_s();
		const double left = (double)(range_hi - range_lo) - (double)pp.text_bytes_done();
		if (rp > 0 && link > 0 && left > 0) pack_rest = rp >= link || left * (1.0 / rp - 1.0 / link) < 1.0;
		if (!pp.done() && !pack_rest) pp.stop();
		pp.join();
		if (!pp.error.empty()) r.error = pp.error;
		const uint64_t submitted = vg_read_store_reads(store);
		if (r.error.empty() && vg_reads_submit_store(ix, store) != VG_OK) r.error = std::string("vg_reads_submit_store failed: ") + vg_last_error();
		r.nrec = pp.records(); r.used = pp.consumed(); r.last = pp.last_record_start(); r.refused = pp.refused() ? 1 : 0;
		done_to = pp.consumed();
		char line[320];
		snprintf(line, sizeof line, "%lu reads packed ahead of / beside the index into %.1f GB of device memory (%.1f GB/s of text on %d threads, done %.2f s after the command line started them%s; link %.1f GB/s)",
		         (unsigned long)submitted, (double)vg_read_store_bytes_used(store) / 1e9, pp.text_bytes_per_s() / 1e9, o.pack_threads, pp.finished_after_s(), pp.store_full() ? ", when the store was full" : "", link / 1e9);
		route = line;
	}
	const uint64_t lo = range_lo + done_to, hi = range_hi;
	if (r.error.empty() && !r.refused && lo < hi) {
		const StreamResult r2 = stream_range(ix, in.fd, lo, hi, o.rest_chunk(pack_rest), o.range_readers(), pack_rest ? o.pack_threads : 0);
		route += pack_rest ? "; rest of the range: framed + packed by host threads" : "; rest of the range: framed on the device";
		if (!r2.error.empty()) r.error = r2.error;
		if (r2.nrec) r.last = done_to + r2.last;
		r.nrec += r2.nrec; r.used = done_to + r2.used; r.refused = r2.refused;
	}
	return r;
}

// Default ingest: the file is a byte stream to the device(s).  One replica takes all of it; several take one contiguous range
// each, cut at record starts, all at once.  A range's text is framed + packed by host threads (what was packed while the index
// was being opened is submitted first) or copied up as it is and framed on the device -- whichever runs faster HERE: the
// pre-packer has measured its rate, vg_link_rate() the link's.  Whatever the stream refuses (from the first chunk with a line
// beyond fgets' 1023 characters on) and the (possibly truncated) tail of the file go through the host reader, which
// reproduces the reference's four-fgets framing exactly, stale buffers included; with several replicas a refusal anywhere but
// in the last range means the ranges after it were framed out of step with the reference, so everything is reset and framed
// on the host.
static HostHandover ranged_route(const GenoOptions &o, const FastqInput &in, const std::vector<vg_index *> &ix, const std::vector<vg_read_store *> &store, const std::vector<std::unique_ptr<PrePacker>> &pre)
{
	HostHandover hand;
	if (!in.cuts_ok) {                                               // no record start found where one should be: the host reader takes the file
		fprintf(stderr, "vargeno: no FASTQ record start within 1 MiB of a range boundary: the whole file is framed on the host (slower)\n");
		return hand;
	}
	const int ngpu = o.ngpu;
	const std::vector<uint64_t> &cut = in.cut;
	const double link = o.pack_threads > 0 ? vg_link_rate(0) : 0.0;    // bytes/s of text the device-side framing can be fed at
	std::vector<StreamResult> res((size_t)ngpu);
	std::vector<std::string> route((size_t)ngpu);
	std::vector<std::thread> th;
	for (int g = 0; g < ngpu; g++)
		if (cut[(size_t)g] < cut[(size_t)g + 1] || g == 0)
			th.emplace_back([&, g] { res[(size_t)g] = ingest_range(o, in, g, link, ix[(size_t)g], store[(size_t)g], pre[(size_t)g].get(), route[(size_t)g]); });
	for (auto &t : th) t.join();
	for (int g = 0; g < ngpu; g++) if (!res[(size_t)g].error.empty()) { fprintf(stderr, "vargeno: %s\n", res[(size_t)g].error.c_str()); exit(EXIT_FAILURE); }
	if (o.verbose) for (int g = 0; g < ngpu; g++) if (!route[(size_t)g].empty()) fprintf(stderr, "ingest, replica %d: %s\n", g, route[(size_t)g].c_str());
	int last_range = 0;                                              // the last range that holds bytes
	for (int g = 0; g < ngpu; g++) if (cut[(size_t)g] < cut[(size_t)g + 1]) last_range = g;
	bool in_step = true;
	for (int g = 0; g < last_range; g++) if (res[(size_t)g].used != cut[(size_t)g + 1] - cut[(size_t)g]) in_step = false;
	if (in_step) {
		for (int g = 0; g <= last_range; g++) hand.total += res[(size_t)g].nrec;
		for (int g = last_range; g >= 0; g--) if (res[(size_t)g].nrec) { hand.prime_from = cut[(size_t)g] + res[(size_t)g].last; break; }
		hand.host_from = cut[(size_t)last_range] + res[(size_t)last_range].used;    // the incomplete tail, or everything from a refused chunk on
		hand.next_gpu = last_range;
	} else {
		// (the file has been streamed once already: a 2x or larger slowdown that must not pass silently)
		fprintf(stderr, "vargeno: a FASTQ range before the last one was refused by the stream framing (a line beyond 1023 characters?): "
		                "counters reset, the whole file is framed on the host\n");
		for (auto *h : ix) VG_CHECK(vg_counts_reset(h));
	}
	return hand;
}

// A stream that is read once: what went into the read stores while the index opened first, then the packer's batches
// straight into the read loops until the stream ends (or is refused)
static HostHandover once_only_route(const GenoOptions &o, PipeIngest &pipe_in, const std::vector<vg_index *> &ix, const std::vector<vg_read_store *> &store)
{
	const int ngpu = o.ngpu;
	for (int g = 0; g < ngpu; g++) if (store[(size_t)g]) { VG_CHECK(vg_read_store_flush(store[(size_t)g])); }
	pipe_in.attach();
	pipe_in.finish();
	for (int g = 0; g < ngpu; g++) if (store[(size_t)g] && vg_read_store_reads(store[(size_t)g])) VG_CHECK(vg_reads_submit_store(ix[(size_t)g], store[(size_t)g]));
	if (!pipe_in.error.empty()) { fprintf(stderr, "vargeno: %s\n", pipe_in.error.c_str()); exit(EXIT_FAILURE); }
	if (o.verbose) fprintf(stderr, "ingest, replica 0: the FASTQ is not a regular file: one descriptor read once, %lu reads framed + packed by %d host threads (%lu into the read stores while the index opened, %lu straight into the read loop), "
	                               "%.2f GB of text in %.2f s (%.2f GB/s), dealt to %d copier threads%s\n", (unsigned long)pipe_in.records, std::max(1, o.pack_threads * ngpu), (unsigned long)pipe_in.to_store, (unsigned long)pipe_in.direct,
	                       (double)pipe_in.bytes_read / 1e9, pipe_in.seconds, pipe_in.seconds > 0 ? (double)pipe_in.bytes_read / 1e9 / pipe_in.seconds : 0.0, pipe_in.copiers, pipe_in.refused ? "; the stream framing refused a chunk: the host reader takes the rest" : "");
	return HostHandover{pipe_in.records, pipe_in.consumed, pipe_in.records ? pipe_in.last : UINT64_MAX, 0};
}

// One replica, a BGZF file, VARGENO_BGZF=device: the compressed file goes to the device through the text route's reader ring
// (vg_fastq_stream_begin_bgzf); no pre-packers, no read store -- reading the file ahead while the index opens is all the overlap.
// The host take-over behind it (a framing refusal, a truncated final record) needs TEXT from the last framed record on:
// vg_fastq_stream_bgzf_locate says which block holds it, the blocks up to the hand-over point are inflated here into a memory
// span, and a BgzfTextPipe inflates the rest of the file into a pipe -- the span plus a descriptor, what the host reader takes.
struct BgzfTakeover {
	std::vector<uint8_t> text;
	std::unique_ptr<vgh::TextPipe> rest;
	HostSpans mem;
};
static HostHandover bgzf_device_route(const GenoOptions &o, const FastqInput &in, vg_index *ix, BgzfTakeover &tk)
{
	struct timespec a, b; clock_gettime(CLOCK_MONOTONIC, &a);
	const StreamResult r = stream_range(ix, in.fd, 0, in.fsize, o.chunk(16), o.range_readers(), 0, STREAM_BGZF);
	if (!r.error.empty()) { fprintf(stderr, "vargeno: %s\n", r.error.c_str()); exit(EXIT_FAILURE); }
	clock_gettime(CLOCK_MONOTONIC, &b);
	const uint64_t from = r.nrec ? r.last : r.used;                      // the span starts with the last framed record (it primes the stale buffers)
	uint64_t block = 0, comp_next = 0;
	uint32_t within = 0;
	VG_CHECK(vg_fastq_stream_bgzf_locate(ix, from, &block, &within));
	std::string err;
	if (!vgh::bgzf_inflate_span(in.fd, block, within + (r.used - from), tk.text, &comp_next, err)) { fprintf(stderr, "vargeno: %s\n", err.c_str()); exit(EXIT_FAILURE); }
	tk.mem.base = from - within;
	tk.mem.spans.assign(1, std::make_pair((const uint8_t *)tk.text.data(), tk.text.size()));
	tk.rest.reset(new vgh::BgzfTextPipe(in.fd, comp_next, 0, o.bgzf_threads));
	if (tk.rest->read_fd() < 0) { fprintf(stderr, "vargeno: %s\n", tk.rest->error.c_str()); exit(EXIT_FAILURE); }
	if (o.verbose) fprintf(stderr, "ingest, replica 0: BGZF inflated on the device: %lu reads framed, %.3f GB compressed (%.2f GB/s), %.3f GB of text (%.2f GB/s) in %.2f s%s\n", (unsigned long)r.nrec,
	                       (double)in.fsize / 1e9, (double)in.fsize / 1e9 / secs(a, b), (double)r.used / 1e9, (double)r.used / 1e9 / secs(a, b), secs(a, b), r.refused ? "; the stream framing refused a chunk: the host reader takes the rest" : "");
	return HostHandover{r.nrec, r.used, r.nrec ? r.last : UINT64_MAX, 0};
}
// One replica, a BAM file, VARGENO_BGZF=device: as above, and the device frames the records too (vg_fastq_stream_begin_bam) -- no
// text exists on this route.  The offsets it reports are offsets in the inflated BAM stream.  The host take-over behind it (a
// refusal: a read beyond the reference's line buffer, ...) needs TEXT: the last kept record is converted here and is the memory span
// that primes the host reader's line buffers (they must hold what they would after that record), and a BamTextPipe converts the
// records from `consumed` on into a pipe.  The reader's offsets are offsets in that text: the span is [0, its length).
static HostHandover bam_device_route(const GenoOptions &o, const FastqInput &in, vg_index *ix, BgzfTakeover &tk)
{
	struct timespec a, b; clock_gettime(CLOCK_MONOTONIC, &a);
	const StreamResult r = stream_range(ix, in.fd, 0, in.fsize, o.chunk(16), o.range_readers(), 0, STREAM_BAM);
	if (!r.error.empty()) { fprintf(stderr, "vargeno: %s\n", r.error.c_str()); exit(EXIT_FAILURE); }
	clock_gettime(CLOCK_MONOTONIC, &b);
	uint64_t kept = 0, skipped_flag = 0, skipped_empty = 0, repairs = 0;
	VG_CHECK(vg_bam_stream_stats(ix, &kept, &skipped_flag, &skipped_empty, &repairs));
	uint64_t block = 0;
	uint32_t within = 0;
	std::string err, primer;
	if (r.nrec) {
		VG_CHECK(vg_fastq_stream_bgzf_locate(ix, r.last, &block, &within));
		if (!vgh::bam_record_text(in.fd, block, within, primer, err)) { fprintf(stderr, "vargeno: %s\n", err.c_str()); exit(EXIT_FAILURE); }
	}
	tk.text.assign(primer.begin(), primer.end());
	tk.mem.base = 0;
	tk.mem.spans.assign(1, std::make_pair((const uint8_t *)tk.text.data(), tk.text.size()));
	VG_CHECK(vg_fastq_stream_bgzf_locate(ix, r.used, &block, &within));
	tk.rest.reset(new vgh::BamTextPipe(in.fd, block, within, o.bgzf_threads, false, r.used));
	if (tk.rest->read_fd() < 0) { fprintf(stderr, "vargeno: %s\n", tk.rest->error.c_str()); exit(EXIT_FAILURE); }
	if (o.verbose) fprintf(stderr, "ingest, replica 0: BAM inflated and framed on the device: %lu records kept, %lu skipped by flag, %lu skipped empty, %lu window repairs; %.3f GB compressed (%.2f GB/s) in %.2f s%s\n",
	                       (unsigned long)kept, (unsigned long)skipped_flag, (unsigned long)skipped_empty, (unsigned long)repairs, (double)in.fsize / 1e9, (double)in.fsize / 1e9 / secs(a, b), secs(a, b),
	                       r.refused ? "; the device refused a chunk: the host converts the rest" : "");
	return HostHandover{r.nrec, tk.text.size(), r.nrec ? 0 : UINT64_MAX, 0};
}
// One replica, a plain gzip file, VARGENO_GZIP=device: the compressed file goes to the device through the same reader ring
// (vg_fastq_stream_begin_gzip), which inflates it slot by slot and frames the text.  The host take-over behind it (a refused slot, a
// framing refusal, a truncated final record) needs text from the last framed record on: vg_fastq_stream_gzip_checkpoint gives the
// last slot entry at or before it -- a bit offset and the 32 KiB in front of it --, the text from there to the hand-over point is
// inflated here into a memory span, and the same GzipTextPipe inflates the rest of the file into a pipe.
static HostHandover gzip_device_route(const GenoOptions &o, const FastqInput &in, vg_index *ix, BgzfTakeover &tk)
{
	struct timespec a, b; clock_gettime(CLOCK_MONOTONIC, &a);
	const StreamResult r = stream_range(ix, in.fd, 0, in.fsize, o.chunk(16), o.range_readers(), 0, STREAM_GZIP);
	if (!r.error.empty()) { fprintf(stderr, "vargeno: %s\n", r.error.c_str()); exit(EXIT_FAILURE); }
	clock_gettime(CLOCK_MONOTONIC, &b);
	vg_gzip_stats st;
	VG_CHECK(vg_gzip_stream_stats(ix, &st));
	const uint64_t from = r.nrec ? r.last : r.used;                      // the span starts at or before the last framed record (it primes the stale buffers)
	uint64_t at_bit = 0, ck_text = 0;
	uint32_t win_len = 0;
	std::vector<uint8_t> win(32768);
	VG_CHECK(vg_fastq_stream_gzip_checkpoint(ix, from, &at_bit, &ck_text, win.data(), &win_len));
	tk.rest.reset(new vgh::GzipTextPipe(in.fd, at_bit, win.data(), win_len, r.used - ck_text, tk.text));
	if (tk.rest->read_fd() < 0) { fprintf(stderr, "vargeno: %s\n", tk.rest->error.c_str()); exit(EXIT_FAILURE); }
	tk.mem.base = ck_text;
	tk.mem.spans.assign(1, std::make_pair((const uint8_t *)tk.text.data(), tk.text.size()));
	if (o.verbose) fprintf(stderr, "ingest, replica 0: gzip inflated on the device: %lu reads framed, %lu members, %lu chunks, %lu guessed, %lu confirmed, %lu repaired, %lu header tests, %lu slots refused; "
	                               "%.3f GB compressed (%.2f GB/s), %.3f GB of text (%.2f GB/s) in %.2f s%s\n", (unsigned long)r.nrec, (unsigned long)st.members, (unsigned long)st.chunks, (unsigned long)st.guessed,
	                       (unsigned long)st.confirmed, (unsigned long)st.repaired, (unsigned long)st.tested, (unsigned long)st.slots_refused, (double)in.fsize / 1e9, (double)in.fsize / 1e9 / secs(a, b), (double)r.used / 1e9,
	                       (double)r.used / 1e9 / secs(a, b), secs(a, b), st.slots_refused ? "; a slot was refused: the host inflates the rest" : r.refused ? "; the stream framing refused a chunk: the host reader takes the rest" : "");
	return HostHandover{r.nrec, r.used, r.nrec ? r.last : UINT64_MAX, 0};
}
// a TextPipe has met the end of its text: what it has to say (false: a bad block or record, said on stderr)
static bool bgzf_pipe_verdict(const GenoOptions &o, vgh::TextPipe &bp, const char *what, bool tail_of_device_route = false)
{
	bp.finish();
	if (!bp.error.empty()) { fprintf(stderr, "vargeno: %s\n", bp.error.c_str()); return false; }
	if (o.verbose) {
		const std::string line = bp.describe(what, tail_of_device_route);
		if (!line.empty()) fprintf(stderr, "%s\n", line.c_str());
	}
	return true;
}

// The host reader: the file from hand.host_from on -- or, for a stream that is read once, the bytes still in memory and then the
// descriptor (never a second open: a FIFO has lost its writer by then).  Returns the job's reads: the route's and its own.
// submit(replica, batch, n): hands a host-framed batch to a replica's read loop (`geno`: vg_reads_submit; `cohort`: the same after
// selecting the sample's plane, under the replica's mutex).  whole_file: VARGENO_HOST_FASTQ=1, no route ran before.
typedef std::function<void(int, const vgh::ReadBatch &, uint64_t)> BatchSubmit;
static uint64_t host_reader_tail(const GenoOptions &o, const std::string &fastq, int fd, const HostSpans *mem, const HostHandover &hand, bool whole_file, const BatchSubmit &submit)
{
	uint64_t total = hand.total;
	int next_gpu = hand.next_gpu;
	std::unique_ptr<vgh::FastqReader> rdp(mem ? new vgh::FastqReader(fd, mem->base, mem->spans) : new vgh::FastqReader(fastq));
	vgh::FastqReader &rd = *rdp;
	vgh::ReadBatch rb;
	if (!whole_file && hand.prime_from != UINT64_MAX) {       // re-read the last framed record: it only fills the line buffers
		rd.seek(hand.prime_from);
		rb.clear();
		(void)rd.next(rb, 1);
	}
	if (!whole_file) rd.seek(hand.host_from);
	for (;;) {
		rb.clear();
		const uint64_t n = rd.next(rb, o.batch);
		if (!n) break;
		total += n;
		submit(next_gpu, rb, n);
		next_gpu = (next_gpu + 1) % o.ngpu;
	}
	return total;
}

// What the caller needs of the sites themselves (the same for every sample of a cohort)
static void fetch_sites(vg_index *ix, vgh::SiteCounts &sc)
{
	const uint64_t ns = vg_num_sites(ix);
	sc.pos.resize(ns); sc.ref_freq.resize(ns); sc.alt_freq.resize(ns);
	VG_CHECK(vg_sites_fetch(ix, sc.pos.data(), nullptr, nullptr, sc.ref_freq.data(), sc.alt_freq.data()));
}
// The counters of the sample selected on every replica, summed over the replicas.  One process, n devices: one RCCL all-reduce of
// the per-site counters over xGMI (VARGENO_FORCE_RCCL=1 also sends a single device through it, which is the identity)
static void reduce_selected_counts(const GenoOptions &o, std::vector<vg_index *> &ix)
{
	if (o.ngpu > 1 || o.force_rccl) VG_CHECK(vg_counts_allreduce_devices(ix.data(), o.ngpu));
}
static void fetch_reduced_counts(vg_index *ix, vgh::SiteCounts &sc)
{
	const uint64_t ns = vg_num_sites(ix);
	sc.ref_cnt.resize(ns); sc.alt_cnt.resize(ns);
	VG_CHECK(vg_counts_fetch(ix, sc.ref_cnt.data(), sc.alt_cnt.data()));
}
// The calls of the selected sample from the caller kernel, its counters already summed over the replicas.  false: the device had no
// memory for the caller's buffers (VG_ENOMEM; the handle stays usable) -- the host loop over the fetched counters takes its place
static bool fetch_reduced_calls(const GenoOptions &o, vg_index *ix, vgh::SiteCalls &calls)
{
	const uint64_t ns = vg_num_sites(ix);
	calls.gt.resize(ns); calls.gq.resize(ns);
	uint64_t escaped = 0;
	const int rc = vg_sample_calls_fetch(ix, calls.gt.data(), calls.gq.data(), &escaped);
	if (rc == VG_ENOMEM) {
		if (o.verbose) fprintf(stderr, "caller: no device memory for the caller kernel (%s): genotypes are called on the host\n", vg_last_error());
		calls.gt.clear(); calls.gq.clear();
		return false;
	}
	if (rc != VG_OK) { fprintf(stderr, "vargeno: vg_sample_calls_fetch failed (%d): %s\n", rc, vg_last_error()); exit(EXIT_FAILURE); }
	if (o.verbose) fprintf(stderr, "caller: device, %lu sites, %lu recomputed on the host\n", (unsigned long)ns, (unsigned long)escaped);
	return true;
}

// The per-site counters of the whole job, as the caller wants them -- or, with VARGENO_CALLER=device, the calls.  false: said on stderr
static bool fetch_counts(const GenoOptions &o, std::vector<vg_index *> &ix, vgh::SiteCounts &sc, vgh::SiteCalls &calls, bool &have_calls)
{
	{
		// util.c:103: the reference aborts on a read with a character other than ACGTN (and writes no VCF); the library counts
		// such reads whether or not event counting is on
		vg_stats st;
		uint64_t invalid = 0;
		for (auto *h : ix) { VG_CHECK(vg_stats_get(h, &st)); invalid += st.reads_invalid; }
		if (invalid) { fprintf(stderr, "vargeno: %lu reads contain a character other than ACGTN (the reference aborts on these)\n", (unsigned long)invalid); return false; }
	}
	fetch_sites(ix[0], sc);
	reduce_selected_counts(o, ix);
	have_calls = o.caller_device && fetch_reduced_calls(o, ix[0], calls);      // VARGENO_CALLER=device: the calls instead of the counters
	if (!have_calls || o.dump_counts) fetch_reduced_counts(ix[0], sc);
	const uint64_t ns = sc.pos.size();
	if (const char *dump = o.dump_counts) {                              // the saturated counters as the caller gets them: ref counts, then alt counts, one byte per site
		FILE *f = fopen(dump, "wb");
		if (!f || fwrite(sc.ref_cnt.data(), 1, ns, f) != ns || fwrite(sc.alt_cnt.data(), 1, ns, f) != ns) { fprintf(stderr, "vargeno: cannot write %s\n", dump); return false; }
		fclose(f);
	}
	return true;
}

// VARGENO_VERBOSE=1: where the wall time went (t[0] the start, then: index loaded, reads counted, VCF written)
static void verbose_report(uint64_t total, int ngpu, const struct timespec t[4])
{
	struct timespec t1; clock_gettime(CLOCK_MONOTONIC, &t1);
	fprintf(stderr, "reads: %lu  gpus: %d  wall: %.3f s = index load %.3f + FASTQ->counters %.3f (%.2f M reads/s) + call/VCF %.3f + close %.3f\n", (unsigned long)total, ngpu,
	        secs(t[0], t1), secs(t[0], t[1]), secs(t[1], t[2]), (double)total / secs(t[1], t[2]) / 1e6, secs(t[2], t[3]), secs(t[3], t1));
	// how long the process has existed (its start time in /proc/self/stat, 10 ms ticks, against the boot clock): what the loader
	// and the HIP runtime's static start-up took before main() is that minus the wall time above
	if (FILE *f = fopen("/proc/self/stat", "r")) {
		char buf[2048]; const size_t n = fread(buf, 1, sizeof buf - 1, f); buf[n] = 0; fclose(f);
		const char *q = strrchr(buf, ')');
		unsigned long long start = 0; int field = 2;
		for (q = q ? q + 1 : buf; q && *q && field < 22; ) { q = strchr(q + 1, ' '); field++; if (field == 21 && q) start = strtoull(q + 1, nullptr, 10); }
		struct timespec bt; clock_gettime(CLOCK_BOOTTIME, &bt);
		if (start) fprintf(stderr, "process: alive for %.2f s at this point\n", (double)bt.tv_sec + 1e-9 * (double)bt.tv_nsec - (double)start / (double)sysconf(_SC_CLK_TCK));
	}
}

// A regular file with gzip magic but no BGZF header, or a CRAM file: refused by name (framed as text it would yield garbage).  Said on stderr.
static bool plain_gzip(const std::string &fastq)
{
	struct stat sb;
	if (stat(fastq.c_str(), &sb) != 0 || !S_ISREG(sb.st_mode)) return false;      // (a FIFO is opened once, by its reader)
	const int fd = open(fastq.c_str(), O_RDONLY);
	if (fd < 0) return false;                                          // (open_fastq says so)
	const vgh::FastqKind kind = vgh::sniff_fastq(fd);
	const bool plain = kind == vgh::FastqKind::PlainGzip;
	close(fd);
	if (kind == vgh::FastqKind::Cram) {
		fprintf(stderr, "vargeno: %s is a CRAM file: CRAM is not read here -- pipe `samtools fastq %s` through a FIFO (mkfifo reads.fq; samtools fastq %s > reads.fq &) and pass the FIFO\n", fastq.c_str(), fastq.c_str(), fastq.c_str());
		return true;
	}
	if (!plain || gzip_route() != GzipRoute::Refuse) return false;     // (VARGENO_GZIP=device|host: open_fastq / the cohort worker inflate it)
	fprintf(stderr, "vargeno: %s is gzip but not BGZF: only BGZF (bgzip) is inflated here unless VARGENO_GZIP=device|host asks for plain gzip (on the device, or by one host thread) -- or recompress with bgzip, or pass <(zcat %s)\n", fastq.c_str(), fastq.c_str());
	return true;
}

static int run_geno(const std::string &prefix, const std::string &fastq, const std::string &vcf_in, const std::string &vcf_out)
{
	const clock_t begin = clock();
	struct timespec t[4]; clock_gettime(CLOCK_MONOTONIC, &t[0]);       // the start; then: index loaded, reads counted, VCF written
	if (plain_gzip(fastq)) return EXIT_FAILURE;                        // (before the index or a device is asked for)
	std::vector<vgh::ChrLen> chrlens = vgh::read_chrlens(prefix + ".chrlens");
	const int have = vg_device_count();
	if (have <= 0) { fprintf(stderr, "vargeno: no HIP device found (this build has no CPU path)\n"); return EXIT_FAILURE; }
	const GenoOptions o(have);

	fprintf(stderr, "Initializing...\n");
	// ---- the FASTQ file first: where the replicas' ranges are cut, and -- what needs no device -- framing + packing of their text on
	//      host threads, started BEFORE the index is opened and running beside it
	FastqInput in;
	if (!open_fastq(fastq, o, in)) return EXIT_FAILURE;
	std::vector<vg_read_store *> store((size_t)o.ngpu, nullptr);
	std::vector<vg_index *> ix((size_t)o.ngpu, nullptr);
	std::unique_ptr<PipeIngest> pipe_in;
	std::vector<std::unique_ptr<PrePacker>> pre;
	if (in.once_only && !o.host_framing) pipe_in = start_pipe_ingest(o, in.fd, store, ix);
	else if (!in.bgzf_device && !in.gzip_device && !o.host_framing) pre = start_prepackers(o, in, store);
	// the SNP list is read now, beside the index open (the VCF pass at the end of the job starts from its bytes)
	std::string vcf_text;
	bool vcf_ok = false;
	std::thread vcf_reader([&] { vcf_ok = vgh::read_whole_file(vcf_in, vcf_text); });
	struct Joiner { std::thread &t; ~Joiner() { if (t.joinable()) t.join(); } } vcf_joiner{vcf_reader};
	if (!open_indexes(prefix, o, store, ix, pipe_in != nullptr)) return EXIT_FAILURE;
	for (auto *h : ix) VG_CHECK(vg_set_stats(h, o.stats));
	if (o.verbose) { fprintf(stderr, "index replica: %s\n", vg_index_plan(ix[0])); fprintf(stderr, "index start-up: %s\n", vg_index_open_report(ix[0])); }

	fprintf(stderr, "Processing...\n");
	clock_gettime(CLOCK_MONOTONIC, &t[1]);
	// ---- one ingest route (ranged_route has the long story), then the host reader for whatever the route left
	HostHandover hand;
	HostSpans mem;
	const HostSpans *reader_mem = nullptr;                              // what the host reader starts from (null: it opens the path)
	int reader_fd = in.fd;
	BgzfTakeover tk;
	if (pipe_in) { hand = once_only_route(o, *pipe_in, ix, store); mem.base = pipe_in->span_base; mem.spans = pipe_in->spans; reader_mem = &mem; }
	else if (in.bgzf_device) { hand = in.bam ? bam_device_route(o, in, ix[0], tk) : bgzf_device_route(o, in, ix[0], tk); reader_mem = &tk.mem; reader_fd = tk.rest->read_fd(); }
	else if (in.gzip_device) { hand = gzip_device_route(o, in, ix[0], tk); reader_mem = &tk.mem; reader_fd = tk.rest->read_fd(); }
	else if (!o.host_framing) {
		hand = ranged_route(o, in, ix, store, pre);
		pre.clear();
		close(in.fd);
	} else if (in.bz_pipe) reader_mem = &mem;                           // VARGENO_HOST_FASTQ=1 on a BGZF file: the host reader reads the inflated text from its start
	const uint64_t total = host_reader_tail(o, fastq, reader_fd, reader_mem, hand, o.host_framing, [&ix](int g, const vgh::ReadBatch &rb, uint64_t n) {
		VG_CHECK(vg_reads_submit(ix[(size_t)g], rb.bases.data(), rb.quals.data(), rb.offsets.data(), n));
	});
	// a bad block ends a BgzfTextPipe's text early: no VCF from half a file
	if (in.bz_pipe && !bgzf_pipe_verdict(o, *in.bz_pipe, "all replicas")) return EXIT_FAILURE;
	if (tk.rest && !bgzf_pipe_verdict(o, *tk.rest, "the host reader's tail", true)) return EXIT_FAILURE;
	for (auto *h : ix) VG_CHECK(vg_sync(h));
	clock_gettime(CLOCK_MONOTONIC, &t[2]);
	vgh::SiteCounts sc;
	vgh::SiteCalls calls;
	bool have_calls = false;
	if (!fetch_counts(o, ix, sc, calls, have_calls)) return EXIT_FAILURE;
	if (vcf_reader.joinable()) vcf_reader.join();
	vgh::write_genotyped_vcf(sc, chrlens, vcf_in, vcf_out, vcf_ok ? &vcf_text : nullptr, have_calls ? &calls : nullptr, o.vcf_out);
	clock_gettime(CLOCK_MONOTONIC, &t[3]);
	// The output is complete and closed.  What is left is giving back ~240 GB of device memory and the page-locked buffers, which the
	// operating system does for a process that ends anyway: an orderly vg_index_close + runtime shut-down took 0.7 + 0.9 s of an
	// 7 s job at hg38 scale (profiles/job_tail_r05.txt), so the command line ends here unless VARGENO_ORDERLY_EXIT=1 asks for the
	// full tear-down (tests that look for leaks, sanitizer runs).
	if (o.orderly_exit) { for (auto *h : ix) vg_index_close(h); for (auto *rs : store) vg_read_store_destroy(rs); }
	const double cpu = (double)(clock() - begin) / CLOCKS_PER_SEC;
	printf("Time: %f sec\n", cpu);                                       // qv.cc:1749-1751 prints CPU seconds
	if (o.verbose) verbose_report(total, o.ngpu, t);
	if (!o.orderly_exit) { fflush(stdout); fflush(stderr); _exit(EXIT_SUCCESS); }
	return EXIT_SUCCESS;
}

// ---- `vargeno cohort`: many samples against one resident index ----------------------------------------------------------------
// `geno` pays vg_index_open (seconds) per sample and holds the device alone while a decompressor feeds it at a few hundred MB/s.
// Here the index is opened once per replica and K samples are in flight together, each counting into a sample plane of its own
// (vg_samples_reserve / vg_sample_select): K worker threads take the manifest's entries in turn, every one through the once-only
// route (PipeIngest: the path is opened ONCE, whatever it is), attached at once -- nothing is packed ahead of the open, no ranges,
// no device framing.  A handle takes one caller at a time: select + submit happen under the replica's mutex.
struct CohortSample { std::string fastq, out; int line = 0; };

// The manifest: one "<reads.fq><TAB><out.vcf>" per line; blank lines and lines that start with '#' are skipped.  false: said on stderr
// joint: the second field is the sample's NAME, the header of its column (`out` holds it): unique, and without whitespace
static bool read_manifest(const std::string &path, std::vector<CohortSample> &samples, bool joint = false)
{
	std::string text;
	if (!vgh::read_whole_file(path, text)) { fprintf(stderr, "vargeno: cannot open the manifest %s\n", path.c_str()); return false; }
	int line = 0;
	for (size_t at = 0; at < text.size();) {
		size_t nl = text.find('\n', at);
		if (nl == std::string::npos) nl = text.size();
		std::string ln = text.substr(at, nl - at);
		at = nl + 1;
		line++;
		if (!ln.empty() && ln.back() == '\r') ln.pop_back();
		if (ln.empty() || ln[0] == '#') continue;
		const size_t tab = ln.find('\t');
		if (tab == std::string::npos || tab == 0 || tab + 1 >= ln.size()) { fprintf(stderr, "vargeno: %s line %d: expected <input FASTQ><TAB>%s\n", path.c_str(), line, joint ? "<sample name>" : "<output file in VCF>"); return false; }
		CohortSample s;
		s.fastq = ln.substr(0, tab); s.out = ln.substr(tab + 1); s.line = line;
		if (joint && std::any_of(s.out.begin(), s.out.end(), [](char c) { return isspace((unsigned char)c) != 0; })) { fprintf(stderr, "vargeno: %s line %d: the sample name \"%s\" contains whitespace\n", path.c_str(), line, s.out.c_str()); return false; }
		for (const CohortSample &before : samples)
			if (before.out == s.out) {
				if (joint) fprintf(stderr, "vargeno: %s line %d: sample name %s is already the name of line %d\n", path.c_str(), line, s.out.c_str(), before.line);
				else fprintf(stderr, "vargeno: %s line %d: output file %s is already the output of line %d\n", path.c_str(), line, s.out.c_str(), before.line);
				return false;
			}
		samples.push_back(s);
	}
	if (samples.empty()) { fprintf(stderr, "vargeno: the manifest %s names no sample\n", path.c_str()); return false; }
	return true;
}

// The pairwise sample table of VARGENO_JOINT_PAIRS and the hidden `pairstsv` command (format: the comment block at the top);
// counts = [N][N][5] as vg_gmatrix_pairs / vg_pairs_host fill it.
static void write_pairs_table(const std::string &path, const std::vector<std::string> &names, uint64_t n_sites, int min_gq, const std::vector<uint64_t> &counts)
{
	FILE *f = fopen(path.c_str(), "w");
	if (!f) throw vgh::Error{"cannot write " + path};
	const size_t N = names.size();
	auto at = [&](size_t i, size_t j, int k) { return counts[(i * N + j) * 5 + (size_t)k]; };
	auto ratio = [&](double num, uint64_t den) { if (den == 0) fputs("\tnan", f); else fprintf(f, "\t%.6f", num / (double)den); };
	fprintf(f, "##sites=%lu\n##min_gq=%d\n", (unsigned long)n_sites, min_gq);
	for (size_t i = 0; i < N; i++) fprintf(f, "##sample=%s\tcalled=%lu\thet=%lu\n", names[i].c_str(), (unsigned long)at(i, i, 0), (unsigned long)at(i, i, 3));
	fputs("#sample_a\tsample_b\tn\tibs0\tibs2\thethet\thet_a\thet_b\tconcordance\trelatedness\n", f);
	for (size_t i = 0; i < N; i++)
		for (size_t j = i + 1; j < N; j++) {
			const uint64_t n = at(i, j, 0), ibs0 = at(i, j, 1), ibs2 = at(i, j, 2), hethet = at(i, j, 3), het_a = at(i, j, 4), het_b = at(j, i, 4);
			fprintf(f, "%s\t%s\t%lu\t%lu\t%lu\t%lu\t%lu\t%lu", names[i].c_str(), names[j].c_str(), (unsigned long)n, (unsigned long)ibs0, (unsigned long)ibs2, (unsigned long)hethet, (unsigned long)het_a, (unsigned long)het_b);
			ratio((double)ibs2, n);
			ratio((double)((int64_t)hethet - 2 * (int64_t)ibs0), std::min(het_a, het_b));
			fputc('\n', f);
		}
	const bool bad = ferror(f) != 0;
	if (fclose(f) != 0 || bad) throw vgh::Error{"cannot write " + path};
}

// joint: the samples' columns into a genotype matrix on `device`, the table counted there; VG_ENOMEM from the matrix: the host loop
static void joint_pairs_table(const GenoOptions &o, int device, const std::vector<vgh::JointSample> &columns, uint64_t n_sites)
{
	const size_t N = columns.size();
	std::vector<uint64_t> counts(N * N * 5);
	vg_gmatrix *gm = nullptr;
	int rc = vg_gmatrix_create(device, n_sites, (uint32_t)N, &gm);
	for (size_t i = 0; rc == VG_OK && i < N; i++) rc = vg_gmatrix_set(gm, (uint32_t)i, columns[i].calls.gt.data(), columns[i].calls.gq.data(), o.pairs_min_gq);
	if (rc == VG_OK) rc = vg_gmatrix_pairs(gm, 0, counts.data());
	vg_gmatrix_destroy(gm);
	if (rc == VG_ENOMEM) {
		if (o.verbose) fprintf(stderr, "pairs: no device memory for the genotype matrix (%s): the host loop on %d threads\n", vg_last_error(), o.pairs_threads);
		std::vector<uint8_t> gt(N * n_sites);
		std::vector<int32_t> gq(N * n_sites);
		for (size_t i = 0; i < N; i++) { std::copy(columns[i].calls.gt.begin(), columns[i].calls.gt.end(), gt.begin() + i * n_sites); std::copy(columns[i].calls.gq.begin(), columns[i].calls.gq.end(), gq.begin() + i * n_sites); }
		rc = vg_pairs_host(gt.data(), gq.data(), n_sites, (uint32_t)N, o.pairs_min_gq, o.pairs_threads, counts.data());
	}
	if (rc != VG_OK) throw vgh::Error{std::string("the pair table failed: ") + vg_last_error()};
	std::vector<std::string> names;
	for (const auto &c : columns) names.push_back(c.name);
	write_pairs_table(o.joint_pairs, names, n_sites, o.pairs_min_gq, counts);
}

// VARGENO_JOINT_PRIOR=cohort: the samples' columns called again from their counters (kept[s]: ref_cnt and alt_cnt of sample s) with
// the cohort's own allele frequencies -- through a vg_cprior on `device`, or by the header's host loop: where `on_device` is false
// (VARGENO_JOINT_PRIOR_ROUTE=host, jointvcf) and where the device has no memory for the matrix (VG_ENOMEM).  The columns are the same.
static void joint_prior_recall(const JointPrior &jp, bool on_device, int device, int threads, bool verbose, const std::vector<uint8_t> &ref_freq, const std::vector<uint8_t> &alt_freq,
                               const std::vector<vgh::SiteCounts> &kept, std::vector<vgh::JointSample> &columns)
{
	const size_t N = columns.size(), n = ref_freq.size();
	for (size_t i = 0; i < N; i++) {
		if (kept[i].ref_cnt.size() != n || kept[i].alt_cnt.size() != n) throw vgh::Error{"sample " + columns[i].name + " has counters for another number of sites than the index has"};
		columns[i].calls.gt.resize(n); columns[i].calls.gq.resize(n);
	}
	int rc = VG_ENOMEM;
	if (on_device) {
		vg_cprior *cp = nullptr;
		uint64_t escaped = 0;
		rc = vg_cprior_create(device, n, (uint32_t)std::min<size_t>(N, UINT32_MAX), &cp);
		for (size_t i = 0; rc == VG_OK && i < N; i++) rc = vg_cprior_set(cp, (uint32_t)i, kept[i].ref_cnt.data(), kept[i].alt_cnt.data());
		if (rc == VG_OK) rc = vg_cprior_run(cp, ref_freq.data(), alt_freq.data(), jp.iters, jp.pseudo, 0, nullptr, &escaped);
		for (size_t i = 0; rc == VG_OK && i < N; i++) rc = vg_cprior_calls(cp, (uint32_t)i, columns[i].calls.gt.data(), columns[i].calls.gq.data());
		vg_cprior_destroy(cp);
		if (rc == VG_OK && verbose) fprintf(stderr, "cohort prior: device, %lu sites, %lu samples, %lu entries recomputed on the host\n", (unsigned long)n, (unsigned long)N, (unsigned long)escaped);
		if (rc == VG_ENOMEM && verbose) fprintf(stderr, "cohort prior: no device memory for the cohort's counters (%s): the host loop\n", vg_last_error());
	}
	if (rc == VG_ENOMEM) {
		std::vector<uint8_t> r(N * n), a(N * n), gt(N * n);
		std::vector<int32_t> gq(N * n);
		for (size_t i = 0; i < N; i++) { std::copy(kept[i].ref_cnt.begin(), kept[i].ref_cnt.end(), r.begin() + i * n); std::copy(kept[i].alt_cnt.begin(), kept[i].alt_cnt.end(), a.begin() + i * n); }
		rc = vg_cprior_host(r.data(), a.data(), n, (uint32_t)std::min<size_t>(N, UINT32_MAX), ref_freq.data(), alt_freq.data(), jp.iters, jp.pseudo, threads, gt.data(), gq.data(), nullptr);
		for (size_t i = 0; rc == VG_OK && i < N; i++) { std::copy(gt.begin() + i * n, gt.begin() + (i + 1) * n, columns[i].calls.gt.begin()); std::copy(gq.begin() + i * n, gq.begin() + (i + 1) * n, columns[i].calls.gq.begin()); }
		if (rc == VG_OK && verbose) fprintf(stderr, "cohort prior: host (%d threads), %lu sites, %lu samples, 0 entries recomputed on the host\n", threads, (unsigned long)n, (unsigned long)N);
	}
	if (rc != VG_OK) throw vgh::Error{std::string("the cohort prior failed: ") + vg_last_error()};
}

// joint_out: `vargeno joint` -- the same workers, but a finished sample's calls are kept as a column (from the caller kernel; the
// host loop when the device has no memory for it) and ONE file is written after the last sample, if every sample succeeded.
static int run_cohort(const std::string &prefix, const std::string &manifest, const std::string &vcf_in, const std::string *joint_out = nullptr)
{
	struct timespec t0; clock_gettime(CLOCK_MONOTONIC, &t0);
	const bool joint = joint_out != nullptr;
	std::vector<CohortSample> samples;
	if (!read_manifest(manifest, samples, joint)) return EXIT_FAILURE;      // (before any device is touched)
	std::vector<vgh::ChrLen> chrlens = vgh::read_chrlens(prefix + ".chrlens");
	const int have = vg_device_count();
	if (have <= 0) { fprintf(stderr, "vargeno: no HIP device found (this build has no CPU path)\n"); return EXIT_FAILURE; }
	const GenoOptions o(have);
	const int K = (int)std::min<size_t>(samples.size(), (size_t)o.cohort_inflight);

	fprintf(stderr, "Initializing...\n");
	std::string vcf_text;
	bool vcf_ok = false;
	std::thread vcf_reader([&] { vcf_ok = vgh::read_whole_file(vcf_in, vcf_text); });
	struct Joiner { std::thread &t; ~Joiner() { if (t.joinable()) t.join(); } } vcf_joiner{vcf_reader};
	const std::vector<vg_read_store *> no_store((size_t)o.ngpu, nullptr);
	std::vector<vg_index *> ix((size_t)o.ngpu, nullptr);
	if (!open_indexes(prefix, o, no_store, ix, false)) return EXIT_FAILURE;
	for (auto *h : ix) { VG_CHECK(vg_set_stats(h, o.stats)); VG_CHECK(vg_samples_reserve(h, (uint32_t)K)); }
	if (o.verbose) { fprintf(stderr, "index replica: %s\n", vg_index_plan(ix[0])); fprintf(stderr, "index start-up: %s\n", vg_index_open_report(ix[0])); }
	vcf_reader.join();
	if (!vcf_ok) { fprintf(stderr, "Error opening: %s . You have failed.\n", vcf_in.c_str()); return EXIT_FAILURE; }
	vgh::SiteCounts sites;
	fetch_sites(ix[0], sites);
	struct timespec t1; clock_gettime(CLOCK_MONOTONIC, &t1);

	fprintf(stderr, "Processing...\n");
	std::vector<std::mutex> mu((size_t)o.ngpu);                       // one caller at a time per handle
	std::atomic<size_t> next{0};
	std::atomic<int> failed{0};
	std::vector<vgh::JointSample> columns(joint ? samples.size() : 0);      // joint: the samples' calls, in manifest order
	const bool prior = joint && o.joint_prior.cohort;                 // VARGENO_JOINT_PRIOR=cohort: ... and their counters, for the re-call after the last one
	std::vector<vgh::SiteCounts> kept(prior ? samples.size() : 0);
	const char *const nothing = joint ? "no joint file written" : "no VCF written";
	// what happens to a finished sample: its own VCF, or its column of the joint file.  false: said on stderr
	auto deliver = [&](size_t at, vgh::SiteCounts &sc, vgh::SiteCalls &calls, bool have_calls) -> bool {
		const CohortSample &s = samples[at];
		if (joint) {
			if (!have_calls) { sc.pos = sites.pos; sc.ref_freq = sites.ref_freq; sc.alt_freq = sites.alt_freq; vgh::call_sites(sc, calls); }
			columns[at].name = s.out;
			columns[at].calls = std::move(calls);
			if (prior) { kept[at].ref_cnt = std::move(sc.ref_cnt); kept[at].alt_cnt = std::move(sc.alt_cnt); }
			return true;
		}
		sc.pos = sites.pos; sc.ref_freq = sites.ref_freq; sc.alt_freq = sites.alt_freq;
		try { vgh::write_genotyped_vcf(sc, chrlens, vcf_in, s.out, &vcf_text, have_calls ? &calls : nullptr, o.vcf_out); }
		catch (const vgh::Error &e) { fprintf(stderr, "vargeno: %s line %d: %s\n", manifest.c_str(), s.line, e.msg.c_str()); return false; }
		return true;
	};
	auto worker = [&](uint32_t plane) {
		for (;;) {
			const size_t at = next.fetch_add(1);
			if (at >= samples.size()) return;
			if (joint && failed.load()) return;                           // (no joint file any more: the samples left are not read)
			const CohortSample &s = samples[at];
			struct timespec a; clock_gettime(CLOCK_MONOTONIC, &a);
			if (plain_gzip(s.fastq)) { failed.store(1); continue; }
			const int file_fd = open(s.fastq.c_str(), O_RDONLY);
			if (file_fd < 0) { fprintf(stderr, "vargeno: %s line %d: cannot open %s\n", manifest.c_str(), s.line, s.fastq.c_str()); failed.store(1); continue; }
			// a BGZF sample is inflated by host threads into a pipe: the once-only route below takes the pipe's descriptor in place of the file's
			// (a BAM sample likewise, its records converted to text on the way)
			std::unique_ptr<vgh::TextPipe> bz;
			struct stat sb;
			const vgh::FastqKind kind = fstat(file_fd, &sb) == 0 && S_ISREG(sb.st_mode) ? vgh::sniff_fastq(file_fd) : vgh::FastqKind::Text;
			if (kind == vgh::FastqKind::Bgzf) bz.reset(new vgh::BgzfTextPipe(file_fd, 0, 0, std::max(1, o.bgzf_threads / K)));
			else if (kind == vgh::FastqKind::Bam) bz.reset(new vgh::BamTextPipe(file_fd, 0, 0, std::max(1, o.bgzf_threads / K), true, 0));
			else if (kind == vgh::FastqKind::PlainGzip && o.gzip_host) bz.reset(new vgh::GzipTextPipe(file_fd));
			const int fd = bz ? bz->read_fd() : file_fd;
			(void)fcntl(fd, F_SETPIPE_SZ, 1 << 20);
			uint64_t total = 0;
			bool bz_ok = true;
			{
				PipeIngest pin(fd, o.pipe_chunk(), std::max(1, o.pack_threads / K), o.pipe_copiers, no_store,
				               [&](size_t g, const uint64_t *k, const uint64_t *m, const uint64_t *off, uint64_t n) -> std::string {
					               std::lock_guard<std::mutex> lock(mu[g]);
					               if (vg_sample_select(ix[g], plane) != VG_OK) return std::string("vg_sample_select failed: ") + vg_last_error();
					               return vg_reads_submit_packed(ix[g], k, m, off, n) == VG_OK ? std::string() : std::string("vg_reads_submit_packed failed: ") + vg_last_error();
				               });
				pin.attach();
				pin.finish();
				if (!pin.error.empty()) { fprintf(stderr, "vargeno: %s line %d: %s\n", manifest.c_str(), s.line, pin.error.c_str()); exit(EXIT_FAILURE); }
				// what the packer refused, and the possibly truncated tail: the host reader, into the same plane
				const HostHandover hand{pin.records, pin.consumed, pin.records ? pin.last : UINT64_MAX, 0};
				const HostSpans mem{pin.span_base, pin.spans};
				total = host_reader_tail(o, s.fastq, fd, &mem, hand, false, [&](int g, const vgh::ReadBatch &rb, uint64_t n) {
					std::lock_guard<std::mutex> lock(mu[(size_t)g]);
					VG_CHECK(vg_sample_select(ix[(size_t)g], plane));
					VG_CHECK(vg_reads_submit(ix[(size_t)g], rb.bases.data(), rb.quals.data(), rb.offsets.data(), n));
				});
				if (bz) { bz->finish(); if (!bz->error.empty()) { fprintf(stderr, "vargeno: %s line %d: %s: %s\n", manifest.c_str(), s.line, bz->error.c_str(), nothing); bz_ok = false; } }
			}
			bz.reset();
			close(file_fd);
			// the sample is complete: its plane summed over the replicas, fetched and zeroed for the worker's next sample
			vgh::SiteCounts sc;
			vgh::SiteCalls calls;
			bool have_calls = false;
			uint64_t invalid = 0;
			{
				for (auto &m : mu) m.lock();
				for (auto *h : ix) VG_CHECK(vg_sample_select(h, plane));
				for (auto *h : ix) { uint64_t bad = 0; VG_CHECK(vg_sample_invalid_reads(h, plane, &bad)); invalid += bad; }
				if (!invalid && bz_ok) {
					reduce_selected_counts(o, ix);
					have_calls = (joint || o.caller_device) && fetch_reduced_calls(o, ix[0], calls);
					if (!have_calls || prior) fetch_reduced_counts(ix[0], sc);
				}
				for (auto *h : ix) VG_CHECK(vg_sample_reset(h, plane));
				for (auto &m : mu) m.unlock();
			}
			if (!bz_ok) { failed.store(1); continue; }
			if (invalid) {
				// util.c:103: the reference aborts on such a read and writes no VCF; the other samples go on
				fprintf(stderr, "vargeno: %s line %d: %lu reads of %s contain a character other than ACGTN (the reference aborts on these): %s\n", manifest.c_str(), s.line, (unsigned long)invalid, s.fastq.c_str(), nothing);
				failed.store(1);
				continue;
			}
			if (!deliver(at, sc, calls, have_calls)) { failed.store(1); continue; }
			if (o.verbose) { struct timespec b; clock_gettime(CLOCK_MONOTONIC, &b); fprintf(stderr, "sample, line %d: reads: %lu  plane: %u  open -> %s: %.3f s\n", s.line, (unsigned long)total, plane, joint ? "calls" : "VCF", secs(a, b)); }
		}
	};
	std::vector<std::thread> th;
	for (int w = 0; w < K; w++) th.emplace_back(worker, (uint32_t)w);
	for (auto &t : th) t.join();
	if (joint && !failed.load()) {
		try {
			if (prior) joint_prior_recall(o.joint_prior, o.joint_prior.device, 0, o.pairs_threads, o.verbose, sites.ref_freq, sites.alt_freq, kept, columns);      // (replica 0 sits on device 0)
			vgh::write_joint_vcf(sites.pos, chrlens, columns, vcf_in, *joint_out, &vcf_text, o.vcf_out, o.joint_text);
			if (!o.joint_pairs.empty()) joint_pairs_table(o, 0, columns, sites.pos.size());      // (replica 0 sits on device 0)
		}
		catch (const vgh::Error &e) { fprintf(stderr, "vargeno: %s\n", e.msg.c_str()); failed.store(1); }
	}
	struct timespec t2; clock_gettime(CLOCK_MONOTONIC, &t2);
	if (o.verbose) fprintf(stderr, "cohort: samples: %lu  in flight: %d  gpus: %d  index load %.3f s  wall: %.3f s\n", (unsigned long)samples.size(), K, o.ngpu, secs(t0, t1), secs(t0, t2));
	const int status = failed.load() ? EXIT_FAILURE : EXIT_SUCCESS;
	if (o.orderly_exit) { for (auto *h : ix) vg_index_close(h); return status; }
	fflush(stdout); fflush(stderr);
	_exit(status);                                                    // (as `geno`: the outputs are closed, the operating system takes the memory back)
}

// a counts table of the hidden `callvcf` / `jointvcf` commands: "pos ref_freq alt_freq ref_cnt alt_cnt" per line
static void read_counts_table(const std::string &path, vgh::SiteCounts &sc)
{
	FILE *f = fopen(path.c_str(), "r");
	if (!f) throw vgh::Error{"cannot open " + path};
	unsigned long p; unsigned rf, af, rc, ac;
	while (fscanf(f, "%lu %u %u %u %u", &p, &rf, &af, &rc, &ac) == 5) {
		sc.pos.push_back((uint32_t)p); sc.ref_freq.push_back((uint8_t)rf); sc.alt_freq.push_back((uint8_t)af);
		sc.ref_cnt.push_back((uint8_t)rc); sc.alt_cnt.push_back((uint8_t)ac);
	}
	fclose(f);
}

int main(int argc, const char *argv[])
{
	if (argc < 2) { print_help(); return 0; }
	const std::string opt = argv[1];
	try {
		vgh::VcfBgzf vcf_bgzf;
		int vcf_codes = VG_DEFLATE_FIXED;
		bool vcf_index = false;
		if ((opt == "geno" || opt == "cohort" || opt == "joint" || opt == "jointvcf" || opt == "bgzfzip") &&(!vcf_bgzf_route(&vcf_bgzf) || !vcf_bgzf_codes(&vcf_codes) || !vcf_index_switch(&vcf_index, vcf_bgzf))) return EXIT_FAILURE;      // (before anything else is looked at)
		// a VCF that could not be indexed (said on stderr where it was found) is complete, and the command fails like `vargeno ... && tabix` would
		auto with_index = [](int rc) { return rc == EXIT_SUCCESS && vgh::vcf_index_refusals() ? EXIT_FAILURE : rc; };
		vgh::JointTextRoute joint_text;
		if ((opt == "joint" || opt == "jointvcf") && (!joint_text_route(&joint_text) || !joint_info_switch(&joint_text.info_counts))) return EXIT_FAILURE;
		JointPrior joint_prior;
		if ((opt == "joint" || opt == "jointvcf") && !joint_prior_switch(&joint_prior)) return EXIT_FAILURE;
		joint_text.prior_line = joint_prior.header_line();
		// a SNP list that declares a key VARGENO_JOINT_INFO adds: refused here, before an index, a device or the output is looked at
		if (joint_text.info_counts && ((opt == "joint" && argc == 6) || (opt == "jointvcf" && argc >= 6))) {
			const std::string tag = vgh::joint_info_declared(argv[opt == "joint" ? 4 : 3]);
			if (!tag.empty()) {
				fprintf(stderr, "vargeno: %s already declares the INFO key %s, which VARGENO_JOINT_INFO=counts would declare and write again: unset the variable or take the key out of the list\n", argv[opt == "joint" ? 4 : 3], tag.c_str());
				return EXIT_FAILURE;
			}
		}
		if (opt == "index") {
			arg_check(argc, 3);
			vgh::IndexOptions io;
			io.write_lite = !env_int("VARGENO_NO_LITE", 0);
			io.threads = env_int("VARGENO_THREADS", 0);
			vgh::build_index(argv[2], argv[3], argv[4], io);
			return EXIT_SUCCESS;
		} else if (opt == "geno") {
			arg_check(argc, 4);
			return with_index(run_geno(argv[2], argv[3], argv[4], argv[5]));
		} else if (opt == "cohort") {
			arg_check(argc, 3);
			return with_index(run_cohort(argv[2], argv[3], argv[4]));
		} else if (opt == "joint") {
			arg_check(argc, 4);
			const std::string out = argv[5];
			return with_index(run_cohort(argv[2], argv[3], argv[4], &out));
		} else if (opt == "bgzfcat") {
			// hidden: a BGZF file's text on stdout, inflated by the host threads of the BgzfTextPipe (no device needed; tests/test_bgzf_cpu.py)
			arg_check(argc, 1);
			if (plain_gzip(argv[2])) return EXIT_FAILURE;
			const int fd = open(argv[2], O_RDONLY);
			if (fd < 0) throw vgh::Error{std::string("cannot open ") + argv[2]};
			vgh::BgzfTextPipe bp(fd, 0, 0, std::max(1, std::min(env_int("VARGENO_BGZF_THREADS", vgh::bgzf_threads_default(usable_cpus())), 256)));
			if (bp.read_fd() < 0) throw vgh::Error{bp.error};
			std::vector<uint8_t> buf(1 << 20);
			for (;;) {
				const ssize_t n = read(bp.read_fd(), buf.data(), buf.size());
				if (n < 0 && errno == EINTR) continue;
				if (n <= 0) break;
				if (fwrite(buf.data(), 1, (size_t)n, stdout) != (size_t)n) throw vgh::Error{"cannot write to stdout"};
			}
			bp.finish();
			if (!bp.error.empty()) throw vgh::Error{bp.error};
			return EXIT_SUCCESS;
		} else if (opt == "bgzfzip") {
			// hidden: a file written as BGZF through the sink that `geno`, `cohort` and `joint` write their VCF through (the host route
			// needs no device; tests/test_deflate_cpu.py)
			if (argc != 4 && argc != 5) { print_help(); return EXIT_FAILURE; }
			vgh::VcfOutput how;
			how.bgzf = vcf_bgzf == vgh::VcfBgzf::Device ? vgh::VcfBgzf::Device : vgh::VcfBgzf::Host;
			how.codes = vcf_codes;
			how.index = vcf_index;
			how.threads = std::max(1, std::min(env_int("VARGENO_BGZF_THREADS", vgh::bgzf_threads_default(usable_cpus())), 256));
			how.verbose = env_int("VARGENO_VERBOSE", 0) != 0;
			const long block = argc == 5 ? atol(argv[4]) : 0;
			if (block < 0 || block > 65280) throw vgh::Error{"bgzfzip: a block holds 1 to 65280 bytes of text (0: 65280)"};
			how.block = (uint32_t)block;
			if (how.bgzf == vgh::VcfBgzf::Device && vg_device_count() <= 0) { fprintf(stderr, "vargeno: no HIP device found (VARGENO_VCF_BGZF=host compresses on the host)\n"); return EXIT_FAILURE; }
			const int fd = open(argv[2], O_RDONLY);
			if (fd < 0) throw vgh::Error{std::string("cannot open ") + argv[2]};
			struct timespec a, b; clock_gettime(CLOCK_MONOTONIC, &a);
			const std::unique_ptr<vgh::VcfSink> sink = vgh::open_vcf_sink(argv[3], how);
			std::vector<char> buf(8 << 20);
			uint64_t total = 0;
			for (;;) {                                                    // 8 MiB of the file per step
				const ssize_t n = read(fd, buf.data(), buf.size());
				if (n < 0 && errno == EINTR) continue;
				if (n < 0) throw vgh::Error{std::string("error reading ") + argv[2]};
				if (n == 0) break;
				sink->write(buf.data(), (size_t)n);
				total += (uint64_t)n;
			}
			close(fd);
			sink->close();
			clock_gettime(CLOCK_MONOTONIC, &b);
			if (how.verbose) fprintf(stderr, "bgzfzip: %s route, %s codes, %.3f GB of text in %.3f s (%.2f GB/s)\n", how.bgzf == vgh::VcfBgzf::Device ? "device" : "host", how.codes == VG_DEFLATE_DYNAMIC ? "dynamic" : "fixed", (double)total / 1e9, secs(a, b), (double)total / 1e9 / std::max(1e-9, secs(a, b)));
			return with_index(EXIT_SUCCESS);
		} else if (opt == "gzcat") {
			// hidden: a plain gzip file's text on stdout, by the host build of the decoder alone (no device needed; tests/test_gzip_cpu.py)
			arg_check(argc, 1);
			const int fd = open(argv[2], O_RDONLY);
			if (fd < 0) throw vgh::Error{std::string("cannot open ") + argv[2]};
			std::string err;
			if (!vgh::gzip_cat(fd, stdout, err)) throw vgh::Error{std::string(argv[2]) + ": " + err};
			return EXIT_SUCCESS;
		} else if (opt == "bamcat") {
			// hidden: a BAM file's equivalent FASTQ text on stdout, by the host threads of the BamTextPipe (no device needed; tests/test_bam_cpu.py)
			arg_check(argc, 1);
			if (plain_gzip(argv[2])) return EXIT_FAILURE;
			const int fd = open(argv[2], O_RDONLY);
			if (fd < 0) throw vgh::Error{std::string("cannot open ") + argv[2]};
			if (vgh::sniff_fastq(fd) != vgh::FastqKind::Bam) {
				uint64_t end = 0; int32_t n_ref = 0; std::string why;
				(void)vgh::bam_header_info(fd, &end, &n_ref, why);            // (says what is wrong: not BGZF, not BAM, a header cut short)
				throw vgh::Error{std::string(argv[2]) + ": " + (why.empty() ? "not a BAM file" : why)};
			}
			vgh::BamTextPipe bp(fd, 0, 0, std::max(1, std::min(env_int("VARGENO_BGZF_THREADS", vgh::bgzf_threads_default(usable_cpus())), 256)), true, 0);
			if (bp.read_fd() < 0) throw vgh::Error{bp.error};
			std::vector<uint8_t> buf(1 << 20);
			for (;;) {
				const ssize_t n = read(bp.read_fd(), buf.data(), buf.size());
				if (n < 0 && errno == EINTR) continue;
				if (n <= 0) break;
				if (fwrite(buf.data(), 1, (size_t)n, stdout) != (size_t)n) throw vgh::Error{"cannot write to stdout"};
			}
			bp.finish();
			if (!bp.error.empty()) throw vgh::Error{bp.error};
			return EXIT_SUCCESS;
		} else if (opt == "fqcheck") {
			// hidden: the host FASTQ framing alone -- one line per record: read length, then the read and the quality
			// characters the path can see (no device needed; tests/test_host_tools.py)
			arg_check(argc, 1);
			vgh::FastqReader rd(argv[2]);
			vgh::ReadBatch rb;
			for (;;) {
				rb.clear();
				if (!rd.next(rb, 1000)) break;
				for (uint64_t i = 0; i < rb.n(); i++) {
					const uint64_t o = rb.offsets[i], len = rb.offsets[i + 1] - o;
					printf("%lu ", (unsigned long)len);
					fwrite(rb.bases.data() + o, 1, len, stdout);
					printf(" ");
					for (uint64_t j = 0; j < len / 32; j++) printf("%02x", rb.quals[o + j]);
					printf("\n");
				}
			}
			return EXIT_SUCCESS;
		} else if (opt == "fqpipe") {
			// hidden: the once-only FASTQ route of `geno` (PipeIngest + the host reader behind it) without a device -- <path> is
			// opened ONCE, whatever it is (a FIFO, /dev/stdin, a regular file).  One line per record in the form both halves can
			// produce: "<chunks> <trimmed read, upper case> <gate bits, hex>", "N" / "X" for a read the reference skips / aborts on
			// (tests/test_host_tools.py compares with `fqcheck` on the same bytes).  [chunk bytes] [threads]
			if (argc < 3 || argc > 5) { print_help(); return EXIT_FAILURE; }
			const int fd = open(argv[2], O_RDONLY);
			if (fd < 0) throw vgh::Error{std::string("cannot open ") + argv[2]};
			const uint64_t chunk = argc > 3 ? (uint64_t)atoll(argv[3]) : (1ull << 20);
			std::vector<std::string> lines;
			const GenoOptions o(0);
			const bool quiet = o.fqpipe_quiet;                                   // (a rate probe of the route: count, print nothing)
			uint64_t counted = 0;
			auto one = [&](uint64_t nch, const uint64_t *km, uint64_t meta) {
				if (quiet) { counted += 1 + (nch & 0); return; }
				if (meta >> 63) { lines.push_back("X"); return; }
				if ((meta >> 62) & 1u) { lines.push_back("N"); return; }
				std::string l = std::to_string(nch) + " ";
				for (uint64_t c = 0; c < nch; c++) for (int b = 0; b < 32; b++) l.push_back("ACGT"[(km[c] >> (2 * b)) & 3u]);
				char hx[32]; snprintf(hx, sizeof hx, " %x", (unsigned)(meta & 0xFFFFFFFFu));
				lines.push_back(l + hx);
			};
			std::vector<vg_read_store *> none(1, nullptr);
			PipeIngest pin(fd, chunk, argc > 4 ? atoi(argv[4]) : 2, o.pipe_copiers, none, [&](size_t, const uint64_t *k, const uint64_t *m, const uint64_t *o, uint64_t n) -> std::string {
				for (uint64_t r = 0; r < n; r++) one(o[r + 1] - o[r], k + o[r], m[r]);
				return std::string();
			});
			pin.attach();
			pin.finish();
			if (!pin.error.empty()) throw vgh::Error{pin.error};
			fprintf(stderr, "fqpipe: %lu records framed by the packer, %lu bytes consumed of %lu read, refused %d\n", (unsigned long)pin.records, (unsigned long)pin.consumed, (unsigned long)pin.bytes_read, pin.refused ? 1 : 0);
			if (quiet) fprintf(stderr, "fqpipe: %lu reads through the sink, %d copier threads, %.3f s, %.3f GB/s of text\n", (unsigned long)counted, pin.copiers, pin.seconds, pin.seconds > 0 ? (double)pin.bytes_read / pin.seconds / 1e9 : 0.0);
			vgh::FastqReader rd(fd, pin.span_base, pin.spans);
			vgh::ReadBatch rb;
			if (pin.records) { rd.seek(pin.last); rb.clear(); (void)rd.next(rb, 1); }
			rd.seek(pin.consumed);
			for (;;) {
				rb.clear();
				if (!rd.next(rb, 1000)) break;
				for (uint64_t i = 0; i < rb.n(); i++) {
					const uint64_t o = rb.offsets[i], nch = (rb.offsets[i + 1] - o) / 32;
					std::vector<uint64_t> km((size_t)nch, 0);
					uint64_t meta = 0;
					for (uint64_t c = 0; c < nch && !(meta >> 62); c++)
						for (int b = 31; b >= 0; b--) {                       // (the reference's scan order: the first offending character decides, qv.cc:815-828)
							const char ch = (char)(rb.bases[o + 32 * c + (uint64_t)b] & 0xDF);
							const int code = ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : ch == 'T' ? 3 : -1;
							if (code < 0) { meta |= ch == 'N' ? 1ull << 62 : 1ull << 63; break; }
							km[(size_t)c] |= (uint64_t)code << (2 * b);
						}
					for (uint64_t c = 0; c < nch && c < 32; c++) if ((int)(int8_t)rb.quals[o + c] - '8' < 0) meta |= 1ull << c;
					one(nch, km.data(), meta);
				}
			}
			for (const auto &l : lines) puts(l.c_str());
			return EXIT_SUCCESS;
		} else if (opt == "fqcuts") {
			// hidden: where `geno` with n replicas would cut the FASTQ file (no device needed; tests/test_host_tools.py)
			arg_check(argc, 2);
			const int fd = open(argv[2], O_RDONLY);
			struct stat sb;
			if (fd < 0 || fstat(fd, &sb) != 0) throw vgh::Error{std::string("cannot open ") + argv[2]};
			std::vector<uint64_t> cut;
			const bool ok = range_cuts(fd, (uint64_t)sb.st_size, std::max(1, atoi(argv[3])), cut);
			close(fd);
			if (!ok) { printf("none\n"); return EXIT_SUCCESS; }
			for (uint64_t c : cut) printf("%lu\n", (unsigned long)c);
			return EXIT_SUCCESS;
		} else if (opt == "callvcf") {
			// hidden (like the reference's vcfd/ucscd/filt): caller + VCF writer alone, from a counts table
			// "pos ref_freq alt_freq ref_cnt alt_cnt" per line: <chrlens> <counts.txt> <snps.vcf> <out.vcf>
			arg_check(argc, 4);
			vgh::SiteCounts sc;
			read_counts_table(argv[3], sc);
			vgh::write_genotyped_vcf(sc, vgh::read_chrlens(argv[2]), argv[4], argv[5]);
			return EXIT_SUCCESS;
		} else if (opt == "jointvcf") {
			// hidden: the joint writer alone, with the host caller, from one counts table per sample (callvcf's format; all list the same
			// sites): <chrlens> <snps.vcf> <out.vcf> <name>=<counts.txt> ...  (no device needed; tests/test_joint_vcf_cpu.py)
			if (argc < 6) { print_help(); return EXIT_FAILURE; }
			std::vector<vgh::JointSample> columns;
			std::vector<vgh::SiteCounts> kept;                            // VARGENO_JOINT_PRIOR=cohort: the samples' counters, and the sites' frequencies as the first table has them
			std::vector<uint8_t> ref_freq, alt_freq;
			std::vector<uint32_t> pos;
			for (int a = 5; a < argc; a++) {
				const std::string arg = argv[a];
				const size_t eq = arg.find('=');
				if (eq == std::string::npos || eq == 0 || eq + 1 >= arg.size()) { print_help(); return EXIT_FAILURE; }
				vgh::SiteCounts sc;
				read_counts_table(arg.substr(eq + 1), sc);
				if (a == 5) { pos = sc.pos; ref_freq = sc.ref_freq; alt_freq = sc.alt_freq; }
				else if (sc.pos != pos) throw vgh::Error{arg.substr(eq + 1) + " lists other sites than " + std::string(argv[5]).substr(std::string(argv[5]).find('=') + 1)};
				vgh::JointSample js;
				js.name = arg.substr(0, eq);
				vgh::call_sites(sc, js.calls);
				columns.push_back(std::move(js));
				if (joint_prior.cohort) { kept.emplace_back(); kept.back().ref_cnt = std::move(sc.ref_cnt); kept.back().alt_cnt = std::move(sc.alt_cnt); }
			}
			// the output options of `joint`: VARGENO_VCF_BGZF / VARGENO_VCF_CODES (unset: plain text, as ever) and VARGENO_JOINT_TEXT
			vgh::VcfOutput how;
			how.bgzf = vcf_bgzf;
			how.codes = vcf_codes;
			how.index = vcf_index;
			how.threads = std::max(1, std::min(env_int("VARGENO_BGZF_THREADS", vgh::bgzf_threads_default(usable_cpus())), 256));
			how.verbose = env_int("VARGENO_VERBOSE", 0) != 0;
			if (how.bgzf == vgh::VcfBgzf::Device && vg_device_count() <= 0) { fprintf(stderr, "vargeno: no HIP device found (VARGENO_VCF_BGZF=host compresses on the host)\n"); return EXIT_FAILURE; }
			if (joint_prior.cohort) joint_prior_recall(joint_prior, false, 0, std::max(1, env_int("VARGENO_THREADS", usable_cpus())), how.verbose, ref_freq, alt_freq, kept, columns);
			vgh::write_joint_vcf(pos, vgh::read_chrlens(argv[2]), columns, argv[3], argv[4], nullptr, how, joint_text);
			return with_index(EXIT_SUCCESS);
		} else if (opt == "pairstsv") {
			// hidden: the pair table alone, by the host loop, from one calls file per sample ("gt gq" per line; all of one length):
			// <out.tsv> <min_gq> <name>=<calls.txt> ...  (no device needed; tests/test_pairs_cpu.py)
			if (argc < 5) { print_help(); return EXIT_FAILURE; }
			const int min_gq = atoi(argv[3]);
			std::vector<std::string> names;
			std::vector<uint8_t> gt;
			std::vector<int32_t> gq;
			uint64_t n_sites = 0;
			for (int a = 4; a < argc; a++) {
				const std::string arg = argv[a];
				const size_t eq = arg.find('=');
				if (eq == std::string::npos || eq == 0 || eq + 1 >= arg.size()) { print_help(); return EXIT_FAILURE; }
				FILE *f = fopen(arg.substr(eq + 1).c_str(), "r");
				if (!f) throw vgh::Error{"cannot open " + arg.substr(eq + 1)};
				const size_t before = gt.size();
				unsigned g; long q;
				while (fscanf(f, "%u %ld", &g, &q) == 2) { gt.push_back((uint8_t)g); gq.push_back((int32_t)q); }
				fclose(f);
				if (a == 4) n_sites = gt.size();
				else if (gt.size() - before != n_sites) throw vgh::Error{arg.substr(eq + 1) + " lists another number of sites than " + std::string(argv[4]).substr(std::string(argv[4]).find('=') + 1)};
				names.push_back(arg.substr(0, eq));
			}
			std::vector<uint64_t> counts(names.size() * names.size() * 5);
			if (vg_pairs_host(gt.data(), gq.data(), n_sites, (uint32_t)names.size(), min_gq, std::max(1, env_int("VARGENO_THREADS", 1)), counts.data()) != VG_OK) throw vgh::Error{std::string("vg_pairs_host failed: ") + vg_last_error()};
			write_pairs_table(argv[2], names, n_sites, min_gq, counts);
			return EXIT_SUCCESS;
		} else if (opt == "version") {
			// hidden: the build ids (sha256 prefixes of the sources) of this binary and of the HIP library it loaded
#ifndef VG_HOST_BUILD_ID
#define VG_HOST_BUILD_ID "unknown"
#endif
			printf("host %s\nlib %s\n", VG_HOST_BUILD_ID, vg_build_id());
			return EXIT_SUCCESS;
		} else if (opt == "help") {
			print_help();
			return EXIT_SUCCESS;
		}
	} catch (const vgh::Error &e) {
		fprintf(stderr, "vargeno: %s\n", e.msg.c_str());
		return EXIT_FAILURE;
	}
	print_help();
	return EXIT_FAILURE;
}

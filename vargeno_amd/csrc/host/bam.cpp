// bam.cpp -- the command line's BAM routes on the host: a BAM file's header, and a BAM file as a once-only descriptor of its
// equivalent FASTQ text (BamTextPipe: a BgzfTextPipe inflates, a converter thread turns the records into text for a pipe).  The
// record parser and the conversion are the host build of ../vg_bam.h -- the one the device kernels are compiled from.  Included by
// main.cpp behind bgzf.cpp (whose helpers it uses).
#include "../vg_bam.h"

namespace vgh {

static bool read_some(int fd, std::vector<uint8_t> &buf, size_t want)
{
	const size_t have = buf.size();
	buf.resize(have + want);
	ssize_t n;
	do n = read(fd, buf.data() + have, want); while (n < 0 && errno == EINTR);
	buf.resize(have + (n > 0 ? (size_t)n : 0));
	return n > 0;
}

bool bam_header_info(int fd, uint64_t *header_end, int32_t *n_ref, std::string &err)
{
	std::vector<uint8_t> text;
	uint64_t at = 0;
	for (;;) {                                                        // the leading blocks, one span at a time, until the header parses
		std::vector<uint8_t> more;
		uint64_t next = at;
		if (!bgzf_inflate_span(fd, at, 0, more, &next, err)) return false;
		const bool end = next == at;
		text.insert(text.end(), more.begin(), more.end());
		at = next;
		const int rc = vg_bam_header(text.data(), text.size(), header_end, n_ref);
		if (rc == VG_BAM_OK) return true;
		if (rc == VG_BAM_BAD) { err = "not a BAM file: the inflated bytes do not start with the magic BAM\\1 and a header"; return false; }
		if (end) { err = "the BAM stream ends inside its header, at inflated offset " + std::to_string(text.size()); return false; }
	}
}

struct BamTextPipe::Impl {
	std::unique_ptr<BgzfTextPipe> in;
	int rfd = -1, wfd = -1;
	bool at_header = false;
	uint64_t stream_from = 0;
	std::thread converter;
	struct timespec born;
	BamTextPipe *self = nullptr;

	bool write_all(const std::string &text)
	{
		size_t o = 0;
		while (o < text.size()) {
			const ssize_t w = write(wfd, text.data() + o, text.size() - o);
			if (w < 0 && errno == EINTR) continue;
			if (w <= 0) return false;                                     // the reader has gone
			o += (size_t)w;
		}
		return true;
	}
	void convert()
	{
		std::vector<uint8_t> buf;
		uint64_t base = stream_from;                                  // inflated offset of buf[0]
		bool in_header = at_header, more = true;
		std::string text, err;
		VgBamCounts n;
		while (more && err.empty()) {
			more = read_some(in->read_fd(), buf, 1 << 20);
			uint64_t from = 0;
			if (in_header) {
				uint64_t end = 0; int32_t n_ref = 0;
				const int rc = vg_bam_header(buf.data(), buf.size(), &end, &n_ref);
				if (rc == VG_BAM_BAD) { err = "not a BAM file: the inflated bytes do not start with the magic BAM\\1 and a header"; break; }
				if (rc == VG_BAM_MORE) continue;
				in_header = false; from = end;
			}
			uint64_t used = from;
			text.clear();
			const int rc = vg_bam_convert(buf.data(), buf.size(), from, text, &used, n);
			self->text_bytes += text.size();
			if (!write_all(text)) break;
			if (rc == VG_BAM_BAD) err = "BAM record at inflated offset " + std::to_string(base + used) + ": its block_size is smaller than its own fields announce";
			buf.erase(buf.begin(), buf.begin() + (long)used);
			base += used;
		}
		close(wfd); wfd = -1;                                           // the reader sees the end of the text
		self->kept = n.kept; self->skipped_flag = n.skipped_flag; self->skipped_empty = n.skipped_empty;
		if (more) in.reset();                                           // stopped early (the reader has gone, a bad record): the inflating threads are told so
		else {
			in->finish();
			self->comp_bytes = in->comp_bytes;
			if (err.empty() && in_header) err = "the BAM stream ends inside its header, at inflated offset " + std::to_string(base + buf.size());
			else if (err.empty() && !buf.empty()) err = "the BAM stream ends inside a record, at inflated offset " + std::to_string(base);
			if (!in->error.empty()) err = err.empty() ? in->error : err + " (" + in->error + ")";
		}
		self->error = err;
		struct timespec now; clock_gettime(CLOCK_MONOTONIC, &now);
		self->seconds = (double)(now.tv_sec - born.tv_sec) + 1e-9 * (double)(now.tv_nsec - born.tv_nsec);
	}
};

BamTextPipe::BamTextPipe(int fd, uint64_t comp_from, uint32_t skip, int threads, bool at_header, uint64_t stream_from) : p(new Impl)
{
	p->self = this; p->at_header = at_header; p->stream_from = stream_from;
	clock_gettime(CLOCK_MONOTONIC, &p->born);
	p->in.reset(new BgzfTextPipe(fd, comp_from, skip, threads));
	if (p->in->read_fd() < 0) { error = p->in->error; return; }
	int fds[2];
	if (pipe(fds) != 0) { error = "pipe() failed"; return; }
	p->rfd = fds[0]; p->wfd = fds[1];
	(void)fcntl(p->wfd, F_SETPIPE_SZ, 1 << 20);
	p->converter = std::thread([this] { p->convert(); });
}
BamTextPipe::~BamTextPipe()
{
	if (p->rfd >= 0) close(p->rfd);                                  // (a converter blocked on a full pipe wakes up with EPIPE)
	finish();
	delete p;
}
int BamTextPipe::read_fd() const { return p->rfd; }
void BamTextPipe::finish() { if (p->converter.joinable()) p->converter.join(); }
std::string BamTextPipe::describe(const char *what, bool takeover) const
{
	char line[512];
	if (!takeover) snprintf(line, sizeof line, "ingest, %s: BAM inflated and converted by host threads: %lu records kept, %lu skipped by flag, %lu skipped empty, 0 window repairs; %.3f GB compressed, %.3f GB of text in %.2f s", what,
	                        (unsigned long)kept, (unsigned long)skipped_flag, (unsigned long)skipped_empty, (double)comp_bytes / 1e9, (double)text_bytes / 1e9, seconds);
	// (behind the device route: what the host converted after a refusal is a line of its own, nothing when there was none)
	else if (kept + skipped_flag + skipped_empty) snprintf(line, sizeof line, "host take-over, %s: %lu BAM records converted by host threads behind the device's refusal, %lu skipped by flag, %lu skipped empty", what,
	                                                       (unsigned long)kept, (unsigned long)skipped_flag, (unsigned long)skipped_empty);
	else return "";
	return line;
}

bool bam_record_text(int fd, uint64_t block, uint32_t within, std::string &text, std::string &err)
{
	std::vector<uint8_t> raw;
	uint64_t comp_next = 0;
	if (!bgzf_inflate_span(fd, block, (uint64_t)within + 4 + VG_BAM_MAX_BLOCK, raw, &comp_next, err)) return false;
	VgBamRec r;
	if (vg_bam_view(raw.data(), raw.size(), within, &r) != VG_BAM_OK || !vg_bam_sizes_ok(r) || raw.size() - within < 4ull + r.block_size || r.l_seq == 0) {
		err = "no whole BAM record at the hand-over point";
		return false;
	}
	vg_bam_append_fastq(raw.data(), within, r, text);
	return true;
}

}  // namespace vgh

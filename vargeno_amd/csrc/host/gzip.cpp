// gzip.cpp -- the command line's plain-gzip route on the host: a gzip file (RFC 1952, any number of members, no block table) as a
// once-only text descriptor (GzipTextPipe: one thread runs the sequential decoder into a pipe).  The decoder is the host build of
// ../vg_gunzip.h -- the one the device kernels are compiled from --, run piece by piece: the file is read 8 MiB at a time and the
// text leaves 4 MiB at a time, with the last 32 KiB kept as the window.
#include "vg_host.h"

#include "../vg_gunzip.h"

#include <errno.h>
#include <fcntl.h>
#include <signal.h>
#include <time.h>
#include <unistd.h>

#include <algorithm>
#include <memory>
#include <thread>

namespace vgh {

static std::string gzip_error(uint64_t comp_off, int rc) { return "gzip stream at compressed offset " + std::to_string(comp_off) + ": " + vg_gunzip_strerror(rc); }

// The sequential decoder over a file: next() appends the text of the next whole DEFLATE blocks to `out`.
struct GzipHostStream {
	static constexpr uint64_t READ = 8ull << 20, WIN = VG_GZ_WINDOW;
	int fd;
	uint64_t file_at = 0;                      // file offset of in[0]
	std::vector<uint8_t> in;                   // compressed bytes not yet consumed (and what follows them)
	bool eof = false;
	uint64_t bit = 0;                          // where the decoder stands, relative to in[0]: a block boundary, or a member's first byte
	bool in_member = false;
	std::vector<uint8_t> buf;                  // [window | text of this step]
	uint64_t before = 0, cap = 4ull << 20;     // bytes of window in buf; room for text behind it
	uint32_t crc = 0; uint64_t isize = 0;
	uint64_t members = 0, comp_bytes = 0, text_bytes = 0;
	std::string error;
	VgInfTables t;

	bool resumed = false;                      // the decoder started inside this member: its CRC32 and ISIZE cannot be checked here

	explicit GzipHostStream(int fd_) : fd(fd_) {}
	// from a checkpoint of a device stream: compressed bit offset `at_bit` of the file is a block boundary inside a member, and
	// win[0, win_len) is the member's text in front of it (at_bit 0: the file from its first byte)
	GzipHostStream(int fd_, uint64_t at_bit, const uint8_t *win, uint32_t win_len) : fd(fd_)
	{
		if (!at_bit) return;
		file_at = at_bit >> 3; bit = at_bit & 7u;
		in_member = true; resumed = true;
		buf.resize(WIN + cap);
		if (win_len) memcpy(buf.data() + WIN - win_len, win, win_len);
		before = win_len;
	}
	// more of the file behind in[]; what the decoder has passed is dropped.  false: nothing more came (the end of the file, or an error)
	bool refill()
	{
		const uint64_t used = bit >> 3;
		in.erase(in.begin(), in.begin() + (long)used);
		file_at += used; bit &= 7u;
		if (eof) return false;
		const size_t have = in.size();
		in.resize(have + READ);
		uint64_t got = 0;
		while (got < READ) {
			const ssize_t g = pread(fd, in.data() + have + got, (size_t)(READ - got), (off_t)(file_at + have + got));
			if (g < 0 && errno == EINTR) continue;
			if (g < 0) { error = "error reading the gzip file"; in.resize(have + got); eof = true; return false; }
			if (g == 0) { eof = true; break; }
			got += (uint64_t)g;
		}
		in.resize(have + got);
		return got != 0;
	}
	// false: the end of the file, or an error (then `error` says which)
	bool next(std::vector<uint8_t> &out)
	{
		for (;;) {                                                        // every turn consumes input, reads more of the file, or grows the buffer; or returns
			if (!in_member) {
				const uint64_t pos = bit >> 3;
				if (pos >= in.size()) { if (refill()) continue; return false; }
				uint64_t hl = 0;
				const int hrc = vg_gz_header(in.data() + pos, in.size() - pos, &hl);
				if (hrc == 1) { if (refill()) continue; if (error.empty()) error = gzip_error(file_at + in.size(), VG_INF_EINPUT); return false; }
				if (hrc) { error = gzip_error(file_at + pos, hrc); return false; }
				bit = (pos + hl) * 8;
				in_member = true; crc = 0; isize = 0; before = 0;
			}
			buf.resize(WIN + cap);
			VgGzHostBytes io;
			io.in = in.data(); io.len = in.size();
			io.out = buf.data() + WIN; io.before = before;
			io.seek_bit(bit);
			uint64_t x_bit = bit, x_out = 0; uint32_t ended = 0;
			const int rc = vg_gz_stream(io, t, UINT64_MAX, cap, &x_bit, &x_out, &ended);
			if (rc && rc != VG_INF_EINPUT && rc != VG_GZ_ECAP) { error = gzip_error(file_at + io.bitpos() / 8, rc); return false; }
			if (x_bit == bit && !ended) {                                     // not one whole block: more input, or more room
				if (rc == VG_GZ_ECAP) {
					if (cap >= (2ull << 30)) { error = gzip_error(file_at + (bit >> 3), VG_GZ_EBLOCK); return false; }
					cap *= 2;
					continue;
				}
				if (refill()) continue;
				if (error.empty()) error = gzip_error(file_at + in.size(), VG_INF_EINPUT);
				return false;
			}
			const uint8_t *tx = buf.data() + WIN;
			crc = vg_crc32(vg_crc_tab_host(), crc, tx, x_out);
			isize += x_out; text_bytes += x_out;
			out.insert(out.end(), tx, tx + x_out);
			// the window of the next step: the last 32 KiB of window + text, moved in front of the text area
			const uint64_t keep = std::min<uint64_t>(WIN, before + x_out);
			memmove(buf.data() + WIN - keep, tx + x_out - keep, keep);
			before = keep;
			comp_bytes += (x_bit >> 3) - (bit >> 3);
			bit = x_bit;
			if (ended) {
				uint64_t tb = (bit + 7) >> 3;
				if (tb + 8 > in.size()) { (void)refill(); tb = (bit + 7) >> 3; }
				if (tb + 8 > in.size()) { if (error.empty()) error = gzip_error(file_at + in.size(), VG_INF_EINPUT); return false; }
				if (!resumed && crc != vg_gz_le32(in.data() + tb)) { error = gzip_error(file_at + tb, VG_INF_ECRC); return false; }
				if (!resumed && (uint32_t)isize != vg_gz_le32(in.data() + tb + 4)) { error = gzip_error(file_at + tb + 4, VG_INF_ESIZE); return false; }
				resumed = false;
				bit = (tb + 8) * 8;
				comp_bytes += 8;
				in_member = false; members++;
			}
			if (x_out) return true;
		}
	}
};

bool gzip_cat(int fd, FILE *to, std::string &err)
{
	GzipHostStream gs(fd);
	std::vector<uint8_t> text;
	while (gs.next(text)) {
		if (fwrite(text.data(), 1, text.size(), to) != text.size()) { err = "cannot write the text"; return false; }
		text.clear();
	}
	err = gs.error;
	return err.empty();
}

struct GzipTextPipe::Impl {
	int fd = -1, rfd = -1, wfd = -1;
	std::thread producer;
	struct timespec born;
	GzipTextPipe *self = nullptr;
	uint64_t members = 0;
	std::unique_ptr<GzipHostStream> gsp;
	std::vector<uint8_t> pending;               // text decoded before the producer started that belongs in the pipe
	uint64_t span_bytes = 0;                    // text decoded by the constructor for the caller's span (text the device had framed already)

	void produce()
	{
		GzipHostStream &gs = *gsp;
		std::vector<uint8_t> text;
		text.swap(pending);
		bool reader_gone = false;
		while (!reader_gone && (!text.empty() || gs.next(text))) {
			size_t o = 0;
			while (o < text.size()) {
				const ssize_t w = write(wfd, text.data() + o, text.size() - o);
				if (w < 0 && errno == EINTR) continue;
				if (w <= 0) { reader_gone = true; break; }
				o += (size_t)w;
			}
			text.clear();
		}
		if (!reader_gone) self->error = gs.error;
		self->comp_bytes = gs.comp_bytes; self->text_bytes = gs.text_bytes - span_bytes; members = gs.members;
		close(wfd); wfd = -1;                                           // the reader sees the end of the text
		struct timespec now; clock_gettime(CLOCK_MONOTONIC, &now);
		self->seconds = (double)(now.tv_sec - born.tv_sec) + 1e-9 * (double)(now.tv_nsec - born.tv_nsec);
	}
};

GzipTextPipe::GzipTextPipe(int fd) : p(new Impl)
{
	p->gsp.reset(new GzipHostStream(fd));
	start(fd);
}
GzipTextPipe::GzipTextPipe(int fd, uint64_t at_bit, const uint8_t *win, uint32_t win_len, uint64_t span_len, std::vector<uint8_t> &span) : p(new Impl)
{
	p->gsp.reset(new GzipHostStream(fd, at_bit, win, win_len));
	span.clear();
	while (span.size() < span_len && p->gsp->next(span)) {}
	if (span.size() < span_len) { error = p->gsp->error.empty() ? "the gzip file ends before the text the device framed" : p->gsp->error; return; }
	p->pending.assign(span.begin() + (long)span_len, span.end());
	span.resize((size_t)span_len);
	p->span_bytes = span_len;
	start(fd);
}
void GzipTextPipe::start(int fd)
{
	p->self = this; p->fd = fd;
	clock_gettime(CLOCK_MONOTONIC, &p->born);
	signal(SIGPIPE, SIG_IGN);                                        // a reader that goes away early is an EPIPE for the producer, not the end of the process
	int fds[2];
	if (pipe(fds) != 0) { error = "pipe() failed"; return; }
	p->rfd = fds[0]; p->wfd = fds[1];
	(void)fcntl(p->wfd, F_SETPIPE_SZ, 1 << 20);
	p->producer = std::thread([this] { p->produce(); });
}
GzipTextPipe::~GzipTextPipe()
{
	if (p->rfd >= 0) close(p->rfd);                                     // (a producer blocked on a full pipe wakes up with EPIPE)
	finish();
	delete p;
}
int GzipTextPipe::read_fd() const { return p->rfd; }
void GzipTextPipe::finish() { if (p->producer.joinable()) p->producer.join(); }
std::string GzipTextPipe::describe(const char *what, bool takeover) const
{
	char line[512];
	if (takeover && text_bytes == 0) return "";
	snprintf(line, sizeof line, takeover ? "ingest, %s: gzip inflated on the host from the device route's checkpoint on: %lu members, %.3f GB compressed (%.2f GB/s), %.3f GB of text beyond the span the device had framed (%.2f GB/s) in %.2f s"
	                                     : "ingest, %s: gzip inflated by one host thread: %lu members, %.3f GB compressed (%.2f GB/s), %.3f GB of text (%.2f GB/s) in %.2f s", what, (unsigned long)p->members,
	         (double)comp_bytes / 1e9, seconds > 0 ? (double)comp_bytes / 1e9 / seconds : 0.0, (double)text_bytes / 1e9, seconds > 0 ? (double)text_bytes / 1e9 / seconds : 0.0, seconds);
	return line;
}

}  // namespace vgh

// bgzf.cpp -- the command line's BGZF routes on the host: what a FASTQ path is (text, BGZF, plain gzip), a BGZF file as a once-only
// text descriptor (BgzfTextPipe: host threads inflate its blocks in order into a pipe), and the text around a hand-over point as a
// memory span.  The decoder is the host build of ../vg_inflate.h -- the one the device kernel is compiled from.
#include "vg_host.h"

#include "../vg_inflate.h"

#include <errno.h>
#include <fcntl.h>
#include <signal.h>
#include <time.h>
#include <unistd.h>

#include <algorithm>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>

namespace vgh {

static std::string block_error(uint64_t comp_off, int rc) { return "BGZF block at compressed offset " + std::to_string(comp_off) + ": " + vg_inflate_strerror(rc); }

// pread all of [at, at + n); returns the bytes read (short at the end of the file), -1 on an error
static int64_t pread_all(int fd, uint8_t *dst, uint64_t n, uint64_t at)
{
	uint64_t done = 0;
	while (done < n) {
		const ssize_t g = pread(fd, dst + done, (size_t)(n - done), (off_t)(at + done));
		if (g < 0 && errno == EINTR) continue;
		if (g < 0) return -1;
		if (g == 0) break;
		done += (uint64_t)g;
	}
	return (int64_t)done;
}

FastqKind sniff_fastq(int fd)
{
	uint8_t head[4096];
	const ssize_t n = pread(fd, head, sizeof head, 0);
	if (n >= 4 && !memcmp(head, "CRAM", 4)) return FastqKind::Cram;
	if (n < 3 || !vg_is_gzip(head, (uint64_t)n)) return FastqKind::Text;
	vg_bgzf_block b;
	if (vg_bgzf_header(head, (uint64_t)n, &b) == VG_INF_EHEADER) return FastqKind::PlainGzip;     // (0 / 1: a BGZF header, whole or as far as 4 KiB show)
	// BGZF: the first four inflated bytes say whether it is BAM (they may lie in several blocks: a block can hold one byte, or none)
	std::vector<uint8_t> lead(1 << 18);
	const int64_t got = pread_all(fd, lead.data(), lead.size(), 0);
	std::vector<vg_bgzf_block> bl;
	uint64_t tail = 0, bad = 0;
	if (got > 0) (void)vg_bgzf_scan(lead.data(), (uint64_t)got, 0, 0, bl, &tail, &bad);
	uint8_t first[4 + VG_BGZF_MAX_ISIZE];
	size_t have = 0;
	for (const vg_bgzf_block &k : bl) {
		if (have >= 4) break;
		if (vg_inflate_block_host(lead.data() + k.in_off, k.in_len, first + have, k.isize, k.crc)) break;
		have += k.isize;
	}
	return have >= 4 && !memcmp(first, "BAM\1", 4) ? FastqKind::Bam : FastqKind::Bgzf;
}

// the whole blocks of buf inflated into text (sized here) by `threads` threads; "" or the first (lowest) block's error
static std::string inflate_blocks(const uint8_t *buf, const std::vector<vg_bgzf_block> &bl, std::vector<uint8_t> &text, int threads)
{
	const uint64_t t0 = bl.empty() ? 0 : bl.front().text_off;
	text.resize(bl.empty() ? 0 : (size_t)(bl.back().text_off + bl.back().isize - t0));
	long first_bad = (long)bl.size();
	int first_rc = 0;
#pragma omp parallel for schedule(dynamic, 8) num_threads(threads)
	for (long i = 0; i < (long)bl.size(); i++) {
		const vg_bgzf_block &b = bl[(size_t)i];
		uint8_t none;
		const int rc = vg_inflate_block_host(buf + b.in_off, b.in_len, b.isize ? text.data() + (b.text_off - t0) : &none, b.isize, b.crc);
		if (rc) {
#pragma omp critical(vg_bgzf_first_bad)
			if (i < first_bad) { first_bad = i; first_rc = rc; }
		}
	}
	return first_bad < (long)bl.size() ? block_error(bl[(size_t)first_bad].comp_off, first_rc) : std::string();
}

bool bgzf_inflate_span(int fd, uint64_t comp_from, uint64_t want_text, std::vector<uint8_t> &text, uint64_t *comp_next, std::string &err)
{
	text.clear();
	uint64_t at = comp_from;
	std::vector<uint8_t> blk(65536);
	for (;;) {                                                        // one block per step, until the span is long enough or the file ends
		const int64_t n = pread_all(fd, blk.data(), blk.size(), at);
		if (n < 0) { err = "error reading the BGZF file"; return false; }
		if (n == 0) break;
		vg_bgzf_block b;
		const int rc = vg_bgzf_header(blk.data(), (uint64_t)n, &b);
		if (rc) { err = rc == 1 ? "BGZF block at compressed offset " + std::to_string(at) + ": incomplete (the file ends inside it)" : block_error(at, rc); return false; }
		const size_t o = text.size();
		text.resize(o + b.isize);
		uint8_t none;
		const int brc = vg_inflate_block_host(blk.data() + b.in_off, b.in_len, b.isize ? text.data() + o : &none, b.isize, b.crc);
		if (brc) { err = block_error(at, brc); return false; }
		at += (uint64_t)b.in_off + b.in_len + 8;
		if (text.size() > want_text) break;
	}
	*comp_next = at;
	return true;
}

int bgzf_threads_default(int usable_cpus) { return std::max(1, std::min(usable_cpus, 8)); }

struct BgzfTextPipe::Impl {
	int fd = -1, rfd = -1, wfd = -1;
	uint64_t at = 0;
	uint32_t skip = 0;
	int threads = 1;
	std::thread producer, writer;
	std::mutex mu; std::condition_variable cv;
	std::deque<std::vector<uint8_t>> q;                               // inflated text waiting for the pipe (at most two buffers)
	bool done = false, reader_gone = false;
	struct timespec born;
	BgzfTextPipe *self = nullptr;

	void fail(const std::string &e) { std::lock_guard<std::mutex> g(mu); if (self->error.empty()) self->error = e; }
	void produce()
	{
		const uint64_t CHUNK = 8ull << 20;
		std::vector<uint8_t> buf;
		std::vector<vg_bgzf_block> bl;
		uint64_t text_pos = 0;
		for (;;) {                                                    // one chunk of the file per step
			const size_t have = buf.size();
			buf.resize(have + CHUNK);
			const int64_t n = pread_all(fd, buf.data() + have, CHUNK, at + have);
			if (n < 0) { fail("error reading the BGZF file"); break; }
			buf.resize(have + (size_t)n);
			if (buf.empty()) break;
			bl.clear();
			uint64_t tail = 0, bad_off = 0;
			const int rc = vg_bgzf_scan(buf.data(), buf.size(), at, text_pos, bl, &tail, &bad_off);
			std::vector<uint8_t> text;
			std::string e = inflate_blocks(buf.data(), bl, text, threads);
			if (e.empty() && rc) e = block_error(bad_off, rc);
			if (e.empty() && n == 0 && tail) e = "BGZF block at compressed offset " + std::to_string(at + buf.size() - tail) + ": incomplete (the file ends inside it)";
			if (!e.empty()) { fail(e); break; }
			text_pos += text.size();
			const uint64_t used = buf.size() - tail;
			self->comp_bytes += used;
			if (skip) { const size_t s = std::min<size_t>(skip, text.size()); text.erase(text.begin(), text.begin() + (long)s); skip -= (uint32_t)s; }
			self->text_bytes += text.size();
			if (!text.empty()) {
				std::unique_lock<std::mutex> g(mu);
				cv.wait(g, [&] { return q.size() < 2 || reader_gone; });
				if (reader_gone) break;
				q.push_back(std::move(text));
				cv.notify_all();
			}
			buf.erase(buf.begin(), buf.begin() + (long)used);
			at += used;
			if (n == 0) break;
		}
		{ std::lock_guard<std::mutex> g(mu); done = true; }
		cv.notify_all();
	}
	void write_out()
	{
		for (;;) {
			std::vector<uint8_t> text;
			{
				std::unique_lock<std::mutex> g(mu);
				cv.wait(g, [&] { return !q.empty() || done; });
				if (q.empty()) break;
				text = std::move(q.front()); q.pop_front();
				cv.notify_all();
			}
			size_t o = 0;
			while (o < text.size()) {
				const ssize_t w = write(wfd, text.data() + o, text.size() - o);
				if (w < 0 && errno == EINTR) continue;
				if (w <= 0) { { std::lock_guard<std::mutex> g(mu); reader_gone = true; } cv.notify_all(); break; }
				o += (size_t)w;
			}
			if (o < text.size()) break;
		}
		close(wfd); wfd = -1;                                           // the reader sees the end of the text
		struct timespec now; clock_gettime(CLOCK_MONOTONIC, &now);
		self->seconds = (double)(now.tv_sec - born.tv_sec) + 1e-9 * (double)(now.tv_nsec - born.tv_nsec);
	}
};

BgzfTextPipe::BgzfTextPipe(int fd, uint64_t comp_from, uint32_t skip, int threads) : p(new Impl)
{
	p->self = this; p->fd = fd; p->at = comp_from; p->skip = skip; p->threads = std::max(1, threads);
	clock_gettime(CLOCK_MONOTONIC, &p->born);
	signal(SIGPIPE, SIG_IGN);                                        // a reader that goes away early is an EPIPE for the writer thread, not the end of the process
	int fds[2];
	if (pipe(fds) != 0) { error = "pipe() failed"; p->done = true; return; }
	p->rfd = fds[0]; p->wfd = fds[1];
	(void)fcntl(p->wfd, F_SETPIPE_SZ, 1 << 20);
	p->producer = std::thread([this] { p->produce(); });
	p->writer = std::thread([this] { p->write_out(); });
}
BgzfTextPipe::~BgzfTextPipe()
{
	{ std::lock_guard<std::mutex> g(p->mu); p->reader_gone = true; }
	p->cv.notify_all();
	if (p->rfd >= 0) close(p->rfd);                                  // (a writer blocked on a full pipe wakes up with EPIPE)
	finish();
	delete p;
}
int BgzfTextPipe::read_fd() const { return p->rfd; }
void BgzfTextPipe::finish()
{
	if (p->producer.joinable()) p->producer.join();
	if (p->writer.joinable()) p->writer.join();
}
std::string BgzfTextPipe::describe(const char *what, bool) const
{
	char line[512];
	snprintf(line, sizeof line, "ingest, %s: BGZF inflated by %d host threads: %.3f GB compressed (%.2f GB/s), %.3f GB of text (%.2f GB/s) in %.2f s", what, p->threads,
	         (double)comp_bytes / 1e9, seconds > 0 ? (double)comp_bytes / 1e9 / seconds : 0.0, (double)text_bytes / 1e9, seconds > 0 ? (double)text_bytes / 1e9 / seconds : 0.0, seconds);
	return line;
}

}  // namespace vgh

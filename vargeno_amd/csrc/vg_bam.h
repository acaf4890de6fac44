// BAM records (SAM/BAM specification, section 4.2) as reads: ONE parser for the host and for the device.  Under hipcc every function
// here is __host__ __device__; under g++ they are ordinary functions (the pattern of vg_inflate.h and vg_caller.h).
//
// A BAM file is a BGZF file whose inflated bytes are: magic "BAM\1", l_text, the header text, n_ref, the references (l_name, name,
// l_ref), then records -- each a little-endian block_size followed by block_size bytes: 32 bytes of fixed fields (refID, pos,
// l_read_name, mapq, bin, n_cigar_op, flag, l_seq, next_refID, next_pos, tlen), the NUL-terminated name, the CIGAR (4 bytes per
// operation), the bases (4 bits each, high nibble first), the qualities (a byte each) and the auxiliary fields.
//
// What a record becomes is THIS PROJECT'S definition of the equivalent FASTQ text:
//   - flag 0x100 (secondary) or 0x800 (supplementary): skipped; l_seq == 0: skipped; every other record is one read, in file order
//   - bases through "=ACMGRSVTWYHKDBN"; with flag 0x10 reverse-complemented (the complement of a 4-bit code is the code with its
//     four bits reversed: A 1 <-> T 8, C 2 <-> G 4, = and N map to themselves) and the qualities reversed
//   - quality character min(q, 93) + 33; a first quality byte of 0xFF (absent) makes every character '"' (Q1)
//   - "@" + read_name (without its NUL), the bases, "+", the qualities: four lines
//
// EVERY read of the buffer is bounds-checked against its length: a wild block_size never becomes a wild load.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

#if defined(__HIPCC__)
#define VG_BAM_HD __host__ __device__ __attribute__((always_inline)) inline
#else
#define VG_BAM_HD inline
#endif

constexpr uint32_t VG_BAM_FIXED = 36;               // block_size + the 32 bytes of fixed fields
constexpr uint32_t VG_BAM_MAX_BLOCK = 65532;        // the largest block_size framed here: a record (4 + block_size bytes) fits one window and the carry gap
constexpr uint32_t VG_BAM_WINDOW = 1u << 16;        // framing works over fixed windows of the inflated bytes
constexpr uint32_t VG_BAM_WIN_RECS = VG_BAM_WINDOW / 36 + 1;   // records that can START inside one window (a record is at least 37 bytes)
constexpr uint32_t VG_BAM_MAX_REPAIRS = 64;         // windows re-walked serially per slot before the chunk is refused: a bound on the serial work, not a tuned number
constexpr uint32_t VG_BAM_MAX_READ = 1022;          // the longest read the reference's line buffer holds (BUF_SIZE 1024, qv.cc:700)
constexpr uint32_t VG_BAM_NONE = 0xffffffffu;       // no offset

enum { VG_BAM_OK = 0, VG_BAM_MORE = 1, VG_BAM_BAD = 2 };

// the fields of the record at an offset, as far as reads are concerned
struct VgBamRec {
	uint32_t block_size;
	int32_t ref_id, pos, next_ref_id, next_pos;
	uint32_t l_read_name, n_cigar, flag, l_seq;
	VG_BAM_HD uint64_t name_off(uint64_t off) const { return off + VG_BAM_FIXED; }
	VG_BAM_HD uint64_t seq_off(uint64_t off) const { return off + VG_BAM_FIXED + l_read_name + 4ull * n_cigar; }
	VG_BAM_HD uint64_t qual_off(uint64_t off) const { return seq_off(off) + ((uint64_t)l_seq + 1) / 2; }
	VG_BAM_HD uint64_t min_block() const { return 32ull + l_read_name + 4ull * n_cigar + ((uint64_t)l_seq + 1) / 2 + l_seq; }
	VG_BAM_HD bool skipped_by_flag() const { return (flag & 0x900u) != 0; }
	VG_BAM_HD bool reversed() const { return (flag & 0x10u) != 0; }
};

// little-endian 32 bits at off; the caller has checked off + 4 <= len
VG_BAM_HD uint32_t vg_bam_le32(const uint8_t *buf, uint64_t off)
{
	return (uint32_t)buf[off] | (uint32_t)buf[off + 1] << 8 | (uint32_t)buf[off + 2] << 16 | (uint32_t)buf[off + 3] << 24;
}

// The field view of the record at buf[off ..): VG_BAM_MORE when its fixed part is not wholly inside [0, len)
VG_BAM_HD int vg_bam_view(const uint8_t *buf, uint64_t len, uint64_t off, VgBamRec *r)
{
	if (off > len || len - off < VG_BAM_FIXED) return VG_BAM_MORE;
	r->block_size = vg_bam_le32(buf, off);
	r->ref_id = (int32_t)vg_bam_le32(buf, off + 4);
	r->pos = (int32_t)vg_bam_le32(buf, off + 8);
	r->l_read_name = buf[off + 12];
	r->n_cigar = (uint32_t)buf[off + 16] | (uint32_t)buf[off + 17] << 8;
	r->flag = (uint32_t)buf[off + 18] | (uint32_t)buf[off + 19] << 8;
	r->l_seq = vg_bam_le32(buf, off + 20);
	r->next_ref_id = (int32_t)vg_bam_le32(buf, off + 24);
	r->next_pos = (int32_t)vg_bam_le32(buf, off + 28);
	return VG_BAM_OK;
}

// What framing demands of a record: a name, and a block_size that holds what its own fields announce and is not beyond the limit
VG_BAM_HD bool vg_bam_sizes_ok(const VgBamRec &r)
{
	return r.l_read_name >= 1 && r.block_size <= VG_BAM_MAX_BLOCK && r.min_block() <= r.block_size;
}

// The plausibility predicate of speculation: could a record start at off?  VG_BAM_MORE: the buffer ends before that can be said.
VG_BAM_HD int vg_bam_plausible(const uint8_t *buf, uint64_t len, uint64_t off, int32_t n_ref, VgBamRec *r)
{
	if (vg_bam_view(buf, len, off, r) != VG_BAM_OK) return VG_BAM_MORE;
	if (!vg_bam_sizes_ok(*r)) return VG_BAM_BAD;
	if (r->ref_id < -1 || r->ref_id >= n_ref || r->next_ref_id < -1 || r->next_ref_id >= n_ref) return VG_BAM_BAD;
	if (r->pos < -1 || r->next_pos < -1) return VG_BAM_BAD;
	const uint64_t nul = off + VG_BAM_FIXED + r->l_read_name - 1;
	if (nul >= len) return VG_BAM_MORE;
	return buf[nul] == 0 ? VG_BAM_OK : VG_BAM_BAD;
}

// Speculation's test of a candidate offset: three consecutive plausible records, or a chain of plausible records (at least one)
// that reaches the end of the data
VG_BAM_HD bool vg_bam_chain(const uint8_t *buf, uint64_t len, uint64_t off, int32_t n_ref)
{
	VgBamRec r;
	for (int i = 0; i < 3; i++) {
		const int rc = vg_bam_plausible(buf, len, off, n_ref, &r);
		if (rc == VG_BAM_MORE) return i > 0;
		if (rc != VG_BAM_OK) return false;
		off += 4ull + r.block_size;
	}
	return true;
}

// base j (0 <= j < l_seq) of the emitted read; the caller has checked that the record's bytes are inside the buffer
VG_BAM_HD uint8_t vg_bam_base(const uint8_t *buf, uint64_t seq_off, uint32_t l_seq, bool rev, uint32_t j)
{
	const uint32_t i = rev ? l_seq - 1u - j : j;
	uint32_t c = (buf[seq_off + (i >> 1)] >> ((i & 1u) ? 0 : 4)) & 15u;
	if (rev) c = (c & 1u) << 3 | (c & 2u) << 1 | (c & 4u) >> 1 | (c & 8u) >> 3;
	return (uint8_t)"=ACMGRSVTWYHKDBN"[c];
}
// quality character c of the emitted read
VG_BAM_HD uint8_t vg_bam_qual(const uint8_t *buf, uint64_t qual_off, uint32_t l_seq, bool rev, uint32_t c)
{
	if (buf[qual_off] == 0xff) return (uint8_t)'"';
	const uint32_t q = buf[qual_off + (rev ? l_seq - 1u - c : c)];
	return (uint8_t)((q < 93u ? q : 93u) + 33u);
}
// the read's gate word: bit c set iff emitted quality character c is below '8', for c < min(l_seq >> 5, 32) -- vg_fq_gather's rule
VG_BAM_HD bool vg_bam_gate_bit(const uint8_t *buf, uint64_t qual_off, uint32_t l_seq, bool rev, uint32_t c)
{
	return c < (l_seq >> 5) && c < 32u && vg_bam_qual(buf, qual_off, l_seq, rev, c) < (uint8_t)'8';
}

// What one walk over a window found
struct VgBamWalk {
	uint32_t exit;             // offset of the first record at or beyond the window's end -- or of the record the data ends inside
	uint32_t n_kept;           // records that become reads: their offsets are in the caller's table
	uint32_t n_flag, n_empty;  // skipped: secondary / supplementary; l_seq == 0
	uint32_t bad;              // a record that cannot be framed (sizes; a read of more than VG_BAM_MAX_READ bases): the walk stopped at `exit`
};

// The chain of records from `entry` to the first one at or beyond win_end, in buf[0, len) (len < 2^32).  Offsets of the kept records
// go to offs[0, cap).  The walk ends early, with exit at that record, where the data ends inside a record or a record is bad.
// Every step moves at least 37 bytes on: at most (win_end - entry) / 37 + 1 steps.
VG_BAM_HD void vg_bam_walk(const uint8_t *buf, uint64_t len, uint64_t entry, uint64_t win_end, uint32_t *offs, uint32_t cap, VgBamWalk *w)
{
	uint64_t off = entry;
	w->n_kept = 0; w->n_flag = 0; w->n_empty = 0; w->bad = 0;
	while (off < win_end) {
		VgBamRec r;
		if (vg_bam_view(buf, len, off, &r) != VG_BAM_OK) break;               // the data ends inside the fixed part
		if (!vg_bam_sizes_ok(r)) { w->bad = 1; break; }
		if (len - off < 4ull + r.block_size) break;                             // ... or inside the rest
		if (r.skipped_by_flag()) w->n_flag++;
		else if (r.l_seq == 0) w->n_empty++;
		else if (r.l_seq > VG_BAM_MAX_READ || w->n_kept >= cap) { w->bad = 1; break; }
		else offs[w->n_kept++] = (uint32_t)off;
		off += 4ull + r.block_size;
	}
	w->exit = (uint32_t)off;
}

// The header at buf[0, len): VG_BAM_OK with *end = offset of the first record and *n_ref; VG_BAM_MORE: more bytes are needed;
// VG_BAM_BAD: this is not BAM (magic, or negative lengths).  One step per reference, each at least 8 bytes: at most len / 8 steps.
VG_BAM_HD int vg_bam_header(const uint8_t *buf, uint64_t len, uint64_t *end, int32_t *n_ref)
{
	const uint8_t magic[4] = {'B', 'A', 'M', 1};
	for (uint64_t i = 0; i < 4 && i < len; i++) if (buf[i] != magic[i]) return VG_BAM_BAD;
	if (len < 8) return VG_BAM_MORE;
	const uint32_t l_text = vg_bam_le32(buf, 4);
	if (l_text >> 31) return VG_BAM_BAD;
	uint64_t at = 8ull + l_text;
	if (len < at + 4) return VG_BAM_MORE;
	const uint32_t n = vg_bam_le32(buf, at);
	if (n >> 31) return VG_BAM_BAD;
	at += 4;
	for (uint32_t i = 0; i < n; i++) {
		if (len < at + 4) return VG_BAM_MORE;
		const uint32_t l_name = vg_bam_le32(buf, at);
		if (l_name >> 31) return VG_BAM_BAD;
		at += 8ull + l_name;                                                  // l_name, the name, l_ref
		if (len < at) return VG_BAM_MORE;
	}
	*end = at; *n_ref = (int32_t)n;
	return VG_BAM_OK;
}

// Host: the equivalent FASTQ text of the record at off (a kept record whose bytes are inside the buffer), appended to out
inline void vg_bam_append_fastq(const uint8_t *buf, uint64_t off, const VgBamRec &r, std::string &out)
{
	out.push_back('@');
	out.append((const char *)buf + r.name_off(off), r.l_read_name - 1);
	out.push_back('\n');
	const uint64_t so = r.seq_off(off), qo = r.qual_off(off);
	const bool rev = r.reversed();
	const size_t at = out.size();
	out.resize(at + 2 * (size_t)r.l_seq + 4);
	char *p = &out[at];
	for (uint32_t j = 0; j < r.l_seq; j++) p[j] = (char)vg_bam_base(buf, so, r.l_seq, rev, j);
	p[r.l_seq] = '\n'; p[r.l_seq + 1] = '+'; p[r.l_seq + 2] = '\n';
	char *q = p + r.l_seq + 3;
	for (uint32_t j = 0; j < r.l_seq; j++) q[j] = (char)vg_bam_qual(buf, qo, r.l_seq, rev, j);
	q[r.l_seq] = '\n';
}

// Host: the records of buf[from, len) converted, as many as are whole.  *used = offset of the first byte not converted (a record
// boundary).  VG_BAM_OK: the data ends at a boundary or inside a record (*used < len then); VG_BAM_BAD: the record at *used has a
// block_size smaller than what its own fields announce (or no name).  The host converts records of any length: a read beyond the
// reference's line buffer reaches its framing rules as text.
struct VgBamCounts { uint64_t kept = 0, skipped_flag = 0, skipped_empty = 0; };
inline int vg_bam_convert(const uint8_t *buf, uint64_t len, uint64_t from, std::string &out, uint64_t *used, VgBamCounts &n)
{
	uint64_t off = from;
	int rc = VG_BAM_OK;
	for (;;) {
		VgBamRec r;
		if (vg_bam_view(buf, len, off, &r) != VG_BAM_OK) break;
		if (r.l_read_name < 1 || r.min_block() > r.block_size) { rc = VG_BAM_BAD; break; }
		if (len - off < 4ull + r.block_size) break;
		if (r.skipped_by_flag()) n.skipped_flag++;
		else if (r.l_seq == 0) n.skipped_empty++;
		else { vg_bam_append_fastq(buf, off, r, out); n.kept++; }
		off += 4ull + r.block_size;
	}
	*used = off;
	return rc;
}

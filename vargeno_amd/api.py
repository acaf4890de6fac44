"""Python host mirror of the `vargeno geno` read path over the C-ABI (include/vargeno_hip.h).

The reference is one C++ function (`genotype()`, src/qv.cc:475); its stages map to:
    loader              qv.cc:519-695    -> GenoIndex.open / GenoIndex.create
    FASTQ loop body     qv.cc:760-1558   -> GenoIndex.submit / GenoIndex.process_device
    counters to caller  qv.cc:1573-1626  -> GenoIndex.counts() (+ all_reduce_counts across ranks)
PyTorch appears only as plumbing (device buffers, torch.distributed); the computation is the HIP
library.  Nothing here can run without it.
"""
from __future__ import annotations

import collections
import ctypes as C
import os
import re

import numpy as np

from . import _lib
from ._lib import VgIndexArrays, VgStats, VgTiming, check, lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class GenoIndex:
    """One device-resident index replica + its pile-up counters (one per GPU / rank)."""

    def __init__(self, handle, device):
        self._h = handle
        self.device = device
        self._stores = []                 # read stores whose batches are in flight: they must outlive the next vg_sync

    # ---- construction -------------------------------------------------------------------
    @classmethod
    def open(cls, prefix, device=0, max_device_bytes=None, sharers=1):
        """max_device_bytes: this replica's device-memory budget (vg_index_open_ex); None: vg_index_open (the whole device) --
        or, with sharers > 1 replicas on this device, an equal share of it (vg_share_budget).  vg_share_budget divides what is free
        NOW by the number of sharers: it is only the same number for every sharer when all of them ask BEFORE any of them opens --
        one process that opens its replicas itself (the command line does).  Sharers in different processes must agree on one number
        first and pass it as max_device_bytes (bench.py: every rank asks, the minimum over the ranks is everybody's budget)."""
        h = C.c_void_p()
        if max_device_bytes is None and sharers > 1:
            max_device_bytes = int(lib().vg_share_budget(device, int(sharers))) or None
        if max_device_bytes is None:
            check(lib().vg_index_open(os.fsencode(prefix), device, C.byref(h)))
        else:
            check(lib().vg_index_open_ex(os.fsencode(prefix), device, int(max_device_bytes), C.byref(h)))
        return cls(h, device)

    @property
    def plan(self):
        """What the device-memory budget bought (vg_index_plan): views kept, views left out and what each costs."""
        try:
            return lib().vg_index_plan(self._h).decode()
        except AttributeError:                                   # an older build loaded for an A/B run (VARGENO_HIP_LIB)
            return ""

    @property
    def quiet_bits(self):
        """How many entries of the merged view carry the quiet bits that let a read's pile-up walk be skipped (vg_quiet.h): a dict
        a / b / both / entries as the plan line states them, or None for a handle without direct table (nothing reads the bits).
        VG_NO_QUIET=1 leaves every bit clear: all three counts are 0."""
        m = re.search(r"quiet bits: A (\d+), B (\d+), both (\d+) of (\d+) mx entries", self.plan)
        return dict(zip(("a", "b", "both", "entries"), map(int, m.groups()))) if m else None

    @property
    def open_report(self):
        """Where the handle's start-up time went, phase by phase, and the memory it ended up with (vg_index_open_report)."""
        try:
            return lib().vg_index_open_report(self._h).decode()
        except AttributeError:                                   # an older build loaded for an A/B run (VARGENO_HIP_LIB)
            return ""

    @classmethod
    def create(cls, arrays, device=0):
        """arrays: dict as returned by vargeno_amd.index_io.read_index."""
        keep = {}

        def c(k, dt):
            keep[k] = np.ascontiguousarray(arrays[k], dtype=dt)
            return keep[k]

        a = VgIndexArrays()
        rk = c("ref_kmer", np.uint64)
        a.n_ref = len(rk)
        a.ref_kmer = rk.ctypes.data_as(_lib.u64p)
        a.ref_pos = c("ref_pos", np.uint32).ctypes.data_as(_lib.u32p)
        a.ref_amb = c("ref_amb", np.uint8).ctypes.data_as(_lib.u8p)
        rx = c("ref_aux", np.uint32)
        a.n_ref_aux = rx.size // 10
        a.ref_aux = rx.ctypes.data_as(_lib.u32p)
        sk = c("snp_kmer", np.uint64)
        a.n_snp = len(sk)
        a.snp_kmer = sk.ctypes.data_as(_lib.u64p)
        a.snp_pos = c("snp_pos", np.uint32).ctypes.data_as(_lib.u32p)
        a.snp_info = c("snp_info", np.uint8).ctypes.data_as(_lib.u8p)
        a.snp_amb = c("snp_amb", np.uint8).ctypes.data_as(_lib.u8p)
        a.snp_rf = c("snp_rf", np.uint8).ctypes.data_as(_lib.u8p)
        a.snp_af = c("snp_af", np.uint8).ctypes.data_as(_lib.u8p)
        sxp = c("snp_aux_pos", np.uint32)
        a.n_snp_aux = sxp.size // 10
        a.snp_aux_pos = sxp.ctypes.data_as(_lib.u32p)
        a.snp_aux_info = c("snp_aux_info", np.uint8).ctypes.data_as(_lib.u8p)
        a.ref_bf_bits = int(arrays["ref_bf_bits"])
        a.ref_bf_words = c("ref_bf_words", np.uint64).ctypes.data_as(_lib.u64p)
        a.snp_bf_bits = int(arrays["snp_bf_bits"])
        a.snp_bf_words = c("snp_bf_words", np.uint64).ctypes.data_as(_lib.u64p)
        h = C.c_void_p()
        check(lib().vg_index_create(C.byref(a), device, C.byref(h)))
        return cls(h, device)

    def close(self):
        if self._h:
            lib().vg_index_close(self._h)
            self._h = None
        self._pin = None
        self._stores = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- the read loop -------------------------------------------------------------------
    def submit(self, bases, quals, offsets):
        """Host batch: flat uint8 ASCII bases / quality chars, uint64 offsets[n+1]."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        quals = np.ascontiguousarray(quals, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        check(lib().vg_reads_submit(self._h, _ptr(bases), _ptr(quals), _ptr(offsets), len(offsets) - 1))

    def submit_fastq(self, text):
        """Raw FASTQ bytes (numpy uint8 / bytes): framed on the device.  Returns (records, bytes consumed, start of
        the last complete record)."""
        text = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else np.ascontiguousarray(text, dtype=np.uint8)
        n, used, last = C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(lib().vg_fastq_submit(self._h, _ptr(text), len(text), C.byref(n), C.byref(used), C.byref(last)))
        return int(n.value), int(used.value), int(last.value)

    def submit_packed(self, kmers, meta, chunk_offsets):
        """Host batch that is already framed and 2-bit packed (see HostPacker): uint64 chunk k-mers, uint64 meta words, uint64
        chunk_offsets[n+1]."""
        kmers = np.ascontiguousarray(kmers, dtype=np.uint64)
        meta = np.ascontiguousarray(meta, dtype=np.uint64)
        chunk_offsets = np.ascontiguousarray(chunk_offsets, dtype=np.uint64)
        check(lib().vg_reads_submit_packed(self._h, _ptr(kmers), _ptr(meta), _ptr(chunk_offsets), len(chunk_offsets) - 1))

    def submit_store(self, store):
        """Every batch of a ReadStore (same device) through the read loop, in push order; asynchronous (sync / counts wait)."""
        store.flush()
        check(lib().vg_reads_submit_store(self._h, store._h))
        self._stores.append(store)        # (released by sync / counts / stats / close: the batches read the store's memory until then)

    def fastq_stream(self, chunks, host_threads=None, bgzf=False, bam=False, gzip=False):
        """FASTQ text as a stream of byte chunks cut anywhere (numpy uint8 arrays / bytes; pinned host memory copies at link
        speed): records are framed across the cuts -- on the device (host_threads None or 0), or framed and 2-bit packed by
        that many host threads inside the library (-1: the library picks).  Returns (records, bytes consumed, start of the
        last framed record, refused) once everything pushed has been processed.
        bgzf=True: the chunks are BGZF bytes (cut anywhere too), inflated on the device; the offsets returned are offsets in the
        uncompressed text.  A bad block raises VgError (VG_EIO) naming its compressed offset; what was framed before it counts.
        bam=True: the chunks are a BAM file's bytes, inflated and framed on the device; records counts kept records, the offsets
        are offsets in the inflated BAM stream (bam_stats() has the stream's other counters).  A stream that ends inside the
        header or a record raises VgError (VG_EIO) naming the inflated offset.
        gzip=True: the chunks are plain gzip bytes (cut anywhere), inflated on the device by the chunked route and framed there; the
        offsets returned are text offsets, refused is also set by a refused slot (gzip_stats(), gzip_checkpoint()).  Bad data -- a
        CRC32 mismatch included -- raises VgError (VG_EIO) naming the compressed offset."""
        if gzip:
            check(lib().vg_fastq_stream_begin_gzip(self._h))
        elif bam:
            check(lib().vg_fastq_stream_begin_bam(self._h))
        elif bgzf:
            check(lib().vg_fastq_stream_begin_bgzf(self._h))
        elif host_threads is None:
            check(lib().vg_fastq_stream_begin(self._h))
        else:
            check(lib().vg_fastq_stream_begin_packed(self._h, int(host_threads)))
        for ch in chunks:
            a = np.frombuffer(ch, dtype=np.uint8) if isinstance(ch, (bytes, bytearray, memoryview)) else np.ascontiguousarray(ch, dtype=np.uint8)
            check(lib().vg_fastq_stream_push(self._h, _ptr(a), len(a)))
        n, used, last, refused = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_int()
        check(lib().vg_fastq_stream_end(self._h, C.byref(n), C.byref(used), C.byref(last), C.byref(refused)))
        return int(n.value), int(used.value), int(last.value), bool(refused.value)

    def bam_stats(self):
        """(kept, skipped by flag, skipped empty, repairs) of the handle's last BAM stream."""
        v = [C.c_uint64() for _ in range(4)]
        check(lib().vg_bam_stream_stats(self._h, *[C.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    def gzip_stats(self):
        """vg_gzip_stats of the handle's last gzip stream, as a dict."""
        from ._lib import VgGzipStats
        st = VgGzipStats()
        check(lib().vg_gzip_stream_stats(self._h, C.byref(st)))
        return st.as_dict()

    def gzip_checkpoint(self, text_offset):
        """The last slot entry of the last gzip stream at or before a text offset: (compressed bit offset, text offset, window bytes)."""
        bit, at, n = C.c_uint64(), C.c_uint64(), C.c_uint32()
        win = np.zeros(32768, dtype=np.uint8)
        check(lib().vg_fastq_stream_gzip_checkpoint(self._h, int(text_offset), C.byref(bit), C.byref(at), _ptr(win), C.byref(n)))
        return int(bit.value), int(at.value), win[:int(n.value)].tobytes()

    def bgzf_locate(self, text_offset):
        """(compressed offset of the block, offset inside its text) of an uncompressed offset of the last BGZF stream."""
        block, within = C.c_uint64(), C.c_uint32()
        check(lib().vg_fastq_stream_bgzf_locate(self._h, int(text_offset), C.byref(block), C.byref(within)))
        return int(block.value), int(within.value)

    def process_device(self, d_bases, d_quals, d_offsets, n_reads):
        """Device-resident batch: torch CUDA tensors (uint8, uint8, int64/uint64 offsets[n+1])."""
        check(lib().vg_reads_process_device(self._h, C.c_void_p(d_bases.data_ptr()), C.c_void_p(d_quals.data_ptr()),
                                            C.c_void_p(d_offsets.data_ptr()), int(n_reads)))

    def process_device_gated(self, d_bases, d_gate_words, d_offsets, n_reads):
        """Device-resident batch whose quality strings are reduced to one gate word per read (int32/uint32 tensor; bit c = quality
        character c < '8', see gate_words())."""
        check(lib().vg_reads_process_device_gated(self._h, C.c_void_p(d_bases.data_ptr()), C.c_void_p(d_gate_words.data_ptr()),
                                                  C.c_void_p(d_offsets.data_ptr()), int(n_reads)))

    def sync(self):
        check(lib().vg_sync(self._h))
        self._stores = []

    def set_stats(self, enable):
        check(lib().vg_set_stats(self._h, 1 if enable else 0))

    def stats(self):
        s = VgStats()
        check(lib().vg_stats_get(self._h, C.byref(s)))
        return s.as_dict()

    def timing(self):
        t = VgTiming()
        check(lib().vg_timing_get(self._h, C.byref(t)))
        return dict(ms_total=float(t.ms_total), ms_pack=float(t.ms_pack), ms_main=float(t.ms_main), ms_tail=float(t.ms_tail), ms_deep_lists=float(t.ms_deep_lists), batches=int(t.batches))

    @property
    def held_passes(self):
        """Passes the main wave tier held back for a later iteration's stage B since open / reset (vg_held_passes; sync() first).
        Says how the kernel scheduled its work, never what it computed."""
        fn = getattr(lib(), "vg_held_passes", None)
        if fn is None:
            raise RuntimeError("the library named by VARGENO_HIP_LIB predates vg_held_passes")
        return int(fn(self._h))

    # ---- results -------------------------------------------------------------------------
    @property
    def num_sites(self):
        return int(lib().vg_num_sites(self._h))

    @property
    def device_bytes(self):
        return int(lib().vg_index_device_bytes(self._h))

    VIEW_NAMES = {1: "sec", 2: "mx", 4: "dx", 8: "snp_probe", 16: "snp_jg32", 32: "hx", 64: "snp_sig", 128: "sec_is_bf", 256: "ssec"}

    @property
    def views(self):
        """Names of the optional re-laid-out views this handle holds (vg_index_views): they change speed, never results."""
        m = int(lib().vg_index_views(self._h))
        return [n for b, n in sorted(self.VIEW_NAMES.items()) if m & b]

    def sites(self):
        n = self.num_sites
        pos = np.empty(n, np.uint32)
        u8 = [np.empty(n, np.uint8) for _ in range(4)]
        check(lib().vg_sites_fetch(self._h, _ptr(pos), *[_ptr(x) for x in u8]))
        return dict(pos=pos, ref_base=u8[0], alt_base=u8[1], ref_freq=u8[2], alt_freq=u8[3])

    # ---- sample planes: several samples against one resident index (vg_samples_reserve ...) ----------------------
    def reserve_samples(self, n):
        """Grow the handle to n sample planes (24 bytes of device memory per site each); existing planes keep their counts."""
        check(lib().vg_samples_reserve(self._h, int(n)))

    @property
    def num_samples(self):
        return int(lib().vg_num_samples(self._h))

    @property
    def selected(self):
        return int(lib().vg_sample_selected(self._h))

    def select(self, s):
        """The sample that the batches submitted from now on count into, and that counts() / the all-reduces act on.  No
        synchronisation: batches of different samples are in flight together."""
        check(lib().vg_sample_select(self._h, int(s)))

    def reset_sample(self, s):
        check(lib().vg_sample_reset(self._h, int(s)))

    def invalid_reads(self, s):
        """Reads of sample s that the reference would have aborted on."""
        n = C.c_uint64()
        check(lib().vg_sample_invalid_reads(self._h, int(s), C.byref(n)))
        return int(n.value)

    def counts(self, copy=True, sample=None):
        """Clamped counters (ref, alt) of the selected sample, or of `sample` (the selection is restored).  copy=False: views of a
        page-locked buffer that the next call overwrites (the device-to-host
        copy then runs at link speed instead of through the runtime's pageable staging: bench.py's timed fetch)."""
        if sample is not None:
            before = self.selected
            self.select(sample)
            try:
                return self.counts(copy=copy)
            finally:
                self.select(before)
        n = self.num_sites
        if copy:
            r, a = np.empty(n, np.uint8), np.empty(n, np.uint8)
            check(lib().vg_counts_fetch(self._h, _ptr(r), _ptr(a)))
            return r, a
        if getattr(self, "_pin", None) is None or len(self._pin[0]) != 2 * n:
            self._pin = pinned_buffer(max(2 * n, 1))
        buf = self._pin[0]
        check(lib().vg_counts_fetch(self._h, _ptr(buf[:n]), _ptr(buf[n:])))
        return buf[:n], buf[n:2 * n]

    def calls(self, sample=None):
        """The genotype calls (gt, gq) of the selected sample, or of `sample` (the selection is restored), computed on the device
        from its counters: gt uint8 in the reference's numbering (0 not called, 1 hom-ref, 2 hom-alt, 3 het), gq int32 as the
        reference prints it (0 where gt is 0).  `last_escaped` is the number of sites the host had to recompute."""
        if sample is not None:
            before = self.selected
            self.select(sample)
            try:
                return self.calls()
            finally:
                self.select(before)
        n = self.num_sites
        gt, gq, esc = np.empty(n, np.uint8), np.empty(n, np.int32), C.c_uint64()
        check(lib().vg_sample_calls_fetch(self._h, _ptr(gt), _ptr(gq), C.byref(esc)))
        self.last_escaped = int(esc.value)
        return gt, gq

    def reset(self):
        check(lib().vg_counts_reset(self._h))

    def counts_device(self):
        p, n = C.c_void_p(), C.c_uint64()
        check(lib().vg_counts_device_ptr(self._h, C.byref(p), C.byref(n)))
        return int(p.value or 0), int(n.value)

    def counts_tensor(self):
        """The device counter array as a torch int32 tensor aliasing the library's memory (a u32 sum
        and an i32 sum are the same bits), for torch.distributed.all_reduce over RCCL."""
        import torch

        ptr, n = self.counts_device()

        class _Alias:
            __cuda_array_interface__ = {"shape": (n,), "typestr": "<i4", "data": (ptr, False), "version": 2, "strides": None}

        return torch.as_tensor(_Alias(), device="cuda:%d" % self.device)


class HostPacker:
    """The host-side FASTQ framing + 2-bit packing of the library on its own (vg_packer_*: no device involved)."""

    def __init__(self, threads=1):
        self._h = C.c_void_p()
        check(lib().vg_packer_create(int(threads), C.byref(self._h)))

    def close(self):
        if self._h:
            lib().vg_packer_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def begin(self):
        check(lib().vg_packer_begin(self._h))

    def push(self, text):
        """-> (kmers uint64[chunks], meta uint64[n], chunk_offsets uint64[n+1], n_invalid) of the complete records framed."""
        a = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else np.ascontiguousarray(text, dtype=np.uint8)
        rc_, kc_ = int(lib().vg_packer_reads_cap(len(a))), int(lib().vg_packer_kmers_cap(len(a)))
        kmers, meta, offs = np.zeros(kc_, np.uint64), np.zeros(rc_, np.uint64), np.zeros(rc_ + 1, np.uint64)
        n, nc, bad = C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(lib().vg_packer_push(self._h, _ptr(a), len(a), _ptr(kmers), kc_, _ptr(meta), _ptr(offs), rc_, C.byref(n), C.byref(nc), C.byref(bad)))
        return kmers[:nc.value].copy(), meta[:n.value].copy(), offs[:n.value + 1].copy(), int(bad.value)

    def end(self):
        """-> (records, bytes consumed, start of the last framed record, refused)"""
        n, used, last, refused = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_int()
        check(lib().vg_packer_end(self._h, C.byref(n), C.byref(used), C.byref(last), C.byref(refused)))
        return int(n.value), int(used.value), int(last.value), bool(refused.value)


class ReadStore:
    """Packed batches parked in device memory before an index handle exists (vg_read_store_*): what the command line packs while
    vg_index_open runs.  `GenoIndex.submit_store(store)` runs them through an open handle on the same device."""

    def __init__(self, device=0, max_bytes=1 << 30):
        self._h = C.c_void_p()
        self._keep = None
        check(lib().vg_read_store_create(int(device), int(max_bytes), C.byref(self._h)))

    def push(self, kmers, meta, chunk_offsets):
        kmers = np.ascontiguousarray(kmers, dtype=np.uint64)
        meta = np.ascontiguousarray(meta, dtype=np.uint64)
        chunk_offsets = np.ascontiguousarray(chunk_offsets, dtype=np.uint64)
        check(lib().vg_read_store_push(self._h, _ptr(kmers), _ptr(meta), _ptr(chunk_offsets), len(chunk_offsets) - 1))
        self._keep = (kmers, meta, chunk_offsets)          # untouched until the next push / flush returns

    def flush(self):
        check(lib().vg_read_store_flush(self._h))
        self._keep = None

    @property
    def reads(self):
        return int(lib().vg_read_store_reads(self._h))

    @property
    def bytes_used(self):
        return int(lib().vg_read_store_bytes_used(self._h))

    def close(self):
        if self._h:
            lib().vg_read_store_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _u8(data):
    return np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8)


def bgzf_scan(data):
    """The BGZF header walk (host): ([(compressed offset, text offset, payload offset, payload length, ISIZE, CRC32), ...] of the
    whole blocks, bytes consumed, compressed offset of bytes that are no BGZF header or None)."""
    a = _u8(data)
    cap = len(a) // 20 + 1                                     # a block is at least 20 bytes
    tab = np.zeros(6 * cap, dtype=np.uint64)
    n, used, bad = C.c_uint64(), C.c_uint64(), C.c_uint64()
    check(lib().vg_bgzf_scan_host(_ptr(a), len(a), _ptr(tab), cap, C.byref(n), C.byref(used), C.byref(bad)))
    blocks = [tuple(int(v) for v in tab[6 * i:6 * i + 6]) for i in range(int(n.value))]
    return blocks, int(used.value), (None if bad.value == 2 ** 64 - 1 else int(bad.value))


def bgzf_inflate(data, device=0, out=None, text_cap=None):
    """The whole BGZF blocks of `data` inflated: on `device` by the stream's kernel, or (device=None) by the host build of the
    same decoder.  Returns (text as bytes, compressed bytes consumed, compressed offset of the first bad block or None); the
    text stops before a bad block.  out / text_cap: a caller's uint8 buffer and how much of it may be written (default: a new
    buffer of the blocks' ISIZE sum)."""
    a = _u8(data)
    if text_cap is None:
        text_cap = sum(b[4] for b in bgzf_scan(a)[0]) if out is None else len(out)
    if out is None:
        out = np.zeros(max(1, text_cap), dtype=np.uint8)
    n, used, bad = C.c_uint64(), C.c_uint64(), C.c_uint64()
    if device is None:
        check(lib().vg_bgzf_inflate_host(_ptr(a), len(a), _ptr(out), int(text_cap), C.byref(n), C.byref(used), C.byref(bad)))
    else:
        check(lib().vg_bgzf_inflate_device(int(device), _ptr(a), len(a), _ptr(out), int(text_cap), C.byref(n), C.byref(used), C.byref(bad)))
    return out[:int(n.value)].tobytes(), int(used.value), (None if bad.value == 2 ** 64 - 1 else int(bad.value))


DEFLATE_CODES = {"fixed": 0, "dynamic": 1}                     # VG_DEFLATE_FIXED, VG_DEFLATE_DYNAMIC


class VcfIndexRefused(ValueError):
    """A data line of the VCF breaks one of the index's rules (csrc/vg_vcfidx.h): .rule names it, .offset is the line's offset in
    the text."""

    def __init__(self, rule, offset):
        super().__init__("the VCF cannot be indexed: %s (the line at text offset %d)" % (rule, offset))
        self.rule, self.offset = rule, offset


class VcfIndex:
    """The streaming handle behind a .tbi (vg_vcfidx_*): VCF text in pieces cut anywhere (text), the file's BGZF blocks as they are
    made (bgzf), then the raw index bytes (finish); a refused index raises VcfIndexRefused there."""

    def __init__(self, block=0):
        self._h = None
        h = C.c_void_p()
        check(lib().vg_vcfidx_create(int(block), C.byref(h)))
        self._h = h

    def close(self):
        if self._h:
            lib().vg_vcfidx_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def text(self, data, device=None, threads=1):
        a = _u8(data)
        self._text_at(a.ctypes.data, len(a), device, threads)

    def _text_at(self, address, n, device, threads):
        if device is None:
            check(lib().vg_vcfidx_text_host(self._h, C.c_void_p(address), n, int(threads)))
        else:
            check(lib().vg_vcfidx_text_device(self._h, int(device), C.c_void_p(address), n))

    def bgzf(self, data):
        a = _u8(data)
        check(lib().vg_vcfidx_bgzf(self._h, _ptr(a), len(a)))

    def error(self):
        """None, or (rule, offset) of the data line that refused the index."""
        at = C.c_uint64()
        rule = lib().vg_vcfidx_error(self._h, C.byref(at))
        return None if rule is None else (rule.decode(), int(at.value))

    def stats(self):
        out = np.zeros(5, dtype=np.uint64)
        check(lib().vg_vcfidx_stats(self._h, _ptr(out)))
        return dict(zip(("data_lines", "chromosomes", "bins", "chunks", "scan_us"), (int(v) for v in out)))

    def finish(self):
        """The raw index bytes (the .tbi file is bgzf_deflate of them)."""
        cap = int(lib().vg_vcfidx_bound(self._h))
        out = np.zeros(max(1, cap), dtype=np.uint8)
        n = C.c_uint64()
        rc = lib().vg_vcfidx_finish(self._h, _ptr(out), cap, C.byref(n))
        err = self.error()
        if err is not None:
            raise VcfIndexRefused(*err)
        check(rc)
        return out[:int(n.value)].tobytes()


def vcf_index(text, block=0, device=None, pieces=None, threads=1):
    """The raw tabix index bytes of `text` written as BGZF with `block` text bytes per block (csrc/vg_vcfidx.h has the rules).
    device=None: the host scanner on `threads` threads; else the scan kernels on that device.  pieces: ascending cut points of the
    streaming feed (the text goes in as text[0:c0], text[c0:c1], ...).  Raises VcfIndexRefused (rule, offset) when a data line breaks
    a rule."""
    a = _u8(text)
    cuts = [0] + [int(c) for c in (pieces or [])] + [len(a)]
    with VcfIndex(block) as ix:
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            if not 0 <= lo <= hi <= len(a):
                raise ValueError("pieces are ascending offsets into the text")
            if hi > lo:
                ix._text_at(a.ctypes.data + lo, hi - lo, device, threads)
        ix.bgzf(bgzf_deflate(a, block=block))
        return ix.finish()


def bgzf_deflate(text, device=None, block=0, eof=True, threads=None, codes="fixed", index=False):
    """`text` written as BGZF (vg_bgzf_deflate_*_coded): on `device` by the deflate kernel, or (device=None) by the host build of the
    same compressor on `threads` threads (default: the CPUs of this process, at most 16).  block: text bytes per block, 0 = 65 280;
    eof: append the empty end-of-file block.  codes: "fixed" (fixed Huffman codes) or "dynamic" (per block the smallest of stored,
    fixed and dynamic codes); anything else is a ValueError.  The bytes depend on the text, `block` and `codes` alone.  Returns bytes.
    index=True (a device is needed): the fused call, vg_bgzf_deflate_device_indexed -- the text is a VCF and is scanned while it is
    resident; returns (bgzf, raw tabix index bytes) or raises VcfIndexRefused."""
    if not isinstance(codes, str) or codes not in DEFLATE_CODES:
        raise ValueError("codes is \"fixed\" or \"dynamic\", not %r" % (codes,))
    mode = DEFLATE_CODES[codes]
    a = _u8(text)
    cap = int(lib().vg_bgzf_deflate_bound(len(a), int(block)))
    out = np.zeros(max(1, cap), dtype=np.uint8)
    n = C.c_uint64()
    if index:
        if device is None:
            raise ValueError("bgzf_deflate(index=True) is the fused device call: name a device (vcf_index is the host's scanner)")
        with VcfIndex(block) as ix:
            check(lib().vg_bgzf_deflate_device_indexed(int(device), _ptr(a), len(a), int(block), int(bool(eof)), mode, ix._h, _ptr(out), cap, C.byref(n)))
            return out[:int(n.value)].tobytes(), ix.finish()
    if device is None:
        if threads is None:
            threads = min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1))
        check(lib().vg_bgzf_deflate_host_coded(_ptr(a), len(a), int(block), int(bool(eof)), int(threads), mode, _ptr(out), cap, C.byref(n)))
    else:
        check(lib().vg_bgzf_deflate_device_coded(int(device), _ptr(a), len(a), int(block), int(bool(eof)), mode, _ptr(out), cap, C.byref(n)))
    return out[:int(n.value)].tobytes()


def deflate_code_lengths(freq, limit=15, device=None):
    """Huffman code lengths, none above `limit`, of the histograms freq[n_sets, n_sym] (or one histogram freq[n_sym]) of unsigned
    counts (vg_deflate_code_lengths_*): on `device` one wave per histogram, or (device=None) on the host; the same lengths either
    way.  2 <= n_sym <= 288, n_sym <= 2 ** limit <= 2 ** 15.  Returns a uint8 array of freq's shape."""
    f = np.ascontiguousarray(freq, dtype=np.uint32)
    if f.ndim not in (1, 2):
        raise ValueError("freq is [n_sym] or [n_sets, n_sym]")
    f2 = f.reshape(-1, f.shape[-1])
    lens = np.zeros(f2.shape, dtype=np.uint8)
    if device is None:
        check(lib().vg_deflate_code_lengths_host(_ptr(f2), f2.shape[0], f2.shape[1], int(limit), _ptr(lens)))
    else:
        check(lib().vg_deflate_code_lengths_device(int(device), _ptr(f2), f2.shape[0], f2.shape[1], int(limit), _ptr(lens)))
    return lens.reshape(f.shape)


class GunzipResult(collections.namedtuple("GunzipResult", "text consumed bad_offset stats error")):
    """text: the bytes of the members decoded whole and verified; consumed: compressed bytes up to there; bad_offset / error: the
    compressed offset and the library's message when the data is bad (None otherwise); stats: vg_gzip_stats as a dict (chunked
    routes; None for the sequential decoder)."""


def gunzip(data, device=0, chunked=False, text_cap=None, chunk=None, slot=None, ratio=None, slot_max=None, push=None):
    """Plain gzip (RFC 1952, any number of members) inflated: on `device` by the chunked kernels, or (device=None) on the host --
    by the sequential reference decoder, or with chunked=True by the same chunked stages the kernels run.  chunk / slot / ratio /
    slot_max: the sizes of this call, passed as vg_gzip_opts (one left None is the environment's VG_GZ_CHUNK / VG_GZ_SLOT /
    VG_GZ_MAX_RATIO / VG_GZ_SLOT_MAX, or the default).  text_cap: room for the
    text (default 16 bytes per compressed byte + 64 KiB).  Returns a GunzipResult; bad data is reported in it, not raised."""
    from ._lib import VgGzipOpts, VgGzipStats

    a = _u8(data)
    if text_cap is None:
        text_cap = 16 * len(a) + 65536
    out = np.zeros(max(1, int(text_cap)), dtype=np.uint8)
    n, used, bad = C.c_uint64(), C.c_uint64(), C.c_uint64()
    st = VgGzipStats()
    op = VgGzipOpts(*[int(v or 0) for v in (chunk, slot, ratio, slot_max)])
    if push is not None:                                       # (host only: the push driver over the host stages, `push` bytes at a time)
        rc = lib().vg_gunzip_pushed_host(_ptr(a), len(a), int(push), _ptr(out), int(text_cap), C.byref(n), C.byref(used), C.byref(bad), C.byref(st), C.byref(op))
    elif device is not None:
        rc = lib().vg_gunzip_device(int(device), _ptr(a), len(a), _ptr(out), int(text_cap), C.byref(n), C.byref(used), C.byref(bad), C.byref(st), C.byref(op))
    elif chunked:
        rc = lib().vg_gunzip_chunked_host(_ptr(a), len(a), _ptr(out), int(text_cap), C.byref(n), C.byref(used), C.byref(bad), C.byref(st), C.byref(op))
    else:
        rc = lib().vg_gunzip_host(_ptr(a), len(a), _ptr(out), int(text_cap), C.byref(n), C.byref(used), C.byref(bad))
    error = None
    if rc == -2:                                               # VG_EIO: bad data
        error = lib().vg_last_error().decode()
    else:
        check(rc)
    stats = st.as_dict() if (device is not None or chunked or push is not None) else None
    return GunzipResult(out[:int(n.value)].tobytes(), int(used.value), (None if bad.value == 2 ** 64 - 1 else int(bad.value)), stats, error)


def bam_to_fastq(data):
    """The equivalent FASTQ text of a BAM file's bytes, by the host build of the record parser (no device): (text as bytes, records
    converted, inflated offset where conversion stopped or None when the whole stream was converted).  Raises VgError (VG_EIO) when
    the bytes are not BAM."""
    a = _u8(data)
    cap = 64 + 3 * sum(b[4] for b in bgzf_scan(a)[0])          # a record's text: name + 2 characters per base + 7, from >= 37 + name + 1.5 bytes per base
    out = np.zeros(cap, dtype=np.uint8)
    n, recs, bad = C.c_uint64(), C.c_uint64(), C.c_uint64()
    check(lib().vg_bam_to_fastq_host(_ptr(a), len(a), _ptr(out), cap, C.byref(n), C.byref(recs), C.byref(bad)))
    return out[:int(n.value)].tobytes(), int(recs.value), (None if bad.value == 2 ** 64 - 1 else int(bad.value))


def bam_frame(data, device=0):
    """A BAM file's bytes framed on `device` by the stream's kernels, as one slot: (offsets uint64[n + 1], bases uint8, gate words
    uint32[n], (kept, skipped by flag, skipped empty, repairs), inflated offset of the first byte not framed or None)."""
    a = _u8(data)
    text_n = sum(b[4] for b in bgzf_scan(a)[0])
    cap_rec, cap_bases = text_n // 36 + 2, text_n // 3 * 2 + 64
    offsets = np.zeros(cap_rec + 1, dtype=np.uint64)
    bases = np.zeros(cap_bases, dtype=np.uint8)
    gate = np.zeros(cap_rec, dtype=np.uint32)
    stats = np.zeros(4, dtype=np.uint64)
    n, bad = C.c_uint64(), C.c_uint64()
    check(lib().vg_bam_frame_device(int(device), _ptr(a), len(a), _ptr(offsets), cap_rec, _ptr(bases), cap_bases, _ptr(gate), C.byref(n), _ptr(stats), C.byref(bad)))
    k = int(n.value)
    return offsets[:k + 1].copy(), bases[:int(offsets[k])].copy(), gate[:k].copy(), tuple(int(v) for v in stats), (None if bad.value == 2 ** 64 - 1 else int(bad.value))


# the caller kernel's launch: lanes per block, and the most blocks of a grid (a longer array wraps round the grid-stride loop)
CALL_BLOCK, CALL_MAX_GRID = 256, 4096


def call_device(ref_cnt, alt_cnt, ref_freq, alt_freq, device=0, guard=0.0):
    """The caller kernel over flat arrays (no index): (gt, gq, n_escaped) for the quadruples (counters are clamped at 63, frequencies
    are the dictionary's n/255 bytes).  gt / gq are final, as GenoIndex.calls() returns them; n_escaped counts the entries the
    kernel left to the host (guard: how close to an integer -10 ln(confidence) may lie before it does; <= 0: the default, 1e-6)."""
    cols = [np.ascontiguousarray(a, dtype=np.uint8) for a in (ref_cnt, alt_cnt, ref_freq, alt_freq)]
    n = len(cols[0])
    if any(len(c) != n for c in cols):
        raise ValueError("call_device: four arrays of one length")
    gt, gq, esc = np.empty(n, np.uint8), np.empty(n, np.int32), C.c_uint64()
    check(lib().vg_call_device(int(device), _ptr(cols[0]), _ptr(cols[1]), _ptr(cols[2]), _ptr(cols[3]), n, float(guard), _ptr(gt), _ptr(gq), C.byref(esc)))
    return gt, gq, int(esc.value)


# the pair kernel's launch: a workgroup owns a PAIR_TILE x PAIR_TILE tile of sample pairs and, unless the caller says otherwise,
# PAIR_WORDS_DEFAULT 64-site words; counts[i, j] = (n, ibs0, ibs2, hethet, het_i), PAIR_COUNTERS of them
PAIR_TILE, PAIR_WORDS_DEFAULT, PAIR_COUNTERS, PAIR_MAX_SAMPLES = 32, 1024, 5, 16384


class GenotypeMatrix:
    """The calls of a cohort as bit planes on a device (vg_gmatrix_*), and the pairwise sample table over them."""

    def __init__(self, n_sites, n_samples, device=0):
        self._h = None
        self.n_sites, self.n_samples = int(n_sites), int(n_samples)
        if self.n_sites < 0 or self.n_samples < 0:
            raise ValueError("GenotypeMatrix: negative size")
        h = C.c_void_p()
        check(lib().vg_gmatrix_create(int(device), self.n_sites, min(self.n_samples, 2 ** 32 - 1), C.byref(h)))
        self._h = h

    def close(self):
        if self._h:
            lib().vg_gmatrix_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def device_bytes(self):
        return int(lib().vg_gmatrix_device_bytes(self._h))

    def set(self, sample, gt, gq, min_gq=0):
        """One sample's final calls (as GenoIndex.calls() returns them); a call counts iff gt != 0 and gq >= min_gq."""
        gt = np.ascontiguousarray(gt, dtype=np.uint8)
        gq = np.ascontiguousarray(gq, dtype=np.int32)
        if gt.shape != (self.n_sites,) or gq.shape != (self.n_sites,):
            raise ValueError("GenotypeMatrix.set: gt and gq hold one entry per site")
        if not 0 <= int(sample) < 2 ** 32:
            raise ValueError("GenotypeMatrix.set: sample out of range")
        check(lib().vg_gmatrix_set(self._h, int(sample), _ptr(gt), _ptr(gq), int(min_gq)))

    def pairs(self, words_per_block=0):
        """uint64[N, N, 5]: (n, ibs0, ibs2, hethet, het_i) of every ordered pair of samples."""
        out = np.empty((self.n_samples, self.n_samples, PAIR_COUNTERS), dtype=np.uint64)
        check(lib().vg_gmatrix_pairs(self._h, int(words_per_block), _ptr(out)))
        return out


def pairs_host(gt, gq, min_gq=0, threads=1):
    """The same table by the host loop (vg_pairs_host; no device): gt, gq are [n_samples, n_sites]."""
    gt = np.ascontiguousarray(gt, dtype=np.uint8)
    gq = np.ascontiguousarray(gq, dtype=np.int32)
    if gt.ndim != 2 or gt.shape != gq.shape:
        raise ValueError("pairs_host: gt and gq are [n_samples, n_sites]")
    out = np.empty((gt.shape[0], gt.shape[0], PAIR_COUNTERS), dtype=np.uint64)
    check(lib().vg_pairs_host(_ptr(gt), _ptr(gq), gt.shape[1], gt.shape[0], int(min_gq), int(threads), _ptr(out)))
    return out


# the cohort prior's defaults and limits (csrc/vg_cprior.h), its kernel's launch, and the device bytes of a handle beside its
# 4 * n_samples * n_sites + 12 * n_sites: the caller's factor tables and the escape count
CPRIOR_ITERS, CPRIOR_PSEUDO, CPRIOR_MAX_ITERS, CPRIOR_MAX_SAMPLES = 8, 2.0, 64, 16384
CPRIOR_BLOCK, CPRIOR_MAX_GRID, CPRIOR_FIXED_BYTES = 256, 8192, 5104 + 8


class CohortPrior:
    """The counters of a cohort on a device (vg_cprior_*): every sample called again with the allele frequency the cohort itself
    shows at each site, in place of the dictionary's."""

    def __init__(self, n_sites, n_samples, device=0):
        self._h = None
        self.n_sites, self.n_samples = int(n_sites), int(n_samples)
        if self.n_sites < 0 or self.n_samples < 0:
            raise ValueError("CohortPrior: negative size")
        h = C.c_void_p()
        check(lib().vg_cprior_create(int(device), self.n_sites, min(self.n_samples, 2 ** 32 - 1), C.byref(h)))
        self._h = h
        self.n_escaped = 0

    def close(self):
        if self._h:
            lib().vg_cprior_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def device_bytes(self):
        return int(lib().vg_cprior_device_bytes(self._h))

    def set(self, sample, ref_cnt, alt_cnt):
        """One sample's counters (as GenoIndex.counts() returns them; clamped again at 63)."""
        ref_cnt = np.ascontiguousarray(ref_cnt, dtype=np.uint8)
        alt_cnt = np.ascontiguousarray(alt_cnt, dtype=np.uint8)
        if ref_cnt.shape != (self.n_sites,) or alt_cnt.shape != (self.n_sites,):
            raise ValueError("CohortPrior.set: ref_cnt and alt_cnt hold one entry per site")
        if not 0 <= int(sample) < 2 ** 32:
            raise ValueError("CohortPrior.set: sample out of range")
        check(lib().vg_cprior_set(self._h, int(sample), _ptr(ref_cnt), _ptr(alt_cnt)))

    def run(self, ref_freq, alt_freq, iters=CPRIOR_ITERS, pseudo=CPRIOR_PSEUDO, guard=0):
        """The kernel over the samples set so far: float64[n_sites], the sites' final q.  ref_freq, alt_freq: the dictionary's n/255
        bytes.  n_escaped then holds the entries the kernel left to the host (guard as call_device's)."""
        ref_freq = np.ascontiguousarray(ref_freq, dtype=np.uint8)
        alt_freq = np.ascontiguousarray(alt_freq, dtype=np.uint8)
        if ref_freq.shape != (self.n_sites,) or alt_freq.shape != (self.n_sites,):
            raise ValueError("CohortPrior.run: ref_freq and alt_freq hold one entry per site")
        q, esc = np.empty(self.n_sites, np.float64), C.c_uint64()
        check(lib().vg_cprior_run(self._h, _ptr(ref_freq), _ptr(alt_freq), int(iters), float(pseudo), float(guard), _ptr(q), C.byref(esc)))
        self.n_escaped = int(esc.value)
        return q

    def calls(self, sample):
        """(gt, gq) of one sample after run(): final, as GenoIndex.calls() returns them."""
        if not 0 <= int(sample) < 2 ** 32:
            raise ValueError("CohortPrior.calls: sample out of range")
        gt, gq = np.empty(self.n_sites, np.uint8), np.empty(self.n_sites, np.int32)
        check(lib().vg_cprior_calls(self._h, int(sample), _ptr(gt), _ptr(gq)))
        return gt, gq


def cohort_prior_host(ref_cnt, alt_cnt, ref_freq, alt_freq, iters=CPRIOR_ITERS, pseudo=CPRIOR_PSEUDO, threads=1):
    """The same by the host loop (vg_cprior_host; no device): ref_cnt, alt_cnt are [n_samples, n_sites]; returns (gt, gq, q) with gt,
    gq of that shape and q float64[n_sites]."""
    ref_cnt = np.ascontiguousarray(ref_cnt, dtype=np.uint8)
    alt_cnt = np.ascontiguousarray(alt_cnt, dtype=np.uint8)
    ref_freq = np.ascontiguousarray(ref_freq, dtype=np.uint8)
    alt_freq = np.ascontiguousarray(alt_freq, dtype=np.uint8)
    if ref_cnt.ndim != 2 or ref_cnt.shape != alt_cnt.shape:
        raise ValueError("cohort_prior_host: ref_cnt and alt_cnt are [n_samples, n_sites]")
    n_samples, n_sites = ref_cnt.shape
    if ref_freq.shape != (n_sites,) or alt_freq.shape != (n_sites,):
        raise ValueError("cohort_prior_host: ref_freq and alt_freq hold one entry per site")
    gt, gq, q = np.empty((n_samples, n_sites), np.uint8), np.empty((n_samples, n_sites), np.int32), np.empty(n_sites, np.float64)
    check(lib().vg_cprior_host(_ptr(ref_cnt), _ptr(alt_cnt), n_sites, n_samples, _ptr(ref_freq), _ptr(alt_freq), int(iters), float(pseudo), int(threads), _ptr(gt), _ptr(gq), _ptr(q)))
    return gt, gq, q


# vg_jtext_record: a data line of the joint VCF -- its first eight fields in `heads` and its run of site indices in `sites`
JTEXT_RECORD = np.dtype([("head_off", "<u8"), ("site_at", "<u8"), ("head_len", "<u4"), ("n_sites", "<u4")])


def jtext_records(rows):
    """[(head_off, head_len, site_at, n_sites), ...] (or an array of JTEXT_RECORD) as the array the joint text calls take."""
    if isinstance(rows, np.ndarray) and rows.dtype == JTEXT_RECORD:
        return np.ascontiguousarray(rows)
    a = np.zeros(len(rows), dtype=JTEXT_RECORD)
    for i, (head_off, head_len, site_at, n_sites) in enumerate(rows):
        a[i] = (head_off, site_at, head_len, n_sites)
    return a


def _jtext_span(heads, records, sites):
    return _u8(heads), jtext_records(records), np.ascontiguousarray(sites, dtype=np.uint32)


JT_INFO_NONE, JT_INFO_COUNTS = 0, 1


def jtext_text_bound(head_bytes, n_records, n_samples, info=False):
    """Bytes the text of a span never exceeds: head_bytes + n_records * (7 + 16 * n_samples); info: and 40 bytes per record for
    the NS / AN / AC / AF of the INFO mode."""
    if not info:
        return int(lib().vg_jtext_text_bound(int(head_bytes), int(n_records), int(n_samples)))
    return int(lib().vg_jtext_text_bound_info(int(head_bytes), int(n_records), int(n_samples), JT_INFO_COUNTS))


def jtext_bgzf_bound(text_bytes, block=0):
    """Bytes of BGZF a call of the joint text stream that adds text_bytes of text never exceeds."""
    return int(lib().vg_jtext_bgzf_bound(int(text_bytes), int(block)))


class JointText:
    """The calls of a cohort in columns on a device (vg_jtext_*), and the data lines of the joint VCF rendered from them: as plain
    bytes (render) or joined to a BGZF stream that leaves the device compressed (bgzf_begin / bgzf_text / bgzf_lines / bgzf_end; the
    handle must be made with bgzf=True).  max_records, max_head_bytes, max_site_refs: the largest span a call may take;
    wide_samples: samples that may hold a gq outside 0 .. 16382 (default: all).  info=True: every line's INFO carries the record's
    NS / AN / AC / AF (vg_jtext_create_info with VG_JT_INFO_COUNTS), in render and in the stream alike."""

    def __init__(self, n_sites, n_samples, device=0, max_records=1 << 16, max_head_bytes=1 << 22, max_site_refs=1 << 18, wide_samples=None, bgzf=False, info=False):
        self._h = None
        self.info = bool(info)
        self.n_sites, self.n_samples = int(n_sites), int(n_samples)
        if self.n_sites < 0 or self.n_samples < 0:
            raise ValueError("JointText: negative size")
        self._block = 0
        h = C.c_void_p()
        wide = self.n_samples if wide_samples is None else int(wide_samples)
        sizes = (int(device), self.n_sites, min(self.n_samples, 2 ** 32 - 1), min(wide, 2 ** 32 - 1), int(max_records), int(max_head_bytes), int(max_site_refs), int(bool(bgzf)))
        if self.info:
            check(lib().vg_jtext_create_info(*sizes, JT_INFO_COUNTS, C.byref(h)))
        else:
            check(lib().vg_jtext_create(*sizes, C.byref(h)))
        self._h = h

    def close(self):
        if self._h:
            lib().vg_jtext_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def device_bytes(self):
        return int(lib().vg_jtext_device_bytes(self._h))

    def set(self, sample, gt, gq):
        """One sample's final calls (as GenoIndex.calls() returns them)."""
        gt = np.ascontiguousarray(gt, dtype=np.uint8)
        gq = np.ascontiguousarray(gq, dtype=np.int32)
        if gt.shape != (self.n_sites,) or gq.shape != (self.n_sites,):
            raise ValueError("JointText.set: gt and gq hold one entry per site")
        if not 0 <= int(sample) < 2 ** 32:
            raise ValueError("JointText.set: sample out of range")
        check(lib().vg_jtext_set(self._h, int(sample), _ptr(gt), _ptr(gq)))

    def render(self, heads, records, sites, with_lines=False):
        """The text of a span as bytes (with_lines: and the number of records that produced a line)."""
        h, r, s = _jtext_span(heads, records, sites)
        cap = jtext_text_bound(int(r["head_len"].sum(dtype=np.uint64)), len(r), self.n_samples, self.info)
        out = np.zeros(max(1, cap), dtype=np.uint8)
        n, lines = C.c_uint64(), C.c_uint64()
        check(lib().vg_jtext_render(self._h, _ptr(h), len(h), _ptr(r), len(r), _ptr(s), len(s), _ptr(out), cap, C.byref(n), C.byref(lines)))
        text = out[:int(n.value)].tobytes()
        return (text, int(lines.value)) if with_lines else text

    def counts(self, heads, records, sites):
        """uint32[n_records, 3]: NS, het, hom of every record over the calls its line shows -- zeros for a record that produces no
        line -- without the text (vg_jtext_counts; heads is not read).  Works on a handle of either mode."""
        _, r, s = _jtext_span(heads, records, sites)
        out = np.zeros((len(r), 3), dtype=np.uint32)
        check(lib().vg_jtext_counts(self._h, _ptr(r), len(r), _ptr(s), len(s), _ptr(out)))
        return out

    def bgzf_begin(self, block=0, codes="fixed"):
        if not isinstance(codes, str) or codes not in DEFLATE_CODES:
            raise ValueError("codes is \"fixed\" or \"dynamic\", not %r" % (codes,))
        check(lib().vg_jtext_bgzf_begin(self._h, int(block), DEFLATE_CODES[codes]))
        self._block = int(block)
        self._index = None

    def bgzf_text(self, text):
        """Host bytes joined to the stream; returns the BGZF blocks the call completed."""
        a = _u8(text)
        cap = jtext_bgzf_bound(len(a), self._block)
        out = np.zeros(max(1, cap), dtype=np.uint8)
        n = C.c_uint64()
        check(lib().vg_jtext_bgzf_text(self._h, _ptr(a), len(a), _ptr(out), cap, C.byref(n)))
        return out[:int(n.value)].tobytes()

    def bgzf_lines(self, heads, records, sites, with_counts=False):
        """A span rendered and joined without leaving the device; returns the BGZF blocks the call completed (with_counts: and the
        bytes of text and the lines it added)."""
        h, r, s = _jtext_span(heads, records, sites)
        cap = jtext_bgzf_bound(jtext_text_bound(int(r["head_len"].sum(dtype=np.uint64)), len(r), self.n_samples, self.info), self._block)
        out = np.zeros(max(1, cap), dtype=np.uint8)
        n, tn, lines = C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(lib().vg_jtext_bgzf_lines(self._h, _ptr(h), len(h), _ptr(r), len(r), _ptr(s), len(s), _ptr(out), cap, C.byref(n), C.byref(tn), C.byref(lines)))
        blocks = out[:int(n.value)].tobytes()
        return (blocks, int(tn.value), int(lines.value)) if with_counts else blocks

    def bgzf_index(self):
        """Attaches a tabix index to the open stream (vg_jtext_bgzf_index): what bgzf_text, bgzf_lines and bgzf_end join from now on
        is scanned, and bgzf_end returns (blocks, raw index bytes)."""
        self._index = VcfIndex(self._block)
        check(lib().vg_jtext_bgzf_index(self._h, self._index._h))

    def bgzf_end(self):
        """The last partial block and the end-of-file marker; with an index attached (bgzf_index): (those bytes, the raw index bytes),
        or VcfIndexRefused."""
        cap = jtext_bgzf_bound(0, self._block)
        out = np.zeros(max(1, cap), dtype=np.uint8)
        n = C.c_uint64()
        ix, self._index = getattr(self, "_index", None), None
        try:
            check(lib().vg_jtext_bgzf_end(self._h, _ptr(out), cap, C.byref(n)))
            blocks = out[:int(n.value)].tobytes()
            return blocks if ix is None else (blocks, ix.finish())
        finally:
            if ix is not None:
                ix.close()


def _jtext_columns(gt, gq, sites, n_sites, who):
    cols_gt = [None if g is None else np.ascontiguousarray(g, dtype=np.uint8) for g in gt]
    cols_gq = [None if g is None else np.ascontiguousarray(q, dtype=np.int32) for g, q in zip(gt, gq)]
    n_samples = len(cols_gt)
    s = np.ascontiguousarray(sites, dtype=np.uint32)
    if n_sites is None:                                        # (no sample set: any number of sites above the references will do)
        n_sites = max([len(g) for g in cols_gt if g is not None] or [int(s.max()) + 1 if len(s) else 0])
    if any(g is not None and (g.shape != (n_sites,) or q.shape != (n_sites,)) for g, q in zip(cols_gt, cols_gq)):
        raise ValueError("%s: every sample's gt and gq hold one entry per site" % who)
    pg = (C.c_void_p * max(1, n_samples))(*[None if g is None else g.ctypes.data for g in cols_gt])
    pq = (C.c_void_p * max(1, n_samples))(*[None if q is None else q.ctypes.data for q in cols_gq])
    return (cols_gt, cols_gq), pg, pq, n_samples, n_sites                # (the columns: kept alive beside their pointers)


def joint_text_host(gt, gq, heads, records, sites, threads=1, n_sites=None, with_lines=False, info=False):
    """The same text by the header's host loop (vg_jtext_render_host; no device).  gt, gq: [n_samples, n_sites] arrays, or lists of
    per-sample columns in which None stands for a sample never set.  n_sites: default, the columns' length.  info=True: the lines
    of the INFO mode (vg_jtext_render_host_info with VG_JT_INFO_COUNTS)."""
    h, r, s = _jtext_span(heads, records, sites)
    keep, pg, pq, n_samples, n_sites = _jtext_columns(gt, gq, s, n_sites, "joint_text_host")
    cap = jtext_text_bound(int(r["head_len"].sum(dtype=np.uint64)), len(r), n_samples, info)
    out = np.zeros(max(1, cap), dtype=np.uint8)
    n, lines = C.c_uint64(), C.c_uint64()
    if info:
        check(lib().vg_jtext_render_host_info(n_sites, n_samples, pg, pq, _ptr(h), len(h), _ptr(r), len(r), _ptr(s), len(s), JT_INFO_COUNTS, int(threads), _ptr(out), cap, C.byref(n), C.byref(lines)))
    else:
        check(lib().vg_jtext_render_host(n_sites, n_samples, pg, pq, _ptr(h), len(h), _ptr(r), len(r), _ptr(s), len(s), int(threads), _ptr(out), cap, C.byref(n), C.byref(lines)))
    del keep
    text = out[:int(n.value)].tobytes()
    return (text, int(lines.value)) if with_lines else text


def joint_counts_host(gt, gq, records, sites, n_sites=None):
    """uint32[n_records, 3]: NS, het, hom of every record over the calls its line shows, zeros for a record that produces no line,
    by the header's host loop (vg_jtext_counts_host; no device).  The arguments are joint_text_host's, without the heads."""
    _, r, s = _jtext_span(b"", records, sites)
    keep, pg, pq, n_samples, n_sites = _jtext_columns(gt, gq, s, n_sites, "joint_counts_host")
    out = np.zeros((len(r), 3), dtype=np.uint32)
    check(lib().vg_jtext_counts_host(n_sites, n_samples, pg, pq, _ptr(r), len(r), _ptr(s), len(s), _ptr(out)))
    del keep
    return out


def pinned_buffer(nbytes):
    """Page-locked host memory: (numpy uint8 view, owner).  Keep `owner` alive as long as the view is used."""
    p = lib().vg_host_alloc_pinned(int(nbytes))
    if not p:
        raise MemoryError("vg_host_alloc_pinned(%d)" % nbytes)

    class _Owner:
        def __init__(self, ptr):
            self.ptr = ptr
            self.buf = (C.c_uint8 * int(nbytes)).from_address(ptr)

        def __del__(self):
            lib().vg_host_free_pinned(self.ptr)

    own = _Owner(p)
    return np.ctypeslib.as_array(own.buf), own


def all_reduce_devices(indexes):
    """One process, several devices (what `vargeno geno` does with VARGENO_GPUS=n): RCCL communicator over the handles'
    devices + one grouped all-reduce of their counters, inside the library."""
    arr = (C.c_void_p * len(indexes))(*[ix._h for ix in indexes])
    check(lib().vg_counts_allreduce_devices(arr, len(indexes)))


def all_reduce_sum_(tensor, group=None):
    """In-place sum over ranks of an integer tensor (device or host); no-op for a single process."""
    import torch.distributed as dist

    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.all_reduce(tensor, op=dist.ReduceOp.SUM, group=group)
    return tensor


def clamp_counts(summed):
    """The reference's 6-bit saturation (vartype.h:27) commutes with the sum over shards:
    min(63, sum_i c_i) == min(63, sum_i min(63, c_i)), so ranks may exchange exact or clamped sums."""
    return np.minimum(np.asarray(summed, dtype=np.int64), 63).astype(np.uint8)


def all_reduce_counts(index, group=None):
    """The path's one exchange step: sum the per-site counters over the ranks that each processed a
    shard of the reads.  RCCL (backend 'nccl') over xGMI on GPUs.

    The collective runs on a torch-owned staging tensor, the library's array is copied into it and back (two device
    copies of 8 bytes per site): every rank issues exactly the same collective sequence whatever its allocator thinks
    of memory it does not own, so a refusal on one rank cannot desynchronise the job."""
    import torch
    import torch.distributed as dist

    if not dist.is_initialized() or dist.get_world_size(group) == 1:
        return
    index.sync()
    mine = index.counts_tensor()                       # alias of the library's u32 array (as int32: same bits under a sum)
    # RCCL reduces device memory; any other backend (gloo in the CPU / shared-GPU plumbing tests) gets a host copy
    on_device = dist.get_backend(group) == "nccl"
    stage = torch.empty_like(mine) if on_device else torch.empty(mine.shape, dtype=mine.dtype)
    stage.copy_(mine)
    all_reduce_sum_(stage, group)
    mine.copy_(stage)
    torch.cuda.synchronize(index.device)


def shard_range(n_items, rank, world):
    """Contiguous shard [lo, hi) of n_items for `rank` of `world` (reads shard by index, no exchange)."""
    base, rem = divmod(int(n_items), int(world))
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def gate_words(d_quals, d_offsets):
    """Gate words of a device-resident batch (torch tensors: uint8 quality characters, int64 offsets[n+1]): bit c of word r is set
    iff quality character c of read r is below '8' (qv.cc:836, 943), for the read's chunk numbers c < len // 32."""
    import torch

    off = d_offsets.to(torch.int64)
    n_chunks = ((off[1:] - off[:-1]) >> 5).clamp(max=32)
    out = torch.zeros(len(off) - 1, dtype=torch.int64, device=d_quals.device)
    if d_quals.numel() == 0:
        return out.to(torch.int32)
    sq = d_quals.view(torch.int8)                       # the path compares a signed char with '8' (qv.cc:836): bytes >= 0x80 are below it
    for c in range(int(n_chunks.max().item()) if len(n_chunks) else 0):
        live = n_chunks > c
        idx = torch.where(live, off[:-1] + c, torch.zeros_like(off[:-1]))
        low = (sq[idx].to(torch.int16) < 56) & live
        out |= low.to(torch.int64) << c
    return out.to(torch.int32) if out.numel() == 0 else (out & 0xFFFFFFFF).to(torch.int64).view(torch.int32)[::2].contiguous()

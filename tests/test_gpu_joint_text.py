"""The joint text kernels (api.JointText: vg_jtext_*) against the Python formatter of tests/jtext_cases.py, and the handle's BGZF
stream against the host compressor over the whole text.  Every comparison is exact bytes."""
import numpy as np
import pytest

import jtext_cases as JC
from vargeno_amd import _lib, api

pytestmark = pytest.mark.gpu


def _handle(c, **kw):
    head_bytes = max(64, len(c["heads"]), sum(r[1] for r in c["records"]))      # (heads may overlap: the text's bound counts each record's)
    jt = api.JointText(c["n_sites"], c["n_samples"], max_records=max(1, len(c["records"])), max_head_bytes=head_bytes, max_site_refs=max(8, len(c["sites"])), **kw)
    for s, (g, q) in enumerate(zip(c["gt"], c["gq"])):
        if g is not None:
            jt.set(s, g, q)
    return jt


@pytest.mark.parametrize("n_samples,n_records,unset,drop,long_head", JC.shapes())
def test_render_writes_what_the_formatter_writes(n_samples, n_records, unset, drop, long_head):
    c = JC.make_case(n_samples, n_records, seed=1000 * n_samples + n_records, unset=unset, drop=drop, long_head=long_head)
    want = JC.expected(c)
    with _handle(c) as jt:
        assert jt.device_bytes >= 2 * n_samples * c["n_sites"]
        got, lines = jt.render(c["heads"], c["records"], c["sites"], with_lines=True)
        assert got == want
        assert lines == want.count(b"\n")
        if n_records >= 64:
            # two consecutive calls on one handle: a shorter span after a longer one, then the first again
            half = n_records // 2
            assert jt.render(c["heads"], c["records"][:half], c["sites"]) == JC.expected(c, 0, half)
            assert jt.render(c["heads"], c["records"], c["sites"]) == want


def test_all_records_dropped_is_empty_text():
    c = JC.make_case(3, 70, seed=7, drop=tuple(range(70)))
    with _handle(c) as jt:
        assert jt.render(c["heads"], c["records"], c["sites"], with_lines=True) == (b"", 0)


def test_gq_edges_narrow_and_wide_columns():
    """Samples whose gq all fit 0 .. 16382 take no wide column; 16383 and beyond, negatives and INT_MIN do."""
    c = JC.make_case(5, 200, seed=11, edges=False)
    wide = JC.make_case(5, 200, seed=11)
    for s in (1, 3):
        c["gq"][s] = wide["gq"][s]
    want = JC.expected(c)
    with _handle(c, wide_samples=2) as jt:
        assert jt.render(c["heads"], c["records"], c["sites"]) == want
        # a third wide sample finds no column: VG_ETOOBIG, and the store is unchanged
        with pytest.raises(_lib.VgError) as e:
            jt.set(0, c["gt"][0], wide["gq"][0])
        assert _lib.VG_ERRORS[e.value.code] == "VG_ETOOBIG"
        assert jt.render(c["heads"], c["records"], c["sites"]) == want
        # a wide sample set narrow again gives its column back
        jt.set(1, c["gt"][1], np.clip(c["gq"][1], 0, 16382))
        jt.set(0, c["gt"][0], wide["gq"][0])
        c["gq"][1] = np.clip(c["gq"][1], 0, 16382)
        c["gq"][0] = wide["gq"][0]
        assert jt.render(c["heads"], c["records"], c["sites"]) == JC.expected(c)


def test_a_line_above_the_lds_size():
    """16 384 samples x 3 records: a line of up to 256 KiB spans many tiles."""
    n = 16384
    rng = np.random.default_rng(5)
    n_sites = 7
    c = dict(n_sites=n_sites, n_samples=n, heads=b"chr1\t5\tx" + b"1\t77\trs9\tA\tC\t.\t.\tLONG=" + b"y" * 50, sites=np.array([5, 0, 3, 6], np.uint32),
             records=[(0, 8, 0, 1), (8, 70, 1, 2), (3, 5, 3, 1)])
    gt = rng.choice(np.array([0] + 5 * [1, 2, 3], np.uint8), size=(n, n_sites))
    gq = rng.choice(np.array([2 ** 31 - 1, JC.INT_MIN, -1, 16384, 10000, 99], np.int64), size=(n, n_sites)).astype(np.int32)
    gt[:, 6] = 0                                                                # the last record is dropped
    c["gt"], c["gq"] = [g for g in gt], [q for q in gq]
    c["gt"][777] = c["gq"][777] = None
    want = JC.expected(c)
    assert want.count(b"\n") == 2 and all(len(ln) > 163840 for ln in want.split(b"\n")[:2])
    with _handle(c) as jt:
        assert jt.render(c["heads"], c["records"], c["sites"], with_lines=True) == (want, 2)


def test_set_and_render_refuse_bad_arguments_and_leave_the_store_alone():
    c = JC.make_case(3, 20, seed=2)
    want = JC.expected(c)
    with _handle(c) as jt:
        bad = c["gt"][1].copy()
        bad[-1] = 4
        for args in ((1, bad, c["gq"][1]), (3, c["gt"][1], c["gq"][1])):
            with pytest.raises(_lib.VgError) as e:
                jt.set(*args)
            assert _lib.VG_ERRORS[e.value.code] == "VG_EINVAL"
        assert jt.render(c["heads"], c["records"], c["sites"]) == want
        L = api.lib()
        h, r, s = api._jtext_span(c["heads"], c["records"], c["sites"])
        cap = api.jtext_text_bound(int(r["head_len"].sum()), len(r), 3)
        out = np.full(cap, 0xAA, np.uint8)
        n, lines = api.C.c_uint64(), api.C.c_uint64()
        p = api._ptr
        call = lambda nr=len(r), hl=len(h), ns=len(s), cp=cap: _lib.VG_ERRORS.get(L.vg_jtext_render(jt._h, p(h), hl, p(r), nr, p(s), ns, p(out), cp, api.C.byref(n), api.C.byref(lines)))
        assert call(cp=cap - 1) == "VG_ETOOBIG"
        assert call(hl=len(h) - 1) == "VG_EINVAL" and call(ns=len(s) - 1) == "VG_EINVAL"
        assert (out == 0xAA).all()
        two = api.jtext_records(c["records"] + c["records"])                    # more records than the handle was made for
        assert _lib.VG_ERRORS.get(L.vg_jtext_render(jt._h, p(h), len(h), p(two), len(two), p(s), len(s), p(out), cap, api.C.byref(n), api.C.byref(lines))) == "VG_ETOOBIG"
        s2 = s.copy()
        s2[0] = c["n_sites"]
        assert _lib.VG_ERRORS.get(L.vg_jtext_render(jt._h, p(h), len(h), p(r), len(r), p(s2), len(s2), p(out), cap, api.C.byref(n), api.C.byref(lines))) == "VG_EINVAL"
        assert (out == 0xAA).all()
        with pytest.raises(_lib.VgError):
            jt.bgzf_begin()                                                     # made without the stream's buffers


# ---- the stream -----------------------------------------------------------------------------------------------------------------
HEADER = b"##fileformat=VCFv4.0\n##source=the stream's test\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ta\tb\tc\n"


@pytest.fixture(scope="module")
def stream_case():
    c = JC.make_case(3, 900, seed=42)
    cuts = [(0, 10), (10, 600), (600, 900)]                                     # a span shorter than a block of 1000, then one that crosses many boundaries
    return c, cuts, HEADER + b"".join(JC.expected(c, lo, hi) for lo, hi in cuts)


@pytest.mark.parametrize("codes", ["fixed", "dynamic"])
@pytest.mark.parametrize("block", [0, 1000])
def test_the_stream_is_the_host_compressor_over_the_whole_text(stream_case, block, codes):
    c, cuts, whole = stream_case
    with _handle(c, bgzf=True) as jt:
        jt.bgzf_begin(block=block, codes=codes)
        parts = [jt.bgzf_text(HEADER)]
        text_bytes = lines = 0
        for lo, hi in cuts:
            blocks, t, ln = jt.bgzf_lines(c["heads"], c["records"][lo:hi], c["sites"], with_counts=True)
            parts.append(blocks)
            text_bytes += t
            lines += ln
        parts.append(jt.bgzf_end())
        assert text_bytes == len(whole) - len(HEADER) and lines == whole.count(b"\n") - 3
        assert b"".join(parts) == api.bgzf_deflate(whole, device=None, block=block, codes=codes)
        if block == 1000:                                                       # text short of a block stays pending
            assert len(HEADER) + len(JC.expected(c, 0, 10)) < 1000 and parts[0] == b"" and parts[1] == b""
            assert len(JC.expected(c, 10, 600)) > 3000 and parts[2]
        # a stream of nothing on the same handle: the 28-byte marker
        jt.bgzf_begin(block=block, codes=codes)
        end = jt.bgzf_end()
        assert len(end) == 28 and end == api.bgzf_deflate(b"", device=None, block=block, codes=codes)
        # after the stream, render works again
        assert jt.render(c["heads"], c["records"][:50], c["sites"]) == JC.expected(c, 0, 50)


@pytest.mark.parametrize("codes", ["fixed", "dynamic"])
def test_a_text_that_is_an_exact_multiple_of_the_block(stream_case, codes):
    c, _, _ = stream_case
    lines = JC.expected(c, 0, 300)
    block = 500
    pad = b"#" * ((-len(lines) - 1) % block) + b"\n"                              # header text that makes the total a multiple of the block
    whole = pad + lines
    assert len(whole) % block == 0 and len(whole) > 3 * block
    with _handle(c, bgzf=True) as jt:
        jt.bgzf_begin(block=block, codes=codes)
        got = jt.bgzf_text(pad) + jt.bgzf_lines(c["heads"], c["records"][:300], c["sites"])
        end = jt.bgzf_end()
        assert len(end) == 28                                                   # nothing was pending
        assert got + end == api.bgzf_deflate(whole, device=None, block=block, codes=codes)

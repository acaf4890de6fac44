"""CPU suite of the joint VCF's planned text routes (VARGENO_JOINT_TEXT): the header's host loop (vg_jtext_render_host) against the
Python formatter of tests/jtext_cases.py; the hidden `vargeno jointvcf` with VARGENO_JOINT_TEXT=planned against the same command
without the variable -- the present writer, whose code the routes do not touch -- over the scenarios of test_joint_vcf_cpu.py and the
edges of the list's text; the option and the library's errors; and the host loop under AddressSanitizer + UBSan in a program of its
own.  Every comparison is exact bytes; no device is involved."""
import ctypes as C
import gzip
import os
import random
import subprocess

import numpy as np
import pytest

import jtext_cases as JC
from conftest import BIN
from vargeno_amd import _lib, api

HEADER8 = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"


@pytest.mark.parametrize("n_samples,n_records,unset,drop,long_head", JC.shapes())
def test_the_host_loop_writes_what_the_formatter_writes(n_samples, n_records, unset, drop, long_head):
    c = JC.make_case(n_samples, n_records, seed=1000 * n_samples + n_records, unset=unset, drop=drop, long_head=long_head)
    want = JC.expected(c)
    if n_records >= 64:
        assert want and want.count(b"\n") < n_records                           # lines were written, records were dropped
    for threads in (1, 3):
        got, lines = api.joint_text_host(c["gt"], c["gq"], c["heads"], c["records"], c["sites"], threads=threads, n_sites=c["n_sites"], with_lines=True)
        assert got == want
        assert lines == want.count(b"\n")


def test_every_gq_edge_in_every_genotype():
    """One record per (gt, gq): the cell is the formatter's, whatever the number of digits and the sign."""
    calls = [(g, q) for g in (1, 2, 3) for q in JC.GQ_EDGES]
    gt = [np.array([g for g, _ in calls], np.uint8)]
    gq = [np.array([q for _, q in calls], np.int32)]
    heads = b"H"
    records = [(0, 1, i, 1) for i in range(len(calls))]
    sites = np.arange(len(calls), dtype=np.uint32)
    got = api.joint_text_host(gt, gq, heads, records, sites)
    assert got == JC.format_span(gt, gq, heads, records, sites)
    assert b"H\tGT:GQ\t0/1:-2147483648\n" in got and b"\t1/1:2147483647\n" in got and b"\t0/0:0\n" in got


def test_all_records_dropped_is_empty_text():
    c = JC.make_case(3, 40, seed=7, drop=tuple(range(40)))
    assert api.joint_text_host(c["gt"], c["gq"], c["heads"], c["records"], c["sites"], n_sites=c["n_sites"], with_lines=True) == (b"", 0)
    assert JC.expected(c) == b""


# ---- jointvcf: planned against the present writer ----------------------------------------------------------------------------
def _write(path, text, mode="w"):
    with open(path, mode) as f:
        f.write(text)
    return str(path)


def _counts(tmp, name, rows):
    return _write(tmp / name, "".join("%d %d %d %d %d\n" % r for r in rows))


def _three_samples(tmp, rng, chroms, per_chrom):
    chrlens = _write(tmp / "chrlens", "".join("%s %d\n" % c for c in chroms))
    sites, before = [], 0
    for name, ln in chroms:
        for p in sorted(rng.sample(range(1, ln), per_chrom)):
            sites.append((name, p, before + p))
        before += ln
    kinds = [(20, 0), (0, 20), (10, 10), (0, 0), (3, 1), (63, 63), (63, 0), (0, 0)]
    freqs = [(rng.choice([230, 200, 128, 25]), rng.choice([25, 60, 128, 250])) for _ in sites]
    counts = [_counts(tmp, "counts%d.txt" % s, [(g, freqs[i][0], freqs[i][1]) + (rng.choice(kinds) if (i + s) % 5 else (0, 0)) for i, (_, _, g) in enumerate(sites)]) for s in range(3)]
    return chrlens, sites, counts


def _scenarios(tmp):
    """name -> (chrlens, SNP list path, [(sample, counts)], environment)"""
    rng = random.Random(20261020)
    out = {}
    # one sample
    chrlens = _write(tmp / "chrlens1", "chr1 5000\nchr2 3000\n")
    sites = sorted(rng.sample(range(1, 8000), 1500))
    counts = _counts(tmp, "one.txt", [(g, rng.randrange(256), rng.randrange(256), rng.choice([0, 0, 3, 20, 63]), rng.choice([0, 1, 9, 63])) for g in sites])
    lines = ["%s\t%d\trs%d\tA\tC\t.\t.\tRS=%d" % ((("1", g) if g <= 5000 else ("2", g - 5000)) + (i, i)) for i, g in enumerate(sites)]
    out["one sample"] = (chrlens, _write(tmp / "one.vcf", "##fileformat=VCFv4.0\n##source=test\n" + HEADER8 + "\n" + "\n".join(lines) + "\n"), [("DONOR", counts)], {})
    # three samples with different called sets; chr-less names
    chroms = [("chr1", 50_000), ("chr2", 30_000), ("chrX", 20_000)]
    chrlens3, s3, c3 = _three_samples(tmp, rng, chroms, 1500)
    recs = ["%s\t%d\trs%d\tA\tC\t.\t.\tRS=%d" % (name[3:], p, i, i) for i, (name, p, _) in enumerate(s3)]
    names = [("alpha", c3[0]), ("beta", c3[1]), ("gamma", c3[2])]
    out["three samples"] = (chrlens3, _write(tmp / "three.vcf", "##fileformat=VCFv4.0\n" + HEADER8 + "\n" + "\n".join(recs) + "\n"), names, {})
    # with the chr prefix spelled out
    out["chr names"] = (chrlens3, _write(tmp / "chr.vcf", HEADER8 + "\n" + "\n".join("chr" + r for r in recs) + "\n"), names, {})
    # repeated records, shuffled, keys that name nothing, past the size from which the pass cuts its text into pieces; three threads
    extra = ["1\t%d\tnone%d\tA\tC\t.\t.\t." % (50_001 + k, k) for k in range(50)] + ["2\t0%d\tzero%d\tA\tC\t.\t.\t." % (s3[1500 + k][1], k) for k in range(50)]
    extra += ["7\t%d\tother%d\tA\tC\t.\t.\t." % (k + 1, k) for k in range(50)]
    filler = ["9\t%d\tfill%d\tA\tC\t.\t.\tPADDING=%s" % (k + 1, k, "x" * 60) for k in range(12_000)]
    shuffled = recs + recs[:500] + extra + filler
    rng.shuffle(shuffled)
    text = "##fileformat=VCFv4.0\n" + HEADER8 + "\n" + "\n".join(shuffled) + "\n"
    assert len(text) > (1 << 20)
    out["repeated records"] = (chrlens3, _write(tmp / "rep.vcf", text), names, {"VARGENO_THREADS": "3"})
    # two chromosomes with one name
    chrlens2 = _write(tmp / "chrlens2", "chr1 1000\nchr1 1000\nchr2 1000\n")
    a = _write(tmp / "a.txt", "100 230 25 20 0\n1100 230 25 0 0\n1200 230 25 10 10\n2050 230 25 0 0\n")
    b = _write(tmp / "b.txt", "100 230 25 20 0\n1100 230 25 0 20\n1200 230 25 0 0\n2050 230 25 0 0\n")
    two = ["1\t100\tx\tA\tC\t.\t.\t.", "1\t200\ty\tA\tC\t.\t.\t.", "2\t50\tz\tA\tC\t.\t.\t."]
    out["one name twice"] = (chrlens2, _write(tmp / "two.vcf", HEADER8 + "\n" + "\n".join(two) + "\n"), [("A", a), ("B", b)], {})
    # '#' lines in the middle of the data, and lines with fewer than eight fields (one of them with a single field)
    mid = recs[:200] + ["##note=in the middle", HEADER8] + recs[200:260] + ["#CHROM\tPOS"] + [r.rsplit("\t", 3)[0] for r in recs[260:300]] + ["lonely"] + recs[300:400]
    out["header lines in the data"] = (chrlens3, _write(tmp / "mid.vcf", "##fileformat=VCFv4.0\n" + HEADER8 + "\n" + "\n".join(mid) + "\n"), names, {})
    # CRLF line ends
    out["crlf"] = (chrlens3, _write(tmp / "crlf.vcf", (HEADER8 + "\n" + "\n".join(recs[:300]) + "\n").replace("\n", "\r\n").encode(), "wb"), names, {})
    # no final newline (after eight fields, and after five)
    out["no final newline"] = (chrlens3, _write(tmp / "nonl.vcf", HEADER8 + "\n" + "\n".join(recs[:300])), names, {})
    out["no final newline, short line"] = (chrlens3, _write(tmp / "nonl5.vcf", HEADER8 + "\n" + "\n".join(recs[:100]) + "\n" + recs[100].rsplit("\t", 3)[0]), names, {})
    # input with sample columns that declares GT and GQ
    head = ("##fileformat=VCFv4.0\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n"
            "##FORMAT=<ID=GQ,Number=1,Type=Integer,Description=\"Genotype Quality\">\n" + HEADER8 + "\tFORMAT\tOLD1\tOLD2\n")
    out["declared, with sample columns"] = (chrlens3, _write(tmp / "decl.vcf", head + "\n".join(r + "\tGT:GQ:DP\t0/0:5:9\t1/1:7:3" for r in recs[:300]) + "\n"), names, {})
    return out


def _jointvcf(chrlens, src, samples, out, env):
    return subprocess.run([BIN, "jointvcf", chrlens, src, out] + ["%s=%s" % s for s in samples], env=dict(os.environ, **env), capture_output=True, text=True, timeout=120)


OUTPUTS = {"plain": {}, "bgzf fixed": {"VARGENO_VCF_BGZF": "host", "VARGENO_VCF_CODES": "fixed"}, "bgzf dynamic": {"VARGENO_VCF_BGZF": "host", "VARGENO_VCF_CODES": "dynamic"}}


def test_jointvcf_planned_writes_the_present_writers_bytes(tmp_path):
    for name, (chrlens, src, samples, env) in _scenarios(tmp_path).items():
        plain = None
        for how, out_env in OUTPUTS.items():
            base = str(tmp_path / "base.out")
            p = _jointvcf(chrlens, src, samples, base, dict(env, **out_env))
            assert p.returncode == 0 and "joint text" not in p.stderr, (name, how, p.stderr)
            want = open(base, "rb").read()
            if how == "plain":
                plain = want
                assert want.count(b"\tGT:GQ\t") >= 2, name                      # (data lines were written)
            else:
                assert gzip.decompress(want) == plain, (name, how)
            for lines in ("1", "97", None):
                out = str(tmp_path / "planned.out")
                e = dict(env, VARGENO_JOINT_TEXT="planned", VARGENO_VERBOSE="1", **out_env)
                if lines:
                    e["VARGENO_JOINT_TEXT_LINES"] = lines
                p = _jointvcf(chrlens, src, samples, out, e)
                assert p.returncode == 0, (name, how, lines, p.stderr)
                assert "joint text: planned, " in p.stderr, (name, how, lines, p.stderr)
                assert open(out, "rb").read() == want, (name, how, lines)
                said = [ln for ln in p.stderr.splitlines() if ln.startswith("joint text: planned")][0]
                assert "%d lines written" % plain.count(b"\tGT:GQ\t") in said, (name, said)
                if lines == "1":
                    assert "%d spans" % int(said.split(" records")[0].split()[-1]) in said, said        # a span per record


def test_an_explicit_host_is_the_default(tmp_path):
    chrlens, src, samples, env = _scenarios(tmp_path)["one name twice"]
    a, b = str(tmp_path / "a.vcf"), str(tmp_path / "b.vcf")
    assert _jointvcf(chrlens, src, samples, a, env).returncode == 0
    for v in ("host", ""):
        p = _jointvcf(chrlens, src, samples, b, dict(env, VARGENO_JOINT_TEXT=v, VARGENO_VERBOSE="1"))
        assert p.returncode == 0 and "joint text" not in p.stderr
        assert open(a, "rb").read() == open(b, "rb").read()


# ---- the option and the errors -------------------------------------------------------------------------------------------------
def test_a_wrong_value_is_refused_in_one_line_before_anything_is_looked_at(tmp_path):
    out = str(tmp_path / "never.vcf")
    for args in (["jointvcf", "no_chrlens", "no.vcf", out, "A=no_counts"], ["joint", "no_index", "no_manifest", "no.vcf", out]):
        p = subprocess.run([BIN] + args, env=dict(os.environ, VARGENO_JOINT_TEXT="gpu"), capture_output=True, text=True, timeout=60)
        assert p.returncode == 1, p.stderr
        assert p.stderr.count("\n") == 1 and "VARGENO_JOINT_TEXT=gpu is not understood" in p.stderr and "planned" in p.stderr, p.stderr
        assert not os.path.exists(out)


def test_device_without_a_device_ends_non_zero_and_names_it(tmp_path):
    """(On a machine with a device the route runs, and writes the present writer's bytes.)"""
    chrlens, src, samples, env = _scenarios(tmp_path)["one name twice"]
    out, base = str(tmp_path / "dev.vcf"), str(tmp_path / "base.vcf")
    p = _jointvcf(chrlens, src, samples, out, dict(env, VARGENO_JOINT_TEXT="device"))
    if _lib.lib().vg_device_count() > 0:
        assert p.returncode == 0, p.stderr
        assert _jointvcf(chrlens, src, samples, base, env).returncode == 0
        assert open(out, "rb").read() == open(base, "rb").read()
        return
    assert p.returncode != 0 and "VARGENO_JOINT_TEXT=device" in p.stderr and "no HIP device" in p.stderr, p.stderr


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _code(rc):
    return _lib.VG_ERRORS.get(rc, rc)


def test_the_device_calls_are_enodev_without_a_device():
    L = api.lib()
    if L.vg_device_count() > 0:
        with api.JointText(4, 1, max_records=4, max_head_bytes=64, max_site_refs=8) as jt:
            assert jt.device_bytes > 0
        return
    h = C.c_void_p()
    assert _code(L.vg_jtext_create(0, 100, 3, 0, 10, 100, 10, 0, C.byref(h))) == "VG_ENODEV" and not h.value
    assert b"no HIP device" in L.vg_last_error()
    with pytest.raises(_lib.VgError) as e:
        api.JointText(100, 3)
    assert _lib.VG_ERRORS[e.value.code] == "VG_ENODEV"
    assert L.vg_jtext_device_bytes(None) == 0
    L.vg_jtext_destroy(None)


def test_create_checks_its_sizes_before_it_looks_for_a_device():
    L = api.lib()
    h = C.c_void_p()
    assert _code(L.vg_jtext_create(0, 100, 0, 0, 10, 100, 10, 0, C.byref(h))) == "VG_EINVAL"
    assert _code(L.vg_jtext_create(0, 100, 16385, 0, 10, 100, 10, 0, C.byref(h))) == "VG_ETOOBIG"
    assert _code(L.vg_jtext_create(0, 2 ** 32, 1, 0, 10, 100, 10, 0, C.byref(h))) == "VG_EINVAL"
    assert _code(L.vg_jtext_create(0, 100, 1, 0, 0, 100, 10, 0, C.byref(h))) == "VG_EINVAL"
    assert _code(L.vg_jtext_create(0, 100, 1, 0, 10, 100, 10, 0, None)) == "VG_EINVAL"
    assert not h.value


def test_render_host_returns_einval_and_etoobig_as_specified():
    L = api.lib()
    c = JC.make_case(2, 5, seed=3)
    heads = np.frombuffer(c["heads"], np.uint8)
    recs = api.jtext_records(c["records"])
    sites = c["sites"]
    pg = (C.c_void_p * 2)(*[g.ctypes.data for g in c["gt"]])
    pq = (C.c_void_p * 2)(*[q.ctypes.data for q in c["gq"]])
    bound = api.jtext_text_bound(int(recs["head_len"].sum()), 5, 2)
    out = np.full(bound + 8, 0xAA, np.uint8)
    n, lines = C.c_uint64(), C.c_uint64()

    def call(n_sites=c["n_sites"], n_samples=2, gt=pg, gq=pq, h=heads, hl=len(heads), r=recs, nr=5, s=sites, ns=len(sites), cap=bound, text=out, ln=C.byref(n)):
        return _code(L.vg_jtext_render_host(n_sites, n_samples, gt, gq, None if h is None else _p(h), hl, None if r is None else _p(r), nr, None if s is None else _p(s), ns, 1,
                                            None if text is None else _p(text), cap, ln, C.byref(lines)))
    assert call() == 0 and out[:n.value].tobytes() == JC.expected(c) and (out[bound:] == 0xAA).all()
    out[:] = 0xAA
    assert call(cap=bound - 1) == "VG_ETOOBIG" and (out == 0xAA).all()          # nothing is written
    assert call(gt=None) == "VG_EINVAL" and call(h=None) == "VG_EINVAL" and call(r=None) == "VG_EINVAL" and call(s=None) == "VG_EINVAL"
    assert call(text=None) == "VG_EINVAL" and call(ln=None) == "VG_EINVAL"
    assert call(n_samples=0) == "VG_EINVAL" and call(n_samples=16385) == "VG_ETOOBIG" and call(n_sites=2 ** 32) == "VG_EINVAL"
    assert call(n_sites=int(sites.max())) == "VG_EINVAL" and b"site reference" in L.vg_last_error()      # an index the columns do not have
    assert call(hl=len(heads) - 1) == "VG_EINVAL" and b"head" in L.vg_last_error()                       # the last head ends outside
    assert call(ns=len(sites) - 1) == "VG_EINVAL" and b"site run" in L.vg_last_error()
    assert (out == 0xAA).all()


def test_the_bound_functions_are_the_formula():
    L = api.lib()
    for heads, recs, n in ((0, 0, 1), (50, 1, 1), (123456, 1000, 130), (2 ** 33, 2 ** 20, 16384)):
        assert api.jtext_text_bound(heads, recs, n) == heads + recs * (7 + 16 * n)
    for block in (0, 1000, 65280, 1):
        B = block or 65280
        for t in (0, 1, B - 1, B, B + 1, 10 * B, 12345678):
            assert api.jtext_bgzf_bound(t, block) == L.vg_bgzf_deflate_bound(t + B - 1, block)
            blocks = (t + B - 1 + B - 1) // B
            assert api.jtext_bgzf_bound(t, block) == t + B - 1 + blocks * 31 + 28
    assert api.jtext_bgzf_bound(10, 65281) == 0


def test_the_header_is_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """tests/jtext_check.cpp: the header's host loop on exact-size heap buffers against a naive per-cell snprintf loop, n_samples in
    {1, 63, 64, 65, 129}, one and three threads, a cap exactly at the bound and one byte below it (the C-ABI's refusal, restated there)
    -- compiled with -fsanitize=address,undefined and run on its own."""
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(here, "..", "vargeno_amd", "csrc")
    exe = str(tmp_path / "jtext_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-march=x86-64-v2", "-I" + csrc,
                           os.path.join(here, "jtext_check.cpp"), "-o", exe, "-lpthread"])
    p = subprocess.run([exe], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"), capture_output=True, text=True)
    assert p.returncode == 0 and "ok" in p.stdout, (p.stdout[-500:], p.stderr[-2000:])

"""CPU suite of the joint VCF's INFO mode (VARGENO_JOINT_INFO=counts; vg_jtext_*_info, vg_jtext_counts_host): the header's host loop
against the Python restatement of tests/jinfo_cases.py, mode 0 against the formatter of tests/jtext_cases.py, the hidden `vargeno
jointvcf` on the `host` and `planned` routes over the scenarios of test_joint_text_cpu.py, the refusals, and the host loop under
AddressSanitizer + UBSan in a program of its own.  Every comparison is exact bytes; no device is involved."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

import jinfo_cases as JI
import jtext_cases as JC
import test_joint_text_cpu as CPU
from conftest import BIN
from vargeno_amd import _lib, api


def _host(c, **kw):
    return api.joint_text_host(c["gt"], c["gq"], c["heads"], c["records"], c["sites"], n_sites=c["n_sites"], **kw)


@pytest.mark.parametrize("n_samples,n_records,unset,drop,long_head", JC.shapes())
def test_the_host_loop_writes_the_restated_rule(n_samples, n_records, unset, drop, long_head):
    c = JI.make_case(n_samples, n_records, seed=1000 * n_samples + n_records, unset=unset, drop=drop, long_head=long_head)
    want, counts = JI.expected(c), JI.expected_counts(c)
    if n_records >= 64:
        assert want.count(b"\n") < n_records and want.count(b";NS=") and want.count(b"\tNS=") > want.count(b".\tGT:GQ")      # dropped records; appended and replaced INFO
        assert (counts[list(drop)] == 0).all() and counts[:, 0].max() <= n_samples
    for threads in (1, 7):
        got, lines = _host(c, threads=threads, with_lines=True, info=True)
        assert got == want
        assert lines == want.count(b"\n")
    assert np.array_equal(api.joint_counts_host(c["gt"], c["gq"], c["records"], c["sites"], n_sites=c["n_sites"]), counts)
    # mode 0 on the same case: the bytes of the formatter that knows no INFO mode
    assert _host(c, threads=7) == JC.expected(c) and _host(c, info=False) == JC.expected(c)


def _one_record(gts, head=b"1\t5\trs1\tA\tC\t.\t.\t."):
    gt = [np.array([g], np.uint8) for g in gts]
    gq = [np.array([40 + s % 7], np.int32) for s in range(len(gts))]
    return dict(gt=gt, gq=gq, heads=head, records=[(0, len(head), 0, 1)], sites=np.array([0], np.uint32), n_sites=1, n_samples=len(gts))


def test_all_ref_all_alt_and_one_het_in_130():
    for gts, tag in (([1] * 130, b"NS=130;AN=260;AC=0;AF=0"), ([2] * 130, b"NS=130;AN=260;AC=260;AF=1"), ([1] * 77 + [3] + [1] * 52, b"NS=130;AN=260;AC=1;AF=0.003846"),
                     ([3], b"NS=1;AN=2;AC=1;AF=0.5"), ([1, 3, 0, 1], b"NS=3;AN=6;AC=1;AF=0.166667"), ([3, 1, 1], b"NS=3;AN=6;AC=1;AF=0.166667"), ([2, 1, 1], b"NS=3;AN=6;AC=2;AF=0.333333")):
        c = _one_record(gts)
        assert JI.tag(*[int(v) for v in JI.expected_counts(c)[0]]) == tag
        got = _host(c, info=True)
        assert got == JI.expected(c) and got.startswith(b"1\t5\trs1\tA\tC\t.\t.\t" + tag + b"\tGT:GQ\t")


def test_the_frequency_is_rounded_half_up_in_integers():
    """Through the host loop at the widths where the sixth decimal is decided by a tie or a near-tie: 1 / 2 ^ k and the like."""
    assert [JI.af_text(*p) for p in ((1, 32768), (1, 2), (1, 3), (2, 3), (1, 64), (3, 128), (1, 2_000_000))] == ["0.000031", "0.5", "0.333333", "0.666667", "0.015625", "0.023438", "0.000001"]
    for n, k in ((32, 1), (64, 3), (64, 1), (130, 7), (129, 128), (7, 5)):
        c = _one_record([3] * k + [1] * (n - k))
        assert _host(c, info=True) == JI.expected(c), (n, k)


def test_the_splice_is_a_function_of_the_heads_bytes():
    heads = {b"1\t5\tx\tA\tC\t.\t.\t.": b"1\t5\tx\tA\tC\t.\t.\tT", b"1\t5\tx\tA\tC\t.\t.\t": b"1\t5\tx\tA\tC\t.\t.\tT", b"1\t5\tx\tA\tC\t.\t.\tRS=1": b"1\t5\tx\tA\tC\t.\t.\tRS=1;T",
             b"1\t5\tx\tA\tC\t.\t.\t..": b"1\t5\tx\tA\tC\t.\t.\t..;T", b"1\t5\tx\tA\tC\t.\t.\tA.": b"1\t5\tx\tA\tC\t.\t.\tA.;T", b"\t\t\t\t\t\t\t": b"\t\t\t\t\t\t\tT", b"\t\t\t\t\t\t\t.": b"\t\t\t\t\t\t\tT"}
    for tabs in range(7):                                                       # fewer than eight fields: the line of mode 0
        for h in (b"\t".join([b"f"] * (tabs + 1)), b"\t".join([b"."] * (tabs + 1)), b"\t" * tabs, b"\t" * tabs + b"."):
            heads[h] = h
    heads[b""] = b""
    for h, want in heads.items():
        c = _one_record([3, 1], head=h)
        assert JI.splice(h, b"T") == want
        got = _host(c, info=True)
        assert got == JI.expected(c) and got == want.replace(b"T", b"NS=2;AN=4;AC=1;AF=0.25") + b"\tGT:GQ\t0/1:40\t0/0:41\n", h
        if want == h:
            assert got == _host(c)


def test_the_bound_grows_by_forty_bytes_a_record_and_other_modes_are_refused():
    L = api.lib()
    for heads, recs, n in ((0, 0, 1), (50, 1, 1), (123456, 1000, 130), (2 ** 33, 2 ** 20, 16384)):
        assert api.jtext_text_bound(heads, recs, n, info=True) == heads + recs * (47 + 16 * n)
        assert L.vg_jtext_text_bound_info(heads, recs, n, 0) == api.jtext_text_bound(heads, recs, n) and L.vg_jtext_text_bound_info(heads, recs, n, 2) == 0
    assert len(JI.tag(16384, 1, 5461)) == 38 and JI.tag(16384, 1, 5461) == b"NS=16384;AN=32768;AC=10923;AF=0.333344"
    c = JI.make_case(2, 5, seed=3)
    h, r, s = api._jtext_span(c["heads"], c["records"], c["sites"])
    pg = (C.c_void_p * 2)(*[g.ctypes.data for g in c["gt"]])
    pq = (C.c_void_p * 2)(*[q.ctypes.data for q in c["gq"]])
    bound = api.jtext_text_bound(int(r["head_len"].sum()), 5, 2, info=True)
    out = np.full(bound + 8, 0xAA, np.uint8)
    n, lines = C.c_uint64(), C.c_uint64()
    p = api._ptr
    call = lambda info, cap: _lib.VG_ERRORS.get(L.vg_jtext_render_host_info(c["n_sites"], 2, pg, pq, p(h), len(h), p(r), 5, p(s), len(s), info, 1, p(out), cap, C.byref(n), C.byref(lines)), 0)
    assert call(1, bound) == 0 and out[:n.value].tobytes() == JI.expected(c) and (out[bound:] == 0xAA).all()
    out[:] = 0xAA
    assert call(1, bound - 1) == "VG_ETOOBIG" and call(2, bound) == "VG_EINVAL" and call(-1, bound) == "VG_EINVAL" and (out == 0xAA).all()
    hd = C.c_void_p()
    assert _lib.VG_ERRORS.get(L.vg_jtext_create_info(0, 100, 3, 0, 10, 100, 10, 0, 2, C.byref(hd))) == "VG_EINVAL" and not hd.value
    cnt = np.zeros((5, 3), np.uint32)
    assert _lib.VG_ERRORS.get(L.vg_jtext_counts_host(int(s.max()), 2, pg, pq, p(r), 5, p(s), len(s), p(cnt))) == "VG_EINVAL"       # a site the columns do not have
    assert _lib.VG_ERRORS.get(L.vg_jtext_counts_host(c["n_sites"], 0, pg, pq, p(r), 5, p(s), len(s), p(cnt))) == "VG_EINVAL"
    assert _lib.VG_ERRORS.get(L.vg_jtext_counts(None, p(r), 5, p(s), len(s), p(cnt))) == "VG_EINVAL"


# ---- jointvcf ---------------------------------------------------------------------------------------------------------------------
INFO = {"VARGENO_JOINT_INFO": "counts"}


def test_jointvcf_host_and_planned_write_the_same_counted_file(tmp_path):
    """Over the scenarios of test_joint_text_cpu.py: both routes write the same bytes; without the four declarations and the spliced
    tags the file is the one written without the variable; and every tag holds the counts of its own line's cells."""
    for name, (chrlens, src, samples, env) in CPU._scenarios(tmp_path).items():
        base, host, planned = (str(tmp_path / f) for f in ("base.out", "host.out", "planned.out"))
        assert CPU._jointvcf(chrlens, src, samples, base, env).returncode == 0
        p = CPU._jointvcf(chrlens, src, samples, host, dict(env, VARGENO_VERBOSE="1", **INFO))
        assert p.returncode == 0 and "joint text" not in p.stderr, (name, p.stderr)
        p = CPU._jointvcf(chrlens, src, samples, planned, dict(env, VARGENO_JOINT_TEXT="planned", VARGENO_JOINT_TEXT_LINES="97", VARGENO_VERBOSE="1", **INFO))
        assert p.returncode == 0 and "joint text: planned, info counts, " in p.stderr, (name, p.stderr)
        want, got = open(base, "rb").read(), open(host, "rb").read()
        assert open(planned, "rb").read() == got, name
        for d in JI.INFO_DECL:
            assert got.count(b"\n" + d) == (b"\n" + want).count(b"\n#CHROM"), name
        assert got.index(JI.INFO_DECL[0]) < got.index(b"#CHROM") and got != want
        stripped, found = JI.strip_info(got)
        assert stripped == want, name
        short = sum(1 for ln in want.split(b"\n") if ln[:1] not in (b"#", b"") and ln.count(b"\t") < 8 + len(samples))      # lines of fewer than eight fields carry no tag
        assert len(found) == want.count(b"\tGT:GQ\t") - short and len(found) >= 2, name
        assert (short > 0) == (name in ("header lines in the data", "no final newline, short line")), name
        for ln, ns, an, ac, af in found:
            assert (ns, an, ac) == JI.cells_counts(ln) and af == JI.af_text(ac, an).encode() and 1 <= ns <= len(samples), ln


def test_jointvcf_bgzf_and_tbi_beside_the_counts(tmp_path):
    chrlens, src, samples, env = CPU._scenarios(tmp_path)["three samples"]
    plain, z = str(tmp_path / "plain.vcf"), str(tmp_path / "out.vcf.gz")
    assert CPU._jointvcf(chrlens, src, samples, plain, dict(env, **INFO)).returncode == 0
    for route in ("host", "planned"):
        p = CPU._jointvcf(chrlens, src, samples, z, dict(env, VARGENO_JOINT_TEXT=route, VARGENO_VCF_BGZF="host", VARGENO_VCF_INDEX="tbi", **INFO))
        assert p.returncode == 0, p.stderr
        assert gzip.decompress(open(z, "rb").read()) == open(plain, "rb").read()
        tbi = gzip.decompress(open(z + ".tbi", "rb").read())
        assert tbi[:4] == b"TBI\x01" and len(tbi) > 100
        os.remove(z + ".tbi")


def test_a_wrong_value_and_a_declared_key_are_refused_in_one_line_with_no_output(tmp_path):
    out = str(tmp_path / "never.vcf")
    for args in (["jointvcf", "no_chrlens", "no.vcf", out, "A=no_counts"], ["joint", "no_index", "no_manifest", "no.vcf", out]):
        p = subprocess.run([BIN] + args, env=dict(os.environ, VARGENO_JOINT_INFO="1"), capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and p.stderr.count("\n") == 1 and "VARGENO_JOINT_INFO=1 is not understood" in p.stderr and "counts" in p.stderr, p.stderr
        assert not os.path.exists(out)
    chrlens, src, samples, env = CPU._scenarios(tmp_path)["one name twice"]
    for key in ("AF", "NS", "AN", "AC"):
        text = open(src).read()
        declared = str(tmp_path / ("declares_%s.vcf" % key))
        with open(declared, "w") as f:
            f.write("##fileformat=VCFv4.0\n##INFO=<ID=AFR,Number=1,Type=Float,Description=\"another key\">\n##INFO=<ID=%s,Number=A,Type=Float,Description=\"taken\">\n" % key + text)
        for args in ([BIN, "jointvcf", chrlens, declared, out] + ["%s=%s" % s for s in samples], [BIN, "joint", "no_index", "no_manifest", declared, out]):
            p = subprocess.run(args, env=dict(os.environ, **dict(env, **INFO)), capture_output=True, text=True, timeout=60)
            assert p.returncode == 1 and p.stderr.count("\n") == 1 and "INFO key %s" % key in p.stderr and "VARGENO_JOINT_INFO" in p.stderr, p.stderr
            assert not os.path.exists(out)
        assert CPU._jointvcf(chrlens, declared, samples, out, env).returncode == 0      # without the variable the list is taken as ever
        os.remove(out)
    # a key that only starts like one of the four is none of them
    other = str(tmp_path / "other.vcf")
    with open(other, "w") as f:
        f.write("##INFO=<ID=AFR,Number=1,Type=Float,Description=\"another key\">\n" + open(src).read())
    assert CPU._jointvcf(chrlens, other, samples, out, dict(env, **INFO)).returncode == 0 and b";AF=" in open(out, "rb").read()


def test_the_header_is_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """tests/jinfo_check.cpp: the header's host loop in the INFO mode on exact-size heap buffers against a naive snprintf loop --
    compiled with -fsanitize=address,undefined and run on its own, nothing preloaded."""
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(here, "..", "vargeno_amd", "csrc")
    exe = str(tmp_path / "jinfo_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-march=x86-64-v2", "-I" + csrc,
                           os.path.join(here, "jinfo_check.cpp"), "-o", exe, "-lpthread"])
    p = subprocess.run([exe], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"), capture_output=True, text=True)
    assert p.returncode == 0 and "ok" in p.stdout, (p.stdout[-500:], p.stderr[-2000:])

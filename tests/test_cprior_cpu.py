"""CPU suite of the cohort prior (VARGENO_JOINT_PRIOR=cohort; vg_cprior_host): the header's host loop against the numpy restatement
of tests/cprior_cases.py -- q as bit patterns, gt and gq equal --, the hidden `vargeno jointvcf` with the variable set, the refusals,
and the host loop under AddressSanitizer + UBSan in a program of its own.  No device is involved."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cprior_cases as CC
import test_joint_text_cpu as CPU
from conftest import BIN
from vargeno_amd import _lib, api


def _same(got, want):
    assert np.array_equal(CC.bits(got[2]), CC.bits(want[2]))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("n_samples", CC.SAMPLES)
@pytest.mark.parametrize("n_sites", CC.SITES)
def test_the_host_loop_computes_the_restated_rule(n_sites, n_samples):
    c = CC.shaped(n_sites, n_samples)
    if n_sites > 4:
        r, a = np.minimum(c[0], 63), np.minimum(c[1], 63)
        assert not (r[:, 3] | a[:, 3]).any() and (r[:, 4] == 63).all() and (a[:, 4] == 63).all()      # no informative sample; only saturated ones
    for iters in (1, 8, 64):
        for pseudo in (0.0, 2.0):
            want = CC.expected(*c, iters=iters, pseudo=pseudo)
            for threads in (1, 3):
                got = api.cohort_prior_host(*c, iters=iters, pseudo=pseudo, threads=threads)
                assert got[0].shape == (n_samples, n_sites) and got[2].shape == (n_sites,)
                _same(got, want)
    if n_sites > 4:
        want = CC.expected(*c)
        assert not want[0][:, 3].any() and not want[0][:, 4].any() and not want[1][:, 3:5].any()
        # a site without an informative sample keeps the dictionary's frequency
        assert want[2][3] == min(max(CC.FREQ[c[3][3]] / (CC.FREQ[c[2][3]] + CC.FREQ[c[3][3]]) if int(c[2][3]) + int(c[3][3]) else 0.5, 1e-6), 1 - 1e-6)


def test_a_single_sample_over_every_counter_pair():
    c = CC.all_pairs()
    assert len({(int(r), int(a)) for r, a in zip(c[0][0], c[1][0])}) == 4096 and {(0, 0), (255, 255), (255, 0)} <= set(zip(c[2].tolist(), c[3].tolist()))
    for iters, pseudo in ((1, 0.0), (8, 2.0), (64, 0.0), (64, 2.0)):
        want = CC.expected(*c, iters=iters, pseudo=pseudo)
        assert ((want[0][0] != 0).sum()) == 4094 and len(set(want[0][0].tolist())) == 4
        _same(api.cohort_prior_host(*c, iters=iters, pseudo=pseudo, threads=3), want)


def test_the_new_caller_is_not_the_old_one():
    """On the seeded 4 096 x 24 cohort: the restated rule, and calls that differ from vg_call_site's own."""
    c = CC.cohort(4096, 24, seed=20261021)
    got = api.cohort_prior_host(*c, threads=3)
    _same(got, CC.expected(*c))
    differ = 0
    for s in range(24):
        gt, _ = CC.single_sample_calls(c[0][s], c[1][s], c[2], c[3])
        assert np.array_equal(gt != 0, got[0][s] != 0)                          # the same entries are called
        differ += int((gt != got[0][s]).sum())
    assert differ >= 1


def test_counters_above_the_cap_are_clamped_and_the_arguments_checked():
    c = CC.cohort(65, 3, seed=5)
    hi = (np.where(c[0] >= 63, 255, c[0]).astype(np.uint8), np.where(c[1] >= 63, 200, c[1]).astype(np.uint8), c[2], c[3])
    _same(api.cohort_prior_host(*hi), api.cohort_prior_host(np.minimum(c[0], 63), np.minimum(c[1], 63), c[2], c[3]))
    L, p = api.lib(), api._ptr
    gt, gq, q = np.empty((3, 65), np.uint8), np.empty((3, 65), np.int32), np.empty(65)
    call = lambda n_sites=65, n_samples=3, iters=8, pseudo=2.0, q_out=q: _lib.VG_ERRORS.get(
        L.vg_cprior_host(p(c[0]), p(c[1]), n_sites, n_samples, p(c[2]), p(c[3]), iters, pseudo, 1, p(gt), p(gq), None if q_out is None else p(q_out)), 0)
    assert call() == 0 and call(q_out=None) == 0
    assert call(n_samples=0) == "VG_EINVAL" and call(n_samples=16385) == "VG_ETOOBIG" and call(n_sites=2 ** 32) == "VG_EINVAL"
    assert call(iters=0) == "VG_EINVAL" and call(iters=65) == "VG_EINVAL"
    assert call(pseudo=-1.0) == "VG_EINVAL" and call(pseudo=float("inf")) == "VG_EINVAL" and call(pseudo=float("nan")) == "VG_EINVAL"
    assert _lib.VG_ERRORS.get(L.vg_cprior_host(None, p(c[1]), 65, 3, p(c[2]), p(c[3]), 8, 2.0, 1, p(gt), p(gq), None)) == "VG_EINVAL"
    # the handle's calls say so without a handle; create checks its sizes before it looks for a device
    assert _lib.VG_ERRORS.get(L.vg_cprior_set(None, 0, p(c[0]), p(c[1]))) == "VG_EINVAL" and _lib.VG_ERRORS.get(L.vg_cprior_calls(None, 0, p(gt), p(gq))) == "VG_EINVAL"
    assert L.vg_cprior_device_bytes(None) == 0
    h = C.c_void_p()
    assert _lib.VG_ERRORS.get(L.vg_cprior_create(0, 10, 0, C.byref(h))) == "VG_EINVAL" and _lib.VG_ERRORS.get(L.vg_cprior_create(0, 10, 16385, C.byref(h))) == "VG_ETOOBIG"
    assert _lib.VG_ERRORS.get(L.vg_cprior_create(0, 2 ** 32, 1, C.byref(h))) == "VG_EINVAL" and not h.value


# ---- jointvcf ---------------------------------------------------------------------------------------------------------------------
PRIOR = {"VARGENO_JOINT_PRIOR": "cohort"}
HEADER_LINE = b"##vargenoPrior=cohort,iters=8,pseudo=2\n"
CELL = {1: "0/0", 2: "1/1", 3: "0/1"}


def _table(path):
    return np.loadtxt(path, dtype=np.int64, ndmin=2)                           # pos ref_freq alt_freq ref_cnt alt_cnt


def test_jointvcf_writes_the_restated_columns(tmp_path):
    """The three-sample scenario of test_joint_text_cpu.py (one site per record): every line's cells are the restatement's calls of
    its site, the header says so once in front of #CHROM, the variable unset or empty gives the bytes of before -- on the host and
    the planned text routes, with and without the INFO counts."""
    chrlens, src, samples, env = CPU._scenarios(tmp_path)["three samples"]
    tabs = [_table(path) for _, path in samples]
    gt, gq, _ = CC.expected(np.array([t[:, 3] for t in tabs]), np.array([t[:, 4] for t in tabs]), tabs[0][:, 1], tabs[0][:, 2])
    lens, before = [ln.split() for ln in open(chrlens)], {}
    for name, ln in lens:
        before[name] = sum(int(x) for _, x in lens[:[n for n, _ in lens].index(name)])
    site_of = {int(p): i for i, p in enumerate(tabs[0][:, 0])}
    base, out = str(tmp_path / "base.vcf"), str(tmp_path / "prior.vcf")
    assert CPU._jointvcf(chrlens, src, samples, base, env).returncode == 0
    p = CPU._jointvcf(chrlens, src, samples, out, dict(env, VARGENO_VERBOSE="1", **PRIOR))
    assert p.returncode == 0 and "cohort prior: host (" in p.stderr and ", 4500 sites, 3 samples, " in p.stderr, p.stderr
    got, want = open(out, "rb").read(), open(base, "rb").read()
    assert got.count(HEADER_LINE) == 1 and got.index(HEADER_LINE) + len(HEADER_LINE) == got.index(b"#CHROM") and HEADER_LINE not in want
    lines, shown, changed = [ln for ln in got.decode().split("\n") if ln and ln[0] != "#"], 0, 0
    for ln in lines:
        f = ln.split("\t")
        i = site_of[before["chr" + f[0]] + int(f[1])]
        assert f[8] == "GT:GQ" and f[9:] == ["./.:." if gt[s][i] == 0 else "%s:%d" % (CELL[int(gt[s][i])], gq[s][i]) for s in range(3)], ln
        shown += 1
    assert shown == int((gt != 0).any(axis=0).sum()) > 1000
    old = {tuple(ln.split("\t")[:2]): ln for ln in want.decode().split("\n") if ln and ln[0] != "#"}
    changed = sum(1 for ln in lines if old[tuple(ln.split("\t")[:2])] != ln)
    assert len(old) == len(lines) and changed >= 1                               # the same lines, other cells
    # unset and empty: the bytes of before
    again = str(tmp_path / "again.vcf")
    assert CPU._jointvcf(chrlens, src, samples, again, dict(env, VARGENO_JOINT_PRIOR="")).returncode == 0 and open(again, "rb").read() == want
    # the other consumers take the columns as they are
    for more in ({"VARGENO_JOINT_TEXT": "planned", "VARGENO_JOINT_TEXT_LINES": "97"}, {"VARGENO_JOINT_PRIOR_ROUTE": "device"}, {"VARGENO_JOINT_PRIOR_ROUTE": "host"}):
        assert CPU._jointvcf(chrlens, src, samples, again, dict(env, **PRIOR, **more)).returncode == 0 and open(again, "rb").read() == got, more
    info = {"VARGENO_JOINT_INFO": "counts"}
    assert CPU._jointvcf(chrlens, src, samples, again, dict(env, **PRIOR, **info)).returncode == 0
    counted = open(again, "rb").read()
    assert counted.index(b"##INFO=<ID=AF,") < counted.index(HEADER_LINE) < counted.index(b"#CHROM")
    planned = str(tmp_path / "planned.vcf")
    assert CPU._jointvcf(chrlens, src, samples, planned, dict(env, VARGENO_JOINT_TEXT="planned", **PRIOR, **info)).returncode == 0 and open(planned, "rb").read() == counted
    import jinfo_cases as JI
    stripped, found = JI.strip_info(counted)
    assert stripped == got and len(found) == shown and all((ns, an, ac) == JI.cells_counts(ln) for ln, ns, an, ac, _ in found)


def test_a_wrong_value_and_a_wrong_route_are_refused_in_one_line_with_no_output(tmp_path):
    out = str(tmp_path / "never.vcf")
    for args in (["jointvcf", "no_chrlens", "no.vcf", out, "A=no_counts"], ["joint", "no_index", "no_manifest", "no.vcf", out]):
        p = subprocess.run([BIN] + args, env=dict(os.environ, VARGENO_JOINT_PRIOR="1"), capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and p.stderr.count("\n") == 1 and "VARGENO_JOINT_PRIOR=1 is not understood" in p.stderr and "cohort" in p.stderr, p.stderr
        p = subprocess.run([BIN] + args, env=dict(os.environ, VARGENO_JOINT_PRIOR="cohort", VARGENO_JOINT_PRIOR_ROUTE="gpu"), capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and p.stderr.count("\n") == 1 and "VARGENO_JOINT_PRIOR_ROUTE=gpu is not understood" in p.stderr and "device" in p.stderr and "host" in p.stderr, p.stderr
        assert not os.path.exists(out)


def test_the_header_is_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """tests/cprior_check.cpp: the header's host loop on exact-size heap buffers against a naive loop -- compiled with
    -fsanitize=address,undefined and run on its own, nothing preloaded."""
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(here, "..", "vargeno_amd", "csrc")
    exe = str(tmp_path / "cprior_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-march=x86-64-v2", "-I" + csrc,
                           os.path.join(here, "cprior_check.cpp"), "-o", exe, "-lpthread"])
    p = subprocess.run([exe], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"), capture_output=True, text=True)
    assert p.returncode == 0 and "ok" in p.stdout, (p.stdout[-500:], p.stderr[-2000:])

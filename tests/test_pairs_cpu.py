"""CPU suite of the pairwise sample table: vg_pairs_host (vargeno_amd/csrc/vg_pairs.h on host threads) against the numpy oracle of
tests/pairs_cases.py, the table's text through the hidden `vargeno pairstsv`, and the header's host loop under AddressSanitizer +
UBSan in a program of its own.  Every comparison is exact; no device is involved."""
import os
import subprocess

import numpy as np
import pytest

import pairs_cases as PC
from conftest import BIN
from vargeno_amd import api

SHAPES = [(n, s) for n in (1, 2, 3, 17) for s in (0, 1, 63, 64, 65, 1000)]


@pytest.mark.parametrize("n_samples,n_sites", SHAPES)
def test_pairs_host_equals_the_oracle(n_samples, n_sites):
    for min_gq in (0, 20):
        gt, gq = PC.make_case(n_samples, n_sites, min_gq, seed=1000 * n_samples + n_sites + min_gq)
        want = PC.oracle(gt, gq, min_gq)
        got = api.pairs_host(gt, gq, min_gq=min_gq, threads=1)
        assert got.dtype == np.uint64 and got.shape == (n_samples, n_samples, 5)
        assert np.array_equal(got, want)
        assert np.array_equal(api.pairs_host(gt, gq, min_gq=min_gq, threads=3), got)
        PC.check_identities(got)
        PC.check_adversaries(got, gt, gq, min_gq)
        if n_sites == 0:
            assert not got.any()


def test_int_min_is_never_counted_and_the_default_threshold_is_zero():
    gt = np.array([[1, 2, 3, 3, 0, 1]], np.uint8)
    gq = np.array([[PC.INT_MIN, -1, 0, 7, 50, 2147483647]], np.int32)
    c = api.pairs_host(gt, gq)
    assert c[0, 0].tolist() == [3, 0, 3, 2, 2]
    assert np.array_equal(c, PC.oracle(gt, gq, 0))
    assert api.pairs_host(gt, gq, min_gq=PC.INT_MIN)[0, 0].tolist() == [5, 0, 5, 2, 2]


def both_thread_counts(gt, gq, min_gq):
    """The host table, which one and three threads agree on and which is the oracle's."""
    got = api.pairs_host(gt, gq, min_gq=min_gq, threads=1)
    assert np.array_equal(got, PC.oracle(gt, gq, min_gq))
    assert np.array_equal(api.pairs_host(gt, gq, min_gq=min_gq, threads=3), got)
    PC.check_identities(got)
    return got


@pytest.mark.parametrize("n_samples,n_sites", [(2, 321), (5, 449), (33, 1000)])
def test_gt_values_above_three_are_not_counted(n_samples, n_sites):
    """make_case(wild_gt=True): 4, 5, 7, 128 .. 131 and 255 are no calls, whatever their low bits and their gq."""
    min_gq, seed = 20, 31 * n_samples + n_sites
    gt, gq = PC.make_case(n_samples, n_sites, min_gq, seed, wild_gt=True)
    plain_gt, plain_gq = PC.make_case(n_samples, n_sites, min_gq, seed)
    wild = np.isin(gt, PC.WILD_GT)
    assert wild.any(axis=1).all() and np.array_equal(plain_gt[~wild], gt[~wild]) and np.array_equal(plain_gq, gq)
    assert ((gt[wild] & 3 != 0) & (gq[wild] >= min_gq)).any()                   # some would count if only the low bits were read
    got = both_thread_counts(gt, gq, min_gq)
    PC.check_adversaries(got, gt, gq, min_gq)
    plain = both_thread_counts(plain_gt, plain_gq, min_gq)
    assert got[0, 0, 0] < plain[0, 0, 0] and (got <= plain)[:, :, 0].all()
    # no wild value is in any plane: with every other entry missing the table is empty, and alone they take nothing away
    assert not both_thread_counts(np.where(wild, gt, 0).astype(np.uint8), gq, min_gq).any()
    assert np.array_equal(both_thread_counts(np.where(wild, 0, gt).astype(np.uint8), gq, min_gq), got)


@pytest.mark.parametrize("n_samples,n_sites", [(37, 577), (5, 64)])
def test_the_residue_case_equals_its_closed_form(n_samples, n_sites):
    """The table counted by hand from the residues of the sites (residue_table: no oracle, no matrix product) is the oracle's and
    the host loop's."""
    gt, gq = PC.residue_case(n_samples, n_sites)
    want = PC.residue_table(n_samples, n_sites)
    assert want.dtype == np.uint64 and want[0, 1, 0] > 0 and want[0, 1, 1] > 0 and want[2, 2, 3] > 0
    assert np.array_equal(want, PC.oracle(gt, gq, 0))
    assert np.array_equal(both_thread_counts(gt, gq, 0), want)


@pytest.mark.parametrize("n_sites", [1, 2, 63, 64, 65, 512, 513])
def test_saturated_planes(n_sites):
    """Whole words of one class: every counter is n_sites, n_sites - 1, n_sites - 2 or 0."""
    gt, gq = PC.saturated_case(n_sites, min_gq=20)
    got = both_thread_counts(gt, gq, 20)
    PC.check_saturated(got, n_sites)
    assert not api.pairs_host(gt, gq, min_gq=21).any()                           # every gq is exactly at the threshold


def test_pairs_host_refuses_bad_arguments():
    L = api.lib()
    out = np.zeros(5, np.uint64)
    gt, gq = np.zeros(4, np.uint8), np.zeros(4, np.int32)
    p = lambda a: a.ctypes.data_as(api.C.c_void_p)
    assert L.vg_pairs_host(p(gt), p(gq), 4, 0, 0, 1, p(out)) == -1 and b"no samples" in L.vg_last_error()
    assert L.vg_pairs_host(None, p(gq), 4, 1, 0, 1, p(out)) == -1
    assert L.vg_pairs_host(p(gt), p(gq), 4, 1, 0, 1, None) == -1
    assert L.vg_pairs_host(p(gt), p(gq), 2 ** 32, 1, 0, 1, p(out)) == -1


def _write_calls(path, gt, gq):
    path.write_text("".join("%d %d\n" % (g, q) for g, q in zip(gt.tolist(), gq.tolist())))


def test_pairstsv_writes_the_table_the_oracle_formats(tmp_path):
    """Three samples (the third without a counted het: `nan` in the pairs it is in), at two thresholds, and a single-sample run."""
    gt, gq = PC.make_case(3, 301, 20, seed=5)
    gt[1] = np.random.default_rng(9).integers(0, 4, size=301)                   # (make_case's sample 1 is all-missing: give it calls)
    gt[2] = np.where(gt[2] == 3, 1, gt[2])                                      # no het
    names = ["NA1", "s-two", "third.sample"]
    args = []
    for k, nm in enumerate(names):
        _write_calls(tmp_path / ("calls%d.txt" % k), gt[k], gq[k])
        args.append("%s=%s" % (nm, tmp_path / ("calls%d.txt" % k)))
    for min_gq in (20, 0):
        out = tmp_path / ("pairs%d.tsv" % min_gq)
        p = subprocess.run([BIN, "pairstsv", str(out), str(min_gq)] + args, capture_output=True, text=True, timeout=60)
        assert p.returncode == 0, p.stderr
        want = PC.oracle(gt, gq, min_gq)
        assert want[0, 1, 0] > 50 and want[2, 2, 3] == 0
        text = out.read_text()
        assert text == PC.table_text(names, 301, min_gq, want)
        rows = [ln.split("\t") for ln in text.splitlines() if not ln.startswith("#")]
        assert len(rows) == 3 and rows[1][9] == "nan" and rows[2][9] == "nan" and rows[0][9] != "nan"
    one = tmp_path / "one.tsv"
    p = subprocess.run([BIN, "pairstsv", str(one), "0", args[0]], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr
    assert one.read_text() == PC.table_text(names[:1], 301, 0, PC.oracle(gt[:1], gq[:1], 0))
    assert one.read_text().splitlines()[-1].startswith("#sample_a\t")
    # files of different lengths are refused by name
    _write_calls(tmp_path / "short.txt", gt[0][:10], gq[0][:10])
    p = subprocess.run([BIN, "pairstsv", str(one), "0", args[0], "x=%s" % (tmp_path / "short.txt")], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "another number of sites" in p.stderr


def test_pair_header_is_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """tests/pairs_asan.cpp: the header's host pack + count on exact-size heap arrays against a naive per-site loop, S in
    {0, 1, 63, 64, 65, 129}, one and three threads, gt drawn from 0 .. 3, with values above 3 mixed in, and saturated (a sample all
    of one class at the threshold) -- compiled with -fsanitize=address,undefined and run on its own."""
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(here, "..", "vargeno_amd", "csrc")
    exe = str(tmp_path / "pairs_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-march=x86-64-v2", "-I" + csrc,
                           os.path.join(here, "pairs_asan.cpp"), "-o", exe, "-lpthread"])
    p = subprocess.run([exe], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"), capture_output=True, text=True)
    assert p.returncode == 0 and "ok" in p.stdout, (p.stdout[-500:], p.stderr[-2000:])

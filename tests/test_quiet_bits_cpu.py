"""The quiet bits of the merged view's entries (vargeno_amd/csrc/vg_quiet.h), on the CPU: the one function the loader's kernel and
the wave kernel share, against a scan position by position."""
import os
import subprocess

from conftest import CSRC


def test_quiet_bits_equal_a_scan_for_every_kmer_position_under_sanitizers(tmp_path):
    """tests/quiet_bits_check.cpp: hand-made pile-ups of 0 .. 449 positions -- empty, every bit set, one site at every position in turn
    (so for every k-mer position the site lies at kpos - 97, - 96, - 1, 0, 31, 32, 127, 128 and on both sides of every 64-bit block
    boundary), pairs of sites, random ones -- and every k-mer position from 0 (kpos < 96: positions below 0 hold no site) to 200 past
    the end (kpos + 128 at pile_len - 1, pile_len, pile_len + 1: a window past the end gets a clear bit); the rule
    (c == 0 || A) && (c == n - 1 || B) may only fire where the read's whole window is free of sites.  Compiled with
    -fsanitize=address,undefined and run on its own."""
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "quiet_bits_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I" + CSRC,
                           os.path.join(here, "quiet_bits_check.cpp"), "-o", exe])
    p = subprocess.run([exe], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"), capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("ok "), (p.stdout[-500:], p.stderr[-2000:])
    assert int(p.stdout.split()[1]) > 1_000_000                       # (the checks were really made)

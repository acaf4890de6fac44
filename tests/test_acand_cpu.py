"""Stage A's drained candidates (vargeno_amd/csrc/vg_acand.h; vg_wave.h, "DRAINED CANDIDATES"), on the CPU.

The look-up of a chunk hands every matching entry of its bucket to vg_acand_note and gets back an ordered list of at most six
candidates, which one loop then inserts into the key table.  tests/acand_check.cpp enumerates every combination of pass, strand
bit, palindrome, usable reverse block and 0 .. 4 matching entries (reference / SNP, either strand, flags hit, hit at POS_AMBIGUOUS,
ambiguous, PAIR, quiet A, quiet B, both) and compares the list, read slot by slot the way the kernel's drain reads it, with a plain
restatement of the per-site look-up the drain replaced -- and the state of the reverse block with it.  Under sanitizers, on its own."""
import os
import subprocess

from conftest import CSRC


def test_candidate_lists_equal_the_per_site_look_up_under_sanitizers(tmp_path):
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "acand_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I" + CSRC,
                           os.path.join(here, "acand_check.cpp"), "-o", exe])
    p = subprocess.run([exe], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"), capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("ok "), (p.stdout[-500:], p.stderr[-2000:])
    f = p.stdout.split()
    # 16 settings x (1 + 28 + 28^2 + 28^3 + 28^4) entry lists were really compared, the bound of six is reached, and lists with a
    # third reverse-strand candidate (which no index holds) were among them
    assert int(f[1]) >= 16 * (1 + 28 + 28 ** 2 + 28 ** 3 + 28 ** 4) and int(f[-1]) == 6 and int(f[3]) > 0, p.stdout

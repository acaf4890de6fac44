"""`vargeno cohort <index_prefix> <manifest> <input SNPs in VCF>`: what the command line decides before it touches a device.  The
manifest is read and validated first, so a bad one is refused with the line's number on any host; a good one on a host without a
device fails the way `geno` does there."""
import gzip
import os
import subprocess

from conftest import BIN, GOLDEN

NO_DEVICE = "no HIP device found"


def _cohort(cwd, prefix, manifest_text, vcf="snps.vcf"):
    man = os.path.join(cwd, "manifest.tsv")
    with open(man, "w") as f:
        f.write(manifest_text)
    return subprocess.run([BIN, "cohort", prefix, man, vcf], cwd=cwd, capture_output=True, text=True)


def test_an_empty_manifest_is_refused_before_any_device_is_touched(tmp_path):
    for text in ("", "\n\n# only a comment\n\n"):
        p = _cohort(str(tmp_path), "nope", text)
        assert p.returncode == 1, p.stderr
        assert "names no sample" in p.stderr and "manifest.tsv" in p.stderr
        assert NO_DEVICE not in p.stderr


def test_a_line_without_a_tab_is_refused_with_its_number(tmp_path):
    p = _cohort(str(tmp_path), "nope", "# cohort\na.fq\ta.vcf\n\nb.fq b.vcf\nc.fq\tc.vcf\n")
    assert p.returncode == 1, p.stderr
    assert "line 4" in p.stderr and "<TAB>" in p.stderr
    assert NO_DEVICE not in p.stderr
    # an empty field on either side of the tab is no sample either
    for bad in ("a.fq\t\n", "\ta.vcf\n"):
        p = _cohort(str(tmp_path), "nope", "x.fq\tx.vcf\n" + bad)
        assert p.returncode == 1 and "line 2" in p.stderr and NO_DEVICE not in p.stderr, p.stderr


def test_two_samples_with_one_output_are_refused_with_the_line_number(tmp_path):
    p = _cohort(str(tmp_path), "nope", "a.fq\tout/a.vcf\n# a comment\nb.fq\tout/b.vcf\nc.fq\tout/a.vcf\n")
    assert p.returncode == 1, p.stderr
    assert "line 4" in p.stderr and "out/a.vcf" in p.stderr and "line 1" in p.stderr
    assert NO_DEVICE not in p.stderr
    assert not os.path.exists(tmp_path / "out")


def test_a_wrong_argument_count_prints_the_usage_which_lists_cohort(tmp_path):
    for args in (["cohort"], ["cohort", "idx", "manifest.tsv"], ["cohort", "idx", "manifest.tsv", "snps.vcf", "extra"]):
        p = subprocess.run([BIN] + args, cwd=str(tmp_path), capture_output=True, text=True)
        assert p.returncode == 1
        assert "Usage: vargeno <option>" in p.stderr
        lines = [ln for ln in p.stderr.splitlines() if ln.startswith("cohort ")]
        assert len(lines) == 1 and "<index_prefix>" in lines[0] and "<input SNPs in VCF>" in lines[0], p.stderr
    # `index` and `geno` are listed as before
    assert any(ln.startswith("index ") for ln in p.stderr.splitlines()) and any(ln.startswith("geno ") for ln in p.stderr.splitlines())


def test_a_valid_manifest_needs_a_device_like_geno(ftiny_dir, tmp_path):
    """Without a device: the message and exit status of `geno` on the same host.  With one (the suite on a GPU box): the cohort of
    one sample writes the reference's VCF."""
    from vargeno_amd import _lib

    out = tmp_path / "a.vcf"
    prefix = os.path.join(ftiny_dir, "idx")
    p = _cohort(str(tmp_path), prefix, "%s\t%s\n" % (os.path.join(ftiny_dir, "reads.fq"), out), vcf=os.path.join(ftiny_dir, "snps.vcf"))
    if _lib.lib().vg_device_count() <= 0:
        g = subprocess.run([BIN, "geno", prefix, os.path.join(ftiny_dir, "reads.fq"), os.path.join(ftiny_dir, "snps.vcf"), str(tmp_path / "g.vcf")],
                           cwd=str(tmp_path), capture_output=True, text=True)
        assert g.returncode == 1 and NO_DEVICE in g.stderr
        assert p.returncode == 1 and [ln for ln in p.stderr.splitlines() if NO_DEVICE in ln] == [ln for ln in g.stderr.splitlines() if NO_DEVICE in ln]
        assert not out.exists()
    else:
        assert p.returncode == 0, p.stderr
        assert out.read_bytes() == gzip.open(os.path.join(GOLDEN, "ftiny.out.vcf.gz"), "rb").read()

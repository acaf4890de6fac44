"""The joint (multi-sample) VCF writer without a device: the hidden `vargeno jointvcf <chrlens> <snps.vcf> <out.vcf> <name>=<counts>
...` runs the writer of `vargeno joint` over counts tables in `callvcf`'s format, with the host caller.  The definition of the joint
file is "per sample what that sample's own VCF would show", so every check here is against `callvcf` (pinned to the reference by
test_host_tools.py) on the same counts.  Then what `vargeno joint` decides before it touches a device: its manifest and its usage."""
import os
import random
import subprocess

from conftest import BIN

HEADER8 = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"
NO_DEVICE = "no HIP device found"
MISSING = "./.:."


def _write(path, text):
    with open(path, "w") as f:
        f.write(text)
    return str(path)


def _callvcf(tmp, chrlens, counts, src, name, env=None):
    out = str(tmp / (name + ".single.vcf"))
    subprocess.check_call([BIN, "callvcf", chrlens, counts, src, out], env=env)
    return out


def _jointvcf(tmp, chrlens, src, samples, env=None, name="joint.vcf"):
    out = str(tmp / name)
    subprocess.check_call([BIN, "jointvcf", chrlens, src, out] + ["%s=%s" % (n, c) for n, c in samples], env=env)
    return out


def _data(path):
    return [ln for ln in open(path).read().split("\n") if ln and ln[0] != "#"]


def _check_against_singles(src_lines, joint_path, single_paths, key=lambda c: (c[0], c[1], c[2])):
    """Every joint line, in the input's order: the record's first eight fields, GT:GQ, and per sample the sample column of that
    sample's own VCF for the record (./.:. where it lacks the record); the records written are the union of the singles'.
    key: what identifies a record of the input (repeated records give identical lines, so a dictionary is enough)."""
    singles = []
    for p in single_paths:
        d = {}
        for ln in _data(p):
            c = ln.split("\t")
            assert c[-2] == "GT:GQ"
            d[key(c)] = c[-1]
        singles.append(d)
    expect = []
    for ln in src_lines:
        c = ln.split("\t")
        if len(c) < 2:
            continue
        cols = [d.get(key(c), MISSING) for d in singles]
        if any(v != MISSING for v in cols):
            expect.append("\t".join(c[:8] + ["GT:GQ"] + cols))
    got = _data(joint_path)
    assert got == expect
    return got


def test_one_sample_named_donor_is_the_single_sample_vcf(tmp_path):
    rng = random.Random(5)
    chrlens = _write(tmp_path / "chrlens", "chr1 5000\nchr2 3000\n")
    sites = sorted(rng.sample(range(1, 8000), 1500))
    counts = _write(tmp_path / "counts.txt", "".join("%d %d %d %d %d\n" % (g, rng.randrange(256), rng.randrange(256), rng.choice([0, 0, 3, 20, 63]), rng.choice([0, 1, 9, 63])) for g in sites))
    lines = ["%s\t%d\trs%d\tA\tC\t.\t.\tRS=%d" % ((("1", g) if g <= 5000 else ("2", g - 5000)) + (i, i)) for i, g in enumerate(sites)]
    src = _write(tmp_path / "in.vcf", "##fileformat=VCFv4.0\n##source=test\n" + HEADER8 + "\n" + "\n".join(lines) + "\n")
    single = _callvcf(tmp_path, chrlens, counts, src, "donor")
    joint = _jointvcf(tmp_path, chrlens, src, [("DONOR", counts)])
    assert open(joint, "rb").read() == open(single, "rb").read()
    assert len(_data(joint)) > 500


def _three_samples(tmp_path, rng, chroms, per_chrom):
    chrlens = _write(tmp_path / "chrlens", "".join("%s %d\n" % c for c in chroms))
    sites, before = [], 0
    for name, ln in chroms:
        for p in sorted(rng.sample(range(1, ln), per_chrom)):
            sites.append((name, p, before + p))
        before += ln
    freqs = [(rng.choice([230, 200, 128, 25]), rng.choice([25, 60, 128, 250])) for _ in sites]
    kinds = [(20, 0), (0, 20), (10, 10), (0, 0), (3, 1), (63, 63), (63, 0)]
    plan = [rng.randrange(4) for _ in sites]               # 0: called in no sample, 1: in one, 2: in all, 3: whatever comes
    counts = []
    for s in range(3):
        rows = []
        for i, (_, _, g) in enumerate(sites):
            if plan[i] == 0:
                rc, ac = rng.choice([(0, 0), (63, 63)])
            elif plan[i] == 1:
                rc, ac = rng.choice(kinds[:3]) if i % 3 == s else (0, 0)
            elif plan[i] == 2:
                rc, ac = rng.choice([k for k in kinds if k not in ((0, 0), (63, 63))])
            else:
                rc, ac = rng.choice(kinds)
            rows.append("%d %d %d %d %d\n" % (g, freqs[i][0], freqs[i][1], rc, ac))
        counts.append(_write(tmp_path / ("counts%d.txt" % s), "".join(rows)))
    return chrlens, sites, counts, plan


def test_three_samples_column_by_column(tmp_path):
    rng = random.Random(20261018)
    chroms = [("chr1", 50_000), ("chr2", 30_000), ("chrX", 20_000)]
    chrlens, sites, counts, plan = _three_samples(tmp_path, rng, chroms, 4000)
    lines = ["%s\t%d\trs%d\tA\tC\t.\t.\tRS=%d" % (name[3:], p, i, i) for i, (name, p, _) in enumerate(sites)]
    src = _write(tmp_path / "in.vcf", "##fileformat=VCFv4.0\n" + HEADER8 + "\n" + "\n".join(lines) + "\n")
    singles = [_callvcf(tmp_path, chrlens, c, src, "s%d" % k) for k, c in enumerate(counts)]
    joint = _jointvcf(tmp_path, chrlens, src, [("alpha", counts[0]), ("beta", counts[1]), ("gamma", counts[2])])
    got = _check_against_singles(lines, joint, singles)
    head = [ln for ln in open(joint).read().split("\n") if ln.startswith("#")]
    assert head[-1] == HEADER8 + "\tFORMAT\talpha\tbeta\tgamma"
    assert [ln for ln in head if "##FORMAT=<ID=GT," in ln] and [ln for ln in head if "##FORMAT=<ID=GQ," in ln] and len(head) == 4
    # sites called in none, in one and in all of the samples are all there
    by_id = {ln.split("\t")[2]: ln.split("\t")[9:] for ln in got}
    n_missing = [sum(v == MISSING for v in by_id.get("rs%d" % i, [MISSING] * 3)) for i in range(len(sites))]
    assert n_missing.count(3) > 1000 and n_missing.count(2) > 1000 and n_missing.count(0) > 1000
    assert all(n_missing[i] == 3 for i in range(len(sites)) if plan[i] == 0)
    assert len(got) == sum(m < 3 for m in n_missing)


def test_the_order_of_the_list_and_the_thread_count_do_not_matter(tmp_path):
    """The list of test_vcf_pass_finds_every_record_whatever_the_order_of_the_list: shuffled, records repeated, positions that name
    no site, a non-canonical spelling, an unknown chromosome, padded past the size from which the pass cuts its text into pieces."""
    rng = random.Random(20261004)
    chroms = [("chr1", 50_000), ("chr2", 30_000), ("chrX", 20_000)]
    chrlens, sites, counts, _ = _three_samples(tmp_path, rng, chroms, 4000)
    recs = ["%s\t%d\trs%d\tA\tC\t.\t.\tRS=%d" % (name[3:], p, i, i) for i, (name, p, _) in enumerate(sites)]
    extra = ["1\t%d\tnone%d\tA\tC\t.\t.\t." % (50_001 + k, k) for k in range(50)]
    extra += ["2\t0%d\tzero%d\tA\tC\t.\t.\t." % (sites[4000 + k][1], k) for k in range(50)]
    extra += ["7\t%d\tother%d\tA\tC\t.\t.\t." % (k + 1, k) for k in range(50)]
    filler = ["9\t%d\tfill%d\tA\tC\t.\t.\tPADDING=%s" % (k + 1, k, "x" * 60) for k in range(12_000)]
    shuffled = recs + recs[:500] + extra + filler
    rng.shuffle(shuffled)
    text = "##fileformat=VCFv4.0\n" + HEADER8 + "\n" + "\n".join(shuffled) + "\n"
    assert len(text) > (1 << 20)
    src = _write(tmp_path / "in.vcf", text)
    singles = [_callvcf(tmp_path, chrlens, c, src, "s%d" % k, env=dict(os.environ, VARGENO_THREADS="1")) for k, c in enumerate(counts)]
    names = [("a", counts[0]), ("b", counts[1]), ("c", counts[2])]
    one = _jointvcf(tmp_path, chrlens, src, names, env=dict(os.environ, VARGENO_THREADS="1"), name="t1.vcf")
    eight = _jointvcf(tmp_path, chrlens, src, names, env=dict(os.environ, VARGENO_THREADS="8"), name="t8.vcf")
    assert open(one, "rb").read() == open(eight, "rb").read()
    got = _check_against_singles(shuffled, one, singles)
    assert 6000 < len(got) and all(ln.split("\t")[2].startswith("rs") for ln in got)


def test_two_chromosomes_with_one_name_share_a_key_space(tmp_path):
    """Two sites under the key chr1$100; sample A has called only the earlier one: its column shows that site's call, B's shows
    the later site's -- per sample the last CALLED site in genome order, as in each sample's own VCF."""
    chrlens = _write(tmp_path / "chrlens", "chr1 1000\nchr1 1000\nchr2 1000\n")
    # genome positions 100 (first chr1), 1100 (second chr1, local 100), 1200 (second chr1, local 200), 2050 (chr2, local 50)
    a = _write(tmp_path / "a.txt", "100 230 25 20 0\n1100 230 25 0 0\n1200 230 25 10 10\n2050 230 25 0 0\n")
    b = _write(tmp_path / "b.txt", "100 230 25 20 0\n1100 230 25 0 20\n1200 230 25 0 0\n2050 230 25 0 0\n")
    lines = ["1\t100\tx\tA\tC\t.\t.\t.", "1\t200\ty\tA\tC\t.\t.\t.", "2\t50\tz\tA\tC\t.\t.\t."]
    src = _write(tmp_path / "in.vcf", HEADER8 + "\n" + "\n".join(lines) + "\n")
    singles = [_callvcf(tmp_path, chrlens, c, src, n) for n, c in (("a", a), ("b", b))]
    joint = _jointvcf(tmp_path, chrlens, src, [("A", a), ("B", b)])
    got = _check_against_singles(lines, joint, singles)
    cols = {ln.split("\t")[2]: ln.split("\t")[9:] for ln in got}
    assert cols["x"][0].startswith("0/0:") and cols["x"][1].startswith("1/1:")
    assert cols["y"][0].startswith("0/1:") and cols["y"][1] == MISSING
    assert "z" not in cols


def test_an_input_with_sample_columns_that_declares_gt_and_gq(tmp_path):
    chrlens = _write(tmp_path / "chrlens", "chr1 1000\n")
    a = _write(tmp_path / "a.txt", "10 230 25 20 0\n20 230 25 0 0\n30 230 25 5 5\n")
    b = _write(tmp_path / "b.txt", "10 230 25 0 20\n20 230 25 0 0\n30 230 25 0 0\n")
    head = ("##fileformat=VCFv4.0\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n"
            "##FORMAT=<ID=GQ,Number=1,Type=Integer,Description=\"Genotype Quality\">\n" + HEADER8 + "\tFORMAT\tOLD1\tOLD2\n")
    lines = ["1\t%d\tr%d\tA\tC\t.\t.\tX=1\tGT:GQ:DP\t0/0:5:9\t1/1:7:3" % (p, p) for p in (10, 20, 30)]
    src = _write(tmp_path / "in.vcf", head + "\n".join(lines) + "\n")
    joint = _jointvcf(tmp_path, chrlens, src, [("A", a), ("B", b)])
    text = open(joint).read()
    assert text.count("##FORMAT=<ID=GT,") == 1 and text.count("##FORMAT=<ID=GQ,") == 1
    assert "OLD1" not in text and "DP" not in text
    rows = text.split("\n")
    assert rows[3] == HEADER8 + "\tFORMAT\tA\tB"
    got = [r.split("\t") for r in rows[4:] if r]
    assert [g[2] for g in got] == ["r10", "r30"] and all(len(g) == 11 and g[7] == "X=1" and g[8] == "GT:GQ" for g in got)
    assert got[0][9].startswith("0/0:") and got[0][10].startswith("1/1:") and got[1][9].startswith("0/1:") and got[1][10] == MISSING
    # the calls are those of each sample's own VCF over the eight-column form of the same records
    src8 = _write(tmp_path / "in8.vcf", HEADER8 + "\n" + "\n".join("\t".join(ln.split("\t")[:8]) for ln in lines) + "\n")
    singles = [_callvcf(tmp_path, chrlens, c, src8, n) for n, c in (("a", a), ("b", b))]
    _check_against_singles(lines, joint, singles)


def _joint(cwd, manifest_text, prefix="nope"):
    man = os.path.join(cwd, "manifest.tsv")
    with open(man, "w") as f:
        f.write(manifest_text)
    return subprocess.run([BIN, "joint", prefix, man, "snps.vcf", os.path.join(cwd, "joint.vcf")], cwd=cwd, capture_output=True, text=True)


def test_joint_refuses_a_bad_manifest_before_any_device_is_touched(tmp_path):
    cwd = str(tmp_path)
    p = _joint(cwd, "a.fq\tS1\n# a comment\nb.fq\tS2\nc.fq\tS1\n")
    assert p.returncode == 1 and "line 4" in p.stderr and "S1" in p.stderr and "line 1" in p.stderr and NO_DEVICE not in p.stderr, p.stderr
    p = _joint(cwd, "# cohort\na.fq\tS1\n\nb.fq S2\n")
    assert p.returncode == 1 and "line 4" in p.stderr and "<TAB>" in p.stderr and NO_DEVICE not in p.stderr, p.stderr
    for text in ("", "\n# nothing\n"):
        p = _joint(cwd, text)
        assert p.returncode == 1 and "names no sample" in p.stderr and NO_DEVICE not in p.stderr, p.stderr
    for bad in ("b.fq\tS 2\n", "b.fq\tS2\textra\n"):
        p = _joint(cwd, "a.fq\tS1\n" + bad)
        assert p.returncode == 1 and "line 2" in p.stderr and "whitespace" in p.stderr and NO_DEVICE not in p.stderr, p.stderr
    assert not os.path.exists(os.path.join(cwd, "joint.vcf"))


def test_wrong_argument_counts_print_the_usage_which_lists_joint(tmp_path):
    for args in (["joint"], ["joint", "idx", "manifest.tsv", "snps.vcf"], ["joint", "idx", "manifest.tsv", "snps.vcf", "out.vcf", "extra"],
                 ["jointvcf", "chrlens", "snps.vcf", "out.vcf"], ["jointvcf", "chrlens", "snps.vcf", "out.vcf", "no_equals_sign"]):
        p = subprocess.run([BIN] + args, cwd=str(tmp_path), capture_output=True, text=True)
        assert p.returncode == 1, args
        assert "Usage: vargeno <option>" in p.stderr
        lines = [ln for ln in p.stderr.splitlines() if ln.startswith("joint ")]
        assert len(lines) == 1 and "<index_prefix>" in lines[0] and "<sample name>" in lines[0] and "<output file in VCF>" in lines[0], p.stderr

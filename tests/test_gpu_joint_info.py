"""The joint text kernels in the INFO mode (api.JointText(info=True): vg_jtext_create_info, vg_jtext_counts) against the Python
restatement of tests/jinfo_cases.py: the rendered text, the counts alone, the BGZF stream from an unaligned start, and heads whose
spliced bytes fall on and across the border of the write kernel's first 16 384-byte tile.  Every comparison is exact bytes."""
import gzip

import numpy as np
import pytest

import jinfo_cases as JI
import jtext_cases as JC
from vargeno_amd import api

pytestmark = pytest.mark.gpu


def _handle(c, **kw):
    head_bytes = max(64, len(c["heads"]), sum(r[1] for r in c["records"]))
    jt = api.JointText(c["n_sites"], c["n_samples"], max_records=max(1, len(c["records"])), max_head_bytes=head_bytes, max_site_refs=max(8, len(c["sites"])), **kw)
    for s, (g, q) in enumerate(zip(c["gt"], c["gq"])):
        if g is not None:
            jt.set(s, g, q)
    return jt


@pytest.mark.parametrize("n_samples,n_records,unset,drop,long_head", JC.shapes())
def test_render_and_counts_are_the_restated_rule(n_samples, n_records, unset, drop, long_head):
    c = JI.make_case(n_samples, n_records, seed=1000 * n_samples + n_records, unset=unset, drop=drop, long_head=long_head)
    want, counts = JI.expected(c), JI.expected_counts(c)
    with _handle(c, info=True) as jt:
        got_counts = jt.counts(c["heads"], c["records"], c["sites"])
        assert got_counts.shape == (n_records, 3) and np.array_equal(got_counts, counts)      # (first: a wrong text with right counts is the rendering's fault)
        got, lines = jt.render(c["heads"], c["records"], c["sites"], with_lines=True)
        assert got == want
        assert lines == want.count(b"\n")
        if n_records >= 64:
            half = n_records // 2
            assert jt.render(c["heads"], c["records"][:half], c["sites"]) == JI.expected(c, 0, half)
            assert np.array_equal(jt.counts(c["heads"], c["records"][half:], c["sites"]), counts[half:])
            assert jt.render(c["heads"], c["records"], c["sites"]) == want


def test_a_handle_without_the_mode_renders_todays_bytes_and_still_counts():
    c = JI.make_case(65, 200, seed=9, unset=(64,), drop=(0, 7, 199))
    with _handle(c) as jt:
        assert jt.render(c["heads"], c["records"], c["sites"]) == JC.expected(c)
        assert np.array_equal(jt.counts(c["heads"], c["records"], c["sites"]), JI.expected_counts(c))
        assert jt.render(c["heads"], c["records"], c["sites"]) == JC.expected(c)
    with _handle(c, info=False, bgzf=True) as jt:
        jt.bgzf_begin(block=1000)
        z = jt.bgzf_text(b"##x\n") + jt.bgzf_lines(c["heads"], c["records"], c["sites"]) + jt.bgzf_end()
        assert gzip.decompress(z) == b"##x\n" + JC.expected(c)


@pytest.mark.parametrize("pending", [1, 2, 3])
def test_the_stream_from_an_unaligned_start(pending):
    """The stream holds 1, 2 or 3 pending bytes when the span is rendered behind them: the first dword is shared with them."""
    c = JI.make_case(65, 300, seed=17, unset=(3,), drop=(0, 150))
    want = JI.expected(c)
    with _handle(c, info=True, bgzf=True) as jt:
        for block, codes in ((0, "fixed"), (1000, "dynamic")):
            jt.bgzf_begin(block=block, codes=codes)
            first = b"#" * (pending - 1) + b"\n"
            parts = [jt.bgzf_text(first)]
            blocks, text_bytes, lines = jt.bgzf_lines(c["heads"], c["records"][:120], c["sites"], with_counts=True)
            parts += [blocks, jt.bgzf_lines(c["heads"], c["records"][120:], c["sites"]), jt.bgzf_end()]
            assert text_bytes == len(JI.expected(c, 0, 120)) and lines == JI.expected(c, 0, 120).count(b"\n")
            assert b"".join(parts) == api.bgzf_deflate(first + want, device=None, block=block, codes=codes)
            assert gzip.decompress(b"".join(parts)) == first + want


BORDER = [(16380, "."), (16383, "."), (16384, "."), (16370, "RS=5;VC=SNV"), (16384 + 16380, "."), (16375, ""), (70_000, ".")]


@pytest.mark.parametrize("head_len,info", BORDER)
def test_the_splice_on_and_across_a_tile_border(head_len, info):
    """The render starts at byte 0 and the first record's head ends at the first border of the write kernel's tiles: the replaced
    ".", the ";" and the tag lie in front of it, on it and across it."""
    fixed = "7\t123456\t\tA\tC\t.\t.\t" + info
    head = fixed.replace("\t\tA", "\trs" + "9" * (head_len - len(fixed) - 2) + "\tA").encode()
    assert len(head) == head_len and head.count(b"\t") == 7
    c = JI.with_heads(JC.make_case(67, 40, seed=head_len), first=head, seed=1)
    _, _, site_at, n = c["records"][0]
    for g in c["gt"]:
        g[c["sites"][site_at:site_at + n]] = 3                                   # record 0 is written, a het in every sample
    want = JI.expected(c)
    kept = head_len - (info == ".")
    tag_at = kept + (1 if info not in (".", "") else 0)
    assert want[:kept] == head[:kept] and want[tag_at:tag_at + 25] == b"NS=67;AN=134;AC=67;AF=0.5"
    if head_len < 16384 + 16380 and head_len != 70_000:
        assert tag_at <= 16384 < tag_at + 25 + 7                                # the border falls in the tag or in "\tGT:GQ" behind it
    with _handle(c, info=True) as jt:
        assert np.array_equal(jt.counts(c["heads"], c["records"], c["sites"]), JI.expected_counts(c))
        assert jt.render(c["heads"], c["records"], c["sites"]) == want

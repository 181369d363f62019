"""tests/deflate_craft.py (an encoder that does what it is told), tests/lz_cases.py (the catalogue and the model of k_lz_stage's batching)
and the BAM files tests/test_gpu_inflate_edges.py makes of them, checked without a GPU: zlib accepts every stream and inflates it to the
tokens' plain expansion, every case reaches the branch it is named after, the files are what the CPU readers read."""
import zlib

import numpy as np
import pytest

from tests import deflate_craft as dc
from tests import lz_cases as lc

CASES = lc.all_cases()


def test_bit_writer_and_block_writers_against_zlib():
    rng = np.random.default_rng(1)
    data = rng.integers(0, 256, 3000, dtype=np.uint8).tobytes()
    for kind in ("stored", "fixed", "dynamic"):
        w = dc.BW()
        if kind == "stored":
            dc.stored(w, data, True)
        elif kind == "fixed":
            dc.fixed(w, list(data), True)
        else:
            dc.dynamic(w, list(data), *lc.plain_lens(), True)
        assert zlib.decompress(w.bytes(), -15) == data, kind
    t = [65, 66, 67, (3, 3), (258, 1), 68, (4, 2), (10, 268)]
    assert dc.expand(t) == b"ABCABC" + b"C" * 258 + b"D" + b"CDCD" + (b"ABCABC" + b"C" * 258 + b"DCDCD")[1:11]
    assert [dc.len_sym(x) for x in (3, 10, 11, 12, 257, 258)] == [(0, 0), (7, 0), (8, 0), (8, 1), (27, 30), (28, 0)]
    assert [dc.dist_sym(x) for x in (1, 4, 5, 6, 24577, 32768)] == [(0, 0), (3, 0), (4, 0), (4, 1), (29, 0), (29, 8191)]
    lens = [3, 3, 0, 0, 0, 5, 5, 5, 5, 5, 5, 5, 5] + [0] * 140 + [2, 0, 0]
    assert dc.expand_clseq(dc.rle(lens)) == lens and (18, 127) in dc.rle(lens) and (16, 3) in dc.rle(lens) and (17, 0) in dc.rle(lens)
    assert dc.kraft(dc.split_to({1: 2}, 200)) == 32768 and dc.kraft(dc.complete_clen_lens([0, 5, 18])) == 32768


def test_planner_on_a_hand_made_block():
    """P0a = the first match's position moved down to a 4-byte ADDRESS; far / in / straddle relative to it; a batch ends with the span or
    at 64 tokens"""
    t = [200] * 10 + [(4, 10)] + [201] * 2 + [(4, 8)] + [202] * 3000 + [(258, 3000)]
    b = lc.plan(t, out_off=1)
    assert [(x.P0, x.mis, x.P0a, x.classes()) for x in b] == [(10, 3, 7, ["far", "in"]), (3020, 1, 3019, ["far"])]
    assert b[0].fill == 20 - 7
    b = lc.plan(t, out_off=2)
    assert (b[0].P0a, b[0].classes()) == (10, ["far", "straddle"])
    assert lc.plan([200] * 9 + [(4, 2)], 2)[0].classes() == ["in+ov"] and lc.plan([200] * 9 + [(4, 2)], 0)[0].classes() == ["straddle+ov"]
    assert [len(x.toks) for x in lc.plan([200] * 3 + [(3, 3)] * 100, 0)] == [64, 36]
    assert lc.resolve_rounds([200] * 3 + [(3, 3)] * 100) == [64, 36]


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_case_is_valid_and_reaches_its_branch(case):
    """zlib inflates every block's payload to the tokens' expansion, no block is larger than a BGZF block may be, and the planner confirms
    the branch the case is named after (which depends on LZ_SPAN, read from the kernel's header)"""
    for b in case.blocks:
        assert len(b.data) <= 65536 and len(b.payload) + 26 <= 65536
    lc.check(case)
    if case.family in ("lz", "chains"):
        assert case.aim is not None and all(b.tokens is not None for b in case.blocks)


def test_a_changed_span_un_aims_the_cases_loudly():
    """with another LZ_SPAN the batches fall elsewhere: the span's edge case must notice"""
    c = lc.span_edge(0)
    c.aim(c.plans())
    off = c.offsets()
    with pytest.raises(AssertionError):
        c.aim([lc.plan(b.tokens, o, span=lc.SPAN - 4) for b, o in zip(c.blocks, off)])
    with pytest.raises(AssertionError):
        c.aim([lc.plan(b.tokens, o, span=lc.SPAN + 4) for b, o in zip(c.blocks, off)])


def test_the_bam_files_are_what_the_cpu_readers_read(tmp_path):
    """the files of tests/test_gpu_inflate_edges.py: every case's pattern begins at the address it wants, the records are there, the long
    ones counted"""
    from coverm_amd import bam as cbam
    from oracle import bamio
    from tests import test_gpu_inflate_edges as E
    for k, (name, make) in enumerate(E.FILES.items()):
        p = str(tmp_path / ("f%d.bam" % k))
        meta = E.build_file(p, make())
        assert b"".join(zlib.decompress(pl, -15) for _, _, pl, _ in meta["blocks"]) == meta["stream"]
        ob = bamio.read_bam(p)
        assert ob.n_records == meta["n"], name
        whole = cbam.read_alignment_file(p, threads=2, want_names=False)
        assert whole.records.n_records == meta["n"], name
        assert meta["long"] >= (0 if name.startswith("1 ") else 1)

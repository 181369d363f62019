"""csrc/gene_reads_core.h (the per-gene read aggregates of --gff as the kernels of csrc/gene_kernels.hip.h compute them: classification,
verdict keys, lower_bound over a contig's slice, the layout of the identity checkpoints) against tests/gene_reads_ref.py, the reference's
scan (genes.rs:258-304, 493-524) restated record by record.  tests/c/gene_reads_host.cpp is built twice, plainly and with
-fsanitize=address,undefined, and run as a program over the same cases.  Then covh_gene_coverage_reads, fed those aggregates, against
covh_gene_coverage over the records: the same text."""
import itertools
import os
import struct
import subprocess

import numpy as np
import pytest

from coverm_amd import host, native, synth
from tests import gene_reads_ref as G
from tests import harness_cli as cli
from tests import test_genes as TG
from tests.fixtures import load_fixture
from tests.golden import cases

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("gnrc")
    src = os.path.join(HERE, "c", "gene_reads_host.cpp")
    plain, san = str(d / "gene_reads_host"), str(d / "gene_reads_host_san")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", plain, src])
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", "-o", san, src])
    return str(d), (plain, san)


def f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", float(np.float32(x))))[0]


def f64_bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def write_case(fh, f, n_targets, rec, ivs, want):
    fh.write("S %d %d %d %d %d %d %x %x %d %d %d %d\n" % (f.include_improper_pairs, f.include_supplementary, f.include_secondary, f.filter_single, f.min_mapq,
                                                           f.min_aligned_length, f32_bits(f.min_percent_identity), f32_bits(f.min_aligned_percent), n_targets,
                                                           rec.n_records, len(ivs), want))
    for i in range(rec.n_records):
        w = rec.cigar[int(rec.cigar_off[i]):int(rec.cigar_off[i + 1])]
        fh.write("%d %d %d %d %d %d %d %d %s\n" % (rec.tid[i], rec.pos[i], rec.flag[i], rec.mapq[i], rec.nm[i], rec.nm_kind[i], rec.l_seq[i], len(w), " ".join(str(int(x)) for x in w)))
    for t, a, b in ivs:
        fh.write("%d %d %d\n" % (t, a, b))


RULE_STATUS = {0: G.ERR_NM_MISSING, 1: G.ERR_NM_BADTYPE, 2: G.ERR_UNSORTED, 3: G.ERR_BAD_TID}


def run_cases(programs, cases_, tag):
    """cases_: (Filter, n_targets, RecordBatch, intervals, want_identity).  Both builds; every line against the restatement."""
    d, exes = programs
    path = os.path.join(d, tag + ".txt")
    with open(path, "w") as fh:
        for c in cases_:
            write_case(fh, *c)
    want = []
    for f, nT, rec, ivs, wi in cases_:
        cl = G.classify_all(f, rec)
        want.append((cl, G.aggregates(f, nT, rec, ivs, wi, cl)))
    for exe in exes:
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (exe, r.stderr[-2000:])
        lines = iter(r.stdout.splitlines())
        for (f, nT, rec, ivs, wi), (cl, (status, _, rows, mapped, srt)) in zip(cases_, want):
            v = next(lines).split()
            assert v[0] == "V"
            key = int(v[1])
            got_cl = []
            for _ in range(rec.n_records):
                c = next(lines).split()
                got_cl.append((int(c[1]), int(c[2]), int(c[3]), int(c[4], 16)))
            assert got_cl == [(s, p, m, f64_bits(x)) for s, p, m, x in cl], (f, tag)
            if status != G.OK:
                assert key >= 0 and RULE_STATUS[key & 3] == status, (key, status, f)
                continue
            assert key == -1 and int(v[2]) == int(srt) and int(v[3]) == mapped, (v, srt, mapped)
            if not srt:
                continue
            for row in rows:
                g = next(lines).split()
                assert g[0] == "G" and (int(g[1]), int(g[2]), int(g[3], 16), int(g[4])) == (row[0], row[1], f64_bits(row[2]), row[3]), (g, row)
        assert next(lines, None) is None
    return want


def filters():
    for imp, supp, sec in itertools.product((False, True), repeat=3):
        yield G.Filter(imp, supp, sec, False, 255, 0, 0.0, 0.0)
        yield G.Filter(imp, supp, sec, True, 255, 0, 0.0, 0.0)
    yield G.Filter(True, True, False, True, 255, 0, float(np.float32(0.97001)), 0.0)
    yield G.Filter(True, True, False, True, 255, 0, float(np.float32(0.97)), 0.0)
    yield G.Filter(True, True, False, True, 10, 30, 0.0, float(np.float32(0.5)))
    yield G.Filter(True, True, True, True, 0, 0, 0.0, 0.0)


def test_classification(programs):
    """Every class of record under every filter, one record per case so that an NM error does not hide the records behind it."""
    recs = G.class_records(with_nm_errors=True)
    cases_ = []
    for f in filters():
        for r in recs:
            cases_.append((f, 2, G.batch_of([(0, 5) + r]), [(0, 0, 10)], 1))
    want = run_cases(programs, cases_, "classes")
    states = {cl[0][0] for cl, _ in want}
    assert states == {G.SKIP, G.TAKE, G.NM_MISSING, G.NM_BADTYPE}
    idents = [cl[0][3] for cl, _ in want if cl[0][0] == G.TAKE]
    assert min(idents) < 0 and max(idents) == 1.0
    # the f32 edge: 1 - 2999 / 100000 passes f32(0.97001) only as the reference rounds it
    edge = [G.classify(G.Filter(True, True, False, True, 255, 0, float(np.float32(0.97001)), 0.0), 0x2, 30, 1, nm, 100000, 100000, 0)[0] for nm in (2998, 2999, 3000)]
    assert edge[0] == G.TAKE and edge[2] == G.SKIP


def sample(seed, n_reads=3000, n_contigs=5):
    ref = synth.make_reference(n_contigs, 60_000, seed=seed, min_len=2000, max_len=30_000)
    return ref, synth.make_reads(ref, n_reads, seed=seed + 1)


def boundary_intervals(rec, ref_lens, classes, rng, n_random=20):
    ivs = []
    for t, L in enumerate(ref_lens):
        L = int(L)
        ivs += [(t, 0, L), (t, 0, 1), (t, L - 1, L)]
        st = sorted({int(rec.pos[i]) for i in range(rec.n_records) if rec.tid[i] == t and classes[i][0] == G.TAKE and 0 <= rec.pos[i] < L})
        for p in st[:3] + st[-3:] + [st[len(st) // 2]] if st else []:
            for a, b in ((p, p + 1), (p, min(L, p + 50)), (max(0, p - 1), p), (max(0, p - 1), min(L, p + 2)), (min(L - 1, p + 1), L), (0, max(1, p))):
                if a < b <= L:
                    ivs.append((t, a, b))
        for _ in range(n_random):
            a = int(rng.integers(0, L - 1))
            ivs.append((t, a, min(L, a + int(rng.integers(1, 4000)))))
    return ivs


def test_boundaries_and_sums(programs):
    """Equal starts, lo == hi, a gene in front of the first read and one behind the last, a contig without a taken record, hand-made records
    between the synthetic ones; with the single-read filter on and off, identity on and off."""
    rng = np.random.default_rng(3)
    ref, batch = sample(11)
    nT = len(ref.lengths)
    keep = np.flatnonzero(batch.tid != 2)                        # contig 2: no record at all
    batch = G.take(batch, keep)
    # hand-made records between the synthetic ones, at positions that keep the starts sorted
    extra = G.class_records()
    where = np.sort(rng.integers(1, batch.n_records - 1, len(extra)))
    parts, last = [], 0
    for w, r in zip(where, extra):
        parts.append(G.take(batch, np.arange(last, w)))
        parts.append(G.batch_of([(int(batch.tid[w - 1]), int(batch.pos[w - 1])) + r]))      # an equal start
        last = w
    parts.append(G.take(batch, np.arange(last, batch.n_records)))
    rec = G.concat(parts)
    cases_ = []
    for f in (G.Filter(True, True, False, False, 255, 0, 0.0, 0.0), G.Filter(False, False, True, False, 255, 0, 0.0, 0.0),
              G.Filter(True, True, False, True, 20, 50, float(np.float32(0.95)), float(np.float32(0.5)))):
        cl = G.classify_all(f, rec)
        ivs = boundary_intervals(rec, ref.lengths, cl, rng)
        for wi in (0, 1):
            cases_.append((f, nT, rec, ivs, wi))
    want = run_cases(programs, cases_, "bounds")
    for (f, nT_, rec_, ivs, wi), (cl, (status, _, rows, mapped, srt)) in zip(cases_, want):
        assert status == G.OK and srt and mapped > 1000
        assert any(r[3] == 0 for r in rows) and any(r[0] == 0 and r[3] > 0 for r in rows) and any(r[0] > 100 for r in rows)
        assert wi == 0 or any(r[2] != 0.0 and r[2] != float(r[0]) for r in rows)


def test_verdicts_and_fallback(programs):
    """The first offending record in file order decides; at one record: NM, then order, then the header.  Starts that decrease inside a contig
    are no error: sorted = 0."""
    f = G.Filter(True, True, False, False, 255, 0, 0.0, 0.0)
    M = G.cg((50, "M"))
    ok = lambda t, p: (t, p, 0x2, 30, 1, 1, 50, M)      # noqa: E731
    nm0, nm2 = (1, 10, 0x2, 30, 0, 0, 50, M), (1, 10, 0x2, 30, 0, 2, 50, M)
    skipped_nm0 = (1, 10, 0x4, 30, 0, 0, 50, M)                                   # unmapped: never asked for its NM
    rows = {"nm_missing": [ok(0, 5), nm0, ok(1, 20)], "nm_badtype": [ok(0, 5), nm2], "skipped": [ok(0, 5), skipped_nm0, ok(1, 20)],
            "tid_down": [ok(1, 5), ok(0, 5)], "tid_high": [ok(0, 5), ok(2, 5)], "tid_neg": [ok(-1, 5)], "tid_minus2_first": [ok(-2, 5), ok(0, 3)],
            "nm_then_order": [ok(1, 5), nm0, ok(0, 5)], "order_then_nm": [ok(1, 5), ok(0, 5), nm2], "high_then_down": [ok(0, 1), ok(5, 1), ok(1, 1)],
            "badtype_then_missing": [nm2, nm0], "starts_down": [ok(0, 9), ok(0, 8), ok(1, 1)], "starts_down_across_contigs": [ok(0, 9), ok(1, 8)],
            "negative_pos": [ok(0, 3), ok(0, -1)], "negative_pos_down": [ok(0, -1), ok(0, 3)], "empty": []}
    cases_ = [(f, 2, G.batch_of(r), [(0, 0, 10), (1, 0, 30)], 1) for r in rows.values()]
    want = dict(zip(rows, run_cases(programs, cases_, "verdicts")))
    st = {k: (v[1][0], v[1][4]) for k, v in want.items()}
    assert st["nm_missing"][0] == G.ERR_NM_MISSING and st["nm_badtype"][0] == G.ERR_NM_BADTYPE and st["skipped"] == (G.OK, True)
    assert st["tid_down"][0] == G.ERR_UNSORTED and st["tid_high"][0] == G.ERR_BAD_TID and st["tid_neg"][0] == G.ERR_BAD_TID
    assert st["tid_minus2_first"] == (G.OK, True)
    assert st["nm_then_order"][0] == G.ERR_NM_MISSING and st["order_then_nm"][0] == G.ERR_UNSORTED and st["high_then_down"][0] == G.ERR_BAD_TID
    assert st["badtype_then_missing"][0] == G.ERR_NM_BADTYPE
    assert st["starts_down"] == (G.OK, False) and st["starts_down_across_contigs"] == (G.OK, True)
    assert st["negative_pos"] == (G.OK, True) and st["negative_pos_down"] == (G.OK, False) and st["empty"] == (G.OK, True)


def test_checkpoint_slots_do_not_overlap(programs):
    d, exes = programs
    rng = np.random.default_rng(8)
    lists = [[0], [1], [1023], [1024], [1025], [2048, 0, 1024], [1023, 1, 1024, 1025, 0, 0, 4096]] + [rng.integers(0, 5000, 30).tolist() for _ in range(20)]
    path = os.path.join(d, "ck.txt")
    with open(path, "w") as fh:
        for ls in lists:
            cs, gap, parts = 0, 0, []
            for ln in ls:
                cs += gap                                      # contigs without genes lie between the slices
                parts.append("%d %d" % (cs, ln))
                cs += ln
                gap = int(rng.integers(0, 3000))
            fh.write("K %d %s\n" % (len(ls), " ".join(parts)))
    for exe in exes:
        out = subprocess.run([exe, path], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
        assert len(out) == len(lists)
        for ls, line in zip(lists, out):
            v = [int(x) for x in line.split()[1:]]
            slots, bases = v[0], v[1:]
            end = 0
            for ln, b in zip(ls, bases):
                assert b >= end                                 # behind the previous contig's last slot
                end = b + ln // 1024 + 1                         # slots 0 .. len / CK
            assert end <= slots


# ---- covh_gene_coverage_reads == covh_gene_coverage
def reads_of(records, cfg, n_targets):
    f = G.filter_of(cfg)
    classes = G.classify_all(f, records)

    def fn(ivs, want_identity):
        status, _, rows, mapped, srt = G.aggregates(f, n_targets, records, [(int(v["tid"]), int(v["start"]), int(v["end"])) for v in ivs], want_identity, classes)
        return status, (G.rows_array(rows) if rows is not None else None), mapped, srt
    return fn


@pytest.fixture
def through_the_aggregates(monkeypatch):
    """host.gene_coverage replaced by covh_gene_coverage_reads over aggregates computed here; the original kept for the comparison."""
    original = host.gene_coverage
    calls = []

    def patched(names, target_len, genes, stoit_name, records, cfg, depth_of, prim, taker, ests, print_zeros, namer_mode=0, separator="~", genome_of_tid=None,
                genome_names=None, session=None):
        rm, srt = host.gene_coverage_reads(names, target_len, genes, stoit_name, reads_of(records, cfg, len(names)), depth_of, prim, taker, ests, print_zeros,
                                           namer_mode, separator, genome_of_tid, genome_names, session)
        assert srt
        calls.append(stoit_name)
        return rm
    return original, patched, calls, monkeypatch


@pytest.mark.parametrize("case", cases.GENE_API_CASES, ids=[c["id"] for c in cases.GENE_API_CASES])
def test_entry_point_on_the_golden_api_cases(case, through_the_aggregates):
    original, patched, calls, mp = through_the_aggregates
    rm0 = TG._run_api_case(case, TG.FIXTURE_PROVIDER)
    mp.setattr(host, "gene_coverage", patched)
    rm1 = TG._run_api_case(case, TG.FIXTURE_PROVIDER)           # (asserts the expected text itself)
    assert calls and (rm0.num_mapped_reads, rm0.num_reads) == (rm1.num_mapped_reads, rm1.num_reads)


def test_entry_point_on_the_synthetic_sample(tmp_path, through_the_aggregates):
    """The synthetic sample and keyword sets of tests/test_genes.py: cli.run through covh_gene_coverage_reads == the oracle's text."""
    original, patched, calls, mp = through_the_aggregates
    mp.setattr(host, "gene_coverage", patched)
    TG._synthetic_cases(tmp_path, lambda b: TG.oracle_depth_provider(lambda af: b))
    assert len(calls) == 7


def test_entry_point_reports_unsorted_starts_and_errors():
    b = load_fixture("2seqs.bad_read.1.bam")
    af = TG.af_of(b, "tests/data/x.bam")
    genes = host.Genes.from_list([("g1", af.ref_names[0], 0, 100)])
    taker = host.CoverageTaker.new_single_float_coverage_streaming_coverage_printer()
    est = [host.CoverageEstimator.new_estimator_read_count()]
    depth_of = lambda tid: np.zeros(int(af.ref_lens[tid]), np.int32)      # noqa: E731
    rm, srt = host.gene_coverage_reads(af.ref_names, af.ref_lens, genes, "s", lambda ivs, wi: (0, None, 5, False), depth_of, 7, taker, est, True)
    assert not srt and taker.text() == ""
    for status, msg in ((G.ERR_UNSORTED, G.MSG_UNSORTED), (G.ERR_BAD_TID, G.MSG_BAD_TID)):
        with pytest.raises(host.HostError) as e:
            host.gene_coverage_reads(af.ref_names, af.ref_lens, genes, "s", lambda ivs, wi: (status, None, 0, False), depth_of, 7, taker, est, True)
        assert e.value.args and msg in str(e.value)
    assert native.INTERVAL_READS_DTYPE.itemsize == 32

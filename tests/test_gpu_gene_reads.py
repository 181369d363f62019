"""cov_interval_reads_compute (the per-gene read aggregates of --gff computed on the device from the session's record store, 32 bytes per
gene back and no record) against tests/gene_reads_ref.py, the reference's scan (genes.rs:206-304, 493-524) restated record by record, and
`coverm-amd --gff` behind a device reader against the oracle and against the run whose records come back (COVERM_GENE_READS_ON_HOST=1).
sum_identity is compared bit for bit: it is the difference of two serial f64 running sums, replayed on the device in file order."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from coverm_amd import bam as cbam
from coverm_amd import host, native, synth
from coverm_amd.engine import FilterConfig, RecordBatch, Session
from coverm_amd.native import CovError
from oracle import bamio
from oracle import oracle as O
from oracle.bamio import BamData
from tests import binary, samtext
from tests import gene_reads_ref as G
from tests.grouping import grouped_order, shuffles, take_bamdata
from tests.knobs import set_knobs
from tests.test_gene_reads_core import boundary_intervals

pytestmark = pytest.mark.gpu

TIMING = {"COVERM_CLI_TIMING": "1"}


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def check(got, mapped, srt, want):
    """Session.interval_reads' result against gene_reads_ref.aggregates'."""
    status, _, rows, want_mapped, want_sorted = want
    assert status == G.OK and want_sorted
    assert srt is True, "the device handed the sample to the host path"
    assert mapped == want_mapped
    exp = G.rows_array(rows)
    for k in ("n_reads", "mismatches", "contig_taken"):
        np.testing.assert_array_equal(got[k], exp[k], err_msg=k)
    bad = np.flatnonzero(bits(got["sum_identity"]) != bits(exp["sum_identity"]))
    assert len(bad) == 0, (len(bad), got["sum_identity"][bad[:5]], exp["sum_identity"][bad[:5]])


# ---- 1. ABI parity
@pytest.fixture(scope="module")
def mixed_sample():
    """6 contigs, ~30 000 synthetic reads, and the hand-made records of every class between them (each at the start of the record in front
    of it: an equal start, taken or skipped)."""
    rng = np.random.default_rng(31)
    ref = synth.make_reference(6, 400_000, seed=32, min_len=20_000, max_len=150_000)
    batch = synth.make_reads(ref, 30_000, seed=33)
    extra = G.class_records() * 3
    where = np.sort(rng.choice(np.arange(1, batch.n_records - 1), len(extra), replace=False))
    parts, last = [], 0
    for w, r in zip(where, extra):
        parts.append(batch.slice(last, int(w)))
        parts.append(G.batch_of([(int(batch.tid[w - 1]), int(batch.pos[w - 1])) + r]))
        last = int(w)
    parts.append(batch.slice(last, batch.n_records))
    return ref, G.concat(parts)


FILTERS = {"flags": FilterConfig(), "single": FilterConfig(True, True, False, True, 20, 50, float(np.float32(0.97001)), float(np.float32(0.5))),
           "proper_only_secondary_in": FilterConfig(False, False, True)}


@pytest.mark.parametrize("filt", list(FILTERS))
def test_abi_parity(mixed_sample, filt):
    ref, rec = mixed_sample
    f = G.filter_of(FILTERS[filt])
    classes = G.classify_all(f, rec)
    rng = np.random.default_rng(34)
    ivs = boundary_intervals(rec, ref.lengths, classes, rng, n_random=250)
    assert len(ivs) > 6 * 280
    with Session(0, FILTERS[filt], 0) as s:
        s.set_targets(ref.lengths)
        s.push(rec)
        for want_identity in (False, True):
            got, mapped, srt = s.interval_reads(ivs, want_identity)
            check(got, mapped, srt, G.aggregates(f, len(ref.lengths), rec, ivs, want_identity, classes))
            ms, launches = s.gene_reads_kernel_ms()
            assert launches == (7 if want_identity else 5) and ms > 0
        if filt == "flags":                                          # (the negative identity of the hand-made NM > aligned record shows)
            assert (got["sum_identity"] != 0).any() and (got["sum_identity"] < 0).any()
        got0, _, _ = s.interval_reads([], True)                     # no interval: the verdict and the count alone
        assert len(got0) == 0


# ---- 2. checkpoint and block edges
EDGE_N = (63, 64, 65, 1023, 1024, 1025, 2049)
PATTERNS = {"ones": [(100, 0)], "halves": [(100, 50), (100, 25), (100, 25), (100, 50)], "thirds": [(3, 1), (100, 3), (3, 1)],
            "negative_early": [(100, 0), (10, 2010), (100, 3), (3, 1), (100, 0)], "zeros": [(100, 100), (100, 0), (100, 100), (100, 100)]}


def test_checkpoint_and_block_edges():
    """One contig per (pattern, n) with exactly n taken records at positions 0 .. n - 1 and skipped records between them: a gene [a, b) has
    lo = a and hi = min(b, n), so the boundaries land on the block (64) and checkpoint (1024) edges by construction.  All 1.0 crosses the
    binades 2 .. 2048; 0.5 / 0.75 stay exact; 2 / 3 and 97 / 100 round at every step; the negative value (-200) keeps S < 0 (plain adds) over the
    first blocks, until the sum recovers; zeros take the integer path with nothing to add.  (An exact rounding tie needs ulp(S) above the identity's last
    bit: S >= 2^25 for identities made of CIGAR lengths — out of a quick test's reach; tests/test_gpu_identity_edges.py feeds such values
    to the same id_block_add through k_id_combine.)"""
    rows, lens, ivs = [], [], []
    for pat, seq in PATTERNS.items():
        for n in EDGE_N:
            t = len(lens)
            lens.append(n + 10)
            for j in range(n):
                al, nm = seq[j % len(seq)] if not (pat == "negative_early" and j >= 5) else seq[2 + j % 3]
                rows.append((t, j, 0x2, 30, nm, 1, al, G.cg((al, "M"))))
                if j % 3 == 0:
                    rows.append((t, j, 0x4, 0, 0, 0, 50, []))                               # unmapped, without NM: skipped
                if j % 7 == 0:
                    rows.append((t, j, 0x102, 30, 1, 1, 50, G.cg((50, "M"))))              # secondary: skipped by the default flag filter
            edges = sorted({e for e in (0, 63, 64, 65, 1023, 1024, 1025, n) if e <= n})
            ivs += [(t, a, min(b, n + 10)) for a in edges for b in edges + [n + 10] if a < b]
    rec = G.batch_of(rows)
    f = G.filter_of(FilterConfig())
    want = G.aggregates(f, len(lens), rec, ivs, True)
    exp = G.rows_array(want[2])
    assert exp["sum_identity"].max() == 2049.0 and exp["sum_identity"].min() < 0 and (exp["contig_taken"] == 1024).any()
    with Session(0, FilterConfig(), 0) as s:
        s.set_targets(lens)
        s.push(rec)
        got, mapped, srt = s.interval_reads(ivs, True)
        check(got, mapped, srt, want)


# ---- 3. errors
def copy_records(s):
    L = native.lib()
    n, nc = C.c_uint64(0), C.c_uint64(0)
    assert L.cov_copy_records(s._h, None, C.byref(n), C.byref(nc)) == 0
    n, nc = int(n.value), int(nc.value)
    a = dict(tid=np.zeros(n, np.int32), pos=np.zeros(n, np.int32), flag=np.zeros(n, np.uint16), mapq=np.zeros(n, np.uint8), nm=np.zeros(n, np.uint32),
             nm_kind=np.zeros(n, np.uint8), l_seq=np.zeros(n, np.uint32), cigar_off=np.zeros(n + 1, np.uint32), cigar=np.zeros(nc + 1, np.uint32))
    cb = native.CovBatch()
    for k, v in a.items():
        setattr(cb, k, v.ctypes.data)
    cb.n_records = n
    assert L.cov_copy_records(s._h, C.byref(cb), None, None) == 0
    return RecordBatch(**a)


M50 = G.cg((50, "M"))


def _ok(t, p):
    return (t, p, 0x2, 30, 1, 1, 50, M50)


NM0, NM2 = (1, 10, 0x2, 30, 0, 0, 50, M50), (1, 10, 0x2, 30, 0, 2, 50, M50)
ERROR_STORES = {"nm_missing": ([_ok(0, 5), (0, 6, 0x4, 0, 0, 0, 50, []), NM0, _ok(1, 20)], G.ERR_NM_MISSING),
                "nm_badtype": ([_ok(0, 5), NM2, _ok(1, 20)], G.ERR_NM_BADTYPE),
                "tid_decreasing": ([_ok(1, 5), (1, 6, 0x4, 0, 0, 0, 50, []), _ok(0, 5)], G.ERR_UNSORTED),
                "tid_outside_header": ([_ok(0, 5), _ok(2, 5)], G.ERR_BAD_TID),
                "nm_then_order": ([_ok(1, 5), NM0, _ok(0, 5)], G.ERR_NM_MISSING),
                "order_then_nm": ([_ok(1, 5), _ok(0, 5), NM2], G.ERR_UNSORTED),
                "outside_then_decreasing": ([_ok(0, 1), _ok(5, 1), _ok(1, 1)], G.ERR_BAD_TID),
                "badtype_then_missing": ([NM2, NM0], G.ERR_NM_BADTYPE)}


@pytest.mark.parametrize("name", list(ERROR_STORES))
def test_errors_are_the_host_drivers(name):
    """Status and message of covh_gene_coverage_reads over the session == covh_gene_coverage's over the same records copied back.  The
    errors are padded with 3000 good records in front, so that the first offender lies in a later tile than the store's first."""
    rows, status = ERROR_STORES[name]
    t0 = rows[0][0]
    rec = G.batch_of([_ok(t0, 1)] * 3000 + rows)
    names, lens = ["c0", "c1"], [1000, 1000]
    genes = host.Genes.from_list([("g0", "c0", 0, 100), ("g1", "c1", 0, 100)])
    est = [host.CoverageEstimator.new_estimator_read_count()]
    depth_of = lambda tid: np.zeros(lens[tid], np.int32)      # noqa: E731
    with Session(0, FilterConfig(), 0) as s:
        s.set_targets(lens)
        s.push(rec)
        back = copy_records(s)
        with pytest.raises(host.HostError) as on_host:
            host.gene_coverage(names, lens, genes, "s", back, s.cfg, depth_of, 0, host.CoverageTaker.new_single_float_coverage_streaming_coverage_printer(), est, True)
        with pytest.raises(host.HostError) as on_device:
            host.gene_coverage_reads(names, lens, genes, "s", None, depth_of, 0, host.CoverageTaker.new_single_float_coverage_streaming_coverage_printer(), est, True,
                                     reads_session=s)
        assert on_host.value.status == status and on_device.value.status == status
        assert str(on_device.value) == str(on_host.value)
        with pytest.raises(CovError) as abi:
            s.interval_reads([(0, 0, 100)])
        assert abi.value.status == status and abi.value.message
        if status in (G.ERR_UNSORTED, G.ERR_BAD_TID):
            assert abi.value.message in str(on_host.value)


# ---- 4. fallback and refusal
def test_decreasing_start_inside_a_contig_is_left_to_the_host():
    rec = G.batch_of([_ok(0, 1)] * 2000 + [_ok(0, 9), _ok(0, 8), _ok(1, 1)])
    with Session(0, FilterConfig(), 0) as s:
        s.set_targets([1000, 1000])
        s.push(rec)
        got, mapped, srt = s.interval_reads([(0, 0, 100)], True)
        assert got is None and srt is False and mapped == 2003
        s.reset()
        s.push(G.batch_of([_ok(0, 9), _ok(1, 8), _ok(1, 8)]))        # a start that decreases ACROSS contigs is in order
        got, mapped, srt = s.interval_reads([(0, 0, 100), (1, 8, 9), (1, 9, 10)])
        assert srt and got["n_reads"].tolist() == [1, 2, 0] and got["contig_taken"].tolist() == [1, 2, 2]


def test_refuses_after_a_spill(monkeypatch):
    set_knobs(monkeypatch, store_cap_records=20000, store_cap_cigar=200000)
    ref = synth.make_reference(60, 6_000_000, seed=41, min_len=1500, max_len=300_000)
    batch = synth.make_reads(ref, 60_000, seed=42)
    with Session(0, FilterConfig(), 75) as s:
        s.set_targets(ref.lengths)
        for lo in range(0, batch.n_records, 7001):
            s.push(batch.slice(lo, min(batch.n_records, lo + 7001)))
        assert s.store_spills() >= 1
        with pytest.raises(CovError) as e:
            s.interval_reads([(0, 0, 10)])
        assert e.value.status == native.ERR_STATE and "bounded record store" in e.value.message


def test_second_sample_after_reset_and_after_finish():
    """The work arrays are kept by the session: a larger sample, then a smaller one, then the call behind a finish."""
    f = G.filter_of(FilterConfig())
    rng = np.random.default_rng(51)
    with Session(0, FilterConfig(), 75, want_identity=True) as s:
        for seed, n_reads in ((52, 20_000), (54, 5_000)):
            ref = synth.make_reference(8, 300_000, seed=seed, min_len=5000, max_len=80_000)
            batch = synth.make_reads(ref, n_reads, seed=seed + 1)
            classes = G.classify_all(f, batch)
            ivs = boundary_intervals(batch, ref.lengths, classes, rng, n_random=20)
            want = G.aggregates(f, len(ref.lengths), batch, ivs, True, classes)
            s.reset()
            s.set_targets(ref.lengths)
            s.push(batch)
            check(*s.interval_reads(ivs, True), want)
            stats, _ = s.finish()
            check(*s.interval_reads(ivs, True), want)
            assert int(stats["n_primary"].sum()) == want[3]


# ---- 5. through the binary
@pytest.fixture(scope="module")
def binary_sample(tmp_path_factory):
    """The shapes of tests/test_genes.py::test_gene_coverage_through_the_binary_takes_the_device_ingest: 240 k reads, mates by adjacency."""
    d = tmp_path_factory.mktemp("gene_reads")
    ref = synth.make_reference(25, 1_500_000, seed=83, min_len=1500, max_len=200_000)
    batch = synth.make_reads(ref, 240_000, seed=84)
    n = batch.n_records
    i = np.arange(n, dtype=np.int64)
    m = i ^ 1
    same = (m < n) & (batch.tid[np.minimum(m, n - 1)] == batch.tid)
    b = BamData(ref.names, ref.lengths, batch.tid, batch.pos, batch.flag, batch.mapq, batch.l_seq.astype(np.int32), batch.nm, batch.nm_kind,
                batch.cigar_off, batch.cigar, batch.tid.copy(), np.zeros(n, np.int32), np.zeros(n, np.int32), [b"n%d" % k for k in np.where(same, i & ~1, i)], "")
    path = str(d / "syn.bam")
    cbam.write_bam(path, ref.names, ref.lengths, batch, with_seq=3, threads=4)
    rng = np.random.default_rng(5)
    lines = ["##gff-version 3"]
    for name, L in zip(ref.names, ref.lengths):
        for k in range(int(rng.integers(1, 9))):
            s = int(rng.integers(1, L))
            lines.append("%s\tsyn\tgene\t%d\t%d\t.\t+\t.\tID=%s_g%d" % (name, s, min(int(L), s + int(rng.integers(1, 3000))), name.replace("~", "_"), k))
    gff = d / "syn.gff"
    gff.write_text("\n".join(lines) + "\n")
    return dict(dir=d, ref=ref, b=b, path=path, gff=str(gff))


def run_both(mode, path, **kw):
    """The default run and the run whose records come back: (default process, host-aggregates process)."""
    dev = subprocess.run(binary.argv(mode, [path], **kw), capture_output=True, text=True, env=dict(os.environ, **TIMING), timeout=300)
    hst = subprocess.run(binary.argv(mode, [path], **kw), capture_output=True, text=True, env=dict(os.environ, COVERM_GENE_READS_ON_HOST="1", **TIMING), timeout=300)
    assert dev.returncode == 0 and hst.returncode == 0, (dev.stderr[-2000:], hst.stderr[-2000:])
    assert "--gff over the device ingest" in dev.stderr and "read aggregates on the device" in dev.stderr and "records came back" not in dev.stderr, dev.stderr[-3000:]
    assert "records came back from the store (COVERM_GENE_READS_ON_HOST)" in hst.stderr and "read aggregates on the device" not in hst.stderr
    assert dev.stdout == hst.stdout
    return dev, hst


@pytest.mark.parametrize("kw", [dict(methods=["mean", "variance", "covered_fraction", "count", "anir"]),
                                dict(methods=["mean", "trimmed_mean"], min_read_percent_identity=97, proper_pairs_only=True, output_format="sparse"),
                                dict(methods=["mean", "count"], min_read_percent_identity_pair=95, proper_pairs_only=True)], ids=["anir", "single_filter", "pair_filter"])
def test_through_the_binary(binary_sample, kw):
    S = binary_sample
    dev, _ = run_both("contig", S["path"], gff=S["gff"], **kw)
    assert dev.stdout == O.run_cli("contig", [S["path"]], bams=[S["b"]], gff=S["gff"], **kw)
    assert dev.stdout.count("\n") > 20


def test_through_the_binary_genome_mode(binary_sample):
    S = binary_sample
    kw = dict(methods=["mean", "count", "anir"], separator="~", min_covered_fraction=0, gff=S["gff"])
    dev, _ = run_both("genome", S["path"], **kw)
    assert dev.stdout == O.run_cli("genome", [S["path"]], bams=[S["b"]], **kw)


def test_through_the_binary_sam_text(tmp_path):
    ref = synth.make_reference(10, 400_000, seed=91, min_len=1500, max_len=100_000)
    batch = synth.make_reads(ref, 20_000, seed=92)
    z = np.zeros(batch.n_records, np.int32)
    b = BamData(ref.names, ref.lengths, batch.tid, batch.pos, batch.flag, batch.mapq, batch.l_seq.astype(np.int32), batch.nm, batch.nm_kind, batch.cigar_off,
                batch.cigar, z - 1, z - 1, z, [], "")
    p = str(tmp_path / "s.sam")
    samtext.write(p, b)
    lines = ["%s\tx\tCDS\t%d\t%d\t.\t+\t0\tID=g%d_%d" % (n, 1 + 97 * k, min(int(l), 400 + 211 * k), t, k) for t, (n, l) in enumerate(zip(ref.names, ref.lengths)) for k in range(4)]
    gff = tmp_path / "s.gff"
    gff.write_text("\n".join(lines) + "\n")
    kw = dict(methods=["mean", "count", "anir"], min_covered_fraction=0, gff=str(gff))
    dev, _ = run_both("contig", p, **kw)
    assert "device SAM decode" in dev.stderr
    assert dev.stdout == O.run_cli("contig", [p], bams=[bamio.read_sam(p)], **kw)


def test_unsorted_starts_through_the_binary_come_back(tmp_path):
    """A shuffled file under --unsorted is grouped by reference, not sorted: the device says so, the records come back, the text is
    the host path's (the oracle's over the grouped sequence)."""
    ref = synth.make_reference(12, 1_200_000, seed=23, min_len=1500, max_len=400_000)
    batch = synth.make_reads(ref, 20_000, seed=24)
    z = np.zeros(batch.n_records, np.int32)
    b = BamData(ref.names, ref.lengths, batch.tid, batch.pos, batch.flag, batch.mapq, batch.l_seq.astype(np.int32), batch.nm, batch.nm_kind, batch.cigar_off,
                batch.cigar, z, z, z, [], "")
    sh = take_bamdata(b, shuffles(len(b.tid), 24)["blocks"])
    p = str(tmp_path / "s.bam")
    bamio.write_bam(p, sh, level=1)
    rng = np.random.default_rng(25)
    lines = []
    for t, (n, l) in enumerate(zip(ref.names, ref.lengths)):
        for k in range(3):
            a = int(rng.integers(1, max(2, l - 600)))
            lines.append("%s\tx\tCDS\t%d\t%d\t.\t+\t0\tID=g%d_%d" % (n, a, min(int(l), a + int(rng.integers(50, 500))), t, k))
    gff = tmp_path / "s.gff"
    gff.write_text("\n".join(lines) + "\n")
    g = take_bamdata(sh, grouped_order(sh.tid, len(sh.ref_lens)))
    kw = dict(methods=["mean", "covered_fraction", "count"], min_covered_fraction=0, gff=str(gff))
    r = subprocess.run(binary.argv("contig", [p], **kw) + ["--unsorted"], capture_output=True, text=True, timeout=300, env=dict(os.environ, **TIMING))
    assert r.returncode == 0, r.stderr[-3000:]
    assert "records came back from the store (starts decrease inside a reference)" in r.stderr and "read aggregates on the device" not in r.stderr
    assert r.stdout == O.run_cli("contig", [p], bams=[g], **kw)

"""The contig-names genome scan on the device (cov_set_genomes / cov_fetch_genome_estimates / cov_fetch_genome_stats, the kernels of
csrc/genome_kernels.hip.h) against the host aggregation of the SAME session's per-contig statistics (covh_estimator_*: add_contig per
seen contig in ascending tid order, calculate_coverage with the unobserved lengths — what covh_genome_coverage_with_contig_names runs,
the reference's src/genome.rs:137-153, 252-302): the same f32 bit for bit, the same reads and lengths.  No tolerance: the accumulators
are integers and the one f64 sum has a prescribed order.  Then the product binary: `coverm-amd genome --genome-definition | -d -x` with
and without COVERM_HOST_ESTIMATES=1 equals the oracle's text, and the device path fetches no histogram."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from coverm_amd import bam as cbam
from coverm_amd import host, native, synth
from coverm_amd.engine import FilterConfig, RecordBatch, Session
from coverm_amd.host import CoverageEstimator as E
from coverm_amd.native import CovError
from oracle import oracle as O
from tests import binary
from tests.fixtures import load_fixture
from tests.golden import cases
from tests.knobs import set_knobs, with_knobs
from tests.test_gpu_abi_parity import to_bamdata, to_batch

pytestmark = pytest.mark.gpu


def estimator_sets(excl):
    """mean, trimmed_mean, covered_fraction, covered_bases, variance, length, count, reads_per_base, rpkm, anir — with and without a
    minimum covered fraction, several trims."""
    return [
        [E.new_estimator_mean(0.0, excl, False), E.new_estimator_trimmed_mean(0.05, 0.95, 0.0, excl), E.new_estimator_covered_fraction(0.0),
         E.new_estimator_covered_bases(0.0), E.new_estimator_variance(0.0, excl), E.new_estimator_length(), E.new_estimator_read_count(),
         E.new_estimator_reads_per_base(), E.new_estimator_rpkm(0.0), E.new_estimator_anir()],
        [E.new_estimator_mean(0.1, excl, True), E.new_estimator_trimmed_mean(0.1, 0.9, 0.1, excl), E.new_estimator_covered_fraction(0.1),
         E.new_estimator_covered_bases(0.5), E.new_estimator_variance(0.1, excl), E.new_estimator_rpkm(0.1),
         E.new_estimator_trimmed_mean(0.0, 1.0, 0.0, excl), E.new_estimator_trimmed_mean(0.25, 0.75, 0.0, excl)],
    ]


def _estimator_api():
    L = host._lib()
    L.covh_estimator_new.restype = C.c_void_p
    L.covh_estimator_new.argtypes = [C.c_void_p]
    L.covh_estimator_free.argtypes = [C.c_void_p]
    L.covh_estimator_setup.argtypes = [C.c_void_p]
    L.covh_estimator_add_contig_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_double]
    L.covh_estimator_calculate_coverage.restype = C.c_float
    L.covh_estimator_calculate_coverage.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    return L


def host_aggregation(st, hist, lens, g_of, n_genomes, est):
    """(floats n_genomes x n_est, reads_in_genome, genome_len, n_contigs_seen) from one session's per-contig statistics, by the host's own
    estimator states."""
    L = _estimator_api()
    lens = np.asarray(lens, np.uint64)
    order = np.argsort(g_of, kind="stable")
    order = order[g_of[order] >= 0]
    bounds = np.searchsorted(g_of[order], np.arange(n_genomes + 1))
    seen = st["n_pass"] > 0
    rows = np.zeros((n_genomes, len(est)), np.float32)
    hp = hist.ctypes.data if hist is not None and hist.size else None
    base = st.ctypes.data
    for k, e in enumerate(est):
        state = L.covh_estimator_new(C.byref(e))
        for g in range(n_genomes):
            tids = order[bounds[g]:bounds[g + 1]]
            L.covh_estimator_setup(state)
            for t in tids[seen[tids]]:
                L.covh_estimator_add_contig_stats(state, base + int(t) * st.dtype.itemsize, int(lens[t]), hp, int(st["n_pass"][t]),
                                                  float(st["sum_identity_nonsupp"][t]))
            un = np.ascontiguousarray(lens[tids[~seen[tids]]], np.uint64)
            rows[g, k] = L.covh_estimator_calculate_coverage(state, un.ctypes.data if un.size else None, un.size)
        L.covh_estimator_free(state)
    reads = np.zeros(n_genomes, np.uint64)
    glen = np.zeros(n_genomes, np.uint64)
    nseen = np.zeros(n_genomes, np.uint32)
    m = g_of >= 0
    np.add.at(reads, g_of[m], st["n_pass"][m])
    np.add.at(glen, g_of[m], lens[m])
    np.add.at(nseen, g_of[m], seen[m].astype(np.uint32))
    return rows, reads, glen, nseen


def check_sample(lens, batch, g_of, n_genomes, excl, ff=(True, True, False), sets=None, chunks=1):
    g_of = np.ascontiguousarray(g_of, np.int32)
    for est in (sets or estimator_sets(excl)):
        with Session(0, FilterConfig(*ff), excl, want_hist=True, want_identity="nonsupp") as s:
            s.set_targets(lens)
            s.set_genomes(g_of, n_genomes)
            s.set_estimators(est)
            edges = np.linspace(0, batch.n_records, chunks + 1).astype(int)
            for lo, hi in zip(edges[:-1], edges[1:]):
                s.push(batch.slice(lo, hi))
            st, summ = s.finish()
            ms, launches = s.genome_kernel_ms()
            assert launches > 0, "the genome kernels did not run"
            dev = s.genome_estimates()
            gs = s.genome_stats()
            with pytest.raises(CovError):
                s.estimates()                      # per-contig floats are not offered with a mask
            hist = s.hist()                        # the same finish's bins, for the host side of the comparison
            # cov_finish_genomes: the same results without the per-contig block on the host
            lean = s.finish_genomes()
            assert s.genome_kernel_ms()[1] > 0
            np.testing.assert_array_equal(s.genome_estimates().view(np.uint32), dev.view(np.uint32))
            np.testing.assert_array_equal(s.genome_stats(), gs)
            assert (lean.num_detected_primary_alignments, lean.n_records, lean.n_considered) == (
                summ.num_detected_primary_alignments, summ.n_records, summ.n_considered)
        rows, reads, glen, nseen = host_aggregation(st, hist, lens, g_of, n_genomes, est)
        for k in range(len(est)):
            bad = np.nonzero(dev[:, k].view(np.uint32) != rows[:, k].view(np.uint32))[0]
            assert bad.size == 0, ("estimator %d (kind %d), genome %d: device %r host %r" % (k, est[k].kind, bad[0], dev[bad[0], k], rows[bad[0], k]))
        np.testing.assert_array_equal(gs["reads_in_genome"], reads)
        np.testing.assert_array_equal(gs["genome_len"], glen)
        np.testing.assert_array_equal(gs["n_contigs_seen"], nseen)
        np.testing.assert_array_equal(gs["any_nonzero"] != 0, (rows > 0).any(axis=1))
        # the masked-out contigs take no part, as with cov_set_target_mask
        assert (st["win_sum_d"][g_of < 0] == 0).all()


_NAMES_FIXTURES = []
for _c in cases.API_CASES:
    if _c["api"] == "names" and (_c["bams"][0], _c["geco"]) not in [(b, g) for b, g, _ in _NAMES_FIXTURES]:
        _NAMES_FIXTURES.append((_c["bams"][0], _c["geco"], _c["ff"]))


@pytest.mark.parametrize("fixture", range(len(_NAMES_FIXTURES)), ids=["%s-%d" % (f[0], len(f[1][0])) for f in _NAMES_FIXTURES])
@pytest.mark.parametrize("excl", [0, 75])
def test_genome_fixtures_every_estimator(fixture, excl):
    name, (genomes, c2g), ff = _NAMES_FIXTURES[fixture]
    b = load_fixture(name)
    g_of = np.asarray([c2g.get(n, -1) for n in b.ref_names], np.int32)
    for flags in (ff, (True, True, False)):
        check_sample(np.asarray(b.ref_lens, np.int64), to_batch(b), g_of, len(genomes), excl, ff=flags)


def skewed_genomes(n_contigs, seed):
    """genome_of_tid with one genome holding most contigs, many small ones, contigs outside every genome, interleaved (a genome's contigs are
    not consecutive tids) — and one genome whose contigs are all left without reads by `drop_reads_of`."""
    rng = np.random.default_rng(seed)
    n_small = max(2, n_contigs // 100)
    g = rng.integers(1, 1 + n_small, n_contigs).astype(np.int32)
    g[rng.random(n_contigs) < 0.6] = 0                          # the big one
    g[rng.random(n_contigs) < 0.07] = -1
    n_genomes = n_small + 2                                     # the last genome: see drop_reads_of
    if n_contigs >= 8:
        g[rng.choice(n_contigs, max(2, n_contigs // 200), replace=False)] = n_genomes - 1
    return g, n_genomes


def drop_reads_of(batch, tids):
    idx = np.nonzero(~np.isin(batch.tid, tids))[0]
    n_ops = np.diff(batch.cigar_off.astype(np.int64))[idx]
    off = np.zeros(len(idx) + 1, np.int64)
    np.cumsum(n_ops, out=off[1:])
    src = np.repeat(batch.cigar_off[:-1].astype(np.int64)[idx] - off[:-1], n_ops) + np.arange(off[-1])
    return RecordBatch(batch.tid[idx], batch.pos[idx], batch.flag[idx], batch.mapq[idx], batch.nm[idx], batch.nm_kind[idx], batch.l_seq[idx],
                       off.astype(np.uint32), np.ascontiguousarray(batch.cigar[src], np.uint32))


@pytest.mark.parametrize("n_contigs,total,n_reads", [(1, 80_000, 4_000), (1_000, 40_000_000, 300_000), (200_000, 500_000_000, 900_000)])
def test_synthetic_skewed_genomes(n_contigs, total, n_reads):
    ref = synth.make_reference(n_contigs, total, seed=31, min_len=400 if n_contigs > 1 else 2000, max_len=400_000)
    batch = synth.make_reads(ref, n_reads, seed=32)
    if n_contigs == 1:
        for g_of, n_g in (([0], 1), ([0], 3), ([-1], 2)):       # a genome of one contig; genomes without any contig; the contig outside every genome
            check_sample(ref.lengths, batch, np.asarray(g_of, np.int32), n_g, 75)
        return
    g_of, n_genomes = skewed_genomes(n_contigs, seed=33)
    batch = drop_reads_of(batch, np.concatenate([np.nonzero(g_of == n_genomes - 1)[0], np.nonzero(g_of == 0)[0][:3], np.nonzero(g_of == 1)[0][:1]]))
    seen = np.zeros(n_contigs, bool)
    seen[batch.tid[batch.tid >= 0]] = True
    assert (~seen[g_of == 0]).any() and seen[g_of == 0].any()          # unobserved lengths beside seen contigs in one genome
    assert not seen[g_of == n_genomes - 1].any() and (g_of == n_genomes - 1).any()
    assert (g_of == 0).sum() > n_contigs // 2 and (g_of < 0).any()
    check_sample(ref.lengths, batch, g_of, n_genomes, 75, chunks=3)
    check_sample(ref.lengths, batch, g_of, n_genomes, 0, ff=(True, False, True))
    check_sample(ref.lengths, batch, g_of, n_genomes, 600)      # contigs shorter than 2 x 600: no window when seen, their whole length when unobserved


def test_deep_genomes_histograms_of_many_batches():
    """Depths in the hundreds: merged histograms of several 64-bin batches, contigs of different depth in one genome."""
    ref = synth.make_reference(12, 60_000, seed=3, min_len=900, max_len=9_000)
    batch = synth.make_reads(ref, 180_000, seed=4)
    g_of = np.asarray([0, 0, 1, 0, 1, -1, 2, 2, 2, 0, 1, 3], np.int32)
    for excl in (0, 75, 600):
        check_sample(ref.lengths, batch, g_of, 5, excl)


def test_every_genome_its_own_contig_lane_per_genome():
    """More than 65 536 genomes: k_genome_estimate_lanes."""
    ref = synth.make_reference(70_000, 90_000_000, seed=21, min_len=1000, max_len=40_000)
    batch = synth.make_reads(ref, 600_000, seed=22)
    g_of = np.arange(70_000, dtype=np.int32)
    g_of[::13] = -1
    check_sample(ref.lengths, batch, g_of, 70_000, 75)


@pytest.mark.parametrize("n_contigs", [1025, 2049])
def test_one_and_two_blocks_of_genomes_and_contigs_in_front(n_contigs):
    """Every contig its own genome, one tile each: the layout of the merged histograms (a scan over genomes) and the order rule of
    cov_finish_genomes (a running maximum over contigs) have exactly one and two workgroups of 1 024 in front of their last one, with
    reads in the genomes and contigs on both sides of every border."""
    ref = synth.make_reference(n_contigs, n_contigs * 650, seed=71, min_len=400, max_len=1000)
    batch = synth.make_reads(ref, 8 * n_contigs, seed=74)
    considered = np.bincount(batch.tid[(batch.flag & 0x904) == 0], minlength=n_contigs)
    borders = [63, 64] + [k for k in (1023, 1024, 2047, 2048) if k < n_contigs]
    assert (considered[borders] > 0).all()
    check_sample(ref.lengths, batch, np.arange(n_contigs, dtype=np.int32), n_contigs, 75, sets=estimator_sets(75)[:1])


def test_after_a_spill_the_genome_fetches_say_so(monkeypatch):
    set_knobs(monkeypatch, store_cap_records=40000)
    ref = synth.make_reference(150, 12_000_000, seed=11, min_len=1500, max_len=300_000)
    batch = synth.make_reads(ref, 200_000, seed=12)
    est = estimator_sets(75)[0]
    with Session(0, FilterConfig(), 75, want_hist=True, want_identity="nonsupp") as s:
        s.set_targets(ref.lengths)
        s.set_genomes(ref.genome_of_contig, len(ref.genomes))
        s.set_estimators(est)
        edges = np.linspace(0, batch.n_records, 20).astype(int)
        for lo, hi in zip(edges[:-1], edges[1:]):
            s.push(batch.slice(lo, hi))
        st, summ = s.finish()
        assert s.store_spills() >= 1
        for fetch in (s.genome_estimates, s.genome_stats, s.finish_genomes):
            with pytest.raises(CovError) as ei:
                fetch()
            assert ei.value.status == native.ERR_STATE
        hist = s.hist()                      # the host path still has everything it needs
        assert hist.size == int(summ.hist_total)
        s.reset()                            # the next sample of the session is whole again
        s.set_estimators(est)
        s.push(batch.slice(0, 30000))
        s.finish()
        assert s.store_spills() == 0 and s.genome_estimates().shape == (len(ref.genomes), len(est))


def test_finish_genomes_gives_the_verdicts_of_finish():
    """Unsorted input, a record without NM, an unsorted file whose first error comes earlier: cov_finish_genomes judges them on the device
    and returns what cov_finish returns, message included."""
    ref = synth.make_reference(3_000, 60_000_000, seed=61, min_len=1500, max_len=200_000)
    batch = synth.make_reads(ref, 200_000, seed=62)
    est = estimator_sets(75)[0][:5]

    def permuted(b, order):
        n_ops = np.diff(b.cigar_off.astype(np.int64))[order]
        off = np.zeros(len(order) + 1, np.int64)
        np.cumsum(n_ops, out=off[1:])
        src = np.repeat(b.cigar_off[:-1].astype(np.int64)[order] - off[:-1], n_ops) + np.arange(off[-1])
        return RecordBatch(b.tid[order], b.pos[order], b.flag[order], b.mapq[order], b.nm[order], b.nm_kind[order].copy(), b.l_seq[order],
                           off.astype(np.uint32), np.ascontiguousarray(b.cigar[src], np.uint32))

    n = batch.n_records
    ident = np.arange(n)
    # the records of one contig in the middle moved behind those of a contig 1 500 blocks of 1 024 contigs... further on (two scan blocks apart)
    lo, hi = np.searchsorted(batch.tid, [700, 701])
    cut = np.searchsorted(batch.tid, 2_500)
    moved = np.concatenate([ident[:lo], ident[hi:cut], ident[lo:hi], ident[cut:]])
    assert hi > lo
    considered = np.nonzero((batch.flag & 0x904) == 0)[0]
    cases_ = []
    cases_.append(("unsorted", permuted(batch, moved), native.ERR_UNSORTED))
    nonm = permuted(batch, ident)
    nonm.nm_kind[considered[len(considered) // 2]] = 0
    cases_.append(("nm missing", nonm, native.ERR_NM_MISSING))
    both = permuted(batch, moved)
    both.nm_kind[np.nonzero((both.flag & 0x904) == 0)[0][10]] = 0          # the error comes first in file order
    cases_.append(("nm missing before the order breaks", both, native.ERR_NM_MISSING))
    late = permuted(batch, moved)
    late.nm_kind[np.nonzero((late.flag & 0x904) == 0)[0][-10]] = 0         # the order breaks first
    cases_.append(("order breaks before the nm error", late, native.ERR_UNSORTED))
    for what, b, status in cases_:
        with Session(0, FilterConfig(), 75, want_hist=True, want_identity="nonsupp") as s:
            s.set_targets(ref.lengths)
            s.set_genomes(ref.genome_of_contig, len(ref.genomes))
            s.set_estimators(est)
            s.push(b)
            with pytest.raises(CovError) as full:
                s.finish()
            with pytest.raises(CovError) as lean:
                s.finish_genomes()
            assert full.value.status == status, what
            assert (lean.value.status, lean.value.message) == (full.value.status, full.value.message), what
    with Session(0, FilterConfig(), 75) as s:                   # nothing set: refused, not answered per contig
        s.set_targets(ref.lengths)
        with pytest.raises(CovError) as ei:
            s.finish_genomes()
        assert ei.value.status == native.ERR_STATE


def test_genomes_off_drops_a_genome_only_anir():
    """ANIr over the not-supplementary sum is a genome estimator: with the genomes off nothing may evaluate it per contig."""
    with Session(0, FilterConfig(), 75, want_identity="nonsupp") as s:
        s.set_targets([1000, 2000])
        s.set_genomes([0, 0], 1)
        s.set_estimators([E.new_estimator_anir(), E.new_estimator_length()])
        s.finish()
        assert s.genome_estimates().shape == (1, 2)
        s.set_genomes(None, 0)
        s.finish()
        with pytest.raises(CovError):
            s.estimates()                                        # the estimators went with the genomes
        with pytest.raises(CovError):
            s.set_estimators([E.new_estimator_anir()])           # and per contig this session cannot offer it


def test_arguments():
    with Session(0, FilterConfig(), 75, want_hist=True, want_identity="primary") as s:
        s.set_targets([1000, 2000])
        with pytest.raises(CovError):
            s.set_genomes([0, 5], 2)                             # outside [-1, n_genomes)
        s.set_genomes([0, -1], 1)
        with pytest.raises(CovError):
            s.set_estimators([E.new_estimator_anir()])           # a genome's ANIr takes the not-supplementary sum
        s.set_estimators([E.new_estimator_mean(0.0, 75, False)])
        s.finish()
        assert s.genome_estimates().shape == (1, 1)
        s.set_genomes(None, 0)                                   # off: per-contig floats again
        s.finish()
        with pytest.raises(CovError):
            s.genome_estimates()
        assert s.estimates().shape == (2, 1)


# ---------------------------------------------------------------------------------------------------- through the binary
def _sample(tmp_path, n_contigs, total, n_reads, seed, name="synth"):
    ref = synth.make_reference(n_contigs, total, seed=seed, min_len=1500, max_len=400_000)
    batch = synth.make_reads(ref, n_reads, seed=seed + 1)
    path = os.path.join(str(tmp_path), name + ".bam")
    cbam.write_bam(path, ref.names, ref.lengths, batch, with_seq=1, threads=8)
    return ref, to_bamdata(batch, ref.lengths, ref.names), path


DEVICE_METHODS = ["relative_abundance", "rpkm", "mean", "trimmed_mean", "covered_fraction", "variance"]


def test_config3_through_the_binary_both_paths(tmp_path):
    """Config 3's workload at test size; genomes by --genome-definition and by -d/-x; the device path (default) and the host path
    (COVERM_HOST_ESTIMATES=1) print the oracle's text, and only the host path fetches the histogram."""
    ref, b, path = _sample(tmp_path, 200, 10_000_000, 200_000, seed=43)
    gd = tmp_path / "genomes.tsv"
    per = {}
    for n in ref.names[:170]:                                   # 30 contigs in no genome
        per.setdefault(n.split("~")[0], []).append(n)
    order = sorted(per)                                          # -d lists its files bytewise: the definition in the same genome order
    gd.write_text("".join("%s\t%s\n" % (g, n) for g in order for n in per[g]))
    gdir = tmp_path / "genomes"
    gdir.mkdir()
    for g in order:
        (gdir / (g + ".fna")).write_text("".join(">%s\nACGTACGT\n" % n for n in per[g]))
    for fmt, extra in (("dense", {}), ("sparse", dict(no_zeros=True)), ("dense", dict(min_covered_fraction=0, methods=["mean", "variance", "length", "count", "reads_per_base", "anir"]))):
        args = dict(dict(methods=DEVICE_METHODS, output_format=fmt), **extra)
        want = O.run_cli("genome", [path], bams=[b], genome_definition=str(gd), **args)
        assert want.count("\n") > 10
        for env in (dict(COVERM_CLI_TIMING="1"), dict(COVERM_CLI_TIMING="1", COVERM_HOST_ESTIMATES="1")):
            for src in (["--genome-definition", str(gd)], ["-d", str(gdir), "-x", "fna"]):
                r = subprocess.run(binary.argv("genome", [path], **args) + src, capture_output=True, text=True, timeout=900, env=dict(os.environ, **env))
                assert r.returncode == 0, r.stderr[-3000:]
                assert r.stdout == want, (env, src)
                needs_hist = "trimmed_mean" in args["methods"]
                if "COVERM_HOST_ESTIMATES" in env:
                    assert "genome results from the device" not in r.stderr
                    assert ("histogram fetch:" in r.stderr) == needs_hist
                else:
                    assert "genome results from the device" in r.stderr and "histogram fetch:" not in r.stderr
    # config 3's own methods: TPM is evaluated on the host, the whole run keeps the host path
    args = dict(methods=["relative_abundance", "rpkm", "tpm"], genome_definition=str(gd))
    r = binary.run_full("genome", [path], env=dict(COVERM_CLI_TIMING="1"), **args)
    assert r.stdout == O.run_cli("genome", [path], bams=[b], **args) and "genome results from the device" not in r.stderr


def test_table_of_skewed_genomes_vs_oracle(tmp_path):
    """1 000 contigs, the skewed genome table of the ABI test, through the binary: the oracle's text."""
    ref, b, path = _sample(tmp_path, 1_000, 40_000_000, 250_000, seed=51)
    g_of, n_genomes = skewed_genomes(1_000, seed=52)
    gd = tmp_path / "genomes.tsv"
    gd.write_text("".join("bin%d\t%s\n" % (g_of[i], ref.names[i]) for i in np.argsort(g_of, kind="stable") if g_of[i] >= 0))
    for extra in (dict(), dict(no_zeros=True, output_format="sparse")):
        args = dict(dict(methods=DEVICE_METHODS, genome_definition=str(gd)), **extra)
        r = binary.run_full("genome", [path], env=dict(COVERM_CLI_TIMING="1"), **args)
        assert r.stdout == O.run_cli("genome", [path], bams=[b], **args)
        assert "genome results from the device" in r.stderr


def test_binary_falls_back_to_the_host_after_a_spill(tmp_path):
    ref, b, path = _sample(tmp_path, 300, 30_000_000, 400_000, seed=101)
    gd = tmp_path / "genomes.tsv"
    gd.write_text("".join("%s\t%s\n" % (n.split("~")[0], n) for n in ref.names[:250]))
    args = dict(methods=DEVICE_METHODS, genome_definition=str(gd))
    want = O.run_cli("genome", [path], bams=[b], **args)
    env = with_knobs(dict(COVERM_CLI_TIMING="1"), ingest_round_blocks=128, store_cap_records=50000, store_cap_cigar=200000)
    r = binary.run_full("genome", [path], env=env, **args)
    assert "bounded store: spill" in r.stderr and "genome results from the device" not in r.stderr
    assert r.stdout == want
    assert binary.run("genome", [path], **args) == want

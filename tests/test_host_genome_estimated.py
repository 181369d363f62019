"""covh_genome_coverage_estimated (coverm_host.h): the contig-names genome scan (genome.rs:236-302) with the genomes already aggregated
and evaluated elsewhere.  On the CPU the floats and the per-genome statistics fed in are the existing host aggregation's own (on a GPU
they come from cov_fetch_genome_estimates / cov_fetch_genome_stats, tests/test_gpu_genome_device.py): entries, zero rows, --no-zeros,
ReadsMapped and the printed table must be those of covh_genome_coverage_with_contig_names."""
import numpy as np
import pytest

from coverm_amd import host, native
from coverm_amd.host import CoverageTaker
from oracle import oracle as O
from tests import harness_cli as cli
from tests.golden import cases
from tests.test_host_golden import alignment_file, oracle_sample

GENOME_FIXTURES = [("2seqs.reads_for_seq1.bam", cases.GECO_SE), ("2seqs.reads_for_seq2.bam", cases.GECO_SE),
                   ("2seqs.reads_for_seq1_and_seq2.bam", cases.GECO_S), (cases.S7 + ".bam", cases.GECO_7), (cases.S7 + ".bam", cases.GECO_23)]
# (methods, --min-covered-fraction): the default of `coverm genome`, every family of estimator, the printer's normalisations
METHOD_SETS = [(["relative_abundance"], 10), (["relative_abundance", "rpkm"], 10), (["mean", "trimmed_mean", "covered_fraction", "variance"], 10),
               (["mean", "covered_bases", "variance", "length", "count", "reads_per_base", "rpkm"], 0), (["anir", "mean"], 0)]


def genome_table(names, geco):
    genomes, c2g = geco
    return list(genomes), np.asarray([c2g.get(n, -1) for n in names], dtype=np.int32)


def host_genome_stats(stats, lens, g_of, n_genomes, est_rows):
    """cov_genome_stats as the device would report them, from per-contig statistics."""
    gs = np.zeros(n_genomes, dtype=native.GENOME_STATS_DTYPE)
    lens = np.asarray(lens, np.uint64)
    for g in range(n_genomes):
        m = g_of == g
        gs["reads_in_genome"][g] = stats["n_pass"][m].sum()
        gs["genome_len"][g] = lens[m].sum()
        gs["n_contigs_seen"][g] = int((stats["n_pass"][m] > 0).sum())
        gs["any_nonzero"][g] = int((est_rows[g] > 0).any())
    return gs


def host_genome_rows(names, lens, sample, genomes, g_of, est):
    """The existing host aggregation's floats, one row per genome (zero rows as print_zero_coverage leaves them)."""
    t = CoverageTaker.new_cached_single_float_coverage_taker(len(est))
    host.mosdepth_genome_coverage_with_contig_names(names, lens, [sample], genomes, g_of, t, True, est)
    v = t.cached_coverages(0)
    return v.reshape(len(genomes), len(est)) if v.size else np.zeros((len(genomes), len(est)), np.float32)


def table(et, entry, rms):
    host.finalise_printing(et.taker, et.printer, "Genome", et.headers(), rms, et.columns_to_normalise, et.rpkm_column, et.tpm_column)
    return et.taker.text()


@pytest.mark.parametrize("fixture", range(len(GENOME_FIXTURES)))
@pytest.mark.parametrize("methods", range(len(METHOD_SETS)))
@pytest.mark.parametrize("no_zeros", [False, True])
@pytest.mark.parametrize("fmt", ["dense", "sparse"])
def test_estimated_equals_aggregated(fixture, methods, no_zeros, fmt):
    name, geco = GENOME_FIXTURES[fixture]
    meth, mcf = METHOD_SETS[methods]
    af = alignment_file(name)
    names, lens = af.ref_names, af.ref_lens
    genomes, g_of = genome_table(names, geco)
    fp = O.FilterParameters(O.FlagFilter(True, True, False))
    texts, rmss = [], []
    for estimated in (False, True):
        et = cli.EstimatorsAndTaker.generate(meth, mcf, 75, 5, 95, fmt)
        want_hist, want_id = host.wants(et.estimators)
        sample = oracle_sample(af, fp, 75, want_hist, want_id, mask=(g_of >= 0).astype(np.uint8))
        host.print_headers(et.taker, et.printer, "Genome", et.headers())
        if estimated:
            rows = host_genome_rows(names, lens, sample, genomes, g_of, et.estimators)
            gs = host_genome_stats(sample.stats, lens, g_of, len(genomes), rows)
            rm = host.genome_coverage_estimated(sample.stoit_name, sample.num_detected_primary_alignments, bool((sample.stats["n_pass"] > 0).any()),
                                                genomes, et.taker, not no_zeros, et.estimators, rows, gs)
            rms = [rm]
        else:
            rms = host.mosdepth_genome_coverage_with_contig_names(names, lens, [sample], genomes, g_of, et.taker, not no_zeros, et.estimators)
        rmss.append([(r.num_mapped_reads, r.num_reads) for r in rms])
        texts.append(table(et, "Genome", rms))
    assert texts[0] == texts[1]
    assert rmss[0] == rmss[1]
    assert texts[0].count("\n") >= 1


def test_a_sample_without_any_alignment_prints_no_entry():
    """genome.rs:230-234: no reference seen and no primary alignment: the sample contributes no entry, zero rows included."""
    genomes = ["g0", "g1"]
    est = [host.CoverageEstimator.new_estimator_mean(0.1, 75, False), host.CoverageEstimator.new_estimator_length()]
    gs = np.zeros(2, dtype=native.GENOME_STATS_DTYPE)
    gs["genome_len"] = [5000, 7000]
    rows = np.asarray([[0.0, 5000.0], [0.0, 7000.0]], np.float32)
    t = CoverageTaker.new_single_float_coverage_streaming_coverage_printer()
    rm = host.genome_coverage_estimated("s", 0, False, genomes, t, True, est, rows, gs)
    assert t.text() == "" and (rm.num_mapped_reads, rm.num_reads) == (0, 0)
    t = CoverageTaker.new_single_float_coverage_streaming_coverage_printer()
    rm = host.genome_coverage_estimated("s", 3, False, genomes, t, True, est, rows, gs)      # unmapped primaries only: zero rows are printed
    assert t.text() == "s\tg0\t0\t5000\ns\tg1\t0\t7000\n" and (rm.num_mapped_reads, rm.num_reads) == (0, 3)


def test_histogram_and_tpm_estimators_are_refused():
    gs = np.zeros(1, dtype=native.GENOME_STATS_DTYPE)
    for bad in (host.CoverageEstimator.new_estimator_tpm(0.0), host.CoverageEstimator.new_estimator_pileup_counts(0.0, 75)):
        t = CoverageTaker.new_cached_single_float_coverage_taker(1)
        with pytest.raises(Exception):
            host.genome_coverage_estimated("s", 1, True, ["g"], t, True, [bad], np.zeros((1, 1), np.float32), gs)

"""covh_genome_coverage_separator_estimated (coverm_host.h): the separator / single-genome scan (genome.rs:419-797) over entries that were
aggregated and evaluated elsewhere.  On the CPU the entries come from the oracle's per-contig statistics through csrc/sep_entry_core.h's CPU
emulation and the host's EntryAcc (covh_genome_separator_entries; on a GPU they come from cov_fetch_genome_entries /
cov_fetch_genome_estimates, tests/test_gpu_separator_device.py): entries, zero rows, --no-zeros, ReadsMapped and the printed text must be
those of covh_genome_coverage_separator, for every separator and single-genome case of tests/golden/cases.py."""
import numpy as np
import pytest

from coverm_amd import host
from coverm_amd.host import CoverageEstimator as E
from coverm_amd.host import CoverageTaker
from tests import harness_cli as cli
from tests.golden import cases
from tests.test_host_golden import alignment_file, excl_of, make_est, oracle_sample

SEP_CASES = [c for c in cases.API_CASES if c["api"] == "sep"]


def estimator_sets(case):
    """The case's own estimators, then every family the device evaluates (the excl of the case)."""
    excl = excl_of(case["est"])
    return [[make_est(e) for e in case["est"]],
            [E.new_estimator_mean(0.1, excl, False), E.new_estimator_trimmed_mean(0.05, 0.95, 0.0, excl), E.new_estimator_covered_fraction(0.0),
             E.new_estimator_variance(0.0, excl)],
            [E.new_estimator_mean(0.0, excl, True), E.new_estimator_covered_bases(0.0), E.new_estimator_length(), E.new_estimator_read_count(),
             E.new_estimator_reads_per_base(), E.new_estimator_rpkm(0.0), E.new_estimator_anir()]]


def scan(case, est, print_zero, estimated, takers, excl=None):
    files = [alignment_file(b) for b in case["bams"]]
    excl = excl_of(case["est"]) if excl is None else excl
    want_hist, want_id = host.wants(est)
    fp = cli.FilterParameters(cli.FlagFilter(*case["ff"]))
    names, lens = files[0].ref_names, files[0].ref_lens
    taker = takers()
    rms, used = [], 0
    for af in files:
        sample = oracle_sample(af, fp, excl, want_hist, want_id)
        gid, n_gids = host.genome_separator_ids(names, lens, case["sep"], case["single"])
        if estimated and n_gids and (sample.stats["n_pass"] > 0).any():
            entries, floats = host.genome_separator_entries(names, lens, sample, gid, est)
            assert len(entries) > 0 and (entries["n_contigs_seen"] > 0).all()
            np.testing.assert_array_equal(entries["any_nonzero"] != 0, (floats > 0).any(axis=1))
            rms.append(host.genome_coverage_separator_estimated(names, lens, sample.stoit_name, sample.num_detected_primary_alignments, case["sep"],
                                                                case["single"], taker, print_zero, est, entries, floats))
            used += 1
        else:      # a header with a name that lacks the separator, or a sample without an observed contig: the scan itself
            rms += host.mosdepth_genome_coverage(names, lens, [sample], case["sep"], taker, print_zero, est, case["single"])
    return taker.text(), [(r.num_mapped_reads, r.num_reads) for r in rms], used, rms


@pytest.mark.parametrize("case", SEP_CASES, ids=[c["id"] for c in SEP_CASES])
@pytest.mark.parametrize("print_zero", [True, False])
def test_estimated_equals_the_scan(case, print_zero):
    assert len(SEP_CASES) >= 15
    for k, est in enumerate(estimator_sets(case)):
        if any(e.kind in (host.PILEUP_COUNTS, host.TPM) for e in est):
            continue      # evaluated on the host: refused below
        got = []
        for estimated in (False, True):
            text, rms, used, _ = scan(case, est, print_zero, estimated, CoverageTaker.new_single_float_coverage_streaming_coverage_printer)
            got.append((text, rms))
        assert got[0] == got[1], (case["id"], k)
        assert got[0][0] != "" or not print_zero
        if k == 0 and print_zero == case["print_zero"] and case["taker"] == "stream":
            assert got[1][0] == case["expected"]      # and the reference's own text, from the estimated path


# (methods, --min-covered-fraction) through the cached takers and the printers of `coverm genome`
METHOD_SETS = [(["relative_abundance"], 10), (["mean", "trimmed_mean", "covered_fraction", "variance"], 10),
               (["mean", "covered_bases", "variance", "length", "count", "reads_per_base", "rpkm"], 0), (["anir", "mean"], 0)]


@pytest.mark.parametrize("case", SEP_CASES, ids=[c["id"] for c in SEP_CASES])
@pytest.mark.parametrize("no_zeros", [False, True])
def test_printed_tables_are_the_same(case, no_zeros):
    for meth, mcf in METHOD_SETS:
        for fmt in ("dense", "sparse"):
            texts = []
            for estimated in (False, True):
                et = cli.EstimatorsAndTaker.generate(meth, mcf, 75, 5, 95, fmt)
                host.print_headers(et.taker, et.printer, "Genome", et.headers())
                _, rm_pairs, _, rms = scan(case, et.estimators, not no_zeros, estimated, lambda: et.taker, excl=75)
                host.finalise_printing(et.taker, et.printer, "Genome", et.headers(), rms, et.columns_to_normalise, et.rpkm_column, et.tpm_column)
                texts.append((et.taker.text(), rm_pairs))
            assert texts[0] == texts[1], (case["id"], meth, fmt)
            assert texts[0][0].count("\n") >= 1


def test_the_estimated_path_is_taken():
    """Every case whose names all hold the separator has a sample with an observed contig: the comparison above is not vacuous."""
    n_used = 0
    for case in SEP_CASES:
        est = estimator_sets(case)[1]
        n_used += scan(case, est, True, True, CoverageTaker.new_single_float_coverage_streaming_coverage_printer)[2] > 0
    assert n_used >= len(SEP_CASES) - 2


def test_histogram_and_tpm_estimators_are_refused():
    case = SEP_CASES[0]
    af = alignment_file(case["bams"][0])
    ent = np.zeros(1, dtype=host.native.GENOME_ENTRY_DTYPE)
    for bad in (E.new_estimator_tpm(0.0), E.new_estimator_pileup_counts(0.0, 0)):
        t = CoverageTaker.new_cached_single_float_coverage_taker(1)
        with pytest.raises(Exception):
            host.genome_coverage_separator_estimated(af.ref_names, af.ref_lens, "s", 1, case["sep"], False, t, True, [bad], ent, np.zeros((1, 1), np.float32))
    t = CoverageTaker.new_cached_single_float_coverage_taker(1)
    with pytest.raises(Exception):      # no entry: the scan itself prints such a sample
        host.genome_coverage_separator_estimated(af.ref_names, af.ref_lens, "s", 1, case["sep"], False, t, True, [E.new_estimator_length()], ent[:0],
                                                 np.zeros((0, 1), np.float32))


def test_ids_of_a_header():
    gid, n = host.genome_separator_ids(["a~1", "a~2", "b~1", "a~3", "~x", "b~"], [1] * 6, "~", False)
    assert (gid.tolist(), n) == ([0, 0, 1, 0, 2, 1], 3)
    gid, n = host.genome_separator_ids(["a~1", "a2", "b~1"], [1] * 3, "~", False)
    assert n == 0
    gid, n = host.genome_separator_ids(["a~1", "a2", "b~1"], [1] * 3, "~", True)
    assert (gid.tolist(), n) == ([0, 0, 0], 1)

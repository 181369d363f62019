"""The separator / single-genome scan on the device (cov_set_genome_runs / cov_fetch_genome_entries / cov_fetch_genome_estimates, the
kernels of csrc/sep_kernels.hip.h in front of those of csrc/genome_kernels.hip.h) against the host aggregation of the SAME finish's
per-contig statistics (covh_genome_separator_entries: csrc/sep_entry_core.h's CPU emulation, EntryAcc::add_contig in ascending tid order,
calculate_coverage with the unobserved lengths): the same entries, the same reads, the same f32 bit for bit.  No tolerance: the
accumulators are integers and the one f64 sum has a prescribed order.  Then the product binary: `coverm-amd genome -s '~' | --single-genome`
with and without COVERM_HOST_ESTIMATES=1 equals the oracle's text, and the timing line shows which path ran."""
import os
import re
import subprocess

import numpy as np
import pytest

from coverm_amd import bam as cbam
from coverm_amd import host, native, synth
from coverm_amd.engine import FilterConfig, RecordBatch, Session
from coverm_amd.host import CoverageEstimator as E
from coverm_amd.host import SampleResult
from coverm_amd.native import CovError
from oracle import bamio
from oracle import oracle as O
from tests import binary
from tests.fixtures import load_fixture
from tests.golden import cases
from tests.knobs import set_knobs
from tests.test_gpu_abi_parity import to_bamdata, to_batch
from tests.test_gpu_genome_device import drop_reads_of, estimator_sets

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CORE = open(os.path.join(HERE, "..", "coverm_amd", "csrc", "sep_entry_core.h")).read()
SCAN_TILE = int(re.search(r"SCAN_TILE = (\d+)u", CORE).group(1))      # targets per workgroup of the device-wide scans
GENOME_SEG = 256


def check_sample(names, lens, batch, gid, n_gids, excl, ff=(True, True, False), sets=None):
    """Entries and floats of cov_finish and of cov_finish_genomes against the host's aggregation of cov_finish's statistics."""
    gid = np.ascontiguousarray(gid, np.int32)
    lens = np.asarray(lens, np.int64)
    out = None
    for est in (sets or estimator_sets(excl)):
        with Session(0, FilterConfig(*ff), excl, want_hist=True, want_identity="primary") as s:
            s.set_targets(lens)
            s.set_genome_runs(gid, n_gids)
            s.set_estimators(est)
            s.push(batch)
            st, summ = s.finish()
            assert s.sep_kernel_ms()[1] > 0 and s.genome_kernel_ms()[1] > 0, "the table's or the genome kernels did not run"
            ent = s.genome_entries()
            dev = s.genome_estimates()
            with pytest.raises(CovError):
                s.estimates()                      # per-contig floats are not offered: the entries are genomes
            hist = s.hist()
            lean = s.finish_genomes()
            np.testing.assert_array_equal(s.genome_entries(), ent)
            np.testing.assert_array_equal(s.genome_estimates().view(np.uint32), dev.view(np.uint32))
            assert (lean.num_detected_primary_alignments, lean.n_records, lean.n_considered) == (
                summ.num_detected_primary_alignments, summ.n_records, summ.n_considered)
        sample = SampleResult("s", st, hist, int(summ.num_detected_primary_alignments))
        want_e, want_f = host.genome_separator_entries(names, lens, sample, gid, est)
        assert len(ent) == len(want_e)
        for f in ("first_tid", "gid", "reads", "n_contigs_seen", "any_nonzero"):
            np.testing.assert_array_equal(ent[f], want_e[f], err_msg=f)
        for k in range(len(est)):
            bad = np.nonzero(dev[:, k].view(np.uint32) != want_f[:, k].view(np.uint32))[0]
            assert bad.size == 0, ("estimator %d (kind %d), entry %d: device %r host %r" % (k, est[k].kind, bad[0], dev[bad[0], k], want_f[bad[0], k]))
        out = (ent, st)
    return out


_SEP_FIXTURES = []
for _c in cases.API_CASES:
    if _c["api"] == "sep" and (_c["bams"][-1], _c["sep"], _c["single"]) not in [f[:3] for f in _SEP_FIXTURES]:
        _SEP_FIXTURES.append((_c["bams"][-1], _c["sep"], _c["single"], _c["ff"]))


@pytest.mark.parametrize("fixture", range(len(_SEP_FIXTURES)), ids=["%s-%s%s" % (f[0], "single" if f[2] else "sep", "" if f[2] else ord(f[1])) for f in _SEP_FIXTURES])
@pytest.mark.parametrize("excl", [0, 75])
def test_separator_fixtures_every_estimator(fixture, excl):
    name, sep, single, ff = _SEP_FIXTURES[fixture]
    b = load_fixture(name)
    gid, n_gids = host.genome_separator_ids(b.ref_names, b.ref_lens, sep, single)
    assert n_gids > 0, "every fixture name holds its case's separator"
    for flags in (ff, (True, True, False)):
        check_sample(b.ref_names, b.ref_lens, to_batch(b), gid, n_gids, excl, ff=flags)


def _synthetic(n_contigs, n_reads, seed, per_genome=10):
    ref = synth.make_reference(n_contigs, n_contigs * 3000, seed=seed, contigs_per_genome=per_genome, min_len=400, max_len=9_000)
    return ref, synth.make_reads(ref, n_reads, seed=seed + 1)


def test_an_entry_across_segments_and_targets_across_scan_tiles():
    """Genomes of 700 consecutive contigs: entries of more than GENOME_SEG members, runs that straddle the scan's tiles; the reads of whole
    stretches dropped so that unobserved contigs sit in front of, inside and behind the observed ones."""
    n = 3 * SCAN_TILE + 37
    ref, batch = _synthetic(n, 4 * n, seed=71, per_genome=700)
    batch = drop_reads_of(batch, np.concatenate([np.arange(0, 40), np.arange(650, 760), np.arange(SCAN_TILE - 5, SCAN_TILE + 300), np.arange(n - 30, n)]))
    for excl in (0, 75):
        ent, st = check_sample(ref.names, ref.lengths, batch, ref.genome_of_contig, len(ref.genomes), excl)
    seen = st["n_pass"] > 0
    assert ent["n_contigs_seen"].max() > GENOME_SEG and (~seen).sum() > 400 and not seen[0] and not seen[-1]
    assert n > SCAN_TILE and len(ent) == len(ref.genomes)


def test_genomes_interleaved_in_the_header():
    """Blocks of random length over a small pool of genomes, few reads: a genome recurs apart from itself (several entries), unobserved
    contigs that count for the entry in front, the one behind, or none."""
    n = 5_000
    rng = np.random.default_rng(5)
    gid = []
    while len(gid) < n:
        gid += [int(rng.integers(0, 6))] * int(rng.choice([1, 1, 2, 3, 9, 60, 400]))
    gid = np.asarray(gid[:n], np.int32)
    ref, batch = _synthetic(n, n // 2, seed=81)
    names = ["g%d~c%d" % (g, i) for i, g in enumerate(gid)]
    ent, st = check_sample(names, ref.lengths, batch, gid, 6, 75)
    assert len(ent) > 20 and len(np.unique(ent["gid"])) == 6 and len(ent) > len(np.unique(ent["gid"]))
    check_sample(names, ref.lengths, batch, gid, 6, 0, ff=(True, False, True), sets=estimator_sets(0)[:1])


def test_every_contig_its_own_genome_and_single_genome():
    n = 10_000
    ref, batch = _synthetic(n, 3 * n, seed=91)
    names = ["g%d~c" % i for i in range(n)]
    ent, st = check_sample(names, ref.lengths, batch, np.arange(n, dtype=np.int32), n, 75, sets=estimator_sets(75)[:1])
    assert len(ent) == int((st["n_pass"] > 0).sum()) and (ent["n_contigs_seen"] == 1).all()
    ent, st = check_sample(names, ref.lengths, batch, np.zeros(n, np.int32), 1, 75)      # --single-genome: one entry, ANIr one chain of 10 000
    assert len(ent) == 1 and ent["first_tid"][0] == 0 and ent["n_contigs_seen"][0] == int((st["n_pass"] > 0).sum())


def test_no_observed_contig_gives_no_entry():
    ref, batch = _synthetic(1500, 3000, seed=95)
    est = estimator_sets(75)[1]
    with Session(0, FilterConfig(), 75, want_hist=True, want_identity="primary") as s:
        s.set_targets(ref.lengths)
        s.set_genome_runs(ref.genome_of_contig, len(ref.genomes))
        s.set_estimators(est)
        s.finish_genomes()
        assert s.genome_entry_count() == 0 and s.genome_estimates().shape == (0, len(est)) and len(s.genome_entries()) == 0
        s.push(batch)                              # and the next finish of the session has entries
        s.finish_genomes()
        assert s.genome_entry_count() > 0


def test_after_a_spill_the_fetches_say_so(monkeypatch):
    set_knobs(monkeypatch, store_cap_records=40000)
    ref = synth.make_reference(150, 12_000_000, seed=11, min_len=1500, max_len=300_000)
    batch = synth.make_reads(ref, 200_000, seed=12)
    est = estimator_sets(75)[1]
    with Session(0, FilterConfig(), 75, want_hist=True, want_identity="primary") as s:
        s.set_targets(ref.lengths)
        s.set_genome_runs(ref.genome_of_contig, len(ref.genomes))
        s.set_estimators(est)
        edges = np.linspace(0, batch.n_records, 20).astype(int)
        for lo, hi in zip(edges[:-1], edges[1:]):
            s.push(batch.slice(lo, hi))
        st, summ = s.finish()
        assert s.store_spills() >= 1
        for fetch in (s.genome_estimates, s.genome_entries, s.genome_entry_count, s.finish_genomes):
            with pytest.raises(CovError) as ei:
                fetch()
            assert ei.value.status == native.ERR_STATE
        assert s.hist().size == int(summ.hist_total)      # the host path still has everything it needs
        s.reset()
        s.set_estimators(est)
        s.push(batch.slice(0, 30000))
        s.finish()
        assert s.store_spills() == 0 and s.genome_entry_count() > 0


def test_finish_genomes_gives_the_verdict_of_finish():
    ref, batch = _synthetic(3_000, 30_000, seed=61)
    lo, hi = np.searchsorted(batch.tid, [700, 701])
    cut = np.searchsorted(batch.tid, 2_500)
    assert hi > lo
    ident = np.arange(batch.n_records)
    moved = np.concatenate([ident[:lo], ident[hi:cut], ident[lo:hi], ident[cut:]])
    b = batch
    n_ops = np.diff(b.cigar_off.astype(np.int64))[moved]
    off = np.zeros(len(moved) + 1, np.int64)
    np.cumsum(n_ops, out=off[1:])
    src = np.repeat(b.cigar_off[:-1].astype(np.int64)[moved] - off[:-1], n_ops) + np.arange(off[-1])
    unsorted = RecordBatch(b.tid[moved], b.pos[moved], b.flag[moved], b.mapq[moved], b.nm[moved], b.nm_kind[moved].copy(), b.l_seq[moved],
                           off.astype(np.uint32), np.ascontiguousarray(b.cigar[src], np.uint32))
    with Session(0, FilterConfig(), 75, want_hist=True, want_identity="primary") as s:
        s.set_targets(ref.lengths)
        s.set_genome_runs(ref.genome_of_contig, len(ref.genomes))
        s.set_estimators(estimator_sets(75)[1])
        s.push(unsorted)
        with pytest.raises(CovError) as full:
            s.finish()
        with pytest.raises(CovError) as lean:
            s.finish_genomes()
        assert full.value.status == native.ERR_UNSORTED
        assert (lean.value.status, lean.value.message) == (full.value.status, full.value.message)


def test_arguments_and_switching():
    with Session(0, FilterConfig(), 75, want_hist=True, want_identity="primary") as s:
        s.set_targets([1000, 2000, 3000])
        for bad in ([0, -1, 0], [0, 2, 1]):
            with pytest.raises(CovError) as ei:
                s.set_genome_runs(bad, 2)          # outside [0, n_gids)
            assert ei.value.status == native.ERR_INVALID_ARG
        est = [E.new_estimator_mean(0.0, 75, False), E.new_estimator_length()]
        s.set_estimators(est)
        with pytest.raises(CovError) as ei:
            s.finish_genomes()                     # neither genomes nor runs
        assert ei.value.status == native.ERR_STATE
        s.set_genome_runs([0, 0, 1], 2)
        s.finish()
        assert s.genome_entry_count() == 0
        with pytest.raises(CovError):
            s.estimates()
        s.set_genomes([0, -1, 0], 1)               # the contig-names table: the runs are off
        s.finish()
        assert s.genome_estimates().shape == (1, 2)
        for fetch in (s.genome_entry_count, s.genome_entries):
            with pytest.raises(CovError) as ei:
                fetch()
            assert ei.value.status == native.ERR_STATE
        s.set_genome_runs([0, 1, 1], 2)            # and back: the genomes and their mask are off
        st, _ = s.finish()
        assert s.genome_entry_count() == 0
        with pytest.raises(CovError):
            s.estimates()
        s.set_genome_runs(None, 0)                 # off: per-contig floats again
        s.finish()
        assert s.estimates().shape == (3, 2)
        with pytest.raises(CovError):
            s.genome_estimates()
        s.set_genome_runs([0, 1, 1], 2)
        s.set_targets([1000, 2000])                # new targets: off
        s.set_estimators(est)
        s.finish()
        assert s.estimates().shape == (2, 2)


# ---------------------------------------------------------------------------------------------------- through the binary
DEVICE_METHODS = ["relative_abundance", "mean", "trimmed_mean", "covered_fraction", "variance"]
DEVICE_LINE = "separator entries from the device (cov_set_genome_runs)"


def _both_paths(path, b, **args):
    """The table of the device path (default) and of COVERM_HOST_ESTIMATES=1: equal to each other and to the oracle's; only the first
    names cov_set_genome_runs in its timing lines."""
    want = O.run_cli("genome", [path], bams=[b], **args)
    dev = binary.run_full("genome", [path], env=dict(COVERM_CLI_TIMING="1"), **args)
    hst = binary.run_full("genome", [path], env=dict(COVERM_CLI_TIMING="1", COVERM_HOST_ESTIMATES="1"), **args)
    assert dev.stdout == hst.stdout
    assert dev.stdout == want
    assert DEVICE_LINE in dev.stderr and "histogram fetch:" not in dev.stderr
    assert "cov_set_genome_runs" not in hst.stderr
    m = re.search(r"cov_set_genome_runs\): (\d+) entries x (\d+) estimators, (\d+) bytes", dev.stderr)
    assert m and int(m.group(3)) == int(m.group(1)) * (24 + 4 * int(m.group(2)))
    return want


@pytest.mark.parametrize("mode", [dict(separator="~"), dict(single_genome=True)], ids=["separator", "single"])
@pytest.mark.parametrize("no_zeros", [False, True])
def test_fixture_through_the_binary_both_paths(tmp_path, mode, no_zeros):
    name = cases.S7 + ".bam"
    path = str(tmp_path / name)
    bamio.write_bam(path, load_fixture(name), block=3000)
    want = _both_paths(path, load_fixture(name), methods=DEVICE_METHODS, no_zeros=no_zeros, **mode)
    assert want.count("\n") >= 2


@pytest.mark.parametrize("mode", [dict(separator="~"), dict(single_genome=True)], ids=["separator", "single"])
@pytest.mark.parametrize("no_zeros", [False, True])
def test_synthetic_through_the_binary_both_paths(tmp_path, mode, no_zeros):
    """4 000 contigs in 400 genomes of 10 and 300 reads: about half of the genomes are zero rows between the entries, and most contigs of
    an entry are unobserved lengths.  (--min-covered-fraction 0: a few reads must count as coverage.)"""
    ref, batch = _synthetic(4_000, 300, seed=43)
    path = os.path.join(str(tmp_path), "synth.bam")
    cbam.write_bam(path, ref.names, ref.lengths, batch, with_seq=1, threads=8)
    want = _both_paths(path, to_bamdata(batch, ref.lengths, ref.names), methods=DEVICE_METHODS, no_zeros=no_zeros, min_covered_fraction=0, **mode)
    n_rows = want.count("\n") - 2      # (the header and the unmapped row)
    if mode.get("single_genome"):
        assert n_rows == 1
    else:
        assert (100 < n_rows < 300) if no_zeros else n_rows == 400


def test_interleaved_header_through_the_binary_both_paths(tmp_path):
    """Blocks of random length over six genomes and a read for every fifth contig: the header in which an unobserved contig counts for the
    entry in front of it, the one behind it, or none — against the oracle's own walk."""
    n = 2_000
    rng = np.random.default_rng(7)
    gid = []
    while len(gid) < n:
        gid += [int(rng.integers(0, 6))] * int(rng.choice([1, 1, 2, 3, 9, 60]))
    ref, batch = _synthetic(n, n // 5, seed=83)
    names = ["g%d~c%d" % (g, i) for i, g in enumerate(gid[:n])]
    path = os.path.join(str(tmp_path), "mixed.bam")
    cbam.write_bam(path, names, ref.lengths, batch, with_seq=1, threads=8)
    for no_zeros in (False, True):
        want = _both_paths(path, to_bamdata(batch, ref.lengths, names), methods=DEVICE_METHODS, no_zeros=no_zeros, min_covered_fraction=0, separator="~")
        assert want.count("\n") > 50


def test_a_name_without_the_separator_keeps_the_host_scan(tmp_path):
    """One name lacks the separator.  When a read lies on it the scan's own error comes, as the oracle's does; when the scan never asks for
    its genome (--no-zeros, the name in front of every read and apart from the first observed genome) the oracle's table comes — neither
    through the device path."""
    ref, batch = _synthetic(300, 600, seed=47)
    seen = np.zeros(300, bool)
    seen[batch.tid[batch.tid >= 0]] = True
    for tid, fails in ((int(np.nonzero(seen)[0][5]), True), (9, False)):
        names = list(ref.names)
        names[tid] = "noseparator"
        b2 = batch if fails else drop_reads_of(batch, np.arange(0, 20))
        path = os.path.join(str(tmp_path), "n%d.bam" % fails)
        cbam.write_bam(path, names, ref.lengths, b2, with_seq=1, threads=8)
        args = dict(methods=["mean"], separator="~", no_zeros=True, min_covered_fraction=0)
        runs = [subprocess.run(binary.argv("genome", [path], **args), capture_output=True, text=True, timeout=900,
                               env=dict(os.environ, COVERM_CLI_TIMING="1", **env)) for env in (dict(), dict(COVERM_HOST_ESTIMATES="1"))]
        assert runs[0].returncode == runs[1].returncode and runs[0].stdout == runs[1].stdout
        assert DEVICE_LINE not in runs[0].stderr
        if fails:
            assert runs[0].returncode != 0 and "Contig name does not contain split symbol" in runs[0].stderr
            with pytest.raises(O.OracleError):
                O.run_cli("genome", [path], bams=[to_bamdata(b2, ref.lengths, names)], **args)
        else:
            assert runs[0].returncode == 0, runs[0].stderr[-2000:]
            assert runs[0].stdout == O.run_cli("genome", [path], bams=[to_bamdata(b2, ref.lengths, names)], **args)
            assert runs[0].stdout.count("\n") > 20

"""`coverm-amd contig|genome ... --unsorted` through the binary: a BAM / SAM file whose records are not sorted by reference gives, character
for character, the oracle's text over the same records in the stable grouped order (tests/grouping.py) — and, for every method that only
depends on the record multiset, the table of the sorted file.  Without the flag the binary ends in the reference's unsorted message."""
import os
import subprocess

import numpy as np
import pytest

from coverm_amd import synth
from oracle import bamio
from oracle import oracle as O
from tests import binary
from tests.grouping import grouped_order, shuffles, take_bamdata, take_batch
from tests.test_gpu_abi_parity import to_bamdata
from tests.test_host_golden import _paired_sample

pytestmark = pytest.mark.gpu

MULTISET = ["mean", "trimmed_mean", "covered_fraction", "variance", "count", "reads_per_base", "rpkm"]
UNSORTED_MESSAGE = "BAM file appears to be unsorted. Input BAM files must be sorted by reference (i.e. by samtools sort)"


def run_unsorted(mode, paths, env=None, extra=(), **kw):
    v = binary.argv(mode, paths, **kw) + ["--unsorted"] + list(extra)
    r = subprocess.run(v, capture_output=True, text=True, timeout=900, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr[-3000:]
    return r


def sample(n_contigs=120, n_reads=60_000, seed=5):
    ref = synth.make_reference(n_contigs, 12_000_000, seed=seed, min_len=1500, max_len=400_000, contigs_per_genome=7)
    return ref, to_bamdata(synth.make_reads(ref, n_reads, seed=seed + 1), ref.lengths, ref.names)


def genome_definition(tmp_path, ref):
    p = tmp_path / "genomes.tsv"
    p.write_text("".join("g%d\t%s\n" % (i // 7, n) for i, n in enumerate(ref.names) if i % 11 != 3))      # some contigs outside every genome
    return str(p)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("unsorted")
    ref, b = sample()
    out = {"ref": ref, "sorted": b, "sorted_path": str(d / "s.bam"), "dir": d, "shuffled": {}}
    bamio.write_bam(out["sorted_path"], b, level=1)
    for kind, perm in shuffles(len(b.tid), 9).items():
        sh = take_bamdata(b, perm)
        os.makedirs(str(d / kind))
        p = str(d / kind / "s.bam")                                                 # the same file stem: the same sample name in every table
        bamio.write_bam(p, sh, level=1)
        out["shuffled"][kind] = (p, sh, take_bamdata(sh, grouped_order(sh.tid, len(sh.ref_lens))))
    return out


@pytest.mark.parametrize("kind", ["random", "name", "blocks"])
@pytest.mark.parametrize("mode", ["contig", "genome_definition", "genome_separator"])
@pytest.mark.parametrize("methods", [MULTISET, ["anir"]], ids=["multiset", "anir"])
def test_table_is_the_oracles_over_the_grouped_sequence(files, tmp_path, kind, mode, methods):
    p, _, grouped = files["shuffled"][kind]
    kw = dict(methods=methods, min_covered_fraction=0)
    if mode == "genome_definition":
        kw["genome_definition"] = genome_definition(tmp_path, files["ref"])
    elif mode == "genome_separator":
        kw["separator"] = "~"
    m = "contig" if mode == "contig" else "genome"
    r = run_unsorted(m, [p], extra=["-v"], **kw)
    assert r.stdout == O.run_cli(m, [p], bams=[grouped], **kw)
    assert "--unsorted" in r.stderr and "records moved" in r.stderr             # -v: one line with the records moved and the COV_K_GROUP time
    if methods is MULTISET:
        assert r.stdout == binary.run(m, [files["sorted_path"]], **kw)           # the table of the sorted file
        assert r.stdout == O.run_cli(m, [files["sorted_path"]], bams=[files["sorted"]], **kw)


def test_without_the_flag_the_file_is_refused_as_before(files):
    for kind, (p, _, _) in files["shuffled"].items():
        r = subprocess.run(binary.argv("contig", [p], methods=["mean"]), capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and UNSORTED_MESSAGE in r.stderr and "\n" not in r.stdout.strip(), kind


@pytest.mark.parametrize("route", ["device", "cpu_stream", "no_stream"])
def test_every_reader_route(files, route):
    """Device ingest, the streamed CPU reader (COVERM_NO_GPU_INGEST) and the whole-file host reader (--no-stream) end in the same table."""
    p, _, grouped = files["shuffled"]["random"]
    kw = dict(methods=MULTISET + ["anir"], min_covered_fraction=0)
    r = run_unsorted("contig", [p], env={"COVERM_NO_GPU_INGEST": "1"} if route == "cpu_stream" else None, extra=["--no-stream"] if route == "no_stream" else [], **kw)
    assert r.stdout == O.run_cli("contig", [p], bams=[grouped], **kw)


def test_sam_text_input(files, tmp_path):
    _, sh, grouped = files["shuffled"]["name"]
    p = str(tmp_path / "s.sam")
    with open(p, "w") as f:
        for n, l in zip(sh.ref_names, sh.ref_lens):
            f.write("@SQ\tSN:%s\tLN:%d\n" % (n, l))
        ops = "MIDNSHP=X"
        for i in range(len(sh.tid)):
            cig = "".join("%d%s" % (w >> 4, ops[w & 15]) for w in sh.cigar[sh.cigar_off[i]:sh.cigar_off[i + 1]]) or "*"
            t = int(sh.tid[i])
            f.write("r%d\t%d\t%s\t%d\t%d\t%s\t*\t0\t0\t*\t*%s\n" % (i, sh.flag[i], sh.ref_names[t] if t >= 0 else "*", sh.pos[i] + 1, sh.mapq[i], cig,
                                                              "\tNM:i:%d" % sh.nm[i] if sh.nm_kind[i] == 1 else ""))
    # (SEQ '*': l_seq = 0 in the file — compare with the oracle over the records as the file holds them)
    back = bamio.read_sam(p)
    assert len(back.tid) == len(sh.tid) and (np.asarray(back.tid) == np.asarray(sh.tid)).all()
    g = take_bamdata(back, grouped_order(back.tid, len(back.ref_lens)))
    kw = dict(methods=["mean", "covered_fraction", "variance", "count"], min_covered_fraction=0)
    assert run_unsorted("contig", [p], **kw).stdout == O.run_cli("contig", [p], bams=[g], **kw)


@pytest.mark.parametrize("host_pair", [False, True])
def test_pair_mode_filter_on_both_routes(tmp_path, host_pair):
    """A pair-mode threshold: the device's pair filter behind cov_group_records, and the host's (COVERM_PAIR_ON_HOST) behind
    covh_group_by_reference, see the same grouped sequence."""
    b = _paired_sample(20_000, seed=17)
    sh = take_bamdata(b, shuffles(len(b.tid), 18, b.qname)["name"])
    p = str(tmp_path / "pairs.bam")
    bamio.write_bam(p, sh, level=1)
    g = take_bamdata(sh, grouped_order(sh.tid, len(sh.ref_lens)))
    kw = dict(methods=["mean", "count", "covered_fraction"], min_covered_fraction=0, min_read_percent_identity_pair=0.95, proper_pairs_only=True)
    r = run_unsorted("contig", [p], env={"COVERM_PAIR_ON_HOST": "1"} if host_pair else None, **kw)
    assert r.stdout == O.run_cli("contig", [p], bams=[g], **kw)


def test_gff(tmp_path):
    ref, b = sample(n_contigs=12, n_reads=20_000, seed=23)
    sh = take_bamdata(b, shuffles(len(b.tid), 24)["blocks"])
    p = str(tmp_path / "s.bam")
    bamio.write_bam(p, sh, level=1)
    lines = ["##gff-version 3"]
    rng = np.random.default_rng(25)
    for t, (n, l) in enumerate(zip(ref.names, ref.lengths)):
        for k in range(3):
            a = int(rng.integers(1, max(2, l - 600)))
            lines.append("%s\tx\tCDS\t%d\t%d\t.\t+\t0\tID=g%d_%d" % (n, a, min(int(l), a + int(rng.integers(50, 500))), t, k))
    gff = tmp_path / "s.gff"
    gff.write_text("\n".join(lines) + "\n")
    g = take_bamdata(sh, grouped_order(sh.tid, len(sh.ref_lens)))
    kw = dict(methods=["mean", "covered_fraction", "count"], min_covered_fraction=0, gff=str(gff))
    want = O.run_cli("contig", [p], bams=[g], **kw)
    assert run_unsorted("contig", [p], **kw).stdout == want                                  # records back from the grouped store
    assert run_unsorted("contig", [p], extra=["--no-stream"], **kw).stdout == want          # whole-file host reader, grouped on the host

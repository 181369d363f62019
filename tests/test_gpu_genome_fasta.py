"""`coverm genome` with genomes defined by FASTA files (-f, -d -x, --genome-fasta-list) through the coverm-amd binary: the
reference's own golden (test_genome_all_methods), text identity with the --genome-definition path that resolves to the same
genome -> contigs table, the oracle as a checker, config 3 at 20 M reads with 500 genome files, and the errors."""
import os
import shutil
import subprocess

import pytest

from coverm_amd import bam as cbam
from coverm_amd import synth
from oracle import oracle as O
from oracle import bamio
from tests import binary
from tests.fixtures import FIXDIR, load_fixture
from tests.golden import cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FASTA = os.path.join(ROOT, "tests", "golden", "fasta")
RAW = os.path.join(ROOT, "tests", "golden", "raw")
CASE = {c["id"]: c for c in cases.CLI_CASES}


def run(argv, timeout=600):
    return subprocess.run(argv, capture_output=True, text=True, timeout=timeout)


def ok(argv, timeout=600):
    r = run(argv, timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def raw_bam(tmp_path, name):
    p = str(tmp_path / name)
    shutil.copy(os.path.join(RAW, name), p)
    return p


def fasta_from_definition(definition, d):
    """One FASTA file per genome of a definition file (genome order kept), each holding that genome's contigs."""
    os.makedirs(d, exist_ok=True)
    order, contigs = [], {}
    for line in open(definition):
        g, c = line.rstrip("\n").split("\t")
        if g not in contigs:
            order.append(g)
            contigs[g] = []
        contigs[g].append(c.split()[0])
    paths = []
    for g in order:
        p = os.path.join(d, g + ".fna")
        with open(p, "w") as fh:
            fh.write("".join(">%s some description\nACGTACGTAC\nGGTT\n" % c for c in contigs[g]))
        paths.append(p)
    return order, paths


def table(text):
    rows = text.split("\n")
    return [rows[0]] + sorted(rows[1:])


# ---------------------------------------------------------------------------------------------------- reference golden
def test_genome_all_methods_fasta_directory(tmp_path):
    """tests/test_cmdline.rs:2785-2814 literally: -b 7seqs.fnaVbad_read.bam -d genomes_dir_7seqs -x fasta."""
    bam = raw_bam(tmp_path, "7seqs.fnaVbad_read.bam")
    c = CASE["cli_genome_all_methods"]
    m = ["-m", "covered_bases", "covered_fraction", "mean", "variance", "trimmed_mean", "rpkm", "relative_abundance", "length",
         "--min-covered-fraction", "0"]
    d7 = os.path.join(FASTA, "genomes_dir_7seqs")
    files = [os.path.join(d7, "genome%d.fasta" % i) for i in range(1, 7)]
    lst = tmp_path / "genomes.txt"
    lst.write_text("\n".join(files) + "\n")
    defn = os.path.join(FIXDIR, "7seqs.definition")
    for fmt in ("sparse", "dense"):
        base = [binary.BIN, "genome", "-b", bam, "--output-format", fmt] + m
        want = ok(base + ["--genome-definition", defn])
        if fmt == "sparse":
            assert table(want) == table(c["expected"])
        for src in (["-d", d7, "-x", "fasta"], ["-f"] + files, ["--genome-fasta-list", str(lst)]):
            got = ok(base + src)
            assert got == want, (src, got)
            if fmt == "sparse":
                assert table(got) == table(c["expected"])


# ---------------------------------------------------------------------------------------------------- -d == --genome-definition
_DEF_CASES = [c for c in cases.CLI_CASES if c["mode"] == "genome" and "genome_definition" in c["args"]]


@pytest.mark.parametrize("case", _DEF_CASES, ids=[c["id"] for c in _DEF_CASES])
def test_fasta_directory_equals_genome_definition(case, tmp_path):
    paths = []
    for b in case["bams"]:
        p = str(tmp_path / (os.path.splitext(b)[0] + ".bam"))
        bamio.write_bam(p, load_fixture(b), block=3000)
        paths.append(p)
    a = dict(case["args"])
    defn = os.path.join(FIXDIR, a.pop("genome_definition"))
    order, files = fasta_from_definition(defn, str(tmp_path / "genomes"))
    assert order == sorted(order)                 # -d lists the files bytewise: the definition's genome order
    base = binary.argv("genome", paths, **a)
    r_def = run(base + ["--genome-definition", defn])
    r_dir = run(base + ["-d", str(tmp_path / "genomes")])
    assert r_dir.returncode == r_def.returncode
    if case["match"] == "error":
        assert r_dir.returncode != 0 and case["expected"] in r_dir.stderr and r_dir.stdout == ""
        return
    assert r_def.returncode == 0, r_def.stderr
    assert r_dir.stdout == r_def.stdout


def test_fasta_directory_with_gff_equals_genome_definition(tmp_path):
    """--gff in genome mode (tests/test_cmdline.rs:181-206) with the genomes of tests/data/2seqs_split_genomes."""
    c = cases.GENE_CLI_CASES[-1]
    assert c["mode"] == "genome" and c["args"]["genome_definition"] == "2seqs.genome-definition"
    p = str(tmp_path / (os.path.splitext(c["bams"][0])[0] + ".bam"))
    bamio.write_bam(p, load_fixture(c["bams"][0]), block=3000)
    a = dict(c["args"])
    a.pop("genome_definition")
    a["gff"] = os.path.join(FIXDIR, a["gff"])
    base = binary.argv("genome", [p], **a)
    want = ok(base + ["--genome-definition", os.path.join(FIXDIR, "2seqs.genome-definition")])
    got = ok(base + ["-d", os.path.join(FASTA, "2seqs_split_genomes")])
    assert got == want
    for e in c["expected"]:
        assert e in got


def test_compressed_genomes_vs_oracle(tmp_path):
    b = "2seqs.reads_for_seq1_and_seq2.bam"
    p = raw_bam(tmp_path, b)
    defn = tmp_path / "seqs.tsv"
    defn.write_text("seq1\tseq1\nseq2\tseq2\n")
    for fmt in ("dense", "sparse"):
        got = ok(binary.argv("genome", [p], output_format=fmt, min_covered_fraction=0)
                 + ["-d", os.path.join(FASTA, "genomes_dir_compressed"), "-x", "fna.gz"])
        assert got == O.run_cli("genome", [p], bams=[load_fixture(b)], output_format=fmt, min_covered_fraction=0,
                                genome_definition=str(defn))
        assert "seq1" in got and "seq2" in got


# ---------------------------------------------------------------------------------------------------- config 3, 20 M reads
def test_config3_full_size_500_genome_files(tmp_path):
    """Config 3's command (-m relative_abundance rpkm tpm) at 20 M reads over 2 000 contigs, the genomes given as 500 FASTA files:
    character for character the text of the equivalent --genome-definition run, dense and sparse."""
    ref = synth.make_reference(2000, 400_000_000, seed=1)
    batch = synth.make_reads(ref, 20_000_000, seed=2)
    d = "/dev/shm" if os.path.isdir("/dev/shm") else str(tmp_path)
    path = os.path.join(d, "coverm_amd_test_fasta_%d.bam" % os.getpid())
    try:
        cbam.write_bam(path, ref.names, ref.lengths, batch, with_seq=2, threads=16)
        gdir = tmp_path / "genomes"
        gdir.mkdir()
        rows = []
        per = {}
        for i, n in enumerate(ref.names):
            if i % 11 == 3:
                continue                                           # some contigs in no genome (genome.rs:170-171)
            per.setdefault("bin%03d" % (i % 500), []).append(n)
        for g in sorted(per):
            with open(str(gdir / (g + ".fna")), "w") as fh:
                fh.write("".join(">%s len=%d\n%s\n" % (n, k, "ACGT" * 20) for k, n in enumerate(per[g])))
            rows += ["%s\t%s\n" % (g, n) for n in per[g]]
        defn = tmp_path / "genomes.tsv"
        defn.write_text("".join(rows))
        assert len(per) == 500
        for fmt in ("dense", "sparse"):
            base = binary.argv("genome", [path], threads=16, methods=["relative_abundance", "rpkm", "tpm"], output_format=fmt)
            want = ok(base + ["--genome-definition", str(defn)], timeout=900)
            got = ok(base + ["-d", str(gdir)], timeout=900)
            assert got == want
            assert got.count("\n") >= 500
    finally:
        if os.path.exists(path):
            os.remove(path)


# ---------------------------------------------------------------------------------------------------- errors
def test_errors_through_the_binary(tmp_path):
    bam = raw_bam(tmp_path, "7seqs.fnaVbad_read.bam")
    clash = [os.path.join(FASTA, "contig_name_clashing", "genome%d.fna" % i) for i in (1, 2, 3)]
    for sub in ("a", "b"):
        (tmp_path / sub).mkdir()
        (tmp_path / sub / "g.fna").write_text(">%s_contig\nACGT\n" % sub)
    (tmp_path / "empty").mkdir()
    d7 = os.path.join(FASTA, "genomes_dir_7seqs")
    for extra, needle in (
            (["-f"] + clash, "The contig 'random_sequence_length_500_1' has been assigned to multiple genomes, at least 'genome1' and 'genome2'"),
            (["-f", str(tmp_path / "a" / "g.fna"), str(tmp_path / "b" / "g.fna")], "The genome name g was derived from >1 file"),
            (["-d", str(tmp_path / "empty")], "No genome FASTA files with extension .fna"),
            (["-d", d7, "-x", "fasta", "-f", clash[0]], "the argument '--genome-fasta-files' cannot be used with '--genome-fasta-directory'"),
            (["-d", d7, "-x", "fasta", "--single-genome"], "the argument '--genome-fasta-directory' cannot be used with '--single-genome'")):
        r = run([binary.BIN, "genome", "-b", bam] + extra)
        assert r.returncode == 1, (extra, r.stderr)
        assert needle in r.stderr, (extra, r.stderr)
        assert r.stdout == "", extra

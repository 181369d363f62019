"""`coverm-amd depth`: what it refuses while it reads its arguments, before any device is touched (so these run without one)."""
import subprocess

import pytest

from tests import binary

SAM = "@SQ\tSN:c1\tLN:1000\nq\t0\tc1\t5\t30\t10M\t*\t0\t0\tACGTACGTAC\tIIIIIIIIII\tNM:i:0\n"


def _refused(argv, stdin=subprocess.DEVNULL):
    r = subprocess.run(argv, capture_output=True, text=True, timeout=120, stdin=stdin)
    assert r.returncode != 0 and r.stdout == ""
    return r.stderr


@pytest.mark.parametrize("extra", [["-m", "mean"], ["--methods", "mean"], ["--gff", "genes.gff"], ["--devices", "0,1"], ["--contig-end-exclusion", "0"],
                                   ["-s", "~"], ["--separator", "~"], ["--single-genome"], ["--genome-definition", "g.tsv"], ["-f", "a.fna"],
                                   ["--genome-fasta-files", "a.fna"], ["-d", "dir"], ["--genome-fasta-directory", "dir"], ["-x", "fa"],
                                   ["--genome-fasta-list", "l.txt"], ["--use-full-contig-names"], ["--min-covered-fraction", "10"], ["--output-format", "sparse"]])
def test_options_of_the_other_subcommands_are_refused(tmp_path, extra):
    p = tmp_path / "one.sam"
    p.write_text(SAM)
    err = _refused([binary.BIN, "depth", "-b", str(p)] + extra)
    assert "'%s' cannot be used with 'depth'" % extra[0] in err
    err = _refused([binary.BIN, "depth"] + extra + ["-b", str(p)])      # wherever it stands
    assert "'%s' cannot be used with 'depth'" % extra[0] in err


def test_inputs_are_checked_as_for_contig():
    assert "--bam-files is required" in _refused([binary.BIN, "depth"])
    err = _refused([binary.BIN, "depth", "-b", "-", "-"])
    assert "standard input" in err and "once" in err
    err = _refused([binary.BIN, "depth", "-b", "-", "--no-stream"])
    assert "--no-stream" in err and "pipe" in err
    assert "unknown argument --inverse" in _refused([binary.BIN, "depth", "-b", "x.bam", "--inverse"])
    assert "invalid value" in _refused([binary.BIN, "depth", "-b", "x.bam", "--min-mapq", "300"])


def test_usage_names_the_subcommand():
    r = subprocess.run([binary.BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "coverm-amd depth -b" in r.stderr and "--no-zeros" in r.stderr

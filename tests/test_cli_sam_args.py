"""SAM text and pipes on the command line: what coverm-amd refuses while it reads its arguments and its inputs' first bytes, before any
device is touched (so these run without one, like the refusals of tests/test_group_host.py)."""
import subprocess

from oracle import bamio
from tests import binary

SAM = "@SQ\tSN:c1\tLN:1000\nq\t0\tc1\t5\t30\t10M\t*\t0\t0\tACGTACGTAC\tIIIIIIIIII\tNM:i:0\n"


def _refused(argv, stdin=subprocess.DEVNULL):
    r = subprocess.run(argv, capture_output=True, text=True, timeout=120, stdin=stdin)
    assert r.returncode != 0 and r.stdout == ""
    return r.stderr


def test_standard_input_twice_is_refused():
    for mode in (["contig"], ["genome", "-s", "~"]):
        err = _refused([binary.BIN] + mode + ["-b", "-", "-", "-m", "mean"])
        assert "standard input" in err and "once" in err


def test_no_stream_on_a_pipe_is_refused(tmp_path):
    err = _refused([binary.BIN, "contig", "-b", "-", "--no-stream", "-m", "mean"])
    assert "--no-stream" in err and "pipe" in err


def test_span_mode_refuses_sam_text(tmp_path):
    p = tmp_path / "one.sam"
    p.write_text(SAM)
    err = _refused([binary.BIN, "contig", "-b", str(p), "--devices", "0,1", "-m", "mean"])
    assert "--devices" in err and "SAM" in err and "fewer" in err
    err = _refused([binary.BIN, "contig", "-b", "-", "--devices", "0,1", "-m", "mean"])
    assert "--devices" in err and "fewer" in err


def test_bam_on_standard_input_names_what_is_supported(tmp_path):
    p = str(tmp_path / "x.bam")
    bamio.write_bam(p, bamio.read_bam(binary.ROOT + "/tests/golden/raw/tpm_test.bam"), level=1)
    with open(p, "rb") as f:
        err = _refused([binary.BIN, "contig", "-b", "-", "-m", "mean"], stdin=f)
    assert "BAM from a pipe is not supported yet; SAM text is (e.g. `samtools view -h`), or pass the file's path" in err

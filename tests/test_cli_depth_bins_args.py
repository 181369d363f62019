"""`coverm-amd depth --bin-size / --bin-value`: what is refused while the arguments are read, before any device is touched (so these run
without one)."""
import subprocess

import pytest

from tests import binary


def _refused(argv):
    r = subprocess.run(argv, capture_output=True, text=True, timeout=120, stdin=subprocess.DEVNULL)
    assert r.returncode != 0 and r.stdout == ""
    return r.stderr


@pytest.mark.parametrize("value", ["0", "-5", "abc", "1.5", "", "2147483648", "99999999999999999999"])
def test_bin_size_must_be_a_positive_number_below_2_31(value):
    err = _refused([binary.BIN, "depth", "-b", "x.bam", "--bin-size", value])
    assert "invalid value '%s' for '--bin-size'" % value in err


def test_bin_size_needs_a_value():
    assert "missing value for --bin-size" in _refused([binary.BIN, "depth", "-b", "x.bam", "--bin-size"])


@pytest.mark.parametrize("argv", [["--bin-value", "sum"], ["--bin-value", "mean", "-o", "x"], ["--no-zeros", "--bin-value", "max"]])
def test_bin_value_needs_bin_size(argv):
    err = _refused([binary.BIN, "depth", "-b", "x.bam"] + argv)
    assert "--bin-value" in err and "--bin-size" in err


def test_bin_value_is_one_of_five():
    err = _refused([binary.BIN, "depth", "-b", "x.bam", "--bin-size", "100", "--bin-value", "median"])
    assert "invalid value 'median' for '--bin-value'" in err
    assert "missing value for --bin-value" in _refused([binary.BIN, "depth", "-b", "x.bam", "--bin-size", "100", "--bin-value"])


@pytest.mark.parametrize("sub", ["contig", "genome", "filter"])
@pytest.mark.parametrize("opt", ["--bin-size", "--bin-value"])
def test_the_other_subcommands_do_not_know_the_options(sub, opt):
    assert "unknown argument " + opt in _refused([binary.BIN, sub, "-b", "x.bam", opt, "100"])


def test_the_largest_bin_size_passes_the_argument_check():
    """2^31 - 1 is a bin size: the run ends at the missing file, not at the option."""
    err = _refused([binary.BIN, "depth", "-b", "/nonexistent/x.bam", "--bin-size", "2147483647", "--bin-value", "covered"])
    assert "invalid value" not in err and "unknown argument" not in err


def test_usage_names_the_options():
    r = subprocess.run([binary.BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--bin-size N" in r.stderr and "mean|sum|min|max|covered" in r.stderr

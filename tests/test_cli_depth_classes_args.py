"""`coverm-amd depth --quantize / --thresholds`: what is refused while the arguments are read, before any device is touched (so these run
without one)."""
import subprocess

import pytest

from tests import binary


def _refused(argv):
    r = subprocess.run(argv, capture_output=True, text=True, timeout=120, stdin=subprocess.DEVNULL)
    assert r.returncode != 0 and r.stdout == ""
    return r.stderr


DEPTH = [binary.BIN, "depth", "-b", "x.bam"]


@pytest.mark.parametrize("other,argv", [("--regions", ["--regions", "r.bed"]), ("--bin-size", ["--bin-size", "100"]), ("--bin-value", ["--bin-value", "sum"]),
                                        ("--thresholds", ["--thresholds", "1,10"]), ("--no-zeros", ["--no-zeros"])])
@pytest.mark.parametrize("first", [True, False])
def test_quantize_is_refused_beside(other, argv, first):
    q = ["--quantize", "0:1:5:"]
    err = _refused(DEPTH + (q + argv if first else argv + q))
    assert "'--quantize' cannot be used with '%s'" % other in err


def test_no_zeros_beside_quantize_says_what_to_do_instead():
    assert "leave the zero class out of the spec" in _refused(DEPTH + ["--quantize", "0:1:", "--no-zeros"])


@pytest.mark.parametrize("spec", ["5", "1:1", "5:1", "a:b", "1::2", "-1:2", ":".join(map(str, range(17))), "0:2147483648", ""])
def test_bad_quantize_specs(spec):
    err = _refused(DEPTH + ["--quantize", spec])
    assert "invalid value for '--quantize'" in err and "'%s'" % spec in err


@pytest.mark.parametrize("value", ["", "a", "1,,2", "3,2", "1,1", "-1", "2147483648", ",".join(map(str, range(17)))])
def test_bad_thresholds(value):
    err = _refused(DEPTH + ["--bin-size", "100", "--thresholds", value])
    assert "invalid value for '--thresholds'" in err and "'%s'" % value in err


def test_the_options_need_a_value():
    assert "missing value for --quantize" in _refused(DEPTH + ["--quantize"])
    assert "missing value for --thresholds" in _refused(DEPTH + ["--regions", "r.bed", "--thresholds"])


@pytest.mark.parametrize("argv", [["--thresholds", "1,10,30"], ["--thresholds", "1", "-o", "x"], ["--no-zeros", "--thresholds", "0,5"]])
def test_thresholds_need_regions_or_bin_size(argv):
    err = _refused(DEPTH + argv)
    assert "'--thresholds' needs '--regions' or '--bin-size'" in err


@pytest.mark.parametrize("argv", [["--bin-size", "100"], ["--regions", "r.bed"]])
def test_thresholds_refuse_bin_value(argv):
    err = _refused(DEPTH + argv + ["--thresholds", "1,10", "--bin-value", "covered"])
    assert "'--thresholds' cannot be used with '--bin-value'" in err and "value columns" in err


@pytest.mark.parametrize("sub", ["contig", "genome", "filter"])
@pytest.mark.parametrize("opt,value", [("--quantize", "0:1:"), ("--thresholds", "1,10")])
def test_the_other_subcommands_do_not_know_the_options(sub, opt, value):
    assert "unknown argument " + opt in _refused([binary.BIN, sub, "-b", "x.bam", opt, value])


def test_good_values_pass_the_argument_check():
    """The run ends at the missing file, not at the options."""
    for argv in (["--quantize", "0:1:5:150:"], ["--quantize", ":"], ["--bin-size", "100", "--thresholds", "1,10,30", "--no-zeros"],
                 ["--bin-size", "7", "--thresholds", ",".join(map(str, range(16)))]):
        err = _refused([binary.BIN, "depth", "-b", "/nonexistent/x.bam"] + argv)
        assert "invalid value" not in err and "unknown argument" not in err and "cannot be used" not in err and "needs" not in err, argv


def test_usage_names_the_options():
    r = subprocess.run([binary.BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--quantize" in r.stderr and "--thresholds" in r.stderr and "lo:inf" in r.stderr

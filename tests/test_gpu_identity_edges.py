"""The exact parallel identity sums (k_id_approx, k_id_predict, k_id_exact, k_id_combine) where their three conditions bind: the running
sum on a power of two at the end of a chunk and at lanes 0 and 63 of a replayed block, one exact rounding tie at the first and last
record of an interior chunk, at lanes 0 and 63 of a block, in the head and in the tail, contigs that start at records 0, 1 and 1023
(mod 1024), 64, 65 and 129 interior chunks, and records that do not count on chunk borders.  The inputs are the chains of
tests/edge_inputs.py (tests/test_edge_inputs.py proves on the CPU that each tie meets the sum in its binade, that ties round up and down,
and that the other rounding ends in other bits).  Every case goes through tests.test_gpu_abi_parity.compare — both sums as uint64 against
the oracle's serial chain, beside every integer — with the parallel kernels and with the serial one."""
import numpy as np
import pytest

from coverm_amd.engine import FilterConfig, Session
from oracle import oracle as O
from tests import edge_inputs as X
from tests.test_gpu_abi_parity import compare, to_batch

pytestmark = pytest.mark.gpu

MODES = ["parallel", "serial"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("start", [0, 1])
def test_power_of_two_at_a_chunk_end(start, mode, monkeypatch):
    """4 096 records of identity 1.0, then fillers.  From record 0 the sum is exactly 2^11 after chunk 1 and 2^12 after chunk 3, and the
    record that lifts it to 2^k is lane 63 of its block; from record 1 it is lane 0."""
    monkeypatch.setenv("COVERM_IDENTITY", mode)
    compare(X.power_of_two_sample(start))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("e", X.TIE_BINADES)
def test_one_tie_in_binade(e, mode, monkeypatch):
    """One exact rounding tie per contig while the sum is in binade e: first and last record of an interior chunk, lanes 0 and 63 of a
    64-record block, head, tail (no head from binade 10 on: 1023 addends cannot lift the sum there)."""
    monkeypatch.setenv("COVERM_IDENTITY", mode)
    compare(X.tie_sample(e)[0])


@pytest.mark.parametrize("mode", MODES)
def test_contigs_on_chunk_borders(mode, monkeypatch):
    """Read counts 1 .. 3073 back to back: first records at 0, 1 and 1023 (mod 1024), 2 048 records without head and tail, a contig inside
    a chunk, a contig across a border that holds no whole chunk."""
    monkeypatch.setenv("COVERM_IDENTITY", mode)
    compare(X.layout_sample()[0])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n_chunks", [64, 65, 129])
def test_batches_of_chunk_records(n_chunks, mode, monkeypatch):
    """64, 65 and 129 interior chunks: k_id_combine's loop over 64 chunk records runs once, twice, three times; binades 1 to 16, 17 with 129."""
    monkeypatch.setenv("COVERM_IDENTITY", mode)
    compare(X.batches_sample(n_chunks)[0])


@pytest.mark.parametrize("mode", MODES)
def test_records_that_do_not_count(mode, monkeypatch):
    """Supplementary, secondary and unmapped records inside interior chunks and on their borders (the two streams differ), an identity of
    0.0 and a negative one while the sum is above 4 096."""
    monkeypatch.setenv("COVERM_IDENTITY", mode)
    b = X.uncounted_sample()[0]
    compare(b)
    compare(b, ff=(True, False, True))
    st = compare(b, ff=(True, True, True))          # secondary records count for the not-supplementary sum alone: the streams differ
    assert st["sum_identity_primary"][1] != st["sum_identity_nonsupp"][1]


@pytest.mark.parametrize("want", ["primary", "nonsupp"])
def test_a_single_stream(want, monkeypatch):
    """One stream only (COV_WANT_IDENTITY_PRIMARY_ONLY / _NONSUPP_ONLY): the kernels run with the other stream's pointer NULL."""
    monkeypatch.setenv("COVERM_IDENTITY", "parallel")
    b = X.concat([X.tie_sample(10)[0], X.uncounted_sample()[0], X.power_of_two_sample(1)])
    exp = O.integer_stats(b, O.FlagFilter(True, True, False), None, 75)[0]
    with Session(0, FilterConfig(), 75, want_identity=want) as s:
        s.set_targets(b.ref_lens)
        s.push(to_batch(b))
        st, _ = s.finish()
    seen = exp["seen"] == 1
    np.testing.assert_array_equal(st["sum_identity_" + want][seen].view(np.uint64), exp["id_" + want][seen].view(np.uint64))

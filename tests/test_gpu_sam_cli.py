"""SAM text through the binary: for a sorted synthetic sample the table from s.sam (decoded on the device as it streams in) equals, character
for character, the oracle's over oracle.bamio.read_sam's records of the same text, the table with COVERM_SAM_ON_HOST=1 and the table with
--no-stream (the whole-file host route) — for contig with all methods, the three genome modes, a single-read filter, a pair-mode filter
(the device pair filter over name hashes computed from SAM text), --gff and --unsorted.  The same commands with the text on standard input
give the same bytes with `stdin` as the sample name.  No input here may reach the host route: the fallback message must be absent."""
import os
import resource
import subprocess
import threading

import numpy as np
import pytest

from oracle import bamio
from oracle import oracle as O
from tests import binary, samtext
from tests.grouping import grouped_order, shuffles, take_bamdata
from tests.test_gpu_unsorted_cli import genome_definition, sample
from tests.test_host_golden import _paired_sample

pytestmark = pytest.mark.gpu

ALL = ["mean", "trimmed_mean", "covered_fraction", "covered_bases", "variance", "length", "count", "reads_per_base", "rpkm", "tpm", "anir"]
FALLBACK = "handed to the host route"
TIMING = {"COVERM_CLI_TIMING": "1"}


def run(mode, path, env=None, extra=(), stdin=None, **kw):
    v = binary.argv(mode, [path], **kw) + list(extra)
    r = subprocess.run(v, capture_output=True, text=True, timeout=900, env=dict(os.environ, **TIMING, **(env or {})), stdin=stdin if stdin is not None else subprocess.DEVNULL)
    assert r.returncode == 0, r.stderr[-3000:]
    return r


def device_route(r):
    assert "device SAM decode" in r.stderr and FALLBACK not in r.stderr, r.stderr[-2000:]
    return r.stdout


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("samcli")
    ref, b = sample()
    p = str(d / "s.sam")
    samtext.write(p, b, seed=7)
    return {"dir": d, "ref": ref, "path": p, "records": bamio.read_sam(p)}


def check_all_routes(mode, p, records, extra=(), **kw):
    want = O.run_cli(mode, [p], bams=[records], **kw)
    assert device_route(run(mode, p, extra=extra, **kw)) == want
    assert run(mode, p, env={"COVERM_SAM_ON_HOST": "1"}, extra=extra, **kw).stdout == want
    assert run(mode, p, extra=list(extra) + ["--no-stream"], **kw).stdout == want
    with open(p, "rb") as f:
        got = device_route(run(mode, "-", extra=extra, stdin=f, **kw))
    assert got == O.run_cli(mode, ["stdin.sam"], bams=[records], **kw)
    return want


def test_contig_all_methods(files):
    want = check_all_routes("contig", files["path"], files["records"], methods=ALL, min_covered_fraction=0)
    assert want.count("\n") > 100


@pytest.mark.parametrize("mode", ["definition", "separator", "single"])
def test_genome_modes(files, tmp_path, mode):
    kw = dict(methods=["mean", "covered_fraction", "variance", "count"], min_covered_fraction=0)
    if mode == "definition":
        kw["genome_definition"] = genome_definition(tmp_path, files["ref"])
    elif mode == "separator":
        kw["separator"] = "~"
    else:
        kw["single_genome"] = True
    check_all_routes("genome", files["path"], files["records"], **kw)


def test_single_read_filter(files):
    check_all_routes("contig", files["path"], files["records"], methods=["mean", "count"], min_covered_fraction=0, min_read_percent_identity=0.97, min_read_aligned_length=60)


def test_pair_mode_filter(tmp_path):
    b = _paired_sample(20_000, seed=31)
    p = str(tmp_path / "s.sam")
    samtext.write(p, b, seed=8)
    records = bamio.read_sam(p)
    assert records.qname == b.qname
    r = check_all_routes("contig", p, records, methods=["mean", "count", "covered_fraction"], min_covered_fraction=0, min_read_percent_identity_pair=0.95, proper_pairs_only=True)
    assert r.count("\n") > 3


def test_gff(tmp_path):
    ref, b = sample(n_contigs=12, n_reads=20_000, seed=23)
    p = str(tmp_path / "s.sam")
    samtext.write(p, b, seed=9)
    records = bamio.read_sam(p)
    lines = ["##gff-version 3"]
    rng = np.random.default_rng(25)
    for t, (n, l) in enumerate(zip(ref.names, ref.lengths)):
        for k in range(3):
            a = int(rng.integers(1, max(2, l - 600)))
            lines.append("%s\tx\tCDS\t%d\t%d\t.\t+\t0\tID=g%d_%d" % (n, a, min(int(l), a + int(rng.integers(50, 500))), t, k))
    gff = tmp_path / "s.gff"
    gff.write_text("\n".join(lines) + "\n")
    check_all_routes("contig", p, records, methods=["mean", "covered_fraction", "count"], min_covered_fraction=0, gff=str(gff))


@pytest.mark.parametrize("kind", ["random", "name", "blocks"])
def test_unsorted(files, tmp_path, kind):
    b = files["records"]
    sh = take_bamdata(b, shuffles(len(b.tid), 9)[kind])
    p = str(tmp_path / "s.sam")
    samtext.write(p, sh, seed=10)
    back = bamio.read_sam(p)
    g = take_bamdata(back, grouped_order(back.tid, len(back.ref_lens)))
    check_all_routes("contig", p, g, extra=["--unsorted"], methods=["mean", "covered_fraction", "variance", "count", "anir"], min_covered_fraction=0)


def test_a_real_pipe_with_short_reads(files):
    """The text through an os.pipe written by a thread in 4 KiB pieces: read() returns short, the driver keeps the lines whole."""
    kw = dict(methods=["mean", "variance", "count"], min_covered_fraction=0)
    with open(files["path"], "rb") as f:
        text = f.read()
    rd, wr = os.pipe()

    def writer():
        with os.fdopen(wr, "wb", buffering=0) as w:
            for at in range(0, len(text), 4096):
                w.write(text[at:at + 4096])

    t = threading.Thread(target=writer)
    t.start()
    try:
        with os.fdopen(rd, "rb") as r:
            got = device_route(run("contig", "-", env={"COVERM_KNOBS": "sam_window_bytes=1000000"}, stdin=r, **kw))
    finally:
        t.join()
    assert got == O.run_cli("contig", ["stdin.sam"], bams=[files["records"]], **kw)
    with open(files["path"], "rb") as f:
        assert "from a pipe" not in run("contig", "-", stdin=f, **kw).stderr          # (a redirected file is a file: its size is known)


def _max_rss_of(argv, stdin):
    """Peak resident set (bytes) of one run of the binary: ru_maxrss of a child started from a fresh helper process, so that it is that
    child's own peak."""
    code = ("import resource, subprocess, sys\n"
            "r = subprocess.run(sys.argv[1:], stdin=sys.stdin, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)\n"
            "sys.stderr.write(r.stderr.decode()[-2000:])\n"
            "print(resource.getrusage(resource.RUSAGE_CHILDREN).ru_maxrss * 1024 if r.returncode == 0 else -1)\n")
    import sys
    r = subprocess.run([sys.executable, "-c", code] + argv, stdin=stdin, capture_output=True, text=True, timeout=1500)
    v = int(r.stdout.strip().splitlines()[-1])
    assert v > 0, r.stderr[-2000:]
    return v


def test_peak_host_memory_is_bounded_by_the_window(files, tmp_path):
    """About 1 GB of SAM text from standard input.  What the route holds on the host, by design: COV_INGEST_SLOTS = 4 page-locked slots of one
    32 MiB window each (128 MiB), the carry (one cut-off line, < 1 KiB here), the bytes read while the header was looked for (the header,
    ~4 KiB for 120 @SQ lines, plus at most one 64 KiB read), the results (128 B x 120 contigs) — under 129 MiB in all, whatever the
    input's length.  The bound is that, times two, on top of what the same binary needs for a run over a small input (the HIP runtime, the
    library, the device's record-store bookkeeping), measured here with the first 2 MB of the same text: peak(1 GB) <= peak(small) + 2 x 129
    MiB.  The whole-file host route holds the text (1 GB) plus its records and cannot read a pipe at all."""
    with open(files["path"], "rb") as f:
        text = f.read()
    first = 0
    while text[first:first + 1] == b"@":
        first = text.index(b"\n", first) + 1
    body = text[first:].split(b"\n")[:-1]
    rep = (1 << 30) // max(1, len(text) - first) + 1
    big = str(tmp_path / "big.sam")
    with open(big, "wb") as f:
        f.write(text[:first])
        for k in range(0, len(body), 1000):
            f.write(b"".join((l + b"\n") * rep for l in body[k:k + 1000]))          # every line `rep` times in place: still sorted by reference
    small = str(tmp_path / "small.sam")
    with open(small, "wb") as f:
        f.write(text[:text.rindex(b"\n", 0, 2_000_000) + 1])
    assert os.path.getsize(big) >= 1 << 30
    argv = binary.argv("contig", ["-"], methods=["mean"], min_covered_fraction=0)
    with open(small, "rb") as f:
        base = _max_rss_of(argv, f)
    with open(big, "rb") as f:
        peak = _max_rss_of(argv, f)
    bound = base + 2 * (129 << 20)
    print("peak host memory: small input %.1f MiB, 1 GiB input %.1f MiB, bound %.1f MiB" % (base / 2**20, peak / 2**20, bound / 2**20))
    assert peak <= bound, (base, peak, bound)

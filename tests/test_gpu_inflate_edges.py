"""The device ingest's DEFLATE stage (csrc/ingest_kernels.hip.h: k_inflate_wave / k_inflate, k_lz_stage / k_lz_resolve) at its decision
points, fed with streams that tests/deflate_craft.py writes token by token — what zlib and libdeflate never emit for BAM-like bytes.

Every input is a valid BAM file.  A case of the catalogue (tests/lz_cases.py) is the XB:B,C array of one record; the inflated stream is cut
into BGZF blocks exactly where the case's blocks begin, so a case's block is all pattern and its tokens sit where the planner placed them.
What lies between the cases — the header, a plain record, the carrier's fixed part — goes into blocks of literals; the carrier's name
length steers the address (mod 4) at which the pattern begins.  The inflated stream must be zlib's byte for byte, the records the CPU
reader's.  A wrong byte here is quiet in production (the CRC kernel flags the block and the CPU reader takes the file over): this suite is
where it shows."""
import ctypes as C
import os
import re
import struct
import time
import zlib

import numpy as np
import pytest

from coverm_amd import bam as cbam
from coverm_amd import native
from coverm_amd.engine import FilterConfig, Session
from tests import deflate_craft as dc
from tests import lz_cases as lc
from tests.bamraw import header, ingest_and_compare, rec

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_AUX = int(re.search(r"LONG_AUX_BYTES = (\d+)u", open(os.path.join(ROOT, "coverm_amd", "csrc", "bam_record_core.h")).read()).group(1))


@pytest.fixture(autouse=True, params=["default", "lane-per-block", "lz-rounds"])
def inflate_version(request, monkeypatch):
    """as in tests/test_gpu_ingest.py: the kernels that ship (k_inflate_wave + k_lz_stage), the second inflate implementation (k_inflate),
    the second match resolution (k_lz_resolve)"""
    monkeypatch.delenv("COVERM_INFLATE_V", raising=False)
    monkeypatch.delenv("COVERM_LZ_V", raising=False)
    if request.param == "lane-per-block":
        monkeypatch.setenv("COVERM_INFLATE_V", "1")
    elif request.param == "lz-rounds":
        monkeypatch.setenv("COVERM_LZ_V", "1")
    return request.param


# ------------------------------------------------------------------------------------------------ a BAM file around the cases
def glue_block(data, k):
    """bytes between two cases as one BGZF block of literals: fixed codes, dynamic codes and stored in turn"""
    t = list(data)
    if k % 3 == 0:
        return lc.assemble([("fixed", t)])[0]
    if k % 3 == 1:
        return lc.assemble([("dynamic", t) + tuple(lc.plain_lens())])[0]
    return lc.assemble([("stored", bytes(data))])[0]


def build_file(path, cases):
    """-> dict(blocks=[(stream offset, inflated length, payload, label)], long=records the device must take a wave at a time, n=records)"""
    refs = [(b"chr", 5_000_000)]
    stream, pending = bytearray(), bytearray(header(refs))
    blocks, n_rec, n_long = [], 0, 0

    def cut(label):
        nonlocal pending
        for s0 in range(0, len(pending), 40_000):
            piece = bytes(pending[s0:s0 + 40_000])
            blocks.append((len(stream), len(piece), glue_block(piece, len(blocks)), label))
            stream.extend(piece)
        pending = bytearray()

    for i, case in enumerate(cases):
        pending += rec(0, 100 + 200 * i, [90 << 4], 90, b"NMC\1", b"p%d" % i)[0]
        n_rec += 1
        if not case.blocks:
            continue
        pattern = b"".join(b.data for b in case.blocks)
        aux = b"NMC\2" + b"XBBC" + struct.pack("<I", len(pattern)) + pattern
        for pad in range(1, 5):
            r, _, n_aux = rec(0, 150 + 200 * i, [50 << 4], 50, aux, b"c%d" % i + b"x" * pad)
            fixed_part = r[:len(r) - len(pattern)]
            if (len(stream) + len(pending) + len(fixed_part)) % 4 == case.align:
                break
        else:
            raise AssertionError("no name length gives the alignment")
        n_rec += 1
        n_long += n_aux > T_AUX
        pending += fixed_part
        cut("in front of " + case.id)
        assert len(stream) % 4 == case.align
        for k, b in enumerate(case.blocks):
            blocks.append((len(stream), len(b.data), b.payload, "%s [block %d]" % (case.id, k)))
            stream.extend(b.data)
    if pending:
        cut("the file's last records")
    open(path, "wb").write(dc.bgzf_file([(p, bytes(stream[o:o + n])) for o, n, p, _ in blocks]))
    return dict(blocks=blocks, long=n_long, n=n_rec, stream=bytes(stream))


FILES = {}
for _a in range(4):
    FILES["stage, start address %d mod 4" % _a] = lambda a=_a: [c for c in lc.lz_cases(a) if c.family == "lz"]
    FILES["chains, start address %d mod 4" % _a] = lambda a=_a: [c for c in lc.lz_cases(a) if c.family == "chains"]
FILES["codes and code lengths"] = lambda: [c.at(k & 3) for k, c in enumerate(lc.code_cases())]
FILES["stored blocks and k_inflate's stores"] = lambda: [c.at(k & 3) for k, c in enumerate(lc.stored_cases() + lc.flush_cases())]
FILES["wave shares and pass 2"] = lambda: [c.at(k & 3) for k, c in enumerate(lc.share_cases())]
FILES["maximal ratio"] = lambda: [lc.ratio_case()]
for _n in (1, 63, 64, 65):
    FILES["%d blocks of mixed kinds" % _n] = lambda n=_n: [lc.mixed_cases(n - 1, 700 + n)]      # + the block in front of the case


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """every file is built once and serves the three kernel combinations"""
    cache, d = {}, tmp_path_factory.mktemp("edges")

    def get(name):
        if name not in cache:
            path = str(d / ("f%d.bam" % len(cache)))
            cache[name] = (path, build_file(path, FILES[name]()))
        return cache[name]
    return get


def device_stream(path, n):
    """the first n bytes of the inflated stream as the device made it, with the CRC check off: a wrong byte is to be found and named here,
    not turned into a fallback"""
    with Session(0, FilterConfig(), 75) as s:
        try:
            cbam.gpu_ingest(s, path, threads=2, check_crc=False)
        except cbam.IngestFallback as e:
            pytest.fail("the device handed the file back although its CRC check is off: %s" % e)
        L = native.lib()
        L.cov_ingest_copy_inflated.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
        out = np.zeros(n, np.uint8)
        assert L.cov_ingest_copy_inflated(s._h, 0, n, out.ctypes.data) == 0
        return out


@pytest.mark.parametrize("name", list(FILES))
def test_crafted_streams(built, name):
    """One file of cases: the device's inflated stream equals zlib's (a differing byte is reported with the id of the case it lies in, which
    names the branch), the ingest with the CRC check on hands nothing back, columns, statistics and histogram equal the CPU reader's, and the
    long records are counted.  (The pass-2 case's round count is asserted on the CPU emulation, tests/test_inflate_wave_core.py.)"""
    t0 = time.time()
    path, meta = built(name)
    want = b"".join(zlib.decompress(p, -15) for _, _, p, _ in meta["blocks"])
    assert want == meta["stream"]
    if "mixed" in name:
        assert len(meta["blocks"]) == int(name.split()[0])
    # the bytes first: a wrong byte names its case, which a fallback or a differing record column would not
    got = device_stream(path, len(want))
    bad = np.flatnonzero(got != np.frombuffer(want, np.uint8))
    if len(bad):
        hit = [b for b in meta["blocks"] if b[1] and np.any((bad >= b[0]) & (bad < b[0] + b[1]))]
        o, n, _, label = hit[0]
        at = int(bad[0])
        pytest.fail("%s: byte %d of %d differs (0x%02x, zlib has 0x%02x); %d bytes differ in the file, in:\n  %s"
                    % (label, at - o, n, got[at], want[at], len(bad), "\n  ".join(sorted({b[3] for b in hit}))))
    # then the whole ingest with the CRC check on: gpu_ingest raises IngestFallback when the device gives a block up, which fails the test
    whole, stats = ingest_and_compare(path)
    # one window: the file is far below 61 440 blocks and 32 KiB of compressed bytes per block, so offset 0 of cov_ingest_copy_inflated is
    # the file's first byte and the whole stream is still there
    assert stats["windows"] == 1
    assert whole.records.n_records == meta["n"]
    assert stats["long_records"] == meta["long"]
    print("%s: %d blocks, %d inflated bytes, %.2f s" % (name, len(meta["blocks"]), len(want), time.time() - t0))

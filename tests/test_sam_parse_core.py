"""csrc/sam_parse_core.h (the arithmetic of the device's SAM text decode) run on the CPU: tests/c/sam_parse_host.cpp walks the kernels' stages
with their geometry — 16 bytes per lane folded into 64-bit newline / tab words, line ends by a scan over popcounts, a count pass and a
decode pass per line that find their tabs in the masks, window by window with the host driver's cut at the last '\\n' — and, separately,
line by line with the byte-walking tab finder.  Both must equal oracle.bamio.read_sam of the same text field for field (CIGAR words and
offsets and mtid included), for several window sizes.  Lines read_sam does not take (unknown RNAME, `NM:i:` without a value, ...) are
compared with the values parse_sam's rules give, stated here, and with the host's whole-file SAM reader over the same text.

With mates, the emulation also hashes every record's QNAME through the very function the kernels call (csrc/name_hash_core.h, shared with
the BGZF record extraction).  Those hashes must equal the function applied to the names where a BAM record holds them (any alignment)
and the hash written out a second time in tests/namehash.py over the oracle's QNAMEs."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

from coverm_amd import bam as hostbam
from oracle import bamio
from tests import namehash, samtext

HERE = os.path.dirname(os.path.abspath(__file__))
RAW_SAM = sorted(glob.glob(os.path.join(HERE, "golden", "raw_sam", "*.sam")))
RAW_BAM = sorted(glob.glob(os.path.join(HERE, "golden", "raw", "*.bam")))
ERR_MALFORMED, ERR_CIGAR_OPS, ERR_LINE_LONG, ERR_AT_LINE = 1, 2, 3, 4


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("samc") / "samc_host.so")
    subprocess.check_call(["g++", "-O2", "-fno-strict-aliasing", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "c", "sam_parse_host.cpp")])
    L = C.CDLL(so)
    L.samc_host_table_size.restype = C.c_uint32
    L.samc_host_table_size.argtypes = [C.c_uint32]
    L.samc_host_hash_many.argtypes = [C.c_char_p, C.c_void_p, C.c_uint32, C.c_void_p]
    L.samc_host_lookup.argtypes = [C.c_char_p, C.c_void_p, C.c_uint32, C.c_char_p, C.c_void_p, C.c_uint32, C.c_void_p]
    L.samc_host_decode.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_int] + [C.c_void_p] * 12 + [C.POINTER(C.c_uint64)] * 3
    L.samc_host_name_hash_many.argtypes = [C.c_char_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    return L


def blob_of(names):
    enc = [n.encode() if isinstance(n, str) else n for n in names]
    off = np.zeros(len(enc) + 1, np.uint64)
    np.cumsum([len(e) for e in enc], out=off[1:])
    return b"".join(enc), off


def header_names(text):
    """SN of every @SQ line in front of the first alignment line, in order."""
    names = []
    for line in text.split(b"\n"):
        line = line.rstrip(b"\r")
        if line.startswith(b"@SQ"):
            names.append([f[3:] for f in line.split(b"\t")[1:] if f.startswith(b"SN:")][-1])
        elif line and not line.startswith(b"@"):
            break
    return names


def decode(L, text, names=None, window=1 << 30, staged=1):
    names = header_names(text) if names is None else names
    blob, off = blob_of(names)
    cap = text.count(b"\n") + 2
    ccap = len(text) // 2 + 2
    a = dict(tid=np.zeros(cap, np.int32), pos=np.zeros(cap, np.int32), mtid=np.zeros(cap, np.int32), flag=np.zeros(cap, np.uint16), mapq=np.zeros(cap, np.uint8),
             nm_kind=np.zeros(cap, np.uint8), nm=np.zeros(cap, np.uint32), l_seq=np.zeros(cap, np.uint32), cigar_off=np.zeros(cap + 1, np.uint32), cigar=np.zeros(ccap, np.uint32))
    a.update(qh1=np.zeros(cap, np.uint64), qh2=np.zeros(cap, np.uint32))
    n, nc, line = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    rc = L.samc_host_decode(text + b"\0" * 8, len(text), blob, off.ctypes.data, len(names), window, staged, *[a[k].ctypes.data for k in a], C.byref(n), C.byref(nc), C.byref(line))
    if rc:
        return rc, int(line.value)
    n, nc = int(n.value), int(nc.value)
    out = {k: v[:n] for k, v in a.items()}
    out["cigar_off"] = a["cigar_off"][:n + 1]
    out["cigar"] = a["cigar"][:nc]
    return out


def assert_equals_oracle(got, want):
    assert isinstance(got, dict), got
    assert len(got["tid"]) == want.n_records
    for k in ("tid", "pos", "flag", "mapq", "nm", "nm_kind", "mtid"):
        np.testing.assert_array_equal(got[k], np.asarray(getattr(want, k)), err_msg=k)
    np.testing.assert_array_equal(got["l_seq"], np.asarray(want.l_seq).astype(np.uint32))
    np.testing.assert_array_equal(got["cigar_off"], want.cigar_off)
    np.testing.assert_array_equal(got["cigar"], want.cigar)
    k1, k2 = namehash.name_hashes(want.qname)                                              # the read-name hash, over the oracle's QNAMEs
    np.testing.assert_array_equal(got["qh1"], k1)
    np.testing.assert_array_equal(got["qh2"], k2)


def check_text(L, text, tmp_path, windows=(1 << 30, 4096, 700)):
    p = str(tmp_path / "t.sam")
    with open(p, "wb") as f:
        f.write(text)
    want = bamio.read_sam(p)
    longest = max(len(l) for l in text.split(b"\n")) + 2
    assert_equals_oracle(decode(L, text, staged=0), want)
    for w in windows:
        assert_equals_oracle(decode(L, text, window=max(w, longest), staged=1), want)
    return want


@pytest.mark.parametrize("path", RAW_SAM, ids=os.path.basename)
def test_sam_fixtures(host, tmp_path, path):
    assert len(RAW_SAM) == 2
    with open(path, "rb") as f:
        check_text(host, f.read(), tmp_path)


@pytest.mark.parametrize("path", RAW_BAM, ids=os.path.basename)
def test_rendered_bam_fixtures(host, tmp_path, path):
    b = bamio.read_bam(path)
    if b.n_records > 20_000:
        b = b.select(np.arange(20_000))
    want = check_text(host, samtext.render(b, seed=3), tmp_path)
    assert want.n_records == b.n_records
    np.testing.assert_array_equal(want.tid, b.tid)                  # (the rendering kept the records: the comparison above is not empty)
    np.testing.assert_array_equal(want.cigar, b.cigar)
    check_text(host, samtext.render(b, seed=4, eol="\r\n"), tmp_path, windows=(1 << 30, 900))


HDR = b"@HD\tVN:1.6\n@SQ\tSN:c1\tLN:1000\n@SQ\tSN:c2\tLN:2000\n@SQ\tSN:c1\tLN:77\n"      # (a duplicate SN: the first wins)


def rec(qn=b"q", flag=0, rname=b"c1", pos=5, mapq=30, cigar=b"10M", rnext=b"*", seq=b"ACGTACGTAC", tags=(b"NM:i:1",)):
    return b"\t".join([qn, b"%d" % flag, rname, b"%d" % pos, b"%d" % mapq, cigar, rnext, b"0", b"0", seq, b"*" if seq == b"*" else b"I" * len(seq)] + list(tags))


def test_generated_lines(host, tmp_path):
    """Every special case of the specification, with the value parse_sam's rule gives."""
    cases = [  # (line, tid, mtid, n_cigar, l_seq, nm, nm_kind)
        (rec(rname=b"*", cigar=b"*", seq=b"*"), -1, -1, 0, 0, 1, 1),
        (rec(rnext=b"="), 0, 0, 1, 10, 1, 1),
        (rec(rname=b"c2", rnext=b"c1"), 1, 0, 1, 10, 1, 1),
        (rec(rname=b"nope", rnext=b"="), -1, -1, 1, 10, 1, 1),                       # an unknown RNAME: -1, and `=` follows it
        (rec(rnext=b"nope"), 0, -1, 1, 10, 1, 1),
        (rec(tags=(b"NM:i:-1",)), 0, -1, 1, 10, 0, 2),
        (rec(tags=(b"NM:Z:x",)), 0, -1, 1, 10, 0, 2),
        (rec(tags=(b"NM:i:",)), 0, -1, 1, 10, 0, 0),                                 # 5 bytes: too short to be looked at
        (rec(tags=(b"NM:i:3", b"XS:i:2", b"NM:i:9")), 0, -1, 1, 10, 9, 1),           # the last NM wins
        (rec(tags=(b"NM:i:3", b"NM:Z:x")), 0, -1, 1, 10, 3, 2),                      # ... its kind; the earlier value stays, as parse_sam leaves it
        (rec(tags=()), 0, -1, 1, 10, 0, 0),
        (rec(cigar=b"3S4M2I1D5=6X7N8H9P1Q"), 0, -1, 10, 10, 1, 1),                   # an unknown letter: op 15
    ]
    body = b"\n".join(c[0] for c in cases)
    for text in (HDR + body + b"\n", HDR + body, HDR + b"\n\n" + body.replace(b"\n", b"\r\n\r\n") + b"\r\n", HDR.replace(b"\n", b"\r\n") + body.replace(b"\n", b"\n\n")):
        for staged, window in ((0, 1 << 30), (1, 1 << 30), (1, 300), (1, 130)):
            got = decode(host, text, window=window, staged=staged)
            assert isinstance(got, dict), (got, staged, window)
            assert len(got["tid"]) == len(cases)
            for i, (_, tid, mtid, ncig, lseq, nm, nmk) in enumerate(cases):
                have = (got["tid"][i], got["mtid"][i], got["cigar_off"][i + 1] - got["cigar_off"][i], got["l_seq"][i], got["nm"][i], got["nm_kind"][i])
                assert have == (tid, mtid, ncig, lseq, nm, nmk), (i, have)
            assert (got["flag"] == 0).all() and (got["pos"] == 4).all() and (got["mapq"] == 30).all()
            np.testing.assert_array_equal(got["cigar"][-10:], [3 << 4 | 4, 4 << 4, 2 << 4 | 1, 1 << 4 | 2, 5 << 4 | 7, 6 << 4 | 8, 7 << 4 | 3, 8 << 4 | 5, 9 << 4 | 6, 1 << 4 | 15])
    # the host's whole-file reader (the cross-check route) reads the same text the same way
    p = str(tmp_path / "g.sam")
    with open(p, "wb") as f:
        f.write(HDR + body + b"\n")
    h = hostbam.read_alignment_file(p, threads=1)
    got = decode(host, HDR + body + b"\n")
    for k in ("tid", "pos", "flag", "mapq", "nm", "nm_kind", "l_seq", "cigar_off", "cigar"):
        np.testing.assert_array_equal(got[k], getattr(h.records, k), err_msg=k)
    np.testing.assert_array_equal(got["mtid"], h.mtid)


def test_errors_name_the_first_offending_line(host):
    good = rec()
    nine = b"\t".join(good.split(b"\t")[:9])
    long_cigar = rec(cigar=b"1M1I" * 35_000, seq=b"*")                                   # 70 000 operations
    for staged, window in ((0, 1 << 30), (1, 1 << 30), (1, 200_000)):
        assert decode(host, HDR + good + b"\n" + good + b"\n" + nine + b"\n" + good + b"\n", window=window, staged=staged) == (ERR_MALFORMED, 7)
        assert decode(host, HDR + good + b"\n" + nine + b"\n" + nine + b"\n", window=window, staged=staged) == (ERR_MALFORMED, 6)          # the FIRST of two
        assert decode(host, HDR + good + b"\n" + long_cigar + b"\n" + nine + b"\n", window=window, staged=staged) == (ERR_CIGAR_OPS, 6)
        assert decode(host, HDR + good + b"\n@CO\tlate\n" + good + b"\n", window=window, staged=staged) == (ERR_AT_LINE, 6)
    ok = decode(host, HDR + rec(cigar=b"1M" * 65_535, seq=b"*") + b"\n")                  # 65 535 operations are taken
    assert isinstance(ok, dict) and len(ok["cigar"]) == 65_535
    assert decode(host, HDR + good + b"\n" + good + b"\n", window=40, staged=1)[0] == ERR_LINE_LONG      # no line end inside a whole window


def test_lookup_table_collisions_and_scale(host):
    """Names chosen (by search, here) to fall into the same slot of the table resolve by their bytes: 64 names in 8 colliding groups of 8 in
    a table of 256 slots (at most half full: table_size(64)), each group probing through its neighbours, plus absent names that hash into the same occupied runs."""
    cand = [b"ctg%05d" % i for i in range(20_000)]
    blob, off = blob_of(cand)
    h = np.zeros(len(cand), np.uint32)
    host.samc_host_hash_many(blob, off.ctypes.data, len(cand), h.ctypes.data)
    size = host.samc_host_table_size(64)
    assert size == 256
    slot = h & (size - 1)
    groups = [np.flatnonzero(slot == s)[:9] for s in range(8)]
    assert all(len(g) == 9 for g in groups)
    present = [cand[i] for g in groups for i in g[:8]]
    absent = [cand[g[8]] for g in groups]                                                  # same slots, not in the table
    n_collisions = sum(len(g[:8]) - 1 for g in groups)
    assert n_collisions == 56
    pb, po = blob_of(present)
    qb, qo = blob_of(present + absent + [b"", b"ctg"])
    out = np.zeros(len(present) + len(absent) + 2, np.int32)
    host.samc_host_lookup(pb, po.ctypes.data, len(present), qb, qo.ctypes.data, len(out), out.ctypes.data)
    np.testing.assert_array_equal(out[:64], np.arange(64))
    assert (out[64:] == -1).all()
    # 200 000 names: every one resolves, 1 000 absent ones do not; a duplicate resolves to its first occurrence
    names = [b"k141_%d_len_%d" % (i, 1000 + i % 977) for i in range(200_000)]
    names[150_000] = names[7]
    nb, no = blob_of(names)
    queries = names + [b"k141_%d_x" % i for i in range(1000)]
    qb, qo = blob_of(queries)
    out = np.zeros(len(queries), np.int32)
    host.samc_host_lookup(nb, no.ctypes.data, len(names), qb, qo.ctypes.data, len(queries), out.ctypes.data)
    want = np.arange(200_000)
    want[150_000] = 7
    np.testing.assert_array_equal(out[:200_000], want)
    assert (out[200_000:] == -1).all()


def test_host_reader_resolves_names_by_map(tmp_path):
    """parse_sam's lookup (a hash map now, a scan from the front before): the first of duplicate SN values wins, an unknown name is -1 —
    the arrays a scan gives, computed here."""
    rng = np.random.default_rng(5)
    names = ["r%d" % i for i in range(3000)]
    for i in range(100, 3000, 7):
        names[i] = names[int(rng.integers(0, i))]
    first = {}
    for i, n in enumerate(names):
        first.setdefault(n, i)
    lines = ["@SQ\tSN:%s\tLN:%d" % (n, 5000) for n in names]
    want_tid, want_mtid = [], []
    for k in range(5000):
        a, b = names[int(rng.integers(0, 3000))], names[int(rng.integers(0, 3000))]
        rn = a if k % 50 else "missing"
        mt = "=" if k % 3 == 0 else ("*" if k % 3 == 1 else b)
        lines.append("q%d\t0\t%s\t10\t9\t5M\t%s\t1\t0\tACGTA\tIIIII\tNM:i:0" % (k, rn, mt))
        t = first.get(rn, -1)
        want_tid.append(t)
        want_mtid.append(t if mt == "=" else (-1 if mt == "*" else first[b]))
    p = str(tmp_path / "dups.sam")
    with open(p, "w") as f:
        f.write("\n".join(lines) + "\n")
    h = hostbam.read_alignment_file(p, threads=1)
    np.testing.assert_array_equal(h.records.tid, want_tid)
    np.testing.assert_array_equal(h.mtid, want_mtid)


def test_name_hash_is_the_extraction_s(host):
    """covn::name_hash as the BAM record extraction calls it — on the name's bytes inside a record, at every alignment, other bytes around
    it — against tests/namehash.py: names of 0 .. 70 bytes (every length modulo 16, several blocks), each at the four alignments; names
    that differ in their last byte or only in their length (a trailing NUL) hash differently, and the bytes behind a name do not count."""
    rng = np.random.default_rng(11)
    names = [bytes(rng.integers(33, 127, n, dtype=np.uint8)) for n in range(0, 71) for _ in range(4)]
    names += [b"read/1", b"read/2", b"read", b"read\0", b"A00123:45:HXXXXXXX:1:1101:1000:2000", b"A00123:45:HXXXXXXX:1:1101:1000:2001"]
    want1, want2 = namehash.name_hashes(names)
    for shift in range(4):
        off = []
        blob = bytearray(b"\xff" * shift)
        for i, nme in enumerate(names):
            off.append(len(blob))
            blob += nme
            blob += b"\xee" * int(rng.integers(0, 4))                                    # the next name starts at another alignment
        # (offsets and ends given separately: names are not adjacent here)
        k1, k2 = np.zeros(len(names), np.uint64), np.zeros(len(names), np.uint32)
        for i, nme in enumerate(names):
            o = np.asarray([off[i], off[i] + len(nme)], np.uint64)
            host.samc_host_name_hash_many(bytes(blob) + b"\xdd" * 8, o.ctypes.data, 1, k1[i:].ctypes.data, k2[i:].ctypes.data)
        np.testing.assert_array_equal(k1, want1)
        np.testing.assert_array_equal(k2, want2)
    keys = set(zip(want1.tolist(), want2.tolist()))
    assert len(keys) == len(set(names))

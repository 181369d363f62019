"""csrc/bam_record_core.h (the device ingest's "can a record start here, and where does it end", its NM scan and its CG:B,I lookup) run on
the CPU: tests/c/bam_record_host.cpp calls every function with the byte-walking policy (what one lane does) and with the wave's string walk
lane by lane (1024-byte steps of 16 bytes per lane through lane_nul_mask, the function the kernels call).  Both must equal the restatement
written out below in Python.  The program form of the same file runs its own cases built with -fsanitize=address,undefined."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "c", "bam_record_host.cpp")
REF_LEN = np.array([2_000_000, 50_000], np.uint32)
CAP = 1 << 24
NONE = (1 << 64) - 1
SCALAR = {b"A": 1, b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4, b"f": 4}
ELEM = {b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4, b"f": 4}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("bamrec") / "bam_record_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-o", so, SRC])
    L = C.CDLL(so)
    L.bamrec_long_cigar_words.restype = C.c_uint32
    L.bamrec_long_aux_bytes.restype = C.c_uint32
    L.bamrec_is_long.argtypes = [C.c_uint32, C.c_uint64]
    L.bamrec_plausible.restype = C.c_uint64
    L.bamrec_plausible.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_int, C.c_uint64]
    L.bamrec_chain_starts.restype = None
    L.bamrec_chain_starts.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]
    L.bamrec_scan_nm.restype = C.c_uint32
    L.bamrec_scan_nm.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(C.c_uint32)]
    L.bamrec_cg_cigar.restype = C.c_uint64
    L.bamrec_cg_cigar.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(C.c_uint32)]
    return L


# ------------------------------------------------------------------------------------------------ building records
def tag_z(name, n, fill=b"x", ty=b"Z"):
    return name + ty + fill * n + b"\0"


def tag_s(name, ty, v):
    fmt = {b"A": "<B", b"c": "<b", b"C": "<B", b"s": "<h", b"S": "<H", b"i": "<i", b"I": "<I", b"f": "<f"}[ty]
    return name + ty + struct.pack(fmt, v)


def tag_b(name, st, cnt, fill=0):
    return name + b"B" + st + struct.pack("<I", cnt) + bytes([fill]) * (cnt * ELEM[st])


def record(tid, pos, cigar, l_seq, aux, name=b"q"):
    core = struct.pack("<iiBBHHHiiii", tid, pos, len(name) + 1, 30, 4680, len(cigar), 0, l_seq, -1, -1, 0)
    body = core + name + b"\0" + struct.pack("<%dI" % len(cigar), *cigar) + b"\x11" * ((l_seq + 1) // 2) + b"\xff" * l_seq + aux
    return struct.pack("<i", len(body)) + body


def with_aux(aux):
    return record(0, 100, [100 << 4], 100, aux)


def buf(data):
    """4-byte aligned, 64 readable bytes behind the end (the window buffers have as much)"""
    a = np.zeros((len(data) + 64 + 7) // 8, np.uint64).view(np.uint8)
    a[:len(data)] = np.frombuffer(data, np.uint8)
    return a


# ------------------------------------------------------------------------------------------------ the restatement
def py_aux_exact(d, p, end):
    """every tag up to the record's end; the walk must end exactly there"""
    while p < end:
        if p + 3 > end:
            return False
        ty = d[p + 2:p + 3]
        p += 3
        if ty in SCALAR:
            p += SCALAR[ty]
        elif ty in (b"Z", b"H"):
            z = d.find(b"\0", p, end)
            if z < 0:
                return False
            p = z + 1
        elif ty == b"B":
            if p + 5 > end or d[p:p + 1] not in ELEM:
                return False
            cnt = struct.unpack_from("<I", d, p + 1)[0]
            if (end - p - 5) // ELEM[d[p:p + 1]] < cnt:
                return False
            p += 5 + cnt * ELEM[d[p:p + 1]]
        else:
            return False
        if p > end:
            return False
    return True


def py_plausible(d, n, o, cap=CAP, ref_len=REF_LEN):
    if o + 36 > n:
        return 0
    bs, rid, pos, lname = struct.unpack_from("<IiiB", d, o)
    if bs < 32 or bs > cap or o + 4 + bs > n:
        return 0
    ncig, = struct.unpack_from("<H", d, o + 16)
    lseq, nrid = struct.unpack_from("<Ii", d, o + 20)
    if rid < -1 or rid >= len(ref_len) or nrid < -1 or nrid >= len(ref_len) or pos < -1 or lname == 0:
        return 0
    if rid >= 0 and pos > int(ref_len[rid]):
        return 0
    fixed = 32 + lname + 4 * ncig + (lseq + 1) // 2 + lseq
    if fixed > bs or d[o + 36 + lname - 1] != 0:
        return 0
    return o + 4 + bs if py_aux_exact(d, o + 4 + fixed, o + 4 + bs) else 0


def py_chain(d, n, o):
    q, chain = o, 0
    while chain < 8:
        e = py_plausible(d, n, q)
        if not e:
            break
        q = e
        chain += 1
        if q == n:
            break
    return chain == 8 or (chain > 0 and q == n)


def py_scan_nm(d, p, end):
    while p + 3 <= end:
        is_nm, ty = d[p:p + 2] == b"NM", d[p + 2:p + 3]
        p += 3
        if ty in SCALAR:
            if p + SCALAR[ty] > end:
                return 0, 0
            if is_nm:
                fmt = {b"C": "<B", b"S": "<H", b"I": "<I"}.get(ty)
                return (1, struct.unpack_from(fmt, d, p)[0]) if fmt else (2, 0)
            p += SCALAR[ty]
        elif ty in (b"Z", b"H"):
            if is_nm:
                return 2, 0
            z = d.find(b"\0", p, end)
            if z < 0:
                return 0, 0
            p = z + 1
        elif ty == b"B":
            if p + 5 > end:
                return 0, 0
            if is_nm:
                return 2, 0
            es = ELEM.get(d[p:p + 1], 4)
            cnt = struct.unpack_from("<I", d, p + 1)[0]
            if (end - p - 5) // es < cnt:
                return 0, 0
            p += 5 + cnt * es
        else:
            return 0, 0
    return 0, 0


def both(f):
    """a host function's results with the serial and with the wave walk: they must agree"""
    a, b = f(0), f(1)
    assert a == b
    return a


def plausible(L, rec, cap=CAP):
    b = buf(rec)
    end = both(lambda w: L.bamrec_plausible(b.ctypes.data, len(rec), len(REF_LEN), REF_LEN.ctypes.data, cap, w, 0))
    assert end in (0, len(rec))
    assert end == py_plausible(rec, len(rec), 0, cap)
    return end == len(rec)


def scan_nm(L, aux):
    b = buf(aux)

    def one(w):
        nm = C.c_uint32(0)
        return L.bamrec_scan_nm(b.ctypes.data, 0, len(aux), w, C.byref(nm)), nm.value
    got = both(one)
    assert got == py_scan_nm(aux, 0, len(aux))
    return got


# ------------------------------------------------------------------------------------------------ tests
def mixed_stream(n_bytes, seed=5):
    rng = np.random.default_rng(seed)
    out, starts = [], []
    size = 0
    while size < n_bytes:
        aux = tag_s(b"NM", b"C", int(rng.integers(8)))
        if rng.random() < 0.5:
            aux += tag_z(b"MD", int(rng.integers(3000)), b"7")
        if rng.random() < 0.5:
            aux += tag_b(b"ML", b"C", int(rng.integers(5000)), int(rng.integers(256)))
        if rng.random() < 0.5:
            aux += tag_s(b"AS", b"i", -5) + tag_s(b"XA", b"A", 107) + tag_s(b"XS", b"s", -7) + tag_s(b"XF", b"f", 1.0) + tag_s(b"Xc", b"c", -3) + tag_s(b"XU", b"S", 9)
        if rng.random() < 0.5:
            aux += tag_z(b"SA", int(rng.integers(200)), b",") + tag_b(b"XI", b"I", int(rng.integers(40))) + tag_b(b"XH", b"s", 3) + tag_z(b"XQ", 2, b"4", ty=b"H")
        if rng.random() < 0.2:
            aux += tag_b(b"Xf", b"f", 5) + tag_b(b"Xi", b"i", 2) + tag_b(b"Xs", b"S", 1) + tag_b(b"Xc", b"c", 0)
        l_seq = int(rng.integers(30, 300))
        r = record(int(rng.integers(2)), int(rng.integers(40_000)), [l_seq << 4], l_seq, aux, b"read%d" % int(rng.integers(1000)))
        starts.append(size)
        out.append(r)
        size += len(r)
    return b"".join(out), starts


def test_exactly_the_true_starts_head_chains(host):
    """every offset of a 200 kB stream of records with mixed tags"""
    data, starts = mixed_stream(200_000)
    b = buf(data)
    got = []
    for w in (0, 1):
        out = np.zeros(len(data), np.uint8)
        host.bamrec_chain_starts(b.ctypes.data, len(data), len(REF_LEN), REF_LEN.ctypes.data, CAP, w, out.ctypes.data)
        got.append(out)
    want = np.zeros(len(data), np.uint8)
    want[starts] = 1
    np.testing.assert_array_equal(got[0], want)
    np.testing.assert_array_equal(got[1], want)
    py = np.array([py_chain(data, len(data), o) for o in range(len(data))], np.uint8)
    np.testing.assert_array_equal(py, want)


@pytest.mark.parametrize("n", [0, 1, 4095, 4096, 4097, 65_535, 65_536, 200_000])
def test_strings_of_any_length(host, n):
    """(the rule this one replaces accepted 4096 bytes and refused 4097)"""
    assert plausible(host, with_aux(tag_s(b"NM", b"C", 1) + tag_z(b"MM", n)))
    assert plausible(host, with_aux(tag_z(b"MM", n, ty=b"H") + tag_s(b"NM", b"C", 1)))
    assert not plausible(host, with_aux(tag_s(b"NM", b"C", 1) + tag_z(b"MM", n)[:-1] + b"x"))     # no NUL in front of the end


def many_tags(n):
    aux = b""
    for i in range(n):
        name = b"X" + bytes([48 + i % 10])
        aux += tag_z(name, i) if i % 3 == 0 else tag_s(name, [b"c", b"C", b"s", b"S", b"i", b"I", b"f", b"A"][i % 8], i % 100)
    return aux


@pytest.mark.parametrize("n", [1, 31, 32, 33, 64])
def test_any_number_of_tags(host, n):
    assert plausible(host, with_aux(many_tags(n)))


def test_a_malformed_33rd_tag_refuses_the_record(host):
    """(the rule this one replaces stopped looking after 32 tags)"""
    assert plausible(host, with_aux(many_tags(32) + tag_s(b"YY", b"i", 7)))
    assert not plausible(host, with_aux(many_tags(32) + b"YYq\1\2\3\4"))
    assert not plausible(host, with_aux(many_tags(40) + b"YYq\1\2\3\4" + many_tags(3)))


def test_every_tag_type(host):
    for ty, v in [(b"A", 65), (b"c", -1), (b"C", 255), (b"s", -300), (b"S", 65_535), (b"i", -70_000), (b"I", 4_000_000_000), (b"f", 1.5)]:
        assert plausible(host, with_aux(tag_s(b"XT", ty, v)))
    assert plausible(host, with_aux(tag_z(b"XZ", 9) + tag_z(b"XH", 4, b"A", ty=b"H")))
    for st in ELEM:
        for cnt in (0, 1, 11, 300):
            assert plausible(host, with_aux(tag_b(b"XB", st, cnt, 3) + tag_s(b"NM", b"C", 0)))
    assert not plausible(host, with_aux(b"XBBd" + struct.pack("<I", 1) + b"\0" * 8))
    assert not plausible(host, with_aux(b"XBq\0"))


def test_areas_that_do_not_end_on_the_record_end(host):
    b = bytearray(tag_b(b"XB", b"I", 4))
    b[4] = 5
    assert not plausible(host, with_aux(bytes(b)))                              # a B count that runs past the record end
    assert not plausible(host, with_aux(b"XBBI\4\0\0"))                         # ... an array header cut by it
    assert not plausible(host, with_aux(tag_s(b"XI", b"i", 1)[:6]))             # a tag cut by the record end
    assert not plausible(host, with_aux(b"XI"))
    r = with_aux(tag_s(b"NM", b"C", 1) + tag_z(b"XZ", 50))
    assert plausible(host, r)
    bs, = struct.unpack_from("<I", r, 0)
    assert not plausible(host, struct.pack("<I", bs - 1) + r[4:-1])             # the area ends one byte early: the NUL is gone
    assert not plausible(host, struct.pack("<I", bs + 1) + r[4:] + b"\0")       # ... one byte late: a lone byte is no tag


def test_block_size_above_the_walk_bound(host):
    r = with_aux(tag_z(b"MM", 5000))
    assert plausible(host, r, cap=len(r) - 4)
    assert not plausible(host, r, cap=len(r) - 5)
    # a stray offset whose first four bytes read as 900 MB is refused whatever follows (and nothing behind it is walked)
    stray = struct.pack("<I", 900 << 20) + r[4:]
    b = buf(stray)
    for w in (0, 1):
        assert host.bamrec_plausible(b.ctypes.data, 1 << 40, len(REF_LEN), REF_LEN.ctypes.data, CAP, w, 0) == 0


def test_nm_wherever_it_stands(host):
    filler = b"".join(tag_z(b"XZ", i * 37) if i % 4 == 0 else tag_b(b"XB", b"S", i) if i % 4 == 1 else tag_s(b"XS", b"i", i) for i in range(35))
    assert scan_nm(host, tag_s(b"NM", b"C", 200) + filler) == (1, 200)                      # first
    assert scan_nm(host, filler + tag_s(b"NM", b"S", 60_000)) == (1, 60_000)                # 36th and last
    assert scan_nm(host, filler + tag_s(b"NM", b"I", 3_000_000_000) + filler) == (1, 3_000_000_000)      # 36th of 71
    assert scan_nm(host, filler + tag_s(b"NM", b"i", 5)) == (2, 0)                          # a wrong type
    assert scan_nm(host, filler + tag_s(b"NM", b"c", 5)) == (2, 0)
    assert scan_nm(host, filler + tag_z(b"NM", 3)) == (2, 0)
    assert scan_nm(host, filler + tag_b(b"NM", b"C", 3)) == (2, 0)
    assert scan_nm(host, filler) == (0, 0)                                                  # absent
    assert scan_nm(host, b"") == (0, 0)
    assert scan_nm(host, b"XXq\1" + tag_s(b"NM", b"C", 1)) == (0, 0)
    assert scan_nm(host, tag_z(b"MM", 70_000) + tag_s(b"NM", b"C", 9)) == (1, 9)


def test_cg_behind_a_long_string(host):
    n_ops, l_seq = 70_001, 500
    ph = [(l_seq << 4) | 4, (900 << 4) | 3]
    aux = tag_s(b"NM", b"C", 5) + tag_z(b"MM", 8000) + tag_b(b"CG", b"I", n_ops, 0x20)
    r = record(0, 100, ph, l_seq, aux)

    def cg(rec, w):
        b = buf(rec)
        cnt = C.c_uint32(0)
        return host.bamrec_cg_cigar(b.ctypes.data, 0, len(rec), w, C.byref(cnt)), cnt.value
    assert both(lambda w: cg(r, w)) == (len(r) - 4 * n_ops, n_ops)
    assert both(lambda w: cg(record(0, 100, ph, l_seq, tag_z(b"MM", 8000)), w))[0] == NONE                  # no CG
    assert both(lambda w: cg(record(-1, 100, ph, l_seq, aux), w))[0] == NONE                               # unmapped
    assert both(lambda w: cg(record(0, 100, [(l_seq - 1 << 4) | 4, ph[1]], l_seq, aux), w))[0] == NONE      # not `<l_seq>S`
    assert both(lambda w: cg(record(0, 100, ph + [16], l_seq, aux), w))[0] == NONE                         # three operations


def test_what_a_long_record_is(host):
    t, a = host.bamrec_long_cigar_words(), host.bamrec_long_aux_bytes()
    assert (host.bamrec_is_long(t, a), host.bamrec_is_long(t + 1, 0), host.bamrec_is_long(0, a + 1)) == (0, 1, 1)


def test_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "bam_record_host_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    assert r.stdout.strip().endswith("cases, 0 bad")

"""A DEFLATE encoder that does what it is told (RFC 1951): a bit writer and three block writers over an explicit token list, so that a
test decides which branch of a decoder or of the match resolution runs — not an encoder's habits.  A token is an int (a literal) or a
pair (length, distance).  Plain Python; zlib is the judge of every stream made here (tests/test_deflate_craft.py)."""
import struct
import zlib

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CLEN_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 30


class BW:
    """bits leave LSB first (RFC 1951 3.1.1); Huffman codes are packed starting with their most significant bit"""
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def bits(self, v, n):
        assert 0 <= v < (1 << n) or n == 0
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xff)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, n):
        self.bits(int(format(c & ((1 << n) - 1), "0%db" % n)[::-1], 2), n)      # (masked: an over-subscribed set, made on purpose, runs out of codes)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def nbits(self):
        return 8 * len(self.out) + self.n

    def bytes(self):
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")


def canonical(lens):
    """symbol -> (code, length) of the canonical code with these lengths (RFC 1951 3.2.2); nothing is checked: a caller may want a bad set"""
    codes, code = {}, 0
    for l in range(1, max(list(lens) + [1]) + 1):
        for s, x in enumerate(lens):
            if x == l:
                codes[s] = (code, l)
                code += 1
        code <<= 1
    return codes


def kraft(lens):
    """sum of 2^-l in units of 2^-15: 32768 is a complete set"""
    return sum(1 << (15 - l) for l in lens if l)


def len_sym(length):
    if length == 258:
        return 28, 0
    s = max(i for i in range(28) if LEN_BASE[i] <= length)
    return s, length - LEN_BASE[s]


def dist_sym(dist):
    s = max(i for i in range(30) if DIST_BASE[i] <= dist)
    return s, dist - DIST_BASE[s]


def expand(tokens) -> bytes:
    out = bytearray()
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            length, dist = t
            assert 3 <= length <= 258 and 1 <= dist <= min(len(out), 32768), (t, len(out))
            for _ in range(length):
                out.append(out[-dist])
    return bytes(out)


def stored(w, data, final, nlen=None):
    assert len(data) <= 0xffff
    w.bits(1 if final else 0, 1)
    w.bits(0, 2)
    w.align()
    w.bits(len(data), 16)
    w.bits((len(data) ^ 0xffff) if nlen is None else nlen, 16)
    w.out += bytes(data)


def _symbols(w, tokens, lit, dist):
    for t in tokens:
        if isinstance(t, int):
            w.code(*lit[t])
        else:
            s, x = len_sym(t[0])
            w.code(*lit[257 + s])
            w.bits(x, LEN_EXTRA[s])
            s, x = dist_sym(t[1])
            w.code(*dist[s])
            w.bits(x, DIST_EXTRA[s])
    w.code(*lit[256])


def fixed(w, tokens, final):
    w.bits(1 if final else 0, 1)
    w.bits(1, 2)
    _symbols(w, tokens, canonical(FIXED_LIT), canonical(FIXED_DIST))


def expand_clseq(clseq):
    lens = []
    for sym, extra in clseq:
        if sym < 16:
            lens.append(sym)
        elif sym == 16:
            lens += [lens[-1]] * (3 + extra)
        elif sym == 17:
            lens += [0] * (3 + extra)
        else:
            lens += [0] * (11 + extra)
    return lens


def complete_clen_lens(used):
    """a COMPLETE code of at most 7 bits over the code-length symbols in `used` (zlib refuses an incomplete code-length code)"""
    used = sorted(set(used))
    if len(used) == 1:
        used = sorted(set(used + [0 if used[0] else 1]))
    k = len(used).bit_length() - 1
    m = len(used) - (1 << k)
    cl = [0] * 19
    for i, s in enumerate(used):
        cl[s] = k + 1 if i < 2 * m else k
    return cl


def dynamic_header(w, lit_lens, dist_lens, final, clseq=None, clen_lens=None, hlit=None, hdist=None, btype=2):
    """hlit / hdist / clen_lens / btype override what follows from the arguments: for streams that are wrong on purpose"""
    if clseq is None:
        clseq = [(l, 0) for l in list(lit_lens) + list(dist_lens)]
    if clen_lens is None:
        clen_lens = complete_clen_lens([s for s, _ in clseq])
    cc = canonical(clen_lens)
    hclen = max(4, max(i + 1 for i in range(19) if clen_lens[CLEN_ORDER[i]]))
    w.bits(1 if final else 0, 1)
    w.bits(btype, 2)
    w.bits((len(lit_lens) if hlit is None else hlit) - 257, 5)
    w.bits((len(dist_lens) if hdist is None else hdist) - 1, 5)
    w.bits(hclen - 4, 4)
    for i in range(hclen):
        w.bits(clen_lens[CLEN_ORDER[i]], 3)
    for sym, extra in clseq:
        w.code(*cc[sym])
        if sym >= 16:
            w.bits(extra, {16: 2, 17: 3, 18: 7}[sym])


def dynamic(w, tokens, lit_lens, dist_lens, final, clseq=None):
    assert 257 <= len(lit_lens) <= 286 and 1 <= len(dist_lens) <= 30
    if clseq is not None:
        assert expand_clseq(clseq) == list(lit_lens) + list(dist_lens)
    dynamic_header(w, lit_lens, dist_lens, final, clseq)
    _symbols(w, tokens, canonical(lit_lens), canonical(dist_lens))


def split_to(start, n, required=()):
    """A complete set of n code lengths: from the complete multiset `start` ({length: count}), the shortest code that may go (one that
    is not the last of a required length) is split into two codes one bit longer, until there are n.  -> sorted list of lengths"""
    cnt = dict(start)
    assert kraft([l for l, c in cnt.items() for _ in range(c)]) == 32768
    while sum(cnt.values()) < n:
        l = min(x for x, c in cnt.items() if x < 15 and (c >= 2 or (c == 1 and x not in required)))
        cnt[l] -= 1
        cnt[l + 1] = cnt.get(l + 1, 0) + 2
    return sorted(l for l, c in cnt.items() for _ in range(c))


def spread(sorted_lens, n_sym, used):
    """The multiset of lengths laid over n_sym symbols so that the symbols in `used` carry EVERY distinct length of it: one used symbol per
    distinct length first, then the rest in order; symbols beyond the multiset get 0."""
    used = [s for s in used if s < n_sym]
    rest = [s for s in range(n_sym) if s not in set(used)]
    pool = list(sorted_lens)
    assert len(pool) <= n_sym and len(set(pool)) <= len(used)
    lens, order = [0] * n_sym, used + rest
    first = []
    for l in sorted(set(pool)):
        pool.remove(l)
        first.append(l)
    for s, l in zip(order, first + pool):
        lens[s] = l
    return lens


def symbols_of(tokens):
    """(literal/length symbols, distance symbols) that a token list uses, end-of-block included"""
    lit, dist = {256}, set()
    for t in tokens:
        if isinstance(t, int):
            lit.add(t)
        else:
            lit.add(257 + len_sym(t[0])[0])
            dist.add(dist_sym(t[1])[0])
    return sorted(lit), sorted(dist)


def rle(lens):
    """the code-length sequence the way an encoder would write it: runs of zeros as 18 / 17, other runs as the length and 16s"""
    seq, i = [], 0
    while i < len(lens):
        j = i
        while j < len(lens) and lens[j] == lens[i]:
            j += 1
        run = j - i
        if lens[i] == 0:
            while run >= 11:
                n = min(run, 138)
                seq.append((18, n - 11))
                run -= n
            if run >= 3:
                seq.append((17, run - 3))
                run = 0
        else:
            seq.append((lens[i], 0))
            run -= 1
            while run >= 3:
                n = min(run, 6)
                seq.append((16, n - 3))
                run -= n
        seq += [(lens[i], 0)] * run
        i = j
    return seq


BGZF_EOF = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])


def bgzf_file(blocks, eof=True):
    """blocks: (payload, inflated bytes) each -> the file: header with BSIZE, payload, CRC-32 and ISIZE per block (SAM spec 4.1)"""
    out = []
    for payload, data in blocks:
        assert len(payload) + 26 <= 65536 and len(data) <= 65536
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(payload) + 25) + payload + struct.pack("<II", zlib.crc32(data), len(data)))
    if eof:
        out.append(BGZF_EOF)
    return b"".join(out)

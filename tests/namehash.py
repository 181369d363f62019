"""The 96-bit read-name hash the device pair filter joins mates by (csrc/name_hash_core.h), written out a second time from its definition:
MurmurHash3_x86_128's block mixing over the 16-byte blocks of the zero-padded name with the seeds below, its finalisation, then
k1 = h1 | h2 << 32 and k2 = h3 ^ rotl(h4, 16).  Plain Python integers — the expected values of the tests, never read from the code under
test."""
import struct

M = 0xffffffff
SEEDS = (0x9747b28c, 0x2f0b4a27, 0x7ed558cc, 0x1b873593)
C1, C2, C3, C4 = 0x239b961b, 0xab0e9789, 0x38b34ae5, 0xa1e38b93


def _rotl(x, r):
    return ((x << r) | (x >> (32 - r))) & M


def _fmix(h):
    h ^= h >> 16
    h = h * 0x85ebca6b & M
    h ^= h >> 13
    h = h * 0xc2b2ae35 & M
    return h ^ (h >> 16)


def name_hash(name: bytes):
    """(k1, k2) of one read name."""
    h1, h2, h3, h4 = SEEDS
    n = len(name)
    padded = name + b"\0" * (-n % 16)
    for o in range(0, n, 16):
        w1, w2, w3, w4 = struct.unpack_from("<4I", padded, o)
        w1 = _rotl(w1 * C1 & M, 15) * C2 & M
        h1 = ((_rotl(h1 ^ w1, 19) + h2) * 5 + 0x561ccd1b) & M
        w2 = _rotl(w2 * C2 & M, 16) * C3 & M
        h2 = ((_rotl(h2 ^ w2, 17) + h3) * 5 + 0x0bcaa747) & M
        w3 = _rotl(w3 * C3 & M, 17) * C4 & M
        h3 = ((_rotl(h3 ^ w3, 15) + h4) * 5 + 0x96cd1c35) & M
        w4 = _rotl(w4 * C4 & M, 18) * C1 & M
        h4 = ((_rotl(h4 ^ w4, 13) + h1) * 5 + 0x32ac3b17) & M
    h1, h2, h3, h4 = h1 ^ n, h2 ^ n, h3 ^ n, h4 ^ n
    h1 = (h1 + h2 + h3 + h4) & M
    h2, h3, h4 = (h2 + h1) & M, (h3 + h1) & M, (h4 + h1) & M
    h1, h2, h3, h4 = _fmix(h1), _fmix(h2), _fmix(h3), _fmix(h4)
    h1 = (h1 + h2 + h3 + h4) & M
    h2, h3, h4 = (h2 + h1) & M, (h3 + h1) & M, (h4 + h1) & M
    return h1 | (h2 << 32), h3 ^ _rotl(h4, 16)


def name_hashes(names):
    """(k1 array uint64, k2 array uint32) of a list of names (str or bytes)."""
    import numpy as np
    hs = [name_hash(n.encode() if isinstance(n, str) else n) for n in names]
    return np.asarray([h[0] for h in hs], np.uint64), np.asarray([h[1] for h in hs], np.uint32)

// The 96-bit read-name hash the device pair filter joins mates by — written once, called by the BGZF record extraction
// (ingest_kernels.hip.h), by the SAM text decode (sam_kernels.hip.h) and, on the CPU, by tests/c/sam_parse_host.cpp, so that the filter
// cannot tell which format a record came from.  Plain C++: __host__ __device__ under hipcc, no runtime calls.
//
// name_word reads whole aligned dwords: up to 3 bytes in front of p + o (inside p's own dword) and up to 7 behind it may be touched, never
// used.  The callers' buffers allow that (a record or a line goes on behind its name; device allocations are dword multiples).
#pragma once
#include <stdint.h>

#ifndef COVN_FN
#ifdef __HIPCC__
#define COVN_FN __host__ __device__ __forceinline__
#else
#define COVN_FN inline
#endif
#endif

namespace covn {

typedef unsigned int u32;
typedef unsigned long long u64;

// 96-bit hash of a read name (n bytes at p, n >= 0; bytes behind the name are not looked at): MurmurHash3_x86_128's block mixing
// over 16-byte blocks of the zero-padded name, its finalisation, words 1-3 kept.
COVN_FN u32 rotl32(u32 x, int r) { return (x << r) | (x >> (32 - r)); }
COVN_FN u32 fmix32(u32 h) { h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16; return h; }
COVN_FN u32 name_word(const uint8_t *p, u32 o, u32 n) {
    if (o >= n) return 0u;
    const u64 a = (u64)(p + o);
    const u32 *w = (const u32 *)(a & ~3ull);
    const u32 sh = (u32)(a & 3u) * 8u;
    u32 v = sh ? (w[0] >> sh) | (w[1] << (32u - sh)) : w[0];
    if (n - o < 4u) v &= (1u << (8u * (n - o))) - 1u;
    return v;
}
COVN_FN void name_hash(const uint8_t *p, u32 n, u64 &k1, u32 &k2) {
    u32 h1 = 0x9747b28cu, h2 = 0x2f0b4a27u, h3 = 0x7ed558ccu, h4 = 0x1b873593u;
    const u32 c1 = 0x239b961bu, c2 = 0xab0e9789u, c3 = 0x38b34ae5u, c4 = 0xa1e38b93u;
    for (u32 o = 0; o < n; o += 16u) {
        u32 w1 = name_word(p, o, n), w2 = name_word(p, o + 4u, n), w3 = name_word(p, o + 8u, n), w4 = name_word(p, o + 12u, n);
        w1 *= c1; w1 = rotl32(w1, 15); w1 *= c2; h1 ^= w1; h1 = rotl32(h1, 19); h1 += h2; h1 = h1 * 5u + 0x561ccd1bu;
        w2 *= c2; w2 = rotl32(w2, 16); w2 *= c3; h2 ^= w2; h2 = rotl32(h2, 17); h2 += h3; h2 = h2 * 5u + 0x0bcaa747u;
        w3 *= c3; w3 = rotl32(w3, 17); w3 *= c4; h3 ^= w3; h3 = rotl32(h3, 15); h3 += h4; h3 = h3 * 5u + 0x96cd1c35u;
        w4 *= c4; w4 = rotl32(w4, 18); w4 *= c1; h4 ^= w4; h4 = rotl32(h4, 13); h4 += h1; h4 = h4 * 5u + 0x32ac3b17u;
    }
    h1 ^= n; h2 ^= n; h3 ^= n; h4 ^= n;
    h1 += h2 + h3 + h4; h2 += h1; h3 += h1; h4 += h1;
    h1 = fmix32(h1); h2 = fmix32(h2); h3 = fmix32(h3); h4 = fmix32(h4);
    h1 += h2 + h3 + h4; h2 += h1; h3 += h1; h4 += h1;
    k1 = (u64)h1 | ((u64)h2 << 32);
    k2 = h3 ^ rotl32(h4, 16);
}

}  // namespace covn

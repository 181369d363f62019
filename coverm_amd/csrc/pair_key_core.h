// The device pair filter's join key and where it lands — written once, called by k_pair_insert and k_pair_collect (pair_kernels.hip.h),
// by the driver that sizes the table (cov_pair_filter_apply, covermhip.hip) and, on the CPU, by tests/c/pair_key_host.cpp, which
// tests/test_pair_key_core.py compares with a second statement of the same three rules in tests/pair_cases.py: the test cases place keys
// in chosen slots of the table with that statement.  Plain C++: __host__ __device__ under hipcc, no memory, no runtime calls.
//
//   key     (k1, k2t): k1 = name hash words 0-1, with 0 taken for 1 (an all-zero entry is an empty one: the hashes 0 and 1 are one name);
//           k2t = name hash word 2 | (tid + 2) << 32, never 0 (tid >= -1).  Two records are one name of one reference iff both words agree.
//   slot    where the probe run of a key starts in a table of mask + 1 entries (a power of two)
//   size    entries of the table of a chunk of n records: the smallest power of two that is >= 1 024 and >= 2 n
#pragma once
#include <stdint.h>

#ifndef PKEY_FN
#ifdef __HIPCC__
#define PKEY_FN __host__ __device__ __forceinline__
#else
#define PKEY_FN inline
#endif
#endif

namespace pkey {

typedef unsigned int u32;
typedef unsigned long long u64;

PKEY_FN u64 key_k1(u64 qh1) { return qh1 ? qh1 : 1ull; }
PKEY_FN u64 key_k2t(u32 qh2, int32_t tid) { return (u64)qh2 | ((u64)((u32)tid + 2u) << 32); }

PKEY_FN u32 table_slot(u64 k1, u64 k2t, u32 mask) {
    u64 x = k1 ^ (k2t * 0x9e3779b97f4a7c15ull);
    x ^= x >> 29;
    return (u32)x & mask;
}

PKEY_FN u64 table_size(u64 n_records) {
    u64 cc = 1024;
    while (cc < 2ull * n_records) cc <<= 1;
    return cc;
}

}  // namespace pkey

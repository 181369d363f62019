// Host instantiation of csrc/group_rank_core.h: k_group_hist, the digit-major scan and k_group_scatter of csrc/group_kernels.hip.h with the
// workgroups, waves and lanes as loops, a ballot as a loop over the 64 lanes, LDS as arrays.  Test infrastructure
// (tests/test_group_rank_core.py builds it with g++ and compares with numpy's stable argsort); not part of the product.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../coverm_amd/csrc/group_rank_core.h"

using namespace grpk;

// one pass: key_in / idx_in (idx_in == nullptr: item i has index i) -> key_out / idx_out; reverse: the waves of a round and the lanes of a
// wave are visited from the top (no result may depend on it)
static void one_pass(const u32 *key_in, const u32 *idx_in, u32 *key_out, u32 *idx_out, u64 n, u32 pass, int reverse) {
    const u32 n_wg = n_tiles(n);
    std::vector<u32> base((size_t)n_wg * RADIX, 0u);
    for (u32 wg = 0; wg < n_wg; wg++)      // k_group_hist
        for (u64 i = (u64)wg * TILE; i < (u64)(wg + 1) * TILE && i < n; i++) base[hist_index(digit_of(key_in[i], pass), wg, n_wg)]++;
    u32 acc = 0;                           // exclusive scan over [digit][workgroup]
    for (size_t k = 0; k < base.size(); k++) { const u32 c = base[k]; base[k] = acc; acc += c; }
    for (u32 wg = 0; wg < n_wg; wg++) {    // k_group_scatter
        u32 running[RADIX];
        for (u32 t = 0; t < RADIX; t++) running[t] = base[hist_index(t, wg, n_wg)];
        for (u32 r = 0; r < ITEMS; r++) {
            u32 wcnt[WAVES][RADIX];
            memset(wcnt, 0, sizeof wcnt);
            u32 rank[WG], dig[WG];
            bool valid[WG];
            for (u32 wk = 0; wk < WAVES; wk++) {
                const u32 w = reverse ? WAVES - 1u - wk : wk;
                for (u32 l = 0; l < WAVE; l++) {
                    const u64 i = (u64)wg * TILE + r * WG + w * WAVE + l;
                    valid[w * WAVE + l] = i < n;
                    dig[w * WAVE + l] = i < n ? digit_of(key_in[i], pass) : 0u;
                }
                u64 ballot_valid = 0, ballot_bit[RADIX_BITS] = {};
                for (u32 l = 0; l < WAVE; l++) {
                    if (!valid[w * WAVE + l]) continue;
                    ballot_valid |= 1ull << l;
                    for (u32 b = 0; b < RADIX_BITS; b++) if ((dig[w * WAVE + l] >> b) & 1u) ballot_bit[b] |= 1ull << l;
                }
                for (u32 lk = 0; lk < WAVE; lk++) {
                    const u32 l = reverse ? WAVE - 1u - lk : lk, t = w * WAVE + l;
                    u64 peers = ballot_valid;
                    for (u32 b = 0; b < RADIX_BITS; b++) peers = peers_step(peers, dig[t], b, ballot_bit[b]);
                    rank[t] = rank_among(peers, l);
                    if (valid[t] && is_leader(peers, l)) wcnt[w][dig[t]] = popc(peers);
                }
            }
            for (u32 t = 0; t < RADIX; t++) {      // the digit's thread
                u32 cnt[WAVES], out[WAVES];
                for (u32 w = 0; w < WAVES; w++) cnt[w] = wcnt[w][t];
                running[t] = wave_bases(running[t], cnt, out);
                for (u32 w = 0; w < WAVES; w++) wcnt[w][t] = out[w];
            }
            for (u32 t = 0; t < WG; t++) {
                if (!valid[t]) continue;
                const u64 i = (u64)wg * TILE + r * WG + t;
                const u32 p = wcnt[t / WAVE][dig[t]] + rank[t];
                idx_out[p] = idx_in ? idx_in[i] : (u32)i;
                key_out[p] = key_in[i];
            }
        }
    }
}

extern "C" {
uint32_t grpk_host_passes(uint32_t n_targets) { return n_passes(n_targets); }
uint32_t grpk_host_key(int32_t tid, uint32_t n_targets) { return key_of(tid, n_targets); }

// order[new] = old over n records; returns the number of passes run
uint32_t grpk_host_order(const int32_t *tid, uint64_t n, uint32_t n_targets, uint32_t *order, int reverse) {
    const u32 P = n_passes(n_targets);
    std::vector<u32> key[2], idx[2];
    key[0].resize(n); key[1].resize(n); idx[0].resize(n); idx[1].resize(n);
    for (u64 i = 0; i < n; i++) key[1][i] = key_of(tid[i], n_targets);
    for (u32 p = 0; p < P; p++)
        one_pass(key[(p + 1u) & 1u].data(), p ? idx[(p + 1u) & 1u].data() : nullptr, key[p & 1u].data(), idx[p & 1u].data(), n, p, reverse);
    if (n) memcpy(order, idx[(P - 1u) & 1u].data(), n * sizeof(u32));
    return P;
}
}

// Host instantiation of csrc/bgzf_walk_core.h beside the code the device ingest driver (covh_bam_gpu_ingest_span, csrc/host_bam.cpp)
// carried before the header existed, frozen here as it stood: the coordinator's serial header chain, the per-chunk hop with its own header
// test, and find_block_start's header test.  A file is handed over the way the driver does it — piece by piece, each piece in a buffer of
// exactly its size that is freed right behind the call, each chunk of it hopped first.  Test infrastructure
// (tests/test_bgzf_walk_core.py builds it with g++, as a library for the comparisons and as a program — main below walks files of stored
// blocks it makes itself — for a run under the sanitizers); not part of the product.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../coverm_amd/csrc/bgzf_walk_core.h"

namespace frozen {
static uint16_t rd16(const uint8_t *p) { uint16_t v; memcpy(&v, p, 2); return v; }

// find_block_start: is this a header to stop at (before its look at the following header)
static bool find_test(const uint8_t *c) {
    size_t q = 0;
    if (c[q] != 0x1f || c[q + 1] != 0x8b || c[q + 2] != 8 || c[q + 3] != 4) return false;
    if (rd16(&c[q + 10]) != 6 || c[q + 12] != 66 || c[q + 13] != 67 || rd16(&c[q + 14]) != 2) return false;
    const size_t bsize = (size_t)rd16(&c[q + 16]) + 1;
    if (bsize < 26) return false;
    return true;
}

struct PreBlock { uint64_t hdr; uint32_t bsize, crc, isize; };
struct PreChunk { uint64_t first = ~0ull, next = 0; std::vector<PreBlock> blocks; };
static void prewalk(const uint8_t *p, size_t n, uint64_t abs, PreChunk &out) {
    out.first = ~0ull; out.next = 0; out.blocks.clear();
    auto is_hdr = [&](size_t q) {
        return q + 18 <= n && p[q] == 0x1f && p[q + 1] == 0x8b && p[q + 2] == 8 && p[q + 3] == 4 && p[q + 10] == 6 && p[q + 11] == 0 && p[q + 12] == 66 &&
               p[q + 13] == 67 && p[q + 14] == 2 && p[q + 15] == 0;
    };
    size_t q = 0;
    for (;;) {     // first header signature in the chunk
        const void *f = q < n ? memchr(p + q, 0x1f, n - q) : nullptr;
        if (!f) return;
        q = (size_t)((const uint8_t *)f - p);
        if (is_hdr(q)) break;
        q++;
    }
    out.first = abs + q;
    while (is_hdr(q)) {
        const size_t bsize = (size_t)(p[q + 16] | (p[q + 17] << 8)) + 1;
        if (bsize < 26 || q + bsize > n) break;
        PreBlock b; b.hdr = abs + q; b.bsize = (uint32_t)bsize;
        memcpy(&b.crc, p + q + bsize - 8, 4); memcpy(&b.isize, p + q + bsize - 4, 4);
        if (b.isize > 65536u) break;
        out.blocks.push_back(b);
        q += bsize;
    }
    out.next = abs + q;
}

// the coordinator's loop body for one piece; its `return fail(1, "...")` lines return 1..4 in the order of bgzfw::Status
struct Chain {
    uint64_t next_blk, out_off = 0, pending_bsize = 0;
    uint8_t tail[64]; uint64_t tail_end = 0; size_t tail_len = 0;
    uint64_t lists_taken = 0;      // (counted for the test: how often a chunk's own list was taken over)
    explicit Chain(uint64_t start) : next_blk(start) {}
    int piece(const uint8_t *dst, uint64_t off, uint64_t n, const PreChunk *pre, size_t chunk, std::vector<cov_bgzf_block> &blocks) {
        auto byte_at = [&](uint64_t a) -> uint8_t {
            if (a >= off) return dst[a - off];
            return tail[tail_len - (size_t)(tail_end - a)];
        };
        const uint64_t have = off + n;
        for (;;) {
            if (pending_bsize == 0 && next_blk >= off && next_blk < have) {
                const PreChunk &P = pre[(size_t)((next_blk - off) / chunk)];
                if (P.first == next_blk && !P.blocks.empty()) {
                    for (const PreBlock &pb : P.blocks) {
                        cov_bgzf_block b;
                        b.in_off = pb.hdr + 18; b.in_len = pb.bsize - 26; b.crc = pb.crc; b.isize = pb.isize; b.out_off = out_off; b.pad = 0;
                        out_off += pb.isize;
                        blocks.push_back(b);
                    }
                    next_blk = P.next;
                    lists_taken++;
                    continue;
                }
            }
            if (pending_bsize == 0) {
                if (next_blk + 18 > have) break;
                uint8_t hb[18];
                for (int q = 0; q < 18; q++) hb[q] = byte_at(next_blk + (uint64_t)q);
                if (hb[0] != 0x1f || hb[1] != 0x8b || hb[2] != 8 || !(hb[3] & 4)) return 1;
                const uint32_t xlen = hb[10] | (hb[11] << 8);
                if (xlen != 6 || hb[12] != 66 || hb[13] != 67 || hb[14] != 2 || hb[15] != 0) return 2;
                pending_bsize = (uint64_t)(hb[16] | (hb[17] << 8)) + 1;
                if (pending_bsize < 26) return 3;
            }
            const uint64_t bsize = pending_bsize;
            if (next_blk + bsize > have) break;
            cov_bgzf_block b;
            b.in_off = next_blk + 18; b.in_len = (uint32_t)(bsize - 26);
            uint8_t tr[8];
            for (int q = 0; q < 8; q++) tr[q] = byte_at(next_blk + bsize - 8 + (uint64_t)q);
            memcpy(&b.crc, tr, 4); memcpy(&b.isize, tr + 4, 4);
            if (b.isize > 65536u) return 4;
            b.out_off = out_off; b.pad = 0;
            out_off += b.isize;
            blocks.push_back(b);
            next_blk += bsize;
            pending_bsize = 0;
        }
        tail_len = (size_t)std::min<uint64_t>(sizeof tail, n);
        memcpy(tail, dst + n - tail_len, tail_len);
        tail_end = have;
        return 0;
    }
};
}  // namespace frozen

enum { TRUNCATED = 5 };      // the driver's check behind the last piece: next_blk != size

struct Walked {
    int status = 0; uint64_t next_blk = 0, pre_blocks = 0, lists_taken = 0;
    std::vector<cov_bgzf_block> table;
};

// file[0, size) in pieces of `piece` bytes, each hopped in chunks of `chunk` bytes; which = 0: bgzf_walk_core.h, 1: the frozen code
template <class Chain, class PreChunk, class Hop>
static void drive(Chain &w, Hop hop, const uint8_t *file, uint64_t size, uint64_t piece, uint64_t chunk, Walked &r) {
    const size_t cpp = (size_t)((piece + chunk - 1) / chunk);
    std::vector<PreChunk> pre(cpp);
    for (uint64_t off = 0; off < size && r.status == 0; off += piece) {
        const uint64_t n = std::min<uint64_t>(piece, size - off);
        uint8_t *buf = (uint8_t *)malloc((size_t)n);      // exactly the piece: a read past it, or of it after the call, is the sanitizer's
        memcpy(buf, file + off, (size_t)n);
        for (size_t c = 0; c * chunk < n; c++) {
            const uint64_t o0 = c * chunk, e = std::min<uint64_t>(n, o0 + chunk);
            hop(buf + o0, (size_t)(e - o0), off + o0, pre[c]);
            r.pre_blocks += pre[c].blocks.size();
        }
        r.status = (int)w.piece(buf, off, n, pre.data(), (size_t)chunk, r.table);
        free(buf);
    }
    r.next_blk = w.next_blk;
    if (r.status == 0 && w.next_blk != size) r.status = TRUNCATED;
}
static Walked walk(const uint8_t *file, uint64_t size, uint64_t piece, uint64_t chunk, int which) {
    Walked r;
    if (which == 0) {
        bgzfw::Walker w(0);
        drive<bgzfw::Walker, bgzfw::PreChunk>(w, bgzfw::prewalk, file, size, piece, chunk, r);
    } else {
        frozen::Chain w(0);
        drive<frozen::Chain, frozen::PreChunk>(w, frozen::prewalk, file, size, piece, chunk, r);
        r.lists_taken = w.lists_taken;
    }
    return r;
}

extern "C" {
// -> status (bgzfw::Status, or 5 = blocks cut short at the end); at most cap blocks are written to out, *n_out is their full count
int bgzfw_walk(const uint8_t *file, uint64_t size, uint64_t piece, uint64_t chunk, int which, cov_bgzf_block *out, uint64_t cap, uint64_t *n_out,
               uint64_t *next_blk, uint64_t *pre_blocks, uint64_t *lists_taken) {
    const Walked r = walk(file, size, piece, chunk, which);
    for (uint64_t i = 0; i < r.table.size() && i < cap; i++) out[i] = r.table[i];
    *n_out = r.table.size(); *next_blk = r.next_blk; *pre_blocks = r.pre_blocks; *lists_taken = r.lists_taken;
    return r.status;
}
int bgzfw_classify(const uint8_t *h18, int any_flags) { return (int)bgzfw::classify(h18, any_flags != 0); }
int bgzfw_frozen_find_test(const uint8_t *h18) { return frozen::find_test(h18) ? 1 : 0; }
}

// ---- the program: files of stored blocks (no zlib needed: a stored DEFLATE block is 01 LEN ~LEN and the bytes)
static uint32_t g_rng = 12345;
static uint32_t rnd() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }
static void put_block(std::vector<uint8_t> &f, const std::vector<uint8_t> &payload) {
    const uint32_t len = (uint32_t)payload.size(), bsize = len + 5 + 26;
    const uint8_t h[18] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 66, 67, 2, 0, (uint8_t)((bsize - 1) & 255), (uint8_t)((bsize - 1) >> 8)};
    f.insert(f.end(), h, h + 18);
    const uint8_t d[5] = {1, (uint8_t)(len & 255), (uint8_t)(len >> 8), (uint8_t)(~len & 255), (uint8_t)((~len >> 8) & 255)};
    f.insert(f.end(), d, d + 5);
    f.insert(f.end(), payload.begin(), payload.end());
    const uint32_t crc = rnd();      // (the walk carries the CRC, it does not check it)
    uint8_t t[8]; memcpy(t, &crc, 4); memcpy(t + 4, &len, 4);
    f.insert(f.end(), t, t + 8);
}
static std::vector<uint8_t> make_file(int n_blocks, uint32_t lo, uint32_t hi, std::vector<uint64_t> &starts) {
    std::vector<uint8_t> f;
    for (int b = 0; b < n_blocks; b++) {
        std::vector<uint8_t> pay(lo + rnd() % (hi - lo + 1));
        for (auto &x : pay) x = (uint8_t)rnd();
        starts.push_back(f.size());
        put_block(f, pay);
    }
    starts.push_back(f.size());
    const uint8_t eof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 66, 67, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    f.insert(f.end(), eof, eof + 28);
    return f;
}
static bool same(const Walked &a, const Walked &b) {
    if (a.status != b.status || a.next_blk != b.next_blk || a.table.size() != b.table.size() || a.pre_blocks != b.pre_blocks) return false;
    return a.table.empty() || memcmp(a.table.data(), b.table.data(), a.table.size() * sizeof(cov_bgzf_block)) == 0;
}

int main() {
    unsigned long long n = 0, bad = 0;
    for (int variant = 0; variant < 2; variant++) {
        std::vector<uint64_t> starts;
        const std::vector<uint8_t> good = variant == 0 ? make_file(40, 40, 90, starts) : make_file(12, 200, 300, starts);
        // [1] the good file, then five irregular ones: [2] FLG with a further bit, [3] a second subfield, [4] BSIZE below 26, [5] ISIZE above 64 KiB, [6] cut short
        for (int kind = 1; kind < 7; kind++) {
            std::vector<uint8_t> f = good;
            const uint64_t at = starts[starts.size() / 2], end = starts[starts.size() / 2 + 1];
            int want = 0; uint64_t want_next = f.size();
            if (kind == 2) f[at + 3] |= 1;
            if (kind == 3) {
                const uint8_t sub[4] = {'X', 'X', 0, 0};
                f.insert(f.begin() + (long)at + 18, sub, sub + 4);
                f[at + 10] = 10;
                const uint32_t bs = (uint32_t)(end - at) + 4 - 1; f[at + 16] = (uint8_t)(bs & 255); f[at + 17] = (uint8_t)(bs >> 8);
                want = 2; want_next = at;
            }
            if (kind == 4) { f[at + 16] = 10; f[at + 17] = 0; want = 3; want_next = at; }
            if (kind == 5) { f[end - 2] = 2; want = 4; want_next = at; }
            if (kind == 6) { f.resize(f.size() - 5); want = TRUNCATED; want_next = starts.back(); }
            for (uint64_t piece = 64; piece <= 200; piece++)
                for (uint64_t chunk : {32u, 47u, 64u}) {
                    const Walked a = walk(f.data(), f.size(), piece, chunk, 0), b = walk(f.data(), f.size(), piece, chunk, 1);
                    n++;
                    if (!same(a, b) || a.status != want || a.next_blk != want_next) { bad++; continue; }
                    if (want != 0) continue;
                    // against one pass over the whole file
                    uint64_t q = 0, out = 0; size_t i = 0;
                    for (; q < f.size(); i++) {
                        const uint64_t bs = (uint64_t)(f[q + 16] | (f[q + 17] << 8)) + 1;
                        uint32_t isize; memcpy(&isize, &f[q + bs - 4], 4);
                        if (i >= a.table.size() || a.table[i].in_off != q + 18 || a.table[i].in_len != bs - 26 || a.table[i].isize != isize || a.table[i].out_off != out) { bad++; break; }
                        out += isize; q += bs;
                    }
                    if (i != a.table.size()) bad++;
                }
        }
    }
    // chunks that hold whole blocks: the lists are taken over
    {
        std::vector<uint64_t> starts;
        const std::vector<uint8_t> f = make_file(60, 40, 90, starts);
        for (uint64_t piece : {500u, 777u, 1024u})
            for (uint64_t chunk : {128u, 200u, 256u}) {
                const Walked a = walk(f.data(), f.size(), piece, chunk, 0), b = walk(f.data(), f.size(), piece, chunk, 1);
                n++;
                if (!same(a, b) || a.status != 0 || a.table.size() != 61 || b.lists_taken == 0) bad++;
            }
    }
    {      // nothing at all, and the end-of-file block alone
        std::vector<uint64_t> starts;
        const std::vector<uint8_t> f = make_file(0, 1, 1, starts);
        const uint8_t none = 0;
        const Walked e = walk(&none, 0, 64, 32, 0), a = walk(f.data(), f.size(), 64, 32, 0), b = walk(f.data(), f.size(), 64, 32, 1);
        n += 2;
        if (e.status != 0 || !e.table.empty()) bad++;
        if (!same(a, b) || a.status != 0 || a.table.size() != 1 || a.table[0].in_off != 18 || a.table[0].in_len != 2 || a.table[0].isize != 0) bad++;
    }
    printf("%llu cases, %llu bad\n", n, bad);
    return bad ? 1 : 0;
}

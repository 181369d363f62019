// The BGZF block headers of a file that arrives in pieces (host side of the device ingest, csrc/host_bam.cpp): the one test for an
// "ordinary" block header, the per-chunk hop a pool thread runs right behind its copy, and the serial chain that turns the pieces into the
// block table the device is fed.  Plain C++: no threads, no I/O, no HIP; tests/c/bgzf_walk_host.cpp runs it on the CPU against the loop the
// driver carried before, under the sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/covermhip.h"      // cov_bgzf_block

namespace bgzfw {

// The first 18 bytes of a block as every writer of BAM files emits them: 1f 8b 08, FLG = 4 (FEXTRA), XLEN = 6, the one subfield
// 'B' 'C' with SLEN = 2, BSIZE (block size - 1).  The checks run in this order, and the first that fails names the outcome.
//   any_flags: FLG may carry further bits beside FEXTRA, as the whole-file reader's bgzf_block_table allows (the serial chain, which
//   stands at a block's start); without it FLG must be 4 (the searches for a signature among bytes that may be compressed data: the
//   per-chunk hop and find_block_start).  The two acceptances are as the three call sites had them, on purpose.
enum Header { ORDINARY = 0, NOT_BGZF, EXTRA_SUBFIELDS, BAD_BSIZE };
inline uint32_t bsize_of(const uint8_t *h) { return (uint32_t)(h[16] | (h[17] << 8)) + 1; }
inline Header classify(const uint8_t *h, bool any_flags) {
    if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || (any_flags ? !(h[3] & 4) : h[3] != 4)) return NOT_BGZF;
    if (h[10] != 6 || h[11] != 0 || h[12] != 66 || h[13] != 67 || h[14] != 2 || h[15] != 0) return EXTRA_SUBFIELDS;      // rare: the CPU reader takes such a file
    if (bsize_of(h) < 26) return BAD_BSIZE;
    return ORDINARY;
}

// ---- the hop inside one chunk
// Hopping the block headers is a chain of dependent cache misses (~0.3 us per block, 0.28 s for the 944 k blocks of a 200 M-read
// file) if one thread does it after the fact.  The pool thread that has just read a chunk hops the blocks that lie entirely inside it
// while the bytes are still in its cache (first header found by its 16-byte signature); the chain takes over a chunk's list when it
// arrives exactly at the list's first header, and hops by itself otherwise (the blocks that straddle chunks, or a chunk whose first
// signature was a coincidence inside compressed data).
struct PreBlock { uint64_t hdr; uint32_t bsize, crc, isize; };
struct PreChunk { uint64_t first = ~0ull, next = 0; std::vector<PreBlock> blocks; };
inline void prewalk(const uint8_t *p, size_t n, uint64_t abs, PreChunk &out) {
    out.first = ~0ull; out.next = 0; out.blocks.clear();
    auto is_hdr = [&](size_t q) {      // the signature alone: a BSIZE below 26 ends the hop, it does not move the search on
        if (q + 18 > n) return false;
        const Header c = classify(p + q, false);
        return c == ORDINARY || c == BAD_BSIZE;
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
        const size_t bsize = bsize_of(p + q);
        if (bsize < 26 || q + bsize > n) break;                  // ends in a later chunk: the chain's business
        PreBlock b; b.hdr = abs + q; b.bsize = (uint32_t)bsize;
        memcpy(&b.crc, p + q + bsize - 8, 4); memcpy(&b.isize, p + q + bsize - 4, 4);
        if (b.isize > 65536u) break;
        out.blocks.push_back(b);
        q += bsize;
    }
    out.next = abs + q;
}

// ---- the serial chain across pieces
// Contract: the pieces of one byte range arrive in order and are contiguous (piece k + 1 starts at the offset piece k ended at, the first
// at or before `start`), and every piece but the last holds at least 64 bytes: a header (18 bytes) or a trailer (8 bytes) may begin in the
// piece before the one that completes it, never earlier, and the last 64 bytes of that piece are kept for it.  `pre` are the PreChunks of
// this piece, one per `chunk` bytes, each made by prewalk over exactly that chunk.  None of this is checked at run time.
// A status other than OK ends the walk: next_blk is then the offset of the block that was refused.
enum Status { OK = 0, NOT_A_BGZF_BLOCK, BLOCK_WITH_EXTRA_SUBFIELDS, MALFORMED_HEADER, ISIZE_ABOVE_64K };
struct Walker {
    uint64_t next_blk;              // absolute file offset of the next block header; the range was whole blocks iff it ends up at the range's end
    uint64_t out_off = 0;           // running inflated size
    uint64_t pending_bsize = 0;     // BSIZE of a block whose header is read but whose end is not here yet
    uint8_t tail[64]; uint64_t tail_end = 0; size_t tail_len = 0;   // last bytes of the previous piece (a header or a trailer may straddle)
    explicit Walker(uint64_t start) : next_blk(start) {}

    // The blocks completed by the piece bytes[0, n) = file[off, off + n) are appended to `out`.
    Status piece(const uint8_t *bytes, uint64_t off, uint64_t n, const PreChunk *pre, size_t chunk, std::vector<cov_bgzf_block> &out) {
        auto byte_at = [&](uint64_t a) -> uint8_t {   // absolute file offset, within this piece or the saved tail of the previous one
            if (a >= off) return bytes[a - off];
            return tail[tail_len - (size_t)(tail_end - a)];
        };
        const uint64_t have = off + n;
        for (;;) {
            if (pending_bsize == 0 && next_blk >= off && next_blk < have) {     // a chunk's own hop starts exactly here: take its blocks
                const PreChunk &P = pre[(size_t)((next_blk - off) / chunk)];
                if (P.first == next_blk && !P.blocks.empty()) {
                    for (const PreBlock &pb : P.blocks) {
                        cov_bgzf_block b;
                        b.in_off = pb.hdr + 18; b.in_len = pb.bsize - 26; b.crc = pb.crc; b.isize = pb.isize; b.out_off = out_off; b.pad = 0;
                        out_off += pb.isize;
                        out.push_back(b);
                    }
                    next_blk = P.next;
                    continue;
                }
            }
            if (pending_bsize == 0) {          // header of the next block (may straddle into the saved tail of the previous piece)
                if (next_blk + 18 > have) break;
                uint8_t hb[18];
                for (int q = 0; q < 18; q++) hb[q] = byte_at(next_blk + (uint64_t)q);
                switch (classify(hb, true)) {
                    case NOT_BGZF: return NOT_A_BGZF_BLOCK;
                    case EXTRA_SUBFIELDS: return BLOCK_WITH_EXTRA_SUBFIELDS;
                    case BAD_BSIZE: return MALFORMED_HEADER;
                    case ORDINARY: break;
                }
                pending_bsize = bsize_of(hb);
            }
            const uint64_t bsize = pending_bsize;
            if (next_blk + bsize > have) break;             // completed by a later piece (its header is not read again)
            cov_bgzf_block b;
            b.in_off = next_blk + 18; b.in_len = (uint32_t)(bsize - 26);
            uint8_t tr[8];
            for (int q = 0; q < 8; q++) tr[q] = byte_at(next_blk + bsize - 8 + (uint64_t)q);
            memcpy(&b.crc, tr, 4); memcpy(&b.isize, tr + 4, 4);
            if (b.isize > 65536u) return ISIZE_ABOVE_64K;
            b.out_off = out_off; b.pad = 0;
            out_off += b.isize;
            out.push_back(b);
            next_blk += bsize;
            pending_bsize = 0;
        }
        tail_len = (size_t)std::min<uint64_t>(sizeof tail, n);
        memcpy(tail, bytes + n - tail_len, tail_len);
        tail_end = have;
        return OK;
    }
};

}  // namespace bgzfw

// "Can a BAM record start at this offset, and where does it end" — the arithmetic of the device ingest's record search, written once, run two
// ways (the kernels in csrc/ingest_kernels.hip.h; on the CPU in tests/c/bam_record_host.cpp against a Python restatement).  Also here: the
// NM scan and the CG:B,I lookup of the record extraction, which walk the same tags, and the constants that make a record a "long" one.
//
// A record: block_size (u32) | refID pos l_read_name mapq bin n_cigar_op flag l_seq next_refID next_pos tlen (32 bytes) | read_name
// (l_read_name bytes, NUL-terminated) | cigar (4 * n_cigar_op) | seq ((l_seq + 1) / 2) | qual (l_seq) | tags up to 4 + block_size.
//   fixed_fields   the fixed part fits block_size, the references and the position lie inside the header's, the name ends in a NUL, and
//                  block_size is not above walk_cap: a record larger than the carry buffer between two windows is handed to the CPU reader
//                  anyway, so no candidate ever makes anyone walk more than walk_cap bytes (a stray offset whose first four bytes read as
//                  900 MB is refused before a single tag is looked at)
//   aux_exact      EVERY tag up to the record's end, strings of any length, the walk ending exactly on the end
// Tags are walked by one function, next_tag, over a policy W that finds the NUL of a Z / H string: Serial (byte by byte: one lane, or the
// CPU) or the wave's (ingest_kernels.hip.h WaveNul: 16 bytes per lane, the NUL by ballot; Lanes64 below is the same thing lane by lane on
// the CPU, through the very lane_nul_mask the kernel calls).  Fixed-size tags and B arrays are skipped by arithmetic.
#pragma once
#include <stdint.h>

#ifndef BAMREC_FN
#define BAMREC_FN inline
#endif

namespace bamrec {

typedef unsigned int u32;
typedef unsigned long long u64;

// A record is "long" when it has more CIGAR words (the real ones of a CG:B,I record) or more tag bytes than this: k_bam_extract leaves its
// CIGAR copy and NM scan to k_bam_extract_long, a wave per record.
constexpr u32 LONG_CIGAR_WORDS = 64u, LONG_AUX_BYTES = 1024u;
constexpr u32 CHAIN = 8u;            // consecutive plausible records that make a start
constexpr u32 STEP_BYTES = 1024u;    // one wave step of a string walk: 64 lanes x 16 bytes
constexpr u64 NONE = ~0ull;

BAMREC_FN u32 ld16(const uint8_t *p) { return (u32)p[0] | ((u32)p[1] << 8); }
#ifndef BAMREC_LD32
BAMREC_FN u32 ld32(const uint8_t *p) { return (u32)p[0] | ((u32)p[1] << 8) | ((u32)p[2] << 16) | ((u32)p[3] << 24); }
#else
BAMREC_FN u32 ld32(const uint8_t *p) { return BAMREC_LD32(p); }
#endif

struct Stream {
    const uint8_t *u; u64 N;      // bytes [0, N)
    int n_ref; const u32 *ref_len;
    u64 walk_cap;                 // largest block_size a candidate may have
};

// bytes of a record in front of its tags, behind block_size
BAMREC_FN u64 fixed_bytes(u32 l_read_name, u32 n_cig, u32 l_seq) { return 32ull + l_read_name + 4ull * n_cig + ((u64)l_seq + 1ull) / 2 + l_seq; }
BAMREC_FN bool is_long(u32 cigar_words, u64 aux_bytes) { return cigar_words > LONG_CIGAR_WORDS || aux_bytes > LONG_AUX_BYTES; }

// The per-offset filter.  Returns the record's end offset (aux = where its tags begin), or 0.
BAMREC_FN u64 fixed_fields(const Stream &S, u64 o, u64 &aux) {
    if (o + 36 > S.N) return 0;
    const uint8_t *r = S.u + o;
    const u32 bs = ld32(r);
    if (bs < 32u || bs > S.walk_cap || o + 4 + (u64)bs > S.N) return 0;
    const int rid = (int)ld32(r + 4), pos = (int)ld32(r + 8), nrid = (int)ld32(r + 24);
    const u32 lname = r[12], ncig = ld16(r + 16), lseq = ld32(r + 20);
    if (rid < -1 || rid >= S.n_ref || nrid < -1 || nrid >= S.n_ref || pos < -1 || lname == 0u) return 0;
    if (rid >= 0 && (u32)pos > S.ref_len[rid]) return 0;
    const u64 fixed = fixed_bytes(lname, ncig, lseq);
    if (fixed > bs) return 0;
    if (r[36 + lname - 1] != 0) return 0;
    aux = o + 4 + fixed;
    return o + 4 + bs;
}

// ---- tags
BAMREC_FN u32 scalar_size(uint8_t ty) {      // 0: not a fixed-size type
    return (ty == 'A' || ty == 'c' || ty == 'C') ? 1u : (ty == 's' || ty == 'S') ? 2u : (ty == 'i' || ty == 'I' || ty == 'f') ? 4u : 0u;
}
BAMREC_FN bool array_subtype(uint8_t st) { return st == 'c' || st == 'C' || st == 's' || st == 'S' || st == 'i' || st == 'I' || st == 'f'; }
BAMREC_FN u32 array_elem_size(uint8_t st) { return (st == 'c' || st == 'C') ? 1u : (st == 's' || st == 'S') ? 2u : 4u; }

// Bit j of the result: byte j of the 16 bytes at a + 16 * lane is a NUL of the string, that is, lies in [p, end).  `a` is p rounded down to
// a multiple of 4, so the four words are aligned loads; bytes at or beyond `end` may be read (up to 15 of them: the caller's buffer has
// that much room) but never count.
BAMREC_FN u32 zero_bytes(u32 w) { return ~(((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w | 0x7f7f7f7fu); }      // 0x80 in every byte that is 0, exactly
BAMREC_FN u32 lane_nul_mask(const uint8_t *u, u64 a, u32 lane, u64 p, u64 end) {
    const u64 at = a + 16ull * lane;
    if (at >= end) return 0u;
    const u32 *w = reinterpret_cast<const u32 *>(u + at);
    u32 m = 0;
    for (u32 i = 0; i < 4u; i++) {
        const u32 z = zero_bytes(w[i]);
        m |= (((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u)) << (4u * i);
    }
    if (at < p) m &= ~0u << (u32)(p - at);                      // (p - at < 4: only the first lane of the first step)
    if (end - at < 16ull) m &= (1u << (u32)(end - at)) - 1u;
    return m;
}
// position of the lowest set bit (m != 0), without a builtin: host and device
BAMREC_FN u32 low_bit(u32 m) { u32 n = 0; while (!(m & 1u)) { m >>= 1; n++; } return n; }

struct Serial {      // the NUL of the string that starts at p, or NONE if there is none in front of `end`
    BAMREC_FN u64 first_nul(const uint8_t *u, u64 p, u64 end) const { while (p < end && u[p]) p++; return p < end ? p : NONE; }
};
struct Lanes64 {     // the wave's walk, lane by lane (CPU): steps of 1024 bytes, the lowest lane with a hit wins
    BAMREC_FN u64 first_nul(const uint8_t *u, u64 p, u64 end) const {
        for (u64 a = p & ~3ull; a < end; a += STEP_BYTES)      // (u itself is 4-byte aligned, as the window buffers are)
            for (u32 lane = 0; lane < 64u; lane++) { const u32 m = lane_nul_mask(u, a, lane, p, end); if (m) return a + 16ull * lane + low_bit(m); }
        return NONE;
    }
};

struct Tag {
    uint8_t n0, n1, ty, st;      // name, type, subtype of a B array
    u32 cnt;                     // elements of a B array
    u64 val;                     // where the value begins (a B array's first element)
};
enum { TAG_OK = 0, TAG_END = 1, TAG_BAD = 2 };
// The tag at p: name, type and, of an array, subtype and count.  TAG_END at the end of the area; TAG_BAD for fewer than three bytes, an
// unknown type or an array header cut by the end.
BAMREC_FN int tag_head(const uint8_t *u, u64 p, u64 end, Tag &t) {
    if (p >= end) return TAG_END;
    if (p + 3 > end) return TAG_BAD;
    t.n0 = u[p]; t.n1 = u[p + 1]; t.ty = u[p + 2]; t.st = 0; t.cnt = 0; t.val = p + 3;
    if (scalar_size(t.ty) || t.ty == 'Z' || t.ty == 'H') return TAG_OK;
    if (t.ty != 'B' || p + 8 > end) return TAG_BAD;
    t.st = u[p + 3]; t.cnt = ld32(u + p + 4); t.val = p + 8;
    return TAG_OK;
}
// Where the tag behind t begins, or NONE: a value cut by the end, a string without its NUL, an array whose count runs past the end,
// or (strict) an array of an unknown subtype.
template <class W>
BAMREC_FN u64 tag_next(const W &w, const uint8_t *u, const Tag &t, u64 end, bool strict) {
    const u32 sz = scalar_size(t.ty);
    if (sz) return t.val + sz <= end ? t.val + sz : NONE;
    if (t.ty == 'B') {
        if (strict && !array_subtype(t.st)) return NONE;
        const u32 es = array_elem_size(t.st);
        if ((end - t.val) / es < t.cnt) return NONE;
        return t.val + (u64)t.cnt * es;
    }
    const u64 z = w.first_nul(u, t.val, end);
    return z == NONE ? NONE : z + 1;
}

// Do the bytes [p, end) parse as tags that end exactly at `end`?  Without this test a stray offset whose "block_size" happens to jump onto a
// real record start far away passes (the next seven records are then real ones): seen once per ~10^7 tested offsets on a 6 GB stream.
template <class W>
BAMREC_FN bool aux_exact(const W &w, const uint8_t *u, u64 p, u64 end) {
    for (;;) {
        Tag t;
        const int h = tag_head(u, p, end, t);
        if (h != TAG_OK) return h == TAG_END;
        p = tag_next(w, u, t, end, true);
        if (p == NONE) return false;
    }
}

// Can a record start at o?  Its end offset, or 0.
template <class W>
BAMREC_FN u64 plausible_record(const W &w, const Stream &S, u64 o) {
    u64 aux = 0;
    const u64 e = fixed_fields(S, o, aux);
    return e && aux_exact(w, S.u, aux, e) ? e : 0;
}
// Does a chain of CHAIN plausible records (or fewer, ending exactly at N) start at o?
template <class W>
BAMREC_FN bool chain_start(const W &w, const Stream &S, u64 o) {
    u64 q = o; u32 chain = 0;
    while (chain < CHAIN) { const u64 e = plausible_record(w, S, q); if (!e) break; q = e; chain++; if (q == S.N) break; }
    return chain == CHAIN || (chain > 0 && q == S.N);
}

// NM of the tags [p, end) (csrc/host_bam.cpp scan_aux without the CG part): 1 and its value for NM:C / NM:S / NM:I, 2 for NM of another
// type, 0 when there is none in front of the end or of the first tag that does not parse.
template <class W>
BAMREC_FN u32 scan_nm(const W &w, const uint8_t *u, u64 p, u64 end, u32 &nm) {
    for (;;) {
        Tag t;
        if (tag_head(u, p, end, t) != TAG_OK) return 0u;
        const bool is_nm = t.n0 == 'N' && t.n1 == 'M';
        if (is_nm && !scalar_size(t.ty)) return 2u;
        p = tag_next(w, u, t, end, false);
        if (p == NONE) return 0u;
        if (is_nm) {
            if (t.ty == 'C') { nm = u[t.val]; return 1u; }
            if (t.ty == 'S') { nm = ld16(u + t.val); return 1u; }
            if (t.ty == 'I') { nm = ld32(u + t.val); return 1u; }
            return 2u;
        }
    }
}

// A record whose CIGAR has more than 65535 operations stores `<l_seq>S<ref_len>N` in the CIGAR field and the real one in CG:B,I; htslib
// swaps it back in while reading (bam_tag2cigar, sam.c), so record.cigar() at contig.rs:168 sees the real CIGAR.  The conditions of
// csrc/host_bam.cpp real_cigar_from_cg: exactly two operations, mapped, the first one `<l_seq>S`, the first CG tag of type B,I / B,i
// with at least as many words as the placeholder.  r = the record's offset, end = its end; returns where the words are (and their
// count), or NONE.
template <class W>
BAMREC_FN u64 cg_cigar(const W &w, const uint8_t *u, u64 r, u64 end, u32 &cnt) {
    const u32 n_cig = ld16(u + r + 16), l_read_name = u[r + 12], l_seq = ld32(u + r + 20);
    if (n_cig != 2u || (int)ld32(u + r + 4) < 0 || (int)ld32(u + r + 8) < 0) return NONE;
    const u64 c = r + 36 + l_read_name;
    if (c + 8 > end) return NONE;
    const u32 c0 = ld32(u + c);
    if ((c0 & 15u) != 4u || (c0 >> 4) != l_seq) return NONE;
    u64 p = c + 8 + ((u64)l_seq + 1ull) / 2 + l_seq;
    if (p > end) return NONE;
    for (;;) {
        Tag t;
        if (tag_head(u, p, end, t) != TAG_OK) return NONE;
        p = tag_next(w, u, t, end, false);
        if (p == NONE) return NONE;
        if (t.n0 == 'C' && t.n1 == 'G' && t.ty == 'B' && (t.st == 'I' || t.st == 'i')) { cnt = t.cnt; return (t.cnt >= n_cig && t.cnt < (1u << 29)) ? t.val : NONE; }
    }
}

}  // namespace bamrec

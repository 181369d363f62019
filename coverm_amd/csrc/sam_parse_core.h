// SAM text decoded on the device — the arithmetic of one alignment line, written once, run two ways (the kernels in csrc/sam_kernels.hip.h;
// stage by stage on the CPU in tests/c/sam_parse_host.cpp against oracle/bamio.read_sam).  Nothing here calls a runtime: the caller hands in
// the bytes of a line (p, n) and, for the structural variant, the window's 64-bit tab masks, however it got them.
//
// The specification is parse_sam (host_bam.cpp), field for field:
//   flag   decimal                                   tid    `*` -> -1, else the name looked up (unknown -> -1)
//   pos    decimal - 1                               mapq   decimal
//   CIGAR  words len << 4 | op, ops MIDNSHP=X, an unknown letter -> 15, `*` -> no words
//   mtid   `=` -> tid, `*` -> -1, else looked up     l_seq  bytes of SEQ, 0 for `*`
//   NM     the LAST field `NM:...` longer than 5 bytes wins: `NM:i:` + a value that does not begin with `-` -> COV_NM_UNSIGNED and the
//          value, anything else -> COV_NM_BADTYPE; none -> COV_NM_ABSENT (the value of an earlier unsigned NM stays, as parse_sam leaves it)
//   a trailing '\r' is dropped; an empty line is no record; fewer than 11 fields is ERR_MALFORMED.
// Decimals are strtoul's: white space, an optional sign, digits up to the first other byte.
//
// Reference names -> tid: an open-addressing table (linear probing, power-of-two size, at most half full) built on the host from the @SQ
// lines.  A slot holds name index + 1; name_off[index] is the name's offset in the names blob, and a hit is confirmed by comparing the
// bytes there, never by the hash alone.  Names are inserted in header order and a name already present is not inserted again, so a
// duplicate SN resolves to its first occurrence, as parse_sam's lookup does.
#pragma once
#include <stdint.h>

#include "name_hash_core.h"

#ifndef SAMC_FN
#define SAMC_FN inline
#endif

namespace samc {

typedef unsigned int u32;
typedef unsigned long long u64;

constexpr u32 ERR_NONE = 0u, ERR_MALFORMED = 1u, ERR_CIGAR_OPS = 2u, ERR_LINE_LONG = 3u;
constexpr u32 MAX_CIGAR_OPS = 65535u;
constexpr u32 NM_ABSENT = 0u, NM_UNSIGNED = 1u, NM_BADTYPE = 2u;      // COV_NM_* (covermhip.h)

// ---- geometry of the structural pass: a lane holds 16 bytes, four lanes make one 64-bit mask word, a wave covers 1024 bytes
constexpr u32 LANE_BYTES = 16u, WORD_BYTES = 64u, WAVE_BYTES = 64u * LANE_BYTES, MASK_WG = 256u, MASK_WG_BYTES = MASK_WG * LANE_BYTES;

// 16-bit mask of the bytes of one lane's 16 that equal `c` (v = the four little-endian dwords of the load)
SAMC_FN u32 lane_mask16(const u32 v[4], uint8_t c) {
    u32 m = 0u;
    for (u32 k = 0; k < 4u; k++)
        for (u32 b = 0; b < 4u; b++) m |= (((v[k] >> (8u * b)) & 0xffu) == (u32)c ? 1u : 0u) << (4u * k + b);
    return m;
}
// four neighbouring lanes' masks -> the 64-bit word of their 64 bytes
SAMC_FN u64 word_of_lanes(u32 m0, u32 m1, u32 m2, u32 m3) { return (u64)m0 | ((u64)m1 << 16) | ((u64)m2 << 32) | ((u64)m3 << 48); }
SAMC_FN u32 popc64(u64 m) { return (u32)__builtin_popcountll(m); }
SAMC_FN u32 ctz64(u64 m) { return (u32)__builtin_ctzll(m); }

// ---- reference-name table
SAMC_FN u32 name_hash32(const uint8_t *p, u32 n) {
    u32 h = 0x811c9dc5u;
    for (u32 i = 0; i < n; i++) { h ^= p[i]; h *= 0x01000193u; }
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return h;
}
SAMC_FN u32 table_size(u32 n_names) { u32 s = 16u; while (s < 2u * n_names + 1u && s < 0x80000000u) s <<= 1; return s; }
struct Table { const u32 *slots; u32 mask; const uint8_t *blob; const u64 *name_off; };      // name i = blob[name_off[i] .. name_off[i + 1])
SAMC_FN bool bytes_equal(const uint8_t *a, const uint8_t *b, u32 n) { for (u32 i = 0; i < n; i++) if (a[i] != b[i]) return false; return true; }
SAMC_FN int32_t table_find(const Table &T, const uint8_t *p, u32 n) {
    if (!T.slots) return -1;
    for (u32 h = name_hash32(p, n) & T.mask;; h = (h + 1u) & T.mask) {
        const u32 v = T.slots[h];
        if (v == 0u) return -1;
        const u64 o = T.name_off[v - 1u];
        if (T.name_off[v] - o == n && bytes_equal(T.blob + o, p, n)) return (int32_t)(v - 1u);
    }
}
// host side: name i goes in unless an equal name is there already (slots zeroed by the caller, table_size(n_names) of them)
SAMC_FN void table_insert(u32 *slots, u32 mask, const uint8_t *blob, const u64 *name_off, u32 i) {
    const uint8_t *p = blob + name_off[i];
    const u32 n = (u32)(name_off[i + 1] - name_off[i]);
    for (u32 h = name_hash32(p, n) & mask;; h = (h + 1u) & mask) {
        const u32 v = slots[h];
        if (v == 0u) { slots[h] = i + 1u; return; }
        const u64 o = name_off[v - 1u];
        if (name_off[v] - o == n && bytes_equal(blob + o, p, n)) return;
    }
}

// ---- header: the SN and LN of one `@SQ` line (p, n; no line end).  parse_sam takes the last SN / LN of the line.
SAMC_FN void sq_fields(const uint8_t *p, u32 n, u32 &sn_off, u32 &sn_len, u64 &ln) {
    sn_off = 0; sn_len = 0; ln = 0;
    u32 q = 3u;
    while (q < n) {
        const u32 a = q + 1u;
        u32 t = a; while (t < n && p[t] != '\t') t++;
        if (t - a >= 3u && p[a + 2] == ':') {
            if (p[a] == 'S' && p[a + 1] == 'N') { sn_off = a + 3u; sn_len = t - a - 3u; }
            else if (p[a] == 'L' && p[a + 1] == 'N') { u64 v = 0; for (u32 i = a + 3u; i < t && p[i] >= '0' && p[i] <= '9'; i++) v = v * 10u + (u64)(p[i] - '0'); ln = v; }
        }
        if (t >= n) break;
        q = t;
    }
}

// ---- where the tabs of a line are.  ByteTabs walks the bytes; MaskTabs reads the window's tab masks (bit b of word w = byte 64 w + b is a
// tab), so that SEQ and QUAL — two thirds of a short-read line — cost a few words instead of their bytes.  next(i) = the first tab at or
// behind line offset i, n when there is none.
struct ByteTabs {
    const uint8_t *p; u32 n;
    SAMC_FN u32 next(u32 i) const { while (i < n && p[i] != '\t') i++; return i; }
};
struct MaskTabs {
    const u64 *mask; u64 base; u32 n;      // base: the line's first byte, as an offset in the window
    SAMC_FN u32 next(u32 i) const {
        if (i >= n) return n;
        u64 a = base + i;
        const u64 end = base + n;
        u64 w = a >> 6;
        u64 m = mask[w] & (~0ull << (a & 63u));
        while (m == 0ull) { w++; if ((w << 6) >= end) return n; m = mask[w]; }
        const u64 at = (w << 6) + ctz64(m);
        return at < end ? (u32)(at - base) : n;
    }
};

SAMC_FN bool is_space(uint8_t c) { return c == ' ' || (c >= 9u && c <= 13u); }
// strtoul(…, 10) over the field [a, b): value as u64 (negated for a leading '-')
SAMC_FN u64 dec_field(const uint8_t *p, u32 a, u32 b) {
    while (a < b && is_space(p[a])) a++;
    bool neg = false;
    if (a < b && (p[a] == '-' || p[a] == '+')) { neg = p[a] == '-'; a++; }
    u64 v = 0;
    for (; a < b && p[a] >= '0' && p[a] <= '9'; a++) v = v * 10u + (u64)(p[a] - '0');
    return neg ? (u64)0 - v : v;
}
SAMC_FN u32 trim_cr(const uint8_t *p, u32 n) { return (n && p[n - 1] == '\r') ? n - 1u : n; }
SAMC_FN u32 cigar_op(uint8_t c) {
    switch (c) {
    case 'M': return 0u; case 'I': return 1u; case 'D': return 2u; case 'N': return 3u; case 'S': return 4u;
    case 'H': return 5u; case 'P': return 6u; case '=': return 7u; case 'X': return 8u;
    default: return 15u;
    }
}
SAMC_FN bool is_digit(uint8_t c) { return c >= '0' && c <= '9'; }

// The first pass over a line: is it a record, is it well formed, how many CIGAR words.  n = the line's length after trim_cr.
struct LineCount { u32 is_record, n_cigar, err; };
template <typename Tabs>
SAMC_FN LineCount count_line(const uint8_t *p, u32 n, const Tabs &T) {
    LineCount c{0u, 0u, ERR_NONE};
    if (n == 0u) return c;
    c.is_record = 1u;
    u32 t = T.next(0), a5 = 0, b5 = 0;      // CIGAR = field 5
    for (u32 f = 1; f < 11u; f++) {
        if (t >= n) { c.err = ERR_MALFORMED; return c; }
        const u32 a = t + 1u;
        t = T.next(a);
        if (f == 5u) { a5 = a; b5 = t; }
    }
    if (!(b5 - a5 == 1u && p[a5] == '*')) {
        u32 ops = 0;
        for (u32 i = a5; i < b5; i++) ops += is_digit(p[i]) ? 0u : 1u;
        c.n_cigar = ops;
        if (ops > MAX_CIGAR_OPS) c.err = ERR_CIGAR_OPS;
    }
    return c;
}

struct Rec {
    int32_t tid, pos, mtid;
    u32 flag, mapq, nm, nm_kind, l_seq, n_cigar;
    u32 qname_len;      // QNAME = p[0 .. qname_len)
};
// The second pass: every field, CIGAR words to `cigar` (count_line's n_cigar of them; nullptr: not written).  The line is a well-formed
// record (count_line said so).
template <typename Tabs>
SAMC_FN void parse_line(const uint8_t *p, u32 n, const Tabs &T, const Table &names, Rec &r, u32 *cigar) {
    u32 a[11], b[11];
    u32 t = T.next(0);
    a[0] = 0; b[0] = t;
    for (u32 f = 1; f < 11u; f++) { a[f] = t < n ? t + 1u : n; t = T.next(a[f]); b[f] = t; }
    r.qname_len = b[0];
    r.flag = (u32)(uint16_t)dec_field(p, a[1], b[1]);
    r.tid = (b[2] - a[2] == 1u && p[a[2]] == '*') ? -1 : table_find(names, p + a[2], b[2] - a[2]);
    r.pos = (int32_t)(long long)dec_field(p, a[3], b[3]) - 1;
    r.mapq = (u32)(uint8_t)dec_field(p, a[4], b[4]);
    u32 nc = 0;
    if (!(b[5] - a[5] == 1u && p[a[5]] == '*')) {
        u32 num = 0;
        for (u32 i = a[5]; i < b[5]; i++) {
            const uint8_t ch = p[i];
            if (is_digit(ch)) num = num * 10u + (u32)(ch - '0');
            else { if (cigar) cigar[nc] = (num << 4) | cigar_op(ch); nc++; num = 0; }
        }
    }
    r.n_cigar = nc;
    const u32 l6 = b[6] - a[6];
    r.mtid = (l6 == 1u && p[a[6]] == '=') ? r.tid : (l6 == 1u && p[a[6]] == '*') ? -1 : table_find(names, p + a[6], l6);
    r.l_seq = (b[9] - a[9] == 1u && p[a[9]] == '*') ? 0u : b[9] - a[9];
    r.nm = 0; r.nm_kind = NM_ABSENT;
    t = b[10];
    while (t < n) {
        const u32 fa = t + 1u;
        t = T.next(fa);
        if (t - fa > 5u && p[fa] == 'N' && p[fa + 1] == 'M' && p[fa + 2] == ':') {
            if (p[fa + 3] == 'i' && p[fa + 5] != '-') { r.nm = (u32)dec_field(p, fa + 5u, t); r.nm_kind = NM_UNSIGNED; }
            else r.nm_kind = NM_BADTYPE;
        }
    }
}
// With mates wanted: the read-name hash over QNAME's bytes — covn::name_hash, the function the BAM record extraction calls.
SAMC_FN void qname_hash(const uint8_t *p, const Rec &r, u64 &k1, u32 &k2) { covn::name_hash(p, r.qname_len, k1, k2); }

}  // namespace samc

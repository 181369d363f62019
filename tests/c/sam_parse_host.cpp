// CPU emulation of the SAM text decode (csrc/sam_parse_core.h, the arithmetic csrc/sam_kernels.hip.h runs on the device), for
// tests/test_sam_parse_core.py.  staged = 1 walks the kernels' stages with their geometry — lanes of 16 bytes folded four at a time into the
// 64-bit newline / tab words, line ends by an exclusive scan over the words' popcounts, a count pass and a decode pass per line that find
// their tabs in the masks — window by window, each window cut at its last '\n' as the host driver cuts it.  staged = 0 parses line by line
// with the byte-walking tab finder.  Both must give the same records.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../coverm_amd/csrc/sam_parse_core.h"

using samc::u32;
using samc::u64;

namespace {

struct Out {
    int32_t *tid, *pos, *mtid; uint16_t *flag; uint8_t *mapq, *nm_kind; u32 *nm, *l_seq, *cigar_off, *cigar;
    u64 *qh1; u32 *qh2;      // the read-name hash of every record (nullptr: not wanted)
    u64 n_rec = 0, n_cig = 0;
};
struct Err { u64 line = 0; u32 code = 0; };      // 1-based line of the first offending line in file order

void emit(Out &o, const samc::Rec &r, const u32 *words, const uint8_t *p) {
    const u64 i = o.n_rec++;
    if (o.qh1) { u64 k1; u32 k2; samc::qname_hash(p, r, k1, k2); o.qh1[i] = k1; o.qh2[i] = k2; }
    o.tid[i] = r.tid; o.pos[i] = r.pos; o.mtid[i] = r.mtid; o.flag[i] = (uint16_t)r.flag; o.mapq[i] = (uint8_t)r.mapq; o.nm[i] = r.nm; o.nm_kind[i] = (uint8_t)r.nm_kind;
    o.l_seq[i] = r.l_seq; o.cigar_off[i] = (u32)o.n_cig;
    for (u32 k = 0; k < r.n_cigar; k++) o.cigar[o.n_cig + k] = words[k];
    o.n_cig += r.n_cigar;
}

// one window: text[0 .. n) holds whole lines (the last may lack its '\n').  Returns false at the window's first error.
bool window_staged(const uint8_t *text_in, u64 n_in, const samc::Table &T, Out &o, u64 lines_before, bool &seen_record, Err &err, u64 &n_lines_out) {
    // the text as the device holds it: one more '\n' when the last line has none, readable up to the next workgroup boundary
    std::vector<uint8_t> text(text_in, text_in + n_in);
    text.resize(n_in + 1 + samc::MASK_WG_BYTES, 0);
    u64 n = n_in;
    if (n_in && text_in[n_in - 1] != '\n') text[n++] = '\n';
    const u64 n_words = (n + 63) / 64;
    std::vector<u64> nl(n_words, 0), tab(n_words, 0);
    // k_sam_masks: workgroups of 256 lanes, a lane per 16 bytes, lanes 4 j .. 4 j + 3 make word j
    const u64 n_wg = (n + samc::MASK_WG_BYTES - 1) / samc::MASK_WG_BYTES;
    for (u64 wg = 0; wg < n_wg; wg++) {
        u32 mn[samc::MASK_WG], mt[samc::MASK_WG];
        for (u32 t = 0; t < samc::MASK_WG; t++) {
            const u64 g = wg * samc::MASK_WG + t, base = g * samc::LANE_BYTES;
            u32 v[4];
            memcpy(v, text.data() + base, 16);
            const u32 keep = base >= n ? 0u : (n - base >= samc::LANE_BYTES ? 0xffffu : (1u << (u32)(n - base)) - 1u);
            mn[t] = samc::lane_mask16(v, (uint8_t)'\n') & keep; mt[t] = samc::lane_mask16(v, (uint8_t)'\t') & keep;
        }
        for (u32 t = 0; t < samc::MASK_WG; t += 4) {
            const u64 g = wg * samc::MASK_WG + t;
            if (g * samc::LANE_BYTES >= n) continue;
            nl[g >> 2] = samc::word_of_lanes(mn[t], mn[t + 1], mn[t + 2], mn[t + 3]);
            tab[g >> 2] = samc::word_of_lanes(mt[t], mt[t + 1], mt[t + 2], mt[t + 3]);
        }
    }
    // the scan over the words' popcounts, and its consumer
    std::vector<u32> wbase(n_words + 1, 0);
    for (u64 w = 0; w < n_words; w++) wbase[w + 1] = wbase[w] + samc::popc64(nl[w]);
    const u32 n_lines = wbase[n_words];
    n_lines_out = n_lines;
    std::vector<u32> line_end(n_lines);
    for (u64 w = 0; w < n_words; w++) { u32 p = wbase[w]; for (u64 m = nl[w]; m; m &= m - 1ull) line_end[p++] = (u32)(w * 64u + samc::ctz64(m)); }
    // k_sam_count
    std::vector<u32> cnt(n_lines);
    u64 e = ~0ull, first_rec = ~0ull, last_at = 0;
    for (u32 i = 0; i < n_lines; i++) {
        const u32 start = i ? line_end[i - 1] + 1u : 0u, ln = samc::trim_cr(text.data() + start, line_end[i] - start);
        const uint8_t *p = text.data() + start;
        if (ln && p[0] == '@') { cnt[i] = 0; last_at = i + 1ull; continue; }
        const samc::MaskTabs M{tab.data(), start, ln};
        const samc::LineCount c = samc::count_line(p, ln, M);
        cnt[i] = (c.n_cigar << 1) | c.is_record;
        if (c.is_record && i < first_rec) first_rec = i;
        if (c.err) { const u64 v = ((u64)i << 8) | c.err; if (v < e) e = v; }
    }
    u64 bad_line = ~0ull; u32 bad = 0;
    if (e != ~0ull) { bad_line = e >> 8; bad = (u32)(e & 0xffu); }
    if (last_at && (seen_record || (first_rec != ~0ull && last_at - 1 > first_rec)) && last_at - 1 < bad_line) { bad_line = last_at - 1; bad = 4u; }
    if (bad) { err.line = lines_before + bad_line + 1; err.code = bad; return false; }
    if (first_rec != ~0ull) seen_record = true;
    // the two scans, then k_sam_decode
    std::vector<u32> rec_idx(n_lines), cig_idx(n_lines);
    u32 r = 0, c = 0;
    for (u32 i = 0; i < n_lines; i++) { rec_idx[i] = r; cig_idx[i] = c; r += cnt[i] & 1u; c += cnt[i] >> 1; }
    const u64 rec0 = o.n_rec, cig0 = o.n_cig;
    for (u32 i = 0; i < n_lines; i++) {
        if (!(cnt[i] & 1u)) continue;
        const u32 start = i ? line_end[i - 1] + 1u : 0u, ln = samc::trim_cr(text.data() + start, line_end[i] - start);
        const samc::MaskTabs M{tab.data(), start, ln};
        samc::Rec R;
        const u64 at = rec0 + rec_idx[i], coff = cig0 + cig_idx[i];
        samc::parse_line(text.data() + start, ln, M, T, R, o.cigar + coff);
        o.tid[at] = R.tid; o.pos[at] = R.pos; o.mtid[at] = R.mtid; o.flag[at] = (uint16_t)R.flag; o.mapq[at] = (uint8_t)R.mapq; o.nm[at] = R.nm; o.nm_kind[at] = (uint8_t)R.nm_kind;
        o.l_seq[at] = R.l_seq; o.cigar_off[at] = (u32)coff;
        if (o.qh1) { u64 k1; u32 k2; samc::qname_hash(text.data() + start, R, k1, k2); o.qh1[at] = k1; o.qh2[at] = k2; }
    }
    o.n_rec += r; o.n_cig += c;
    return true;
}

}  // namespace

extern "C" {

u32 samc_host_table_size(u32 n_names) { return samc::table_size(n_names); }
void samc_host_hash_many(const uint8_t *blob, const u64 *off, u32 n, u32 *out) { for (u32 i = 0; i < n; i++) out[i] = samc::name_hash32(blob + off[i], (u32)(off[i + 1] - off[i])); }
// covn::name_hash of every name, as the BAM record extraction calls it: on the name's bytes where they lie, at any alignment (8 readable
// bytes behind the blob)
void samc_host_name_hash_many(const uint8_t *blob, const u64 *off, u32 n, u64 *k1, u32 *k2) { for (u32 i = 0; i < n; i++) covn::name_hash(blob + off[i], (u32)(off[i + 1] - off[i]), k1[i], k2[i]); }
// tid of every query name through a table built over (blob, off, n_names)
void samc_host_lookup(const uint8_t *blob, const u64 *off, u32 n_names, const uint8_t *qblob, const u64 *qoff, u32 n_q, int32_t *out) {
    const u32 size = samc::table_size(n_names);
    std::vector<u32> slots(size, 0u);
    for (u32 i = 0; i < n_names; i++) samc::table_insert(slots.data(), size - 1u, blob, off, i);
    const samc::Table T{slots.data(), size - 1u, blob, off};
    for (u32 i = 0; i < n_q; i++) out[i] = samc::table_find(T, qblob + qoff[i], (u32)(qoff[i + 1] - qoff[i]));
}

// The whole text (header lines included).  0 = decoded; else the error code, *err_line = its 1-based line.
int samc_host_decode(const uint8_t *text, u64 n, const uint8_t *blob, const u64 *off, u32 n_names, u64 window, int staged, int32_t *tid, int32_t *pos, int32_t *mtid,
                     uint16_t *flag, uint8_t *mapq, uint8_t *nm_kind, u32 *nm, u32 *l_seq, u32 *cigar_off, u32 *cigar, u64 *qh1, u32 *qh2, u64 *n_rec, u64 *n_cig, u64 *err_line) {
    const u32 size = samc::table_size(n_names);
    std::vector<u32> slots(size, 0u);
    for (u32 i = 0; i < n_names; i++) samc::table_insert(slots.data(), size - 1u, blob, off, i);
    const samc::Table T{n_names ? slots.data() : nullptr, size - 1u, blob, off};
    Out o{tid, pos, mtid, flag, mapq, nm_kind, nm, l_seq, cigar_off, cigar, qh1, qh2};
    Err err;
    if (staged) {
        u64 at = 0, lines = 0; bool seen = false;
        while (at < n) {
            u64 len = n - at < window ? n - at : window;
            if (at + len < n) {      // the host driver's cut: behind the last '\n' of the piece
                u64 k = len;
                while (k && text[at + k - 1] != '\n') k--;
                if (!k) { err.line = lines + 1; err.code = samc::ERR_LINE_LONG; break; }
                len = k;
            }
            u64 nl = 0;
            if (!window_staged(text + at, len, T, o, lines, seen, err, nl)) break;
            lines += nl; at += len;
        }
    } else {
        u64 at = 0, line = 0; bool seen = false;
        std::vector<u32> words;
        while (at < n && !err.code) {
            const uint8_t *nlp = (const uint8_t *)memchr(text + at, '\n', n - at);
            const u64 end = nlp ? (u64)(nlp - text) : n;
            line++;
            const u32 ln = samc::trim_cr(text + at, (u32)(end - at));
            const uint8_t *p = text + at;
            at = nlp ? end + 1 : n;
            if (!ln) continue;
            if (p[0] == '@') { if (seen) { err.line = line; err.code = 4u; } continue; }
            const samc::ByteTabs B{p, ln};
            const samc::LineCount c = samc::count_line(p, ln, B);
            if (c.err) { err.line = line; err.code = c.err; break; }
            seen = true;
            words.resize(c.n_cigar + 1);
            samc::Rec R;
            samc::parse_line(p, ln, B, T, R, words.data());
            emit(o, R, words.data(), p);
        }
    }
    o.cigar_off[o.n_rec] = (u32)o.n_cig;
    *n_rec = o.n_rec; *n_cig = o.n_cig; *err_line = err.line;
    return (int)err.code;
}

}  // extern "C"

// Host instantiation of csrc/ingest_plan_core.h beside what the device ingest's driver carried before its arithmetic had one owner: the loop
// of cov_ingest_feed (validation, round_full, the three copy / upload / launch sites recorded as steps instead of executed), the window
// geometry of launch_round_, the first-window scale of ingest_drain_ and the if-chain of ingest_end_ with cov_ingest_end's wrapper — frozen
// here as they stood, session fields replaced by a plain struct.  Test infrastructure (tests/test_ingest_plan_core.py builds it with g++,
// as a library for the comparisons and as a program — main below walks the same grids — for a run under the sanitizers); not part of the
// product.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../coverm_amd/csrc/ingest_plan_core.h"

typedef unsigned int u32;
typedef unsigned long long u64;
using ingplan::Step;

struct Block { u64 in_off, out_off; u32 in_len, isize; };

static bool same(const Step &x, const Step &y) {
    return x.kind == y.kind && x.round == y.round && x.n == y.n && x.a == y.a && x.b == y.b && x.origin == y.origin;
}

// ------------------------------------------------------------------------------------------------ cov_ingest_feed's loop, frozen
struct FrozenSession {
    u64 ing_round_start = 0, ing_prev_end = 0, ing_ccap = 0, ing_infl = 0, ing_blocks = 0;
    u32 ing_round_n = 0, ing_batch = 0, round_blocks = 0;
    bool ing_fed_any = false;
    std::vector<Step> steps;
    void copy_range(u32 r, u64 origin, u64 a, u64 b) { if (b <= a) return; steps.push_back(Step{Step::COPY, r, 0u, a, b, origin}); }      // ingest_copy_range
    void upload_table(u64 from) { steps.push_back(Step{Step::UPLOAD, 0u, 0u, from, ing_blocks, 0}); }                                 // ingest_upload_table
    void launch_round(u32 n) { steps.push_back(Step{Step::LAUNCH, ing_batch, n, 0, 0, ing_round_start}); ing_batch++; }               // launch_round reads ing_round_start
};
static bool frozen_feed(FrozenSession *s, u64 file_offset, u64 n_bytes, const Block *blocks, u32 n_blocks) {
    if (!s->ing_fed_any) { s->ing_fed_any = true; s->ing_round_start = file_offset; s->ing_prev_end = file_offset; }
    const u64 piece_end = file_offset + n_bytes;
    u64 cursor = file_offset, tbl_from = s->ing_blocks;
    auto round_full = [&](u64 proxy) { return s->ing_round_n > 0 && (s->ing_round_n >= s->round_blocks || proxy + 65536u + 64u - s->ing_round_start > s->ing_ccap); };
    for (uint32_t i = 0; i < n_blocks; i++) {
        const Block &b = blocks[i];
        if (b.in_off < s->ing_prev_end || b.in_off + b.in_len > piece_end || b.isize > 65536u || b.in_len > 65536u || b.out_off != s->ing_infl) return false;
        const u64 proxy = s->ing_prev_end;
        if (round_full(proxy)) {
            if (proxy > cursor) { s->copy_range(s->ing_batch, s->ing_round_start, cursor, proxy); cursor = proxy; }
            { s->upload_table(tbl_from); tbl_from = s->ing_blocks; }
            s->launch_round(s->ing_round_n);
            s->ing_round_start = proxy; s->ing_round_n = 0;
        }
        s->ing_blocks++; s->ing_round_n++;
        s->ing_prev_end = b.in_off + b.in_len; s->ing_infl = b.out_off + b.isize;
    }
    {
        const u64 proxy = s->ing_prev_end;
        if (round_full(proxy)) {
            const u64 cut = std::min(std::max(cursor, proxy), piece_end);
            s->copy_range(s->ing_batch, s->ing_round_start, cursor, cut);
            s->copy_range(s->ing_batch + 1u, proxy, cut, piece_end);
        } else {
            s->copy_range(s->ing_batch, s->ing_round_start, cursor, piece_end);
        }
    }
    s->upload_table(tbl_from);
    return true;
}

// ------------------------------------------------------------------------------------------------ a file of BGZF blocks, fed in pieces
// Block = 18 header bytes, payload, 8 trailer bytes; the table entry points at the payload.  sizes: 0 = 90 B, 1 = 700 B, 2 = 0xFF00 B, 3 = a mix.
static u32 payload_of(int sizes, u64 i) {
    static const u32 mix[7] = {90, 0xFF00, 700, 700, 90, 0xFF00, 90};
    return sizes == 0 ? 90u : sizes == 1 ? 700u : sizes == 2 ? 0xFF00u : mix[(i * 2654435761ull >> 7) % 7];
}
enum Corrupt { NONE = 0, OUT_OF_ORDER, BEYOND_PIECE, ISIZE_LARGE, LEN_LARGE, NOT_CONTIGUOUS };
enum Broken : u32 {      // bits of feed_case's verdict
    B_STEPS_DIFFER = 1, B_REJECT_DIFFERS = 2, B_BYTE_NOT_ONCE = 4, B_COPY_OUTSIDE = 8, B_BLOCK_IN_WRONG_ROUND = 16, B_BLOCK_SUM = 32, B_ROUND_TOO_LONG = 64,
    B_ORDER = 128, B_STATE_DIFFERS = 256, B_NOT_REJECTED = 512,
};

// out: [0] steps, [1] launches, [2] blocks accepted, [3] bytes fed, [4] pieces that ended inside a block opening the next round, [5] rejected (0 / 1)
extern "C" u32 ingplan_feed_case(int sizes, u64 piece_bytes, u32 round_blocks, u64 ccap, int mid_start, int corrupt, u64 *out) {
    const u64 n_all = 3ull * round_blocks + 17, skip = mid_start ? round_blocks / 2 + 3 : 0;
    std::vector<Block> file;
    u64 off = 0, infl = 0, span_off = 0;
    for (u64 i = 0; i < n_all; i++) {
        const u32 len = payload_of(sizes, i);
        if (i == skip) span_off = off;
        if (i >= skip) { file.push_back(Block{off + 18, infl, len, len}); infl += len; }
        off += 18ull + len + 8;
    }
    const u64 file_end = off + 28;      // (the EOF block's bytes follow, untabled)
    std::vector<u64> ends;      // where each payload really ends: the feeder tables a block with the piece that holds its last byte
    for (const Block &b : file) ends.push_back(b.in_off + b.in_len);
    const u64 bad_at = corrupt ? file.size() / 2 + 1 : ~0ull;
    if (corrupt == OUT_OF_ORDER) std::swap(file[bad_at], file[bad_at - 1]);
    if (corrupt == ISIZE_LARGE) file[bad_at].isize = 65537;
    if (corrupt == LEN_LARGE) file[bad_at].in_len = 65537;
    if (corrupt == NOT_CONTIGUOUS) file[bad_at].out_off += 1;

    ingplan::FeedState st; const ingplan::FeedRule rule{round_blocks, ccap};
    FrozenSession fs; fs.round_blocks = round_blocks; fs.ing_ccap = ccap;
    std::vector<Step> steps;
    u32 rounds = 0, broken = 0;
    u64 next_block = 0, straddles = 0, rejected = 0;
    const u64 piece = piece_bytes ? piece_bytes : file_end - span_off;
    for (u64 lo = span_off; lo < file_end && !rejected; lo += piece) {
        u64 hi = std::min(file_end, lo + piece);
        u64 e = next_block;
        while (e < file.size() && ends[e] <= hi) e++;
        if (corrupt == BEYOND_PIECE && next_block <= bad_at && bad_at < e) {      // the piece is cut inside the block's payload, its entry comes all the same
            hi = std::max(lo + 1, ends[bad_at] - 40); e = bad_at + 1;
        }
        const size_t s0 = steps.size();
        const bool ok_new = ingplan::feed_plan(st, rule, rounds, lo, hi - lo, file.data() + next_block, (u32)(e - next_block), [&](const Step &x) { steps.push_back(x); });
        const bool ok_old = frozen_feed(&fs, lo, hi - lo, file.data() + next_block, (u32)(e - next_block));
        for (size_t k = s0; k < steps.size(); k++) if (steps[k].kind == Step::LAUNCH) rounds++;
        if (ok_new != ok_old) broken |= B_REJECT_DIFFERS;
        if (!ok_new || !ok_old) { rejected = 1; break; }
        if (e < file.size() && file[e].in_off - 18 < hi && ingplan::round_full(st, rule, st.prev_end)) straddles++;
        next_block = e;
    }
    if (steps.size() != fs.steps.size()) broken |= B_STEPS_DIFFER;
    else for (size_t k = 0; k < steps.size(); k++) if (!same(steps[k], fs.steps[k])) broken |= B_STEPS_DIFFER;
    if (st.round_start != fs.ing_round_start || st.prev_end != fs.ing_prev_end || st.infl != fs.ing_infl || st.blocks != fs.ing_blocks || st.round_n != fs.ing_round_n ||
        rounds != fs.ing_batch) broken |= B_STATE_DIFFERS;
    if (corrupt && !rejected) broken |= B_NOT_REJECTED;
    if (!corrupt && rejected) broken |= B_REJECT_DIFFERS;

    if (out) { out[0] = steps.size(); out[2] = st.blocks; out[4] = straddles; out[5] = rejected; }
    if (rejected) return broken;
    // ---- the properties of an accepted file, from the new planner's steps alone
    std::vector<u64> round_first(1, 0), round_origin;      // first block of round r; origin of round r's buffer
    u64 next_byte = span_off, uploaded = 0, launched = 0, launches = 0;
    for (const Step &x : steps) {
        if (x.kind == Step::COPY) {
            if (x.a != next_byte || x.b <= x.a) broken |= B_BYTE_NOT_ONCE;
            next_byte = x.b;
            if (x.a < x.origin || x.b - x.origin > ccap + 2 * 65536u + 256u) broken |= B_COPY_OUTSIDE;
            if (x.round != launches && x.round != launches + 1) broken |= B_ORDER;      // the open round, or the one the cut block will open
        } else if (x.kind == Step::UPLOAD) {
            if (x.a != uploaded || x.b < x.a) broken |= B_ORDER;
            uploaded = x.b;
        } else {
            if (x.round != launches || x.n == 0) broken |= B_ORDER;
            if (x.n > round_blocks) broken |= B_ROUND_TOO_LONG;
            if (uploaded < launched + x.n) broken |= B_ORDER;                                                                  // its table entries are on their way
            const Block &last = file[launched + x.n - 1];
            if (next_byte < last.in_off + last.in_len) broken |= B_ORDER;                                                      // and so are its bytes
            launched += x.n; launches++;
            round_first.push_back(launched); round_origin.push_back(x.origin);
        }
    }
    round_origin.push_back(st.round_start);      // the open round: cov_ingest_end launches it with the state's origin
    if (st.round_n > round_blocks) broken |= B_ROUND_TOO_LONG;
    if (launched + st.round_n != st.blocks || st.blocks != file.size() || uploaded != st.blocks) broken |= B_BLOCK_SUM;
    if (next_byte != file_end) broken |= B_BYTE_NOT_ONCE;
    {   // every byte of a block's payload lies in a copy made for the round whose launch contains the block, at that round's origin
        size_t c = 0; u64 r = 0;
        for (u64 i = 0; i < st.blocks; i++) {
            while (r + 1 < round_first.size() && i >= round_first[r + 1]) r++;
            u64 p = file[i].in_off; const u64 pe = p + file[i].in_len;
            while (p < pe) {
                while (c < steps.size() && (steps[c].kind != Step::COPY || steps[c].b <= p)) c++;
                if (c == steps.size() || steps[c].a > p) { broken |= B_BYTE_NOT_ONCE; break; }
                if (steps[c].round != r || steps[c].origin != round_origin[r]) broken |= B_BLOCK_IN_WRONG_ROUND;
                p = std::min(pe, steps[c].b);
            }
        }
    }
    if (out) { out[1] = launches; out[3] = next_byte - span_off; }
    return broken;
}

// ------------------------------------------------------------------------------------------------ geometry and first-window scale, frozen
struct Geometry { u64 est_blocks, full, win_bytes, seg_cap, scr, tok; };
static Geometry frozen_geometry(u64 ing_span_lo, u64 ing_span_hi, u32 n, u32 round_blocks, u64 carry, size_t INF_SCRATCH_BYTES, size_t INF_TOK_CAP) {
    const size_t est_blocks = (size_t)((ing_span_hi - std::min(ing_span_lo, ing_span_hi)) / 4096u + 256u);
    const size_t full = std::max<size_t>(n, std::min<size_t>(round_blocks, est_blocks));
    const size_t win_bytes = (size_t)carry + full * 65536u + 64u;
    const u32 seg_cap = (u32)((win_bytes + 32767u) / 32768u);
    const size_t scr = (full + 63) / 64 * 64u * INF_SCRATCH_BYTES;
    return Geometry{est_blocks, full, win_bytes, seg_cap, scr, full * INF_TOK_CAP};
}
static double frozen_scale(u64 comp_end, u64 ing_span_lo, u64 ing_span_hi) {
    double scale = 0;
    if (comp_end && comp_end + 65536u < ing_span_hi)
        scale = (double)(ing_span_hi - ing_span_lo) / (double)std::max<u64>(1, comp_end - std::min<u64>(comp_end, ing_span_lo)) * 1.1;
    return scale;
}
extern "C" int ingplan_geometry_differs(u64 span_lo, u64 span_hi, u32 n, u32 round_blocks, u64 carry, u64 scratch_per_block, u64 tok_per_block, u64 *out) {
    const ingplan::WindowGeometry g = ingplan::window_geometry(span_lo, span_hi, n, round_blocks, carry, (size_t)scratch_per_block, (size_t)tok_per_block);
    const Geometry f = frozen_geometry(span_lo, span_hi, n, round_blocks, carry, (size_t)scratch_per_block, (size_t)tok_per_block);
    if (out) { out[0] = g.est_blocks; out[1] = g.full; out[2] = g.win_bytes; out[3] = g.seg_cap; out[4] = g.scratch_bytes; out[5] = g.tok_cap; }
    return !(g.est_blocks == f.est_blocks && g.full == f.full && g.win_bytes == f.win_bytes && g.seg_cap == f.seg_cap && g.scratch_bytes == f.scr && g.tok_cap == f.tok);
}
extern "C" u64 ingplan_header_left(u64 first_record, u64 out_off0) { return ingplan::header_left(first_record, out_off0); }
extern "C" double ingplan_scale(u64 comp_end, u64 span_lo, u64 span_hi) { return ingplan::first_window_scale(comp_end, span_lo, span_hi); }
extern "C" double ingplan_scale_frozen(u64 comp_end, u64 span_lo, u64 span_hi) { return frozen_scale(comp_end, span_lo, span_hi); }

// ------------------------------------------------------------------------------------------------ ingest_end_'s if-chain, frozen
// A verdict as two small numbers: which text (the Outcome's number; the frozen chain names its texts by the same numbers), which status
// (0 COV_OK, 1 COV_ERR_INGEST_FALLBACK, 2 COV_ERR_INVALID_ARG, 3 COV_ERR_UNSORTED, 4 COV_ERR_STATE with the "had left the store" suffix).
struct EndCase { u32 ing_fail, inflate_fail, extract_fail; long long ing_key_lo, ing_key_hi; bool ing_search_first, ing_open_end; u64 ing_tail_key, prev_key_word; bool spilled; };
static u32 frozen_end_(const EndCase &s, u32 *text) {
    const u64 glob3 = (u64)s.inflate_fail | ((u64)s.extract_fail << 32), glob7 = s.prev_key_word;
    const u32 inflate_fail = (u32)(glob3 & 0xffffffffu);
    if (inflate_fail) { *text = ingplan::INFLATE_FAILED; return 1; }
    if (s.ing_fail) {
        const u32 f = s.ing_fail;
        const bool span = s.ing_key_lo > 0 || s.ing_key_hi < 0x80000000ll || s.ing_search_first || s.ing_open_end;
        if ((f & 64u) && !span) { *text = ingplan::DISORDER_FILE; return 1; }
        if (f & 64u) { *text = ingplan::UNSORTED; return 3; }
        *text = (f & 16u) ? ingplan::PAST_LIMIT : (f & 32u) ? ingplan::HEADER_LONG : (f & 4u) ? ingplan::CG_CIGAR : (f & 8u) ? ingplan::TAIL_LARGE : (f & 2u) ? ingplan::TRUNCATED : ingplan::CHAIN;
        return (f & 16u) ? 2 : 1;
    }
    if ((u32)(glob3 >> 32)) { *text = ingplan::CORRUPT_RECORD; return 1; }
    if (s.ing_open_end && s.ing_tail_key != ~0ull && (long long)s.ing_tail_key < s.ing_key_hi) { *text = ingplan::SPAN_CUTS_RECORD; return 1; }
    if (s.ing_open_end) {
        const bool seen_beyond = ((glob7 >> 63) && (long long)(u32)glob7 >= s.ing_key_hi) || (s.ing_tail_key != ~0ull && (long long)s.ing_tail_key >= s.ing_key_hi);
        if (!seen_beyond) { *text = ingplan::SPAN_END_UNSEEN; return 1; }
    }
    *text = ingplan::COMMIT;
    return 0;
}
static u32 frozen_end(const EndCase &s, u32 *text) {      // cov_ingest_end around ingest_end_
    const u32 rc = frozen_end_(s, text);
    if (s.spilled && rc == 1) return 4;
    return rc;
}
static u32 new_end(const EndCase &s, u32 *text) {
    ingplan::EndFacts f;
    f.fail = s.ing_fail; f.inflate_failures = ingplan::inflate_failures((u64)s.inflate_fail | ((u64)s.extract_fail << 32));
    f.extract_failures = ingplan::extract_failures((u64)s.inflate_fail | ((u64)s.extract_fail << 32));
    f.span = ingplan::is_span(s.ing_key_lo, s.ing_key_hi, s.ing_search_first, s.ing_open_end); f.open_end = s.ing_open_end;
    f.tail_key = s.ing_tail_key; f.prev_key = s.prev_key_word; f.key_hi = s.ing_key_hi; f.spilled = s.spilled;
    const ingplan::Outcome o = ingplan::outcome(f);
    *text = o;
    switch (ingplan::ending(o, f.spilled)) {
    case ingplan::END_OK: return 0;
    case ingplan::END_HAND_BACK: return 1;
    case ingplan::END_INVALID: return 2;
    case ingplan::END_UNSORTED: return 3;
    default: return 4;
    }
}
// text | status << 8
extern "C" u32 ingplan_end(u32 fail, u32 inflate_fail, u32 extract_fail, long long key_lo, long long key_hi, int search_first, int open_end, u64 tail_key, u64 prev_key, int spilled, int frozen) {
    const EndCase c{fail, inflate_fail, extract_fail, key_lo, key_hi, search_first != 0, open_end != 0, tail_key, prev_key, spilled != 0};
    u32 text = 0; const u32 st = frozen ? frozen_end(c, &text) : new_end(c, &text);
    return text | st << 8;
}
extern "C" int ingplan_is_span(long long key_lo, long long key_hi, int search_first, int open_end) { return ingplan::is_span(key_lo, key_hi, search_first != 0, open_end != 0) ? 1 : 0; }

// ------------------------------------------------------------------------------------------------ the rings, for the Python side
extern "C" void ingplan_rings(u32 *out) {
    out[0] = ingplan::CWIN_RING; out[1] = ingplan::WIN_RING; out[2] = ingplan::PARSE_RING; out[3] = ingplan::TOK_RING; out[4] = ingplan::G_WORDS; out[5] = ingplan::WIN_RESULT_WORDS;
}
extern "C" u32 ingplan_slot(int ring, u32 w) { return ring == 0 ? ingplan::cwin_slot(w) : ring == 1 ? ingplan::win_slot(w) : ring == 2 ? ingplan::parse_slot(w) : ingplan::tok_slot(w); }
extern "C" int ingplan_reused(int ring, u32 w) { return ring == 0 ? ingplan::cwin_reused(w) : ring == 1 ? ingplan::win_reused(w) : ingplan::tok_reused(w); }
extern "C" long long ingplan_extracted_before_launch(u32 w) { return ingplan::extracted_before_launch(w); }

// ------------------------------------------------------------------------------------------------ the same grids, as a program
int main() {
    u64 n = 0, bad = 0;
    const u64 pieces[] = {65536, 200 * 1024, 0};
    const u32 rbs[] = {64, 128, 4096};
    for (int sizes = 0; sizes < 4; sizes++) for (u64 piece : pieces) for (u32 rb : rbs) for (int bytes_rule = 0; bytes_rule < 2; bytes_rule++) for (int mid = 0; mid < 2; mid++) {
        const u64 ccap = bytes_rule ? 256 * 1024 : (u64)rb * 65536u * 2;
        for (int corrupt = 0; corrupt <= NOT_CONTIGUOUS; corrupt++) {
            if (corrupt && (rb == 4096 || mid)) continue;      // (the rejections need no large case)
            if (ingplan_feed_case(sizes, piece, rb, ccap, mid, corrupt, nullptr)) bad++;
            n++;
        }
    }
    const u64 spans[][2] = {{0, 1000}, {0, 3ull << 20}, {0, 200ull << 20}, {5ull << 30, 25ull << 30}, {7, 7}, {9, 3}};
    for (auto &sp : spans) for (u32 rb : {64u, 4096u, 61440u}) for (u32 nb : {0u, 1u, rb - 1, rb, rb + 1}) for (u64 carry : {65536ull, 16ull << 20}) {
        if (ingplan_geometry_differs(sp[0], sp[1], nb, rb, carry, 2048, 16384, nullptr)) bad++;
        for (u64 comp_end : {0ull, 1ull, sp[0], sp[0] + 70000, sp[1] - std::min<u64>(sp[1], 65536), sp[1]})
            if (sp[1] >= sp[0] && ingplan::first_window_scale(comp_end, sp[0], sp[1]) != frozen_scale(comp_end, sp[0], sp[1])) bad++;
        n++;
    }
    for (u32 bits = 0; bits < 128; bits++) {
        const u32 fail = (bits & 31u) | ((bits & 32u) ? 32u : 0u) | ((bits & 64u) ? 64u : 0u);
        for (u32 c = 0; c < 2 * 2 * 16 * 3 * 3 * 2; c++, n++) {
            u32 x = c;
            const u32 inf = (x & 1) ? 5 : 0; x >>= 1; const u32 ext = (x & 1) ? 7 : 0; x >>= 1;
            const long long key_lo = (x & 1) ? 5 : 0; x >>= 1; const long long key_hi = (x & 1) ? 100 : 0x80000000ll; x >>= 1;
            const bool sf = x & 1; x >>= 1; const bool oe = x & 1; x >>= 1;
            const u64 tails[3] = {~0ull, 50, 0x80000000ull}, prevs[3] = {99, (1ull << 63) | 50, (1ull << 63) | 0x80000000ull};
            const u64 tail = tails[x % 3]; x /= 3; const u64 prev = prevs[x % 3]; x /= 3;
            const EndCase e{fail, inf, ext, key_lo, key_hi, sf, oe, tail, prev, (x & 1) != 0};
            u32 t0 = 0, t1 = 0;
            if (frozen_end(e, &t0) != new_end(e, &t1) || t0 != t1) bad++;
        }
    }
    printf("%llu cases, %llu bad\n", n, bad);
    return bad ? 1 : 0;
}

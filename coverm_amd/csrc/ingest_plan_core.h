// The device side of the BGZF ingest (cov_ingest_* in covermhip.hip) as arithmetic: the rings its rounds turn in, the words the device
// reports through, which bytes of a fed piece go to which round, the sizes of a window's buffers, and the verdict of a finished ingest.
// Plain C++, no HIP: the host code and ingest_kernels.hip.h include it, and tests/c/ingest_plan_host.cpp runs it on the CPU against the
// loops and expressions cov_ingest_feed, launch_round_, ingest_drain_ and ingest_end_ carried while each took its decisions in place.
#pragma once
#include <stddef.h>

namespace ingplan {
typedef unsigned int u32;
typedef unsigned long long u64;

// ---------------------------------------------------------------------------------------------------------------------------------- rings
// One round = one k_inflate launch = one window of the inflated stream; rounds and windows share their number w = 0, 1, 2, ...
constexpr u32 CWIN_RING = 3;       // compressed buffers: the copy stream fills round r + 1 (and the head of r + 2) while k_inflate reads round r
constexpr u32 WIN_RING = 3;        // inflated windows [carry area | blocks]
constexpr u32 PARSE_RING = 4;      // parse-state sets (segments, record / CIGAR bases), result blocks, verify events
constexpr u32 TOK_RING = 2;        // token lists, inflate / LZ events: k_lz of round w runs beside k_inflate of round w + 1
// The extraction of window w may run up to WIN_RING windows later (the launch of window w + WIN_RING is what forces it), so its parse
// state and its result block must not share a slot with any window launched meanwhile, nor with window w + WIN_RING itself, whose set
// is sized while w's extraction may still be queued.
static_assert(PARSE_RING > WIN_RING, "the parse-state ring must be deeper than the window ring");

constexpr u32 cwin_slot(u32 r) { return r % CWIN_RING; }
constexpr u32 win_slot(u32 w) { return w % WIN_RING; }
constexpr u32 parse_slot(u32 w) { return w % PARSE_RING; }
constexpr u32 tok_slot(u32 w) { return w % TOK_RING; }

// Reuse distances.  "Window w may be written once window w - WIN_RING is extracted": true from the first window that has such a predecessor.
constexpr bool win_reused(u32 w) { return w >= WIN_RING; }        // k_inflate / k_carry_in of w wait for the extraction of w - WIN_RING
constexpr bool tok_reused(u32 w) { return w >= TOK_RING; }        // k_inflate of w waits for the k_lz that read the token list of w - TOK_RING
constexpr bool cwin_reused(u32 r) { return r >= CWIN_RING; }      // the upload of round r waits for the k_inflate of round r - CWIN_RING
// Before window w is launched every window up to this one must be extracted, waiting for its verification if need be (-1: none).
constexpr long long extracted_before_launch(u32 w) { return win_reused(w) ? (long long)w - (long long)WIN_RING : -1; }

// ----------------------------------------------------------------------------------------------------------------- device result words
// g_result, u64 words.  The first G_WINDOWS are the ingest's own, behind them one block of WIN_RESULT_WORDS per parse slot.
enum GlobalWord : u32 {
    G_FAILURES = 3,       // two u32 counters: [FAIL_INFLATE] blocks that failed to inflate or their CRC-32, [FAIL_EXTRACT] corrupt records met by k_bam_extract
    G_LONG = 4,           // entries in the long-record list (u32, zeroed in front of every k_bam_extract that has long records)
    G_CARRY_LEN = 5,      // bytes in the carry buffer: the tail of the window verified last
    G_P0 = 6,             // offset of the first record of the window being parsed
    G_PREV_KEY = 7,       // key of the last record of the previous window (bit 63: there is one)
    G_WINDOWS = 8,        // result block of window w at G_WINDOWS + WIN_RESULT_WORDS * parse_slot(w)
};
constexpr u32 FAIL_INFLATE = 0, FAIL_EXTRACT = 1;      // u32 halves of G_FAILURES
constexpr u32 inflate_failures(u64 word) { return (u32)(word & 0xffffffffu); }
constexpr u32 extract_failures(u64 word) { return (u32)(word >> 32); }

// A window's result block, written by k_bam_verify and copied to the host behind it.
constexpr u32 WIN_RESULT_WORDS = 12;
enum WinWord : u32 {
    W_RECORDS = 0,        // records of this window (of the span's key range)
    W_CIGAR = 1,          // their CIGAR words
    W_STATUS = 2,         // Status bits, 0 = ok
    W_TAIL = 3,           // offset where the tail starts: the first byte no record of this window owns; [W_TAIL, N) goes to the carry buffer
    W_BAD_SEG = 4,        // first bad segment,
    W_BAD_START = 5,      // its start,
    W_BAD_LANDED = 6,     // and where its hop landed
    W_TAIL_KEY = 7,       // key of the record the tail begins with (~0: no tail, or its tid is not here yet)
    W_LONG = 8,           // long records (k_bam_extract_long's list entries)
    W_REPAIRED = 9,       // starts dropped by the repair
    W_MAX_HOP = 10,       // most records one hop went over
    W_LIVE_SEGS = 11,     // segments with a start
};
static_assert(W_LIVE_SEGS + 1 == WIN_RESULT_WORDS, "every word of a window's result block is named");
constexpr u32 G_WORDS = G_WINDOWS + PARSE_RING * WIN_RESULT_WORDS;
constexpr u32 win_result_at(u32 w) { return G_WINDOWS + WIN_RESULT_WORDS * parse_slot(w); }

// W_STATUS, and the session's sticky failure (the first window's status that was not 0).
enum Status : u32 {
    ST_CHAIN = 1,         // record boundaries did not verify: a hop did not land on the next live segment's start (after the repair's budget)
    ST_TRUNCATED = 2,     // the last window ends inside a record
    ST_CG_CIGAR = 4,      // a record needs the CPU reader (its CIGAR in CG:B,I; the extraction resolves those itself now, the bit is kept)
    ST_TAIL_LARGE = 8,    // the tail is larger than the carry buffer
    ST_PAST_LIMIT = 16,   // host: the window does not fit the store's 32-bit indices
    ST_HEADER_LONG = 32,  // host: the BAM header does not end inside the fed stream (it may run over the first windows)
    ST_DISORDER = 64,     // record keys (tid) decrease somewhere in the window — looked at for spans only: a span trusts the file's order when it
                          // drops its neighbours' records, the whole-file path reports disorder from cov_finish in file order with the other
                          // per-record errors
};

// Records outside [key_lo, key_hi), a searched first record or an open end: the ingest takes one span of a file, not the whole of it.
constexpr long long KEY_END = 0x80000000ll;
constexpr bool is_span(long long key_lo, long long key_hi, bool search_first, bool open_end) {
    return key_lo > 0 || key_hi < KEY_END || search_first || open_end;
}

// ------------------------------------------------------------------------------------------------------------------------ the feed plan
// A round closes when it holds as many blocks as the rule allows, or when the next block might no longer fit its compressed buffer.  The
// decision only looks at where the previous payload ended, so the bytes of a block that is still incomplete at the end of a piece already
// go to the buffer of the round the block will join.
struct FeedState {
    u64 round_start = 0;      // file offset the open round's compressed buffer starts at
    u64 prev_end = 0;         // end of the last payload seen
    u64 infl = 0;             // inflated bytes of the blocks so far
    u64 blocks = 0;           // blocks so far
    u32 round_n = 0;          // blocks of the open round
    bool fed_any = false;
};
struct FeedRule { u32 round_blocks = 0; u64 ccap = 0; };      // blocks / compressed bytes a round may span
constexpr u64 CWIN_SLACK = 2 * 65536u + 256u;                 // a compressed buffer holds ccap + CWIN_SLACK bytes
constexpr u64 cwin_bytes(u64 ccap) { return ccap + CWIN_SLACK; }

struct Step {
    enum Kind : u32 { COPY, UPLOAD, LAUNCH } kind;
    u32 round;      // COPY, LAUNCH
    u32 n;          // LAUNCH: blocks of the round
    u64 a, b;       // COPY: file bytes [a, b); UPLOAD: table entries [a, b) (possibly none: the "fed" mark is still due)
    u64 origin;     // COPY, LAUNCH: file offset of the first byte of the round's compressed buffer
};

inline bool round_full(const FeedState &st, const FeedRule &rule, u64 proxy) {
    return st.round_n > 0 && (st.round_n >= rule.round_blocks || proxy + 65536u + 64u - st.round_start > rule.ccap);
}
template <class Block>
inline bool block_ok(const FeedState &st, const Block &b, u64 piece_end) {
    return !(b.in_off < st.prev_end || b.in_off + b.in_len > piece_end || b.isize > 65536u || b.in_len > 65536u || b.out_off != st.infl);
}

// One piece: file bytes [file_offset, file_offset + n_bytes) and the table entries of the blocks that END inside it.  `rounds` = rounds
// launched so far.  The steps go to sink(const Step &) in the order the streams must see them; the state advances over the whole piece.
// false: block st.blocks - (blocks on entry) of the piece is outside the bytes fed so far, out of order, or not contiguous in the inflated
// stream — the steps of the blocks in front of it have been emitted, nothing for the rest of the piece.
template <class Block, class Sink>
inline bool feed_plan(FeedState &st, const FeedRule &rule, u32 rounds, u64 file_offset, u64 n_bytes, const Block *blocks, u32 n_blocks, Sink &&sink) {
    if (!st.fed_any) { st.fed_any = true; st.round_start = file_offset; st.prev_end = file_offset; }      // a span starts somewhere inside the file
    const u64 piece_end = file_offset + n_bytes;
    u64 cursor = file_offset, tbl_from = st.blocks;
    auto copy = [&](u32 r, u64 origin, u64 a, u64 b) { if (b > a) sink(Step{Step::COPY, r, 0u, a, b, origin}); };
    for (u32 i = 0; i < n_blocks; i++) {
        const Block &b = blocks[i];
        if (!block_ok(st, b, piece_end)) return false;
        const u64 proxy = st.prev_end;
        if (round_full(st, rule, proxy)) {
            if (proxy > cursor) { copy(rounds, st.round_start, cursor, proxy); cursor = proxy; }
            sink(Step{Step::UPLOAD, 0u, 0u, tbl_from, st.blocks, 0}); tbl_from = st.blocks;
            sink(Step{Step::LAUNCH, rounds, st.round_n, 0, 0, st.round_start}); rounds++;
            st.round_start = proxy; st.round_n = 0;
        }
        st.blocks++; st.round_n++;
        st.prev_end = b.in_off + b.in_len; st.infl = b.out_off + b.isize;
    }
    {   // what is left of the piece: the rest of the open round, and the beginning of a block that may open the next one
        const u64 proxy = st.prev_end;
        if (round_full(st, rule, proxy)) {
            const u64 lo = cursor > proxy ? cursor : proxy, cut = lo < piece_end ? lo : piece_end;
            copy(rounds, st.round_start, cursor, cut);
            copy(rounds + 1u, proxy, cut, piece_end);
        } else copy(rounds, st.round_start, cursor, piece_end);
    }
    sink(Step{Step::UPLOAD, 0u, 0u, tbl_from, st.blocks, 0});
    return true;
}

// ------------------------------------------------------------------------------------------------------------------- window geometry
// Buffers are sized for a full round at once (no regrowth between rounds) — or for the blocks a SMALL file can be expected to have: a
// 200 MB file does not need three 4 GB windows and two 2.7 GB token lists.  The estimate is one block per 4 KiB of compressed bytes; a
// file of smaller blocks regrows.  n = blocks of the round at hand.
struct WindowGeometry {
    size_t est_blocks = 0;        // blocks the span's bytes are expected to hold
    size_t full = 0;              // blocks the buffers are sized for
    size_t win_bytes = 0;         // inflated window: carry area, `full` blocks of 64 KiB, 64 bytes of slack
    u32 seg_cap = 0;              // segments of 32 KiB in it: elements of each array of a parse-state set
    size_t scratch_bytes = 0;     // k_inflate's scratch
    size_t tok_cap = 0;           // tokens of one list (its count array holds `full` words)
};
constexpr u32 SEG_BYTES = 32768;
inline WindowGeometry window_geometry(u64 span_lo, u64 span_hi, u32 n, u32 round_blocks, u64 carry, size_t scratch_per_block, size_t tok_per_block) {
    WindowGeometry g;
    g.est_blocks = (size_t)((span_hi - (span_lo < span_hi ? span_lo : span_hi)) / 4096u + 256u);
    const size_t capped = (size_t)round_blocks < g.est_blocks ? (size_t)round_blocks : g.est_blocks;
    g.full = (size_t)n > capped ? (size_t)n : capped;
    g.win_bytes = (size_t)carry + g.full * 65536u + 64u;
    g.seg_cap = (u32)((g.win_bytes + SEG_BYTES - 1u) / SEG_BYTES);
    g.scratch_bytes = (g.full + 63) / 64 * 64u * scratch_per_block;
    g.tok_cap = g.full * tok_per_block;
    return g;
}

// Bytes of the BAM header that lie inside (or run beyond) the window whose first block begins at offset out_off0 of the inflated stream:
// k_carry_in puts the window's first record that far behind the carried tail.  first_record = where the records begin in the stream.
constexpr u64 header_left(u64 first_record, u64 out_off0) { return first_record > out_off0 ? first_record - out_off0 : 0; }

// Window 0 when it is the first of several (it ends in front of the span's end; not "several launched so far": window 0 may be verified
// before window 1 is launched): the whole span is this many times the window, for the store's one sizing (store_plan_core.h).  0: it is not.
// comp_end = file offset behind the window's last block.
inline double first_window_scale(u64 comp_end, u64 span_lo, u64 span_hi) {
    if (!comp_end || comp_end + 65536u >= span_hi) return 0;
    const u64 seen = comp_end - (comp_end < span_lo ? comp_end : span_lo);
    return (double)(span_hi - span_lo) / (double)(seen > 1 ? seen : 1) * 1.1;
}

// --------------------------------------------------------------------------------------------------------------------------- the verdict
// What cov_ingest_end makes of a drained ingest, in the order of precedence.
enum Outcome : u32 {
    COMMIT = 0,                 // the records become the store's content
    INFLATE_FAILED,             // blocks failed to inflate or their CRC-32
    DISORDER_FILE,              // keys decrease in a whole file whose mates were asked for: its pair filter runs on the host
    UNSORTED,                   // keys decrease inside a span: the reference's own error
    PAST_LIMIT, HEADER_LONG, CG_CIGAR, TAIL_LARGE, TRUNCATED, CHAIN,      // the sticky failure, by its highest-ranking bit
    CORRUPT_RECORD,             // k_bam_extract met a corrupt record
    SPAN_CUTS_RECORD,           // the bytes of an open-ended span end inside one of its own records
    SPAN_END_UNSEEN,            // ... or before any record from beyond the span was seen
};
// How an outcome ends the call: HAND_BACK = the file goes to the CPU reader (nothing was appended), LOST = it would, but part of the file
// had already left the bounded record store.
enum Ending : u32 { END_OK, END_HAND_BACK, END_INVALID, END_UNSORTED, END_LOST };
struct EndFacts {
    u32 fail = 0;                       // sticky Status bits
    u32 inflate_failures = 0, extract_failures = 0;
    bool span = false, open_end = false;
    u64 tail_key = ~0ull;               // W_TAIL_KEY of the last window
    u64 prev_key = 0;                   // G_PREV_KEY
    long long key_hi = KEY_END;
    bool spilled = false;               // records of this ingest already left the store
};
inline Outcome outcome(const EndFacts &f) {
    if (f.inflate_failures) return INFLATE_FAILED;
    if (f.fail) {
        if (f.fail & ST_DISORDER) return f.span ? UNSORTED : DISORDER_FILE;
        return (f.fail & ST_PAST_LIMIT) ? PAST_LIMIT : (f.fail & ST_HEADER_LONG) ? HEADER_LONG : (f.fail & ST_CG_CIGAR) ? CG_CIGAR
             : (f.fail & ST_TAIL_LARGE) ? TAIL_LARGE : (f.fail & ST_TRUNCATED) ? TRUNCATED : CHAIN;
    }
    if (f.extract_failures) return CORRUPT_RECORD;
    if (f.open_end) {
        const bool have_tail = f.tail_key != ~0ull;
        if (have_tail && (long long)f.tail_key < f.key_hi) return SPAN_CUTS_RECORD;
        // an open end is only trusted when a record from beyond the span was actually seen (complete, or cut by the end of the bytes):
        // otherwise the span's last records may lie behind the bytes that were fed
        const bool seen_beyond = ((f.prev_key >> 63) && (long long)(u32)f.prev_key >= f.key_hi) || (have_tail && (long long)f.tail_key >= f.key_hi);
        if (!seen_beyond) return SPAN_END_UNSEEN;
    }
    return COMMIT;
}
inline Ending ending(Outcome o, bool spilled) {
    if (o == COMMIT) return END_OK;
    if (o == UNSORTED) return END_UNSORTED;
    if (o == PAST_LIMIT) return END_INVALID;
    return spilled ? END_LOST : END_HAND_BACK;
}
}  // namespace ingplan

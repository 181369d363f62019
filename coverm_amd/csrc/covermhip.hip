// libcovermhip.so — session management and the C ABI declared in include/covermhip.h.
// Host code here only moves bytes and launches kernels; every statistic is computed on the device
// (pileup_kernels.hip.h).  There is deliberately no CPU fallback: without a usable HIP device every
// entry point fails with COV_ERR_HIP.
#include "pileup_kernels.hip.h"
#include "prep_lean.hip.h"
#include "genome_kernels.hip.h"
#include "sep_kernels.hip.h"
#include "ingest_kernels.hip.h"
#include "group_kernels.hip.h"
#include "sam_kernels.hip.h"
#include "gene_kernels.hip.h"
#include "depth_kernels.hip.h"
#include "depth_bins_kernels.hip.h"
#include "depth_regions_kernels.hip.h"

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <chrono>
#include <cstdio>
#include <dlfcn.h>
#include <functional>
#include <sched.h>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <future>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/covermhip.h"
#include "roctx_ranges.h"
#include "knobs.h"
#include "record_store.h"
#include "store_plan_core.h"
#include "finish_plan_core.h"
#include "ingest_plan_core.h"
#include "pair_key_core.h"

using namespace covk;

// The C ABI structs are mirrored by hand elsewhere (numpy dtype in coverm_amd/native.py, #[repr(C)] in INTEGRATION.md):
// pin their layout here so that a change in include/covermhip.h cannot silently diverge from those mirrors.
static_assert(sizeof(cov_config) == 40 && offsetof(cov_config, min_aligned_length) == 12 && offsetof(cov_config, min_percent_identity) == 16 &&
              offsetof(cov_config, contig_end_exclusion) == 24 && offsetof(cov_config, want) == 32, "cov_config layout");
static_assert(sizeof(cov_batch) == 80 && offsetof(cov_batch, cigar) == 64 && offsetof(cov_batch, n_records) == 72, "cov_batch layout");
static_assert(sizeof(cov_contig_stats) == 128 && offsetof(cov_contig_stats, sum_identity_primary) == 40 && offsetof(cov_contig_stats, win_sum_d) == 56 &&
              offsetof(cov_contig_stats, first_record) == 88 && offsetof(cov_contig_stats, win_min_d) == 104 && offsetof(cov_contig_stats, hist_len) == 112 &&
              offsetof(cov_contig_stats, hist_off) == 120, "cov_contig_stats layout");
static_assert(sizeof(cov_ingest_stats) == 56 && offsetof(cov_ingest_stats, max_hop_records) == 32 && offsetof(cov_ingest_stats, repaired_starts) == 48, "cov_ingest_stats layout");
static_assert(sizeof(cov_summary) == 32 && offsetof(cov_summary, hist_total) == 24, "cov_summary layout");
static_assert(sizeof(cov_interval) == 24 && sizeof(cov_interval_stats) == 56, "interval struct layout");
static_assert(COV_DEPTH_MAX_CUTS == dclc::MAX_CUTS, "cut lists");
static_assert(sizeof(cov_depth_run) == 8 && offsetof(cov_depth_run, depth) == 4 && sizeof(cov_depth_runs_info) == 40 && offsetof(cov_depth_runs_info, tid_lo) == 32, "depth run struct layout");
static_assert(sizeof(cov_depth_bin) == 24 && sizeof(cov_depth_bin) == sizeof(dbnc::Bin) && offsetof(cov_depth_bin, min) == 8 && offsetof(dbnc::Bin, min) == 8 && offsetof(cov_depth_bin, max) == 12 &&
              offsetof(dbnc::Bin, max) == 12 && offsetof(cov_depth_bin, covered) == 16 && offsetof(dbnc::Bin, covered) == 16 && offsetof(cov_depth_bin, reserved) == 20 &&
              sizeof(cov_depth_bins_info) == 48 && offsetof(cov_depth_bins_info, tid_lo) == 32 && offsetof(cov_depth_bins_info, bin_size) == 40,
              "cov_depth_bin mirrors the device struct (numpy mirror in coverm_amd/native.py)");
static_assert(sizeof(cov_depth_region) == 16 && sizeof(cov_depth_region) == sizeof(drgc::Region) && offsetof(cov_depth_region, start) == 4 && offsetof(drgc::Region, start) == 4 &&
              offsetof(cov_depth_region, end) == 8 && offsetof(drgc::Region, end) == 8 && offsetof(cov_depth_region, reserved) == 12 && sizeof(drgc::Desc) == 16 &&
              sizeof(cov_depth_regions_info) == 48 && offsetof(cov_depth_regions_info, n_pieces) == 16 && offsetof(cov_depth_regions_info, tid_lo) == 40,
              "cov_depth_region mirrors the core's struct (numpy mirror in coverm_amd/native.py)");
static_assert(sizeof(cov_interval_reads) == 32 && sizeof(cov_interval_reads) == sizeof(covgn::Out) && offsetof(cov_interval_reads, sum_identity) == offsetof(covgn::Out, sum_identity) &&
              offsetof(cov_interval_reads, contig_taken) == offsetof(covgn::Out, contig_taken) && sizeof(cov_interval) == sizeof(gnrc::Interval) &&
              offsetof(cov_interval, start) == offsetof(gnrc::Interval, start), "cov_interval_reads mirrors the device struct");
static_assert(sizeof(cov_genome_stats) == 24 && sizeof(cov_genome_stats) == sizeof(covk::DevGenomeStats) && offsetof(cov_genome_stats, genome_len) == offsetof(covk::DevGenomeStats, genome_len) &&
              offsetof(cov_genome_stats, any_nonzero) == offsetof(covk::DevGenomeStats, any_nonzero), "cov_genome_stats mirrors the device struct");
static_assert(sizeof(cov_genome_entry) == 24 && offsetof(cov_genome_entry, first_tid) == 8 && offsetof(cov_genome_entry, gid) == 12 && offsetof(cov_genome_entry, n_contigs_seen) == 16 &&
              offsetof(cov_genome_entry, any_nonzero) == 20 && sizeof(covk::SepEntry) == 8, "cov_genome_entry layout (numpy mirror in coverm_amd/native.py)");
static_assert(sizeof(cov_estimator) == sizeof(covk::DevEstimator) && offsetof(cov_estimator, contig_end_exclusion) == offsetof(covk::DevEstimator, excl) &&
              offsetof(cov_estimator, trim_max) == offsetof(covk::DevEstimator, trim_max) && COV_EST_MAX == covk::EST_MAX && COV_EST_ANIR == covk::EST_ANIR, "cov_estimator mirrors the device struct");

namespace {

#define HIPCHK(call)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess) {                                                               \
            char b_[512];                                                                     \
            snprintf(b_, sizeof b_, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            s->err = b_;                                                                      \
            return COV_ERR_HIP;                                                               \
        }                                                                                     \
    } while (0)

std::string g_create_error;

// COVERM_CLI_TIMING: the library's and the host layer's stamps on stderr (read once per process)
bool cov_timing_on() { static const bool on = getenv("COVERM_CLI_TIMING") != nullptr; return on; }

}  // namespace

extern "C" int covh_timing_on(void) { return cov_timing_on() ? 1 : 0; }

// Which inflate kernel runs, how many blocks make one round (= one launch = one window of the inflated stream) and the size of the carry area.
//   version 3 (default): k_inflate_wave, one wave per BGZF block; a round is as long as the parse wants it (windows bound the memory and set
//                        the fill and drain of the pipeline);
//   version 1 (COVERM_INFLATE_V=1): k_inflate, one LANE per block, private Huffman tables per lane in LDS — the second implementation the
//                        tests compare with; a launch is cut to exactly the blocks resident at once (a lane decodes a block serially).
struct InflateKernel { int version = 3; int lz_version = 2; u32 round_blocks = 0; u64 carry = 16ull << 20; u64 cwin = 0; u32 ext_parts = covi::EXT_PARTS; };

// Everything the device ingest keeps between its calls.  The rings' depths, the result words and the feed's arithmetic: ingest_plan_core.h.
struct IngestState {
    // ---- shared with the SAM text ingest (cov_sam_*)
    bool active = false;
    uint32_t batch = 0;                                // rounds (= windows) launched so far
    uint32_t extracted = 0;                            // windows whose records are in the store (or skipped after a failure)
    uint64_t rec_total = 0, cig_total = 0;             // records / CIGAR words extracted so far (not committed before cov_ingest_end)
    uint32_t fail = 0;                                 // sticky ingplan::Status bits: the first window's status that was not 0
    uint64_t rec_spilled = 0;                          // records of the running ingest that already left the bounded store
    hipStream_t copy = nullptr;
    // (ONE upload stream.  Its H2D copies are 0.595 ms per 32 MiB piece = 56 GB/s with a ~38 us gap between two of them: the link is busy
    // 91 % of the time the file streams, profiles/r06_ingest_copy_trace.json.  A second stream — the halves of a piece on two DMA engines in
    // round 3, whole pieces in turn in round 6 — is SLOWER both ways: 0.82 s of ingest against 0.50 s at 200 M reads,
    // profiles/r06_copy_streams_ab_200M.json, profiles/r03_copy_queues_50M.log.)
    hipEvent_t ev[COV_INGEST_SLOTS] = {};              // a slot's last upload
    u64 *h_winres = nullptr;                           // page-locked: PARSE_RING x WIN_RESULT_WORDS words, the windows' result blocks
    std::future<hipError_t> prep;      // COV_WANT_INGEST: create() running on a helper thread since cov_create (ingest_prep_wait)

    // ---- the BGZF ingest: compressed file and inflated stream in HBM, BGZF block table, record-boundary scratch
    bool was_span = false;           // records of a cov_ingest_span rank are in the store: cov_group_records refuses (cleared by cov_reset alone)
    DevBuf<uint8_t> g_scratch, g_carry;
    DevBuf<u32> g_crc_tab;             // k_crc32_wave's tables (crcw::build_tables), uploaded by create() or the next cov_ingest_begin
    DevBuf<uint8_t> g_cwin[ingplan::CWIN_RING];            // compressed bytes, one buffer per round in flight (file offsets biased by the round's origin)
    DevBuf<uint8_t> g_win[ingplan::WIN_RING];              // inflated windows (one k_inflate round each): [carry area | blocks]
    DevBuf<covi::BgzfBlock> g_blocks;
    DevBuf<u32> g_status;
    DevBuf<covi::SegInfo> g_seg[ingplan::PARSE_RING];      // per-window parse state
    DevBuf<u64> g_recbase[ingplan::PARSE_RING], g_cigbase[ingplan::PARSE_RING];
    DevBuf<u64> g_result;                                  // ingplan::G_WORDS words (GlobalWord, WinWord)
    DevBuf<covi::LongRec> g_long;                          // the long records of the window being extracted (k_bam_extract -> k_bam_extract_long, one stream)
    DevBuf<covi::tokpos_t> g_tok[ingplan::TOK_RING];
    DevBuf<u32> g_ntok[ingplan::TOK_RING];
    hipStream_t aux = nullptr;                             // k_lz_resolve / k_crc32 of round i run beside k_inflate of round i + 1
    hipStream_t parse = nullptr;                           // record boundaries of window i run beside both
    hipStream_t ext = nullptr;       // extraction of verified windows: the parse stream (a stream of its own made no difference, profiles/r03_tail_variants.log)
    hipEvent_t inf_done[ingplan::TOK_RING] = {}, lz_done[ingplan::TOK_RING] = {};
    hipEvent_t ver_done[ingplan::PARSE_RING] = {}, ext_done[ingplan::WIN_RING] = {}, cdone[ingplan::CWIN_RING] = {};
    hipEvent_t fed = nullptr;                              // everything fed so far is on the device
    ingplan::FeedState feed;                               // the open round, the blocks and bytes so far (ingplan::feed_plan advances it)
    uint64_t ccap = 0;                                     // compressed bytes a round may span
    int64_t copy_cleared = -1;                             // highest round whose compressed buffer the copy stream may already write
    long long key_lo = 0, key_hi = ingplan::KEY_END;       // cov_ingest_span: records outside [key_lo, key_hi) are not taken
    bool search_first = false, open_end = false;
    uint64_t span_lo = 0, span_hi = 0;                     // file bytes the span covers (store size estimate)
    uint64_t tail_key = ~0ull;                             // key of the record cut by the end of the last window (~0: none)
    struct WinInfo { u64 N = 0; u32 n_seg = 0; u64 comp_end = 0; };
    WinInfo win[ingplan::PARSE_RING];
    int check_crc = 1;
    uint64_t fail_dbg[3] = {0, 0, 0};                      // W_BAD_SEG, W_BAD_START, W_BAD_LANDED of the window that failed
    uint64_t first_record = 0;
    uint64_t launched = 0;           // blocks already handed to k_inflate
    covi::BgzfBlock *h_blocks = nullptr; size_t h_blocks_cap = 0;   // page-locked mirror of the block table (async uploads read from it)
    std::vector<ingplan::Step> steps;                      // of the piece being fed
    uint64_t comp = 0;
    InflateKernel K;
    cov_ingest_stats stats{}, stats_last{};                // of the running ingest / of the last cov_ingest_end
    double s_alloc = 0;              // host seconds inside device allocations of the ingest
    double s_part[4] = {0, 0, 0, 0};         // ... inside ingest_drain / launch_round / the upload calls / event waits (COVERM_CLI_TIMING)

    bool is_span() const { return ingplan::is_span(key_lo, key_hi, search_first, open_end); }

    // The part of cov_ingest_begin that does not depend on the file: three streams (a hardware queue with its 173 MB save area each), two dozen
    // events, the page-locked result words and block-table mirror, k_crc32_wave's tables — ~50 ms that used to pass between cov_ingest_begin and
    // the first piece's upload (tools/r06/call39.sh: "first upload after 0.053 s").  With COV_WANT_INGEST cov_create starts it on a helper thread
    // as soon as the runtime is up, beside its own stream and whatever the caller does next (targets, estimators, the file's header).
    hipError_t create(int device) {
        hipError_t e = hipSetDevice(device);
        if (e != hipSuccess || copy) return e;
#define PREP(x) do { e = (x); if (e != hipSuccess) return e; } while (0)
        auto events = [](hipEvent_t *v, u32 n) { hipError_t e = hipSuccess; for (u32 k = 0; k < n && e == hipSuccess; k++) e = hipEventCreateWithFlags(&v[k], hipEventDisableTiming); return e; };
        PREP(hipStreamCreateWithFlags(&copy, hipStreamNonBlocking));
        PREP(events(ev, COV_INGEST_SLOTS));
        PREP(events(&fed, 1));
        PREP(hipStreamCreateWithFlags(&aux, hipStreamNonBlocking));
        // (the boundary search on the LZ / CRC stream — the runtime's four hardware queues put the two on one queue anyway — was measured:
        // ingest 0.650 s against 0.612 s, the extraction of window w then also waits behind the LZ of w + 1, and the exit is no shorter:
        // profiles/r04_e2e_200M_runs_*.log)
        PREP(hipStreamCreateWithFlags(&parse, hipStreamNonBlocking));
        ext = parse;
        for (u32 k = 0; k < ingplan::TOK_RING; k++) { PREP(events(&inf_done[k], 1)); PREP(events(&lz_done[k], 1)); }
        PREP(events(ver_done, ingplan::PARSE_RING));
        for (u32 k = 0; k < ingplan::WIN_RING; k++) { PREP(events(&ext_done[k], 1)); PREP(events(&cdone[k], 1)); }
        PREP(hipHostMalloc((void **)&h_winres, ingplan::PARSE_RING * ingplan::WIN_RESULT_WORDS * sizeof(u64), hipHostMallocDefault));
        {   // page-locked mirror of the block table: room for a 25 GB file of ordinary ~20 KB blocks (cov_ingest_begin replaces it for a larger one)
            const size_t nc = (size_t)3 << 19;
            PREP(hipHostMalloc((void **)&h_blocks, nc * sizeof(covi::BgzfBlock), hipHostMallocDefault));
            h_blocks_cap = nc;
        }
        {
            static const std::vector<u32> crc_tables = [] { std::vector<u32> t(covi::crcw::TABLE_WORDS); covi::crcw::build_tables(t.data()); return t; }();
            PREP(g_crc_tab.reserve(covi::crcw::TABLE_WORDS, copy));
            PREP(hipMemcpyAsync(g_crc_tab.p, crc_tables.data(), covi::crcw::TABLE_WORDS * sizeof(u32), hipMemcpyHostToDevice, copy));
            PREP(hipStreamSynchronize(copy));
        }
#undef PREP
        return hipSuccess;
    }
    static_assert(ingplan::WIN_RING == ingplan::CWIN_RING, "create and destroy walk ext_done and cdone in one loop");

    // The buffers whose size follows the file (cov_ingest_release gives them back between two files; g_result and g_long stay to the end).
    void free_buffers() {
        g_scratch.release(); g_carry.release(); g_blocks.release(); g_status.release();
        g_crc_tab.release();
        for (auto &b : g_win) b.release();
        for (auto &b : g_cwin) b.release();
        for (u32 k = 0; k < ingplan::PARSE_RING; k++) { g_seg[k].release(); g_recbase[k].release(); g_cigbase[k].release(); }
        for (u32 k = 0; k < ingplan::TOK_RING; k++) { g_tok[k].release(); g_ntok[k].release(); }
    }

    // What create made and what the files left (cov_destroy, behind the `side` stream: that may be `aux`, borrowed).
    void destroy() {
        for (hipStream_t st : {aux, parse, ext}) if (st) (void)hipStreamSynchronize(st);
        free_buffers();
        g_result.release(); g_long.release();
        if (aux) (void)hipStreamDestroy(aux);
        if (parse) (void)hipStreamDestroy(parse);
        for (u32 k = 0; k < ingplan::TOK_RING; k++) { if (inf_done[k]) (void)hipEventDestroy(inf_done[k]); if (lz_done[k]) (void)hipEventDestroy(lz_done[k]); }
        for (hipEvent_t e : ver_done) if (e) (void)hipEventDestroy(e);
        for (u32 k = 0; k < ingplan::WIN_RING; k++) { if (ext_done[k]) (void)hipEventDestroy(ext_done[k]); if (cdone[k]) (void)hipEventDestroy(cdone[k]); }
        if (h_winres) (void)hipHostFree(h_winres);
        h_winres = nullptr;
        if (h_blocks) (void)hipHostFree(h_blocks);
        h_blocks = nullptr;
        if (copy) { (void)hipStreamSynchronize(copy); (void)hipStreamDestroy(copy); }
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
        if (fed) (void)hipEventDestroy(fed);
    }

    // The one list of what a new file, or the end of an abandoned one, puts back.
    enum class Reset { BGZF_FILE, SAM_FILE, ABORT };
    void reset_for_file(Reset why) {
        // all three: nothing extracted and uncommitted, no failure, no open round
        rec_total = cig_total = 0; fail = 0; feed.round_n = 0;
        if (why == Reset::ABORT) {
            // The abort keeps `batch` and declares every launched window extracted: the drains of a later call find nothing to do, and
            // cov_ingest_copy_inflated still answers for a file of one window.  rec_spilled stays too: cov_ingest_abort reports it first.
            extracted = batch;
            return;
        }
        batch = 0; extracted = 0; rec_spilled = 0;
        // The text ingest has no rounds, spans or window statistics and never reads the fields below: they keep what the last BGZF file left
        // (cov_ingest_last_stats goes on answering for it).
        if (why == Reset::SAM_FILE) return;
        feed = ingplan::FeedState{}; launched = 0; copy_cleared = -1;
        key_lo = 0; key_hi = ingplan::KEY_END; search_first = false; open_end = false;
        span_lo = 0; tail_key = ~0ull;
        s_alloc = 0; for (double &x : s_part) x = 0;
        stats = cov_ingest_stats{};
        // (not here: was_span describes the store's content, not the file; fail_dbg and win[] are written before they are read; the file's
        // own figures — comp, span_hi, ccap, first_record, check_crc, K — are cov_ingest_begin's arguments)
    }
};

struct cov_session {
    cov_config cfg{};
    hipStream_t stream = nullptr;
    std::string err;
    int tile = 1024;  // bases per tile (one wave per tile: STREAM_TW)
    bool use_fast = true;  // k_pileup_fast + k_pileup_stream on the slow-tile list (default); COVERM_PILEUP=stream: k_pileup_stream alone
    int chunk_tiles = (int)psched::CHUNK_TILES;   // consecutive tiles walked by one wave; COVERM_KNOBS pileup_chunk_tiles overrides both.  A chunk end only moves the wave's bins,
    int chunk_tiles_listed = (int)psched::CHUNK_TILES_LISTED;      // so what decides is balance: without the deep-tile list 4 tiles (0.385 ms; 8: 0.456), with the deep tiles out
                           // of the chunks 8 (0.363; 4: 0.372, 16: 0.378): profiles/pileup_schedule_ab.json
    int prep_kernel = 0;   // 0 = k_prep_lean (prep_lean.hip.h); COVERM_PREP_KERNEL=7 forces k_prep7s, the second implementation (tests)
    int est_lanes = -1;        // k_estimate_lanes / k_genome_estimate_lanes (a lane per contig / genome) from 65 536 of them on; COVERM_EST_LANES=1 | 0 forces it on / off (tests)
    int fast_tables = 1;       // k_pileup_fast (one table of biased deltas: the default) or k_pileup_fast2t (two count tables; COVERM_FAST_TABLES=2)
    int n_cus = 256;

    // targets
    uint32_t n_targets = 0;
    std::vector<uint32_t> h_tlen;
    std::vector<uint32_t> h_tile_first;  // first tile of each contig (+ sentinel)
    uint32_t n_tiles = 0;
    DevBuf<u32> d_tlen, d_tile_contig, d_tile_start;
    DevBuf<u32> d_tile_first, d_tcnt, d_fov, d_tscan, d_ttop;   // TileIdx (pileup_kernels.hip.h)
    DevBuf<u32> d_slow_list;                                    // tiles k_ranges leaves to k_pileup_stream
    DevBuf<u32> d_deep_list;                                    // tiles of deep_min candidate runs or more: k_pileup_fast visits them first, one per wave (pileup_schedule_core.h)
    uint32_t deep_min = psched::DEEP_MIN;                                    // COVERM_KNOBS pileup_deep_min: 0 = no list, flagged tiles do not exist and every tile is walked in its chunk
    uint32_t last_pileup_waves = 0, last_pileup_chunk = 0;      // waves and tiles per chunk of the last k_pileup_fast launch (cov_pileup_schedule)
    uint32_t tile_shift = 10;
    DevBuf<u32> d_cx_list, d_cx_cnt, d_cx_cur, d_cx_scan, d_cx_top;   // CxIdx: long-CIGAR buckets
    DevBuf<uint2> d_cx_runs;
    DevBuf<DevContig> d_ctg_scratch;   // cov_copy_depth works on a copy of the accumulators
    // per-interval statistics (cov_interval_stats_compute): depth of every target, materialised on demand
    DevBuf<int32_t> d_depth_all; DevBuf<u64> d_depth_off; bool depth_all_valid = false;
    DevBuf<DevInterval> d_iv; DevBuf<DevIntervalStats> d_ivst; DevBuf<unsigned long long> d_ivhist; uint64_t ivhist_total = 0;
    // per-interval read aggregates (cov_interval_reads_compute, gene_kernels.hip.h): work arrays per record and per taken record, the tiles'
    // sums, the checkpoints of the identity prefix; sized from the record and interval counts, kept for the next call
    DevBuf<uint8_t> gr_code; DevBuf<u32> gr_mism, gr_trec, gr_pprim, gr_tids; DevBuf<int32_t> gr_ttid, gr_tpos; DevBuf<double> gr_ident, gr_tident, gr_ck;
    DevBuf<u64> gr_bcnt, gr_bmism, gr_pmism, gr_glob; DevBuf<gnrc::Interval> gr_iv; DevBuf<covgn::Out> gr_out; DevBuf<covgn::Bounds> gr_bounds;
    float gene_ms = 0.f; uint32_t gene_launches = 0;      // the last cov_interval_reads_compute (COV_K_GENE_READS)
    // depth runs (cov_depth_runs_compute / _fetch, depth_kernels.hip.h): ONE chunk of whole targets at a time — its arena, start mask and
    // rank, the scan's block sums, the runs and the targets' run offsets; kept for the next chunk
    struct DepthRuns {
        DevBuf<int32_t> arena; DevBuf<u32> woff, mask, rank, sums, run_off; DevBuf<u64> doff, total; DevBuf<dprc::Run> runs;
        std::vector<u32> h_woff, h_run_off;
        u64 chunk_bases = dprc::DEFAULT_CHUNK_BASES;      // COVERM_KNOBS depth_chunk_bases (tests: many chunks)
        bool valid = false;                               // a chunk's runs are on the device: [lo, next), n_runs of them
        u32 lo = 0, next = 0, launches = 0;
        u64 n_runs = 0, arena_bases = 0;
        hipEvent_t ev_mid = nullptr;
        float arena_ms = 0.f, runs_ms = 0.f;              // of the last chunk: the pileup into the arena; the run kernels (COV_K_DEPTH_RUNS)
        // depth bins (cov_depth_bins_compute / _fetch, depth_bins_kernels.hip.h): the same arena, mask and rank; the chunk's bins and the
        // targets' bin offsets.  The arena holds ONE chunk: a compute of the runs drops the bins and the reverse (take_arena below).
        DevBuf<dbnc::Bin> bins; DevBuf<u32> bin_off;
        std::vector<u64> h_bin_off; std::vector<u32> h_bin_off32;
        bool bins_valid = false;
        // The arena holds ONE chunk of ONE of the three parties (runs, bins, regions): taker[x] = the party whose compute took the arena
        // from under x's chunk (0: nobody), which is what x's refused fetch names.
        enum Party : int { RUNS = 0, BINS = 1, REGIONS = 2 };
        uint8_t taker[3] = {0, 0, 0};
        bool &valid_of(int party) { return party == RUNS ? valid : party == BINS ? bins_valid : regs_valid; }
        void take_arena(int party) {
            for (int o = 0; o < 3; o++)
                if (o != party && valid_of(o)) { valid_of(o) = false; taker[o] = (uint8_t)(party + 1); }
            valid_of(party) = false; taker[party] = 0;
        }
        static const char *party_name(int party) { return party == RUNS ? "cov_depth_runs" : party == BINS ? "cov_depth_bins" : "cov_depth_regions"; }
        // the fetch of `party` that lost its chunk: empty when it did not
        std::string lost(int party) const {
            if (!taker[party]) return std::string();
            return std::string(party_name(party)) + "_fetch: the chunk's arena was taken by a " + party_name(taker[party] - 1) + "_compute since (" + party_name(party) + "_compute again)";
        }
        u32 b_lo = 0, b_next = 0, b_launches = 0, bin_size = 0;
        u64 n_bins = 0, b_arena_bases = 0;
        float b_arena_ms = 0.f, bins_ms = 0.f;            // of the last chunk of bins (COV_K_DEPTH_BINS)
        // depth regions (cov_depth_regions_set / _compute / _fetch, depth_regions_kernels.hip.h): the session's regions in a stable order by
        // tid (h_reg; h_reg_input: their positions in the caller's array; h_reg_first: CSR over the targets), and of the last chunk the
        // descriptors, the piece offsets and the results.  cov_set_targets drops the regions; reset and finish keep them.
        std::vector<drgc::Region> h_reg; std::vector<u32> h_reg_input, h_reg_first;
        bool have_regions = false;
        DevBuf<drgc::Desc> reg_desc; DevBuf<u32> reg_piece_off; DevBuf<dbnc::Bin> regs;
        // the thresholds of cov_depth_thresholds_set (thr.n == 0: none; kept over set_targets, reset and finish) and, of the last chunk computed
        // with them, its counts: n_regs x g_thr, row-major in the result order
        dclc::Cuts thr = {}; DevBuf<u32> reg_counts; u32 g_thr = 0;
        std::vector<drgc::Desc> h_reg_desc; std::vector<u32> h_reg_piece_off;
        bool regs_valid = false;
        u32 g_lo = 0, g_next = 0, g_launches = 0, g_first = 0;      // g_first: the chunk's first region in h_reg
        u64 n_regs = 0, n_pieces = 0, g_arena_bases = 0;
        float g_arena_ms = 0.f, regs_ms = 0.f;            // of the last chunk of regions (COV_K_DEPTH_REGIONS)
        void drop() { valid = false; bins_valid = false; regs_valid = false; taker[0] = taker[1] = taker[2] = 0; }      // push / reset / finish: none is there
        void release() { arena.release(); woff.release(); mask.release(); rank.release(); sums.release(); run_off.release(); doff.release(); total.release(); runs.release(); bins.release(); bin_off.release(); reg_desc.release(); reg_piece_off.release(); regs.release(); reg_counts.release(); if (ev_mid) (void)hipEventDestroy(ev_mid); ev_mid = nullptr; }
    } dr;
    DevBuf<uint8_t> d_mask;
    std::vector<uint8_t> h_mask;       // host copy (convert_results lays the compact histogram out itself)
    bool have_mask = false;
    // cov_set_genomes: the table genome -> targets (CSR, ascending tid; rows cut into segments of GENOME_SEG, genome_kernels.hip.h), the
    // genomes' accumulators and merged histogram, and the block the host fetches: [cov_genome_stats x n_genomes][floats x n_genomes x est.n]
    bool have_genomes = false, gen_valid = false;
    bool lean_finish = false;      // inside cov_finish_genomes: order and error verdict on the device, no per-contig block to the host
    bool in_spill = false;         // the pass a spill runs over a partial store: no genome entries
    DevBuf<u64> d_order;           // k_order_*: [0] first record that breaks the order (~0: none), [1 ..] per-block maxima
    uint32_t n_genomes = 0, n_gseg = 0;
    DevBuf<u32> d_grow, d_gtids, d_gseg_genome, d_gseg_start;
    DevBuf<DevGenome> d_genomes;
    DevBuf<u64> d_ghist, d_ghist_top;
    DevBuf<uint8_t> d_gout; uint8_t *h_gout = nullptr; size_t h_gout_cap = 0;
    // cov_set_genome_runs: gid[] / blk[] of the header; the table entry -> targets is built per finish (sep_kernels.hip.h) into the arrays of
    // cov_set_genomes above, which the two modes never hold at once.  The fetched block: [cov_genome_stats x n][floats x n x est.n][SepEntry x n],
    // the counts of the finish in the last 16 bytes of h_gout.  n_genomes = the entries of the last finish.
    bool have_runs = false;
    uint32_t n_gids = 0, sep_ent_cap = 0, sep_seg_cap = 0;
    DevBuf<int32_t> d_sgid; DevBuf<u32> d_sblk, d_sent_pos, d_stop_last1, d_stop_first, d_scounts; DevBuf<uint8_t> d_scode;
    DevBuf<u64> d_stop_cnt, d_stop_seg; DevBuf<SepEntry> d_sent;
    // results of the device pipeline live in ONE block [DevGlobal][DevContig x n_targets] (d_res): one DMA brings them to
    // the host, and cov_gather sends the same block over RCCL.  d_glob / d_ctg are views into it (never freed themselves).
    DevBuf<uint8_t> d_res;
    DevBuf<DevContig> d_ctg;
    DevBuf<DevGlobal> d_glob;
    DevBuf<uint4> d_desc;
    // cov_gather (root session): every rank's block, device and page-locked host copies
    DevBuf<uint8_t> d_gather; uint8_t *h_gather = nullptr; size_t h_gather_cap = 0; uint32_t gather_n = 0; size_t gather_block = 0;

    RecordStore store;               // record store (owned, record_store.h) or adopted device batch
    bool want_mates = false;         // cov_ingest_want_mates: the ingest keeps the mate columns, for cov_pair_filter_apply
    bool want_grouping = false;      // cov_ingest_want_grouping: cov_group_records will follow, so decreasing keys are no reason to hand a file back
    float grp_ms[4] = {};            // the last cov_group_records: whole call on the stream, order check, sort passes, gather
    uint32_t grp_launches = 0;
    bool adopted = false;
    cov_batch adopted_batch{};
    uint64_t adopted_ncig = 0;
    uint32_t adopted_cig_end = 0;

    // ---- bounded record store.  The reference holds ONE contig's state at a time and flushes when the tid changes (contig.rs:128-155), so it
    // has no size limit; the store here keeps as many contigs as fit under a cap.  When a push or an extraction would take it past the cap,
    // the pipeline runs over what the store holds, the contigs that are complete are kept on the host (`spill`), the records from the first
    // considered record of the contig in flight onwards move to the front, and the session goes on.  cov_finish merges.
    uint64_t cap_records = 0x80000000ull, cap_cigar = 0x80000000ull;      // COVERM_STORE_CAP_RECORDS / COVERM_STORE_CAP_CIGAR (tests); the hard limit stays 2^32 - 16 each
    struct Spill {
        bool active = false;
        std::vector<cov_contig_stats> stats; std::vector<DevContig> ctg; std::vector<uint8_t> have;     // per target: taken in an earlier spill
        std::vector<uint64_t> hist;                                       // their histogram bins, stats[c].hist_off indexes this
        uint64_t prim = 0, cons = 0, records = 0;                         // primaries / considered records / records that left the store
        int64_t inflight = -1;                                            // contig in flight at the last spill: a later considered contig below it = unsorted
        uint32_t count = 0;
        void clear() { active = false; stats.clear(); ctg.clear(); have.clear(); hist.clear(); prim = cons = records = 0; inflight = -1; count = 0; }
    } spill;
    // CoverageEstimator::calculate_coverage on the device (cov_set_estimators): parameters, device rows, page-locked copy of the last finish
    EstParams est{};
    float *h_estf = nullptr; bool est_valid = false;      // (views: device rows behind the result block in d_res, host rows behind it in h_res)
    std::vector<float> spill_est;           // rows of the contigs that left in a spill (n_targets x est.n, filled as they leave)
    std::vector<uint64_t> merged_hist;      // histogram of the last cov_finish when it merged spilled contigs (cov_fetch_hist serves it)
    bool merged_valid = false;
    uint64_t merged_records = 0;            // records of the whole sample after a merging finish (cov_gather sends it)
    uint64_t spill_retry_at = 0;            // after a spill that could move nothing: no further attempt below this many records

    DevBuf<uint2> d_runs;
    DevBuf<PrepPartial> d_part;
    DevBuf<u32> d_gen_list;            // steps k_prep_lean leaves to k_prep_generic
    DevBuf<PrepArgs> d_prep_args;      // k_prep_lean's arguments in device memory (its rare branches read them there), written by k_init
    DevBuf<double> d_ident, d_identp;
    DevBuf<IdChunk> d_idch;
    int id_mode = 1;   // 1 = exact parallel identity sums, 0 = serial chain only (COVERM_IDENTITY=serial)
    hipStream_t side = nullptr; bool side_owned = false;     // k_identity overlaps k_ranges / k_pileup (created on first use, or the idle second stream of the ingest)
    hipEvent_t ev_prep_done = nullptr, ev_side_done = nullptr;
    DevBuf<u32> d_arena;
    DevBuf<u64> d_hist_top;            // k_hist_sum / k_hist_off: bins per block of 1024 contigs
    DevBuf<u64> d_chist;
    u64 *h_chist = nullptr; u64 h_chist_cap = 0, hist_prefetched = 0, last_chist_total = 0; bool hist_compacted = false, hist_fetch_seen = false;
    DevBuf<int32_t> d_depth;

    IngestState ing;                 // device ingest (cov_ingest_*), and what the SAM text ingest shares with it

    // SAM text ingest (cov_sam_*): an ingest like the BGZF one as far as the session's state goes (ing.active, ing.rec_total, the slots' events,
    // the upload stream, cov_ingest_abort: the head of IngestState), with sam_active on top.  Two text buffers of one window each take the uploads in turn; masks and
    // line arrays exist once (the windows' kernels run in order on the session stream).
    bool sam_active = false, sam_seen_record = false, sam_decode_timed = false;
    uint64_t sam_window = 0, sam_expected = 0, sam_lines = 0, sam_bytes = 0, sam_err_line = 0;
    uint32_t sam_err = 0, sam_k = 0;
    DevBuf<uint8_t> m_text[2], m_blob;
    DevBuf<u64> m_nl, m_tab, m_res, m_noff;
    DevBuf<u32> m_line_end, m_cnt, m_rec_idx, m_cig_idx, m_bsum[3], m_slots;
    samc::Table m_names{};
    hipEvent_t sam_buf_free[2] = {}, sam_ev[4] = {};
    float sam_ms = 0.f; uint32_t sam_launches = 0;

    // results of the last finish
    bool finished = false;
    // result staging in page-locked memory: [DevGlobal][DevContig x n_targets], one DMA pair per finish
    uint8_t *h_res = nullptr; size_t h_res_cap = 0;
    std::future<std::pair<uint8_t *, size_t>> h_res_prep;      // an assembly's result staging (hundreds of MB of page-locked memory: ~0.17 s per GiB) being obtained since cov_set_targets
    DevContig *h_ctg = nullptr;
    DevGlobal h_glob{};
    bool last_gen_all = false;         // the last finish ran k_prep_generic over every step (cov_last_paths)
    uint32_t last_passes = 0;          // how often the last finish ran the pipeline over the store: 2 when the bucket buffer was too small (cov_last_paths)
    uint64_t algo_bytes = 0;

    hipEvent_t ev[COV_K_COUNT][2] = {};
    hipEvent_t ev_begin[COV_K_COUNT] = {};      // the event a group's time is measured from (its own, or the previous group's end)
    int ev_fresh = -1;                          // group whose end event is the last thing on the stream (-1: something else followed)
    float k_ms[COV_K_COUNT] = {};
    uint32_t k_launches[COV_K_COUNT] = {};
};

static cov_status spill_store(cov_session *s, bool &progress);      // bounded record store (defined behind finish_once and its stages)

namespace {

size_t result_block_bytes(u32 n_targets) { return sizeof(DevGlobal) + (size_t)std::max<u32>(n_targets, 1) * sizeof(DevContig); }
// Page-locked staging for the results of a sample with very many references: the block is [DevGlobal][DevContig x n][floats x n x n_est] —
// 350 MB at 2 M contigs and four estimators, 0.06 s of hipHostMalloc that used to sit in the sample's one cov_finish.  cov_set_targets starts
// it on a helper thread (the ingest or the pushes pass meanwhile); cov_finish takes what the helper got, or allocates as before.
static size_t result_host_bytes(const cov_session *s, u32 nT) {
    // (with a target mask no per-contig floats come back — the entries are genomes — so the block does not grow with the estimators)
    return result_block_bytes(nT) + (size_t)std::max<u32>(nT, 1) * ((s->have_mask || s->have_runs) ? 1u : std::max<u32>(s->est.n, 1u)) * sizeof(float);
}
// A page-locked buffer grows: freed, then allocated for n elements (the content is not kept; cap = 0 when the allocation fails).
template <class T, class N>
static hipError_t pinned_grow(T *&p, N &cap, N n) {
    if (p) (void)hipHostFree(p);
    p = nullptr; cap = 0;
    const hipError_t e = hipHostMalloc((void **)&p, (size_t)n * sizeof(T), hipHostMallocDefault);
    if (e == hipSuccess) cap = n;
    return e;
}
static void result_host_take(cov_session *s) {
    if (!s->h_res_prep.valid()) return;
    const std::pair<uint8_t *, size_t> r = s->h_res_prep.get();
    if (!r.first) return;
    if (r.second > s->h_res_cap) {
        if (s->h_res) (void)hipHostFree(s->h_res);
        s->h_res = r.first; s->h_res_cap = r.second;
    } else (void)hipHostFree(r.first);
}

// [DevGlobal][DevContig x n_targets] (the block cov_gather sends) and, behind it, room for the estimators' floats (COV_EST_MAX per target):
// both come to the host in one copy
hipError_t bind_result_block(cov_session *s, u32 n_targets) {
    hipError_t e = s->d_res.reserve(result_block_bytes(n_targets) + (size_t)std::max<u32>(n_targets, 1) * COV_EST_MAX * sizeof(float), s->stream);
    if (e != hipSuccess) return e;
    s->d_glob.p = reinterpret_cast<DevGlobal *>(s->d_res.p); s->d_glob.cap = 1;
    s->d_ctg.p = reinterpret_cast<DevContig *>(s->d_res.p + sizeof(DevGlobal)); s->d_ctg.cap = std::max<u32>(n_targets, 1);
    return hipSuccess;
}

Records records_of(const cov_session *s) {
    Records r{};
    if (s->adopted) {
        const cov_batch &b = s->adopted_batch;
        r.tid = b.tid; r.pos = b.pos; r.flag = b.flag; r.mapq = b.mapq; r.nm = b.nm; r.nm_kind = b.nm_kind;
        r.l_seq = b.l_seq; r.cigar_off = b.cigar_off; r.cigar = b.cigar;
    } else s->store.view(r);
    r.n = (u32)s->store.n_records;
    r.cigar_end = s->adopted ? s->adopted_cig_end : (u32)s->store.n_cigar;
    return r;
}

__global__ void k_rebase_offsets(u32 *off, u32 n, u32 sub, u32 add) {
    u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) off[i] = off[i] - sub + add;
}

// records [lo, n) with neither the secondary nor the supplementary bit (what num_detected_primary_alignments counts, bam_generator.rs:114-118)
__global__ void k_count_primary(const uint16_t *__restrict__ flag, u32 lo, u32 n, unsigned long long *out) {
    u32 cnt = 0;
    for (u64 i = (u64)lo + blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) cnt += (flag[i] & 0x900u) ? 0u : 1u;
    cnt = wave_sum_u32(cnt);
    if ((threadIdx.x & 63u) == 0u && cnt) atomicAdd(out, (unsigned long long)cnt);
}

cov_status append(cov_session *s, const cov_batch *b, bool from_device) {
    const uint64_t n = b->n_records;
    if (n == 0) return COV_OK;
    const hipMemcpyKind kind = from_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    u32 off0 = 0, offn = 0;
    if (from_device) {
        HIPCHK(hipMemcpyAsync(&off0, b->cigar_off, 4, hipMemcpyDeviceToHost, s->stream));
        HIPCHK(hipMemcpyAsync(&offn, b->cigar_off + n, 4, hipMemcpyDeviceToHost, s->stream));
        HIPCHK(hipStreamSynchronize(s->stream));
    } else {
        off0 = b->cigar_off[0]; offn = b->cigar_off[n];
    }
    const uint64_t ncig = (uint64_t)offn - off0;
    if (s->store.n_records && (s->store.n_records + n > s->cap_records || s->store.n_cigar + ncig > s->cap_cigar) && s->store.n_records >= s->spill_retry_at) {
        // bounded store: the contigs that are complete leave for the host, the contig in flight moves to the front (contig.rs:128-155)
        bool progress = false;
        const cov_status sp = spill_store(s, progress);
        if (sp != COV_OK) return sp;
        // one reference already fills the store: a spill is a whole pass over it that moves nothing — not again before the store has doubled
        s->spill_retry_at = progress ? 0 : 2 * s->store.n_records;
    }
    if (s->store.n_records + n >= 0xfffffff0ull) { s->err = "more than 2^32 records of one reference (or of one batch) in the record store"; return COV_ERR_INVALID_ARG; }
    if (s->store.n_cigar + ncig >= 0xfffffff0ull) { s->err = "more than 2^32 CIGAR words of one reference (or of one batch) in the record store"; return COV_ERR_INVALID_ARG; }
    RecordStore &S = s->store;
    const uint64_t R = S.n_records, N = R + n; hipStream_t st = s->stream;
    HIPCHK(S.reserve(N, S.n_cigar + ncig + 1, st, R, S.n_cigar, false));
    HIPCHK(S.copy_in(*b, n, off0, ncig, kind, st));
    if (off0 != (u32)S.n_cigar) {
        const u32 cnt = (u32)(n + 1);
        hipLaunchKernelGGL(k_rebase_offsets, dim3((cnt + 255) / 256), dim3(256), 0, st, S.cigar_off.p + R, cnt, off0, (u32)S.n_cigar);
        HIPCHK(hipGetLastError());
    }
    S.n_records = N; S.n_cigar += ncig;
    s->finished = false;
    if (!from_device) HIPCHK(hipStreamSynchronize(st));   // contract: host arrays are free to change on return
    return COV_OK;
}

// An adopted device batch becomes the content of the owned store (before anything else is written behind it).
cov_status materialise_adopted(cov_session *s) {
    if (!s->adopted) return COV_OK;
    const cov_batch ab = s->adopted_batch;
    s->adopted = false; s->store.n_records = 0; s->store.n_cigar = 0;
    return append(s, &ab, true);
}

void timing_events(cov_session *s) {
    if (s->ev[0][0]) return;
    for (int k = 0; k < COV_K_COUNT; k++)
        for (int j = 0; j < 2; j++) (void)hipEventCreate(&s->ev[k][j]);
}
// Timing brackets of the kernel groups.  An event record costs the stream ~5 us (profiles/r05b_bench_kernel_trace: the gaps of a step sat
// exactly where its eleven records were), so a group that begins where the previous one ended takes that group's end event for its
// beginning: six records per finish instead of eleven.
void time_begin(cov_session *s, int k) {
    if (s->ev_fresh >= 0) { s->ev_begin[k] = s->ev[s->ev_fresh][1]; return; }
    (void)hipEventRecord(s->ev[k][0], s->stream); s->ev_begin[k] = s->ev[k][0];
}
void time_end(cov_session *s, int k) { (void)hipEventRecord(s->ev[k][1], s->stream); s->k_launches[k]++; s->ev_fresh = k; }

// Resident workgroups per CU of a pileup kernel that takes `smem` bytes of dynamic LDS (allowed here, before its first launch).  The
// dynamic-LDS limit and the occupancy are per-device facts, and span mode launches from one thread per device: cached per device id, in
// atomics (two threads racing for the same device compute the same value); the caller owns one cache per kernel instantiation.
int pileup_occupancy(const cov_session *s, std::atomic<int> (&occ_dev)[64], const void *kern, size_t smem) {
    std::atomic<int> &occ_slot = occ_dev[(unsigned)s->cfg.device & 63u];
    int occ = occ_slot.load(std::memory_order_relaxed);
    if (!occ) {
        (void)hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        int nb = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, 256, smem) != hipSuccess || nb < 1) {
            (void)hipGetLastError();
            nb = (int)std::max<size_t>(1, std::min<size_t>(8, (160 * 1024) / smem));
        }
        occ = nb; occ_slot.store(nb, std::memory_order_relaxed);
    }
    return occ;
}
// Grid = psched::PILEUP_ROUNDS x the resident workgroups (registers, not LDS, bound residency), at most a wave per chunk
// (pileup_schedule_core.h): each wave still walks several chunks, and the hardware dispatcher hands out the successive "rounds".
u32 pileup_grid(const cov_session *s, int occ, u32 n_tiles) {      // (k_pileup_stream; occ = resident workgroups of 256 threads per CU)
    return psched::grid_of(n_tiles, (u32)s->chunk_tiles, (u32)s->n_cus, (u32)occ * 4u, psched::STREAM_WG_WAVES);
}
// the deep-tile list of the last k_ranges, for a k_pileup_fast launch over every tile (nullptr: none was written)
const u32 *pileup_deep_list(const cov_session *s) { return s->use_fast && s->deep_min != 0u ? s->d_deep_list.p : nullptr; }

// k_pileup_fast over every tile (it skips the ones k_ranges flagged TILE_F_SLOW)
template <bool H, int TABLES>
void launch_fast_v(cov_session *s, const PileupArgs &a, u32 n_tiles) {
    const auto kern = TABLES == 1 ? &k_pileup_fast<H> : &k_pileup_fast2t<H>;
    const size_t smem = pileup_fast_smem_bytes(H, TABLES == 1 ? FAST_HB : FAST_HB7, TABLES);
    static std::atomic<int> occ_dev[64];
    const int occ = pileup_occupancy(s, occ_dev, reinterpret_cast<const void *>(kern), smem);
    // the list holds tile numbers of the whole sample: only a launch over all of it, from tile 0, may take it
    const u32 *deep_list = a.tile_base == 0u && n_tiles == s->n_tiles ? pileup_deep_list(s) : nullptr;
    const u32 chunk = (u32)(deep_list != nullptr ? s->chunk_tiles_listed : s->chunk_tiles);
    constexpr u32 WGW = psched::FAST_WG_WAVES;      // (occ = resident workgroups of 256 threads per CU: registers bound residency, so 4 x occ waves)
    const u32 grid = psched::grid_of(n_tiles, chunk, (u32)s->n_cus, (u32)occ * 4u, WGW);
    s->last_pileup_waves = grid * WGW; s->last_pileup_chunk = chunk;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64u * WGW), smem / 4u * WGW, s->stream, a, n_tiles, chunk, deep_list, (const u32 *)&s->d_glob.p->n_deep);
}
template <bool H>
void launch_fast_t(cov_session *s, const PileupArgs &a, u32 n_tiles) {
    if (s->fast_tables == 2) launch_fast_v<H, 2>(s, a, n_tiles);
    else launch_fast_v<H, 1>(s, a, n_tiles);
}

template <bool H, bool W>
void launch_stream_t(cov_session *s, const PileupArgs &a, u32 n_tiles, bool slow_list_only = false) {
    const size_t smem = pileup_stream_smem_bytes();
    static std::atomic<int> occ_dev[64];
    const int occ = pileup_occupancy(s, occ_dev, reinterpret_cast<const void *>(&k_pileup_stream<H, W>), smem);
    if (slow_list_only) {   // the listed tiles only, one per wave step; the count lives on the device (usually 0: waves exit at once)
        hipLaunchKernelGGL((k_pileup_stream<H, W>), dim3((u32)s->n_cus), dim3(256), smem, s->stream, a, 0u, 1u,
                           (const u32 *)s->d_slow_list.p, (const u32 *)&s->d_glob.p->n_slow);
        return;
    }
    hipLaunchKernelGGL((k_pileup_stream<H, W>), dim3(pileup_grid(s, occ, n_tiles)), dim3(256), smem, s->stream, a, n_tiles, (u32)s->chunk_tiles,
                       (const u32 *)nullptr, (const u32 *)nullptr);
}
// dispatches to the configured pileup kernel
template <bool H, bool W>
void launch_any_pileup(cov_session *s, const PileupArgs &a, u32 n_tiles) {
    if (s->use_fast && !W) {
        launch_fast_t<H>(s, a, n_tiles);
        launch_stream_t<H, W>(s, a, n_tiles, true);
    } else launch_stream_t<H, W>(s, a, n_tiles);
}

const uint8_t *device_mask(const cov_session *s) { return s->have_mask ? s->d_mask.p : nullptr; }

// The compact histogram from the arena's bins: the contigs' compact offsets (a block's total, then its scan), then the bins moved
// (d_hist_top and d_chist are sized by the caller: inside a finish, or on the first cov_fetch_hist behind one that left the bins in the arena)
void launch_hist_compact(cov_session *s, const uint8_t *mask, u64 excl) {
    const u32 nT = s->n_targets, hb = (nT + 1023u) / 1024u;
    hipLaunchKernelGGL((k_hist_sum<1>), dim3(hb), dim3(1024), 0, s->stream, (const DevContig *)s->d_ctg.p, nT, s->d_tlen.p, mask, excl, s->d_hist_top.p);
    hipLaunchKernelGGL((k_hist_off<1>), dim3(hb), dim3(1024), 0, s->stream, s->d_ctg.p, nT, s->d_tlen.p, mask, excl, (const u64 *)s->d_hist_top.p, s->d_glob.p);
    hipLaunchKernelGGL(k_hist_compact, dim3((nT + 3u) / 4u), dim3(256), 0, s->stream, s->d_ctg.p, nT, s->d_tlen.p, excl, s->d_arena.p, s->d_chist.p);
}

PileupArgs pileup_args(cov_session *s) {
    PileupArgs a{};
    a.tile_contig = s->d_tile_contig.p; a.tile_start = s->d_tile_start.p; a.desc = s->d_desc.p;
    a.runs = s->d_runs.p; a.cx_runs = s->d_cx_runs.p; a.r = records_of(s); a.ctg = s->d_ctg.p; a.g = s->d_glob.p;
    a.hist_arena = s->d_arena.p; a.excl = s->cfg.contig_end_exclusion; a.depth_out = nullptr; a.tile_base = 0;
    return a;
}

using finplan::FinishPlan;
static_assert(finplan::LEAN_PASSES == 2 * PREP_PASSES, "finish_plan_core.h sizes k_prep_lean's workgroups");

// The device views of one pass over the store, built once (stage_begin) and read by every stage.
struct PassViews {
    hipStream_t st = nullptr;
    u32 R = 0, nT = 0;
    Records r{};
    const uint8_t *mask = nullptr;     // the target mask on the device, when there is one
    u64 excl = 0;                      // cov_config::contig_end_exclusion
    TileIdx ti{};
    CxIdx cx{};
    double *idp = nullptr, *idn = nullptr;      // identity streams actually needed (NULL = skipped by k_prep and the k_id_* kernels)
    FilterCfg f{};
    PrepArgs pa{};
    size_t block = 0;                  // bytes of [DevGlobal][DevContig x nT]: the estimators' floats lie behind it, in d_res and in h_res
};

// The prep kernels of one <IDENTITY, FILTER, MASKED>: k_prep7s, or k_prep_generic over every step, or k_prep_lean and k_prep_generic over its list.
template <bool ID, bool FI, bool MA>
void launch_prep(cov_session *s, const FinishPlan &p, const PassViews &v) {
    const PrepArgs *pa = s->d_prep_args.p;
    if (p.prep7)
        hipLaunchKernelGGL((k_prep7s<ID, FI, MA>), dim3(p.prep_grid), dim3(256), 0, v.st, v.r, s->d_tlen.p, v.nT, v.mask, v.f, s->d_ctg.p,
                           s->d_glob.p, s->d_runs.p, v.idp, v.idn, s->d_part.p, v.ti, p.prep_passes, p.prep_b, v.cx.list, v.cx.list_cap);
    else if (p.gen_all)
        hipLaunchKernelGGL((k_prep_generic<ID, FI, MA>), dim3(p.gen_grid), dim3(256), 0, v.st, pa, p.n_steps);
    else {
        hipLaunchKernelGGL((k_prep_lean<ID, FI, MA>), dim3(p.prep_grid), dim3(256), 0, v.st, v.pa.hot, pa);
        hipLaunchKernelGGL((k_prep_generic<ID, FI, MA>), dim3(p.gen_grid), dim3(256), 0, v.st, pa, 0u);
    }
}
// key = IDENTITY << 2 | FILTER << 1 | MASKED: one bit after the other becomes a template argument, which names the eight instantiations
template <int KEY = 0, int BIT = 4>
void launch_prep_key(int key, cov_session *s, const FinishPlan &p, const PassViews &v) {
    if constexpr (BIT == 0) launch_prep<(KEY & 4) != 0, (KEY & 2) != 0, (KEY & 1) != 0>(s, p, v);
    else if (key & BIT) launch_prep_key<KEY | BIT, BIT / 2>(key, s, p, v);
    else launch_prep_key<KEY, BIT / 2>(key, s, p, v);
}

// The device-wide exclusive scan of scan_ops.hip.h over items [0, n) of f, in two halves, since some callers read the total on the host between
// them.  scan_offsets: bsum (scan_blocks(n) + 1 words, the caller's) receives the blocks' exclusive prefixes and *total64 the grand total.
// scan_apply: out(i, exclusive prefix of item i) for every item.  Two launches and one; neither allocates.
constexpr u32 scan_blocks(u32 n) { return (n + covsc::SCAN_BLOCK - 1) / covsc::SCAN_BLOCK; }
template <typename F>
void scan_offsets(hipStream_t st, F f, u32 n, u32 *bsum, u64 *total64) {
    const u32 nb = scan_blocks(n);
    hipLaunchKernelGGL((covsc::k_scan_sums<F>), dim3(nb), dim3(256), 0, st, f, n, bsum);
    hipLaunchKernelGGL(covsc::k_scan_offsets, dim3(1), dim3(1024), 0, st, bsum, nb, total64);
}
template <typename F, typename O>
void scan_apply(hipStream_t st, F f, O out, u32 n, const u32 *bsum) {
    hipLaunchKernelGGL((covsc::k_scan_apply<F, O>), dim3(scan_blocks(n)), dim3(256), 0, st, f, out, n, bsum);
}

}  // namespace

extern "C" {

int cov_abi_version(void) { return COVERMHIP_ABI_VERSION; }

const char *cov_last_error(const cov_session *s) { return s ? s->err.c_str() : g_create_error.c_str(); }

static hipError_t ingest_prepare_(cov_session *s) { return s->ing.create(s->cfg.device); }
// Everything that looks at the ingest's streams outside cov_ingest_begin waits for the helper first.
static hipError_t ingest_prep_wait(cov_session *s) { return s->ing.prep.valid() ? s->ing.prep.get() : hipSuccess; }

cov_status cov_create(const cov_config *cfg, cov_session **out) {
    if (!cfg || !out) { g_create_error = "null argument"; return COV_ERR_INVALID_ARG; }
    *out = nullptr;
    const bool timing = cov_timing_on();
    const auto tc0 = std::chrono::steady_clock::now();
    auto stamp = [&](const char *what) { if (timing) fprintf(stderr, "[covermhip] cov_create: %s at %.4fs\n", what, std::chrono::duration<double>(std::chrono::steady_clock::now() - tc0).count()); };
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    stamp("hipGetDeviceCount (runtime initialised)");
    if (e != hipSuccess || ndev <= 0) {
        g_create_error = std::string("no usable HIP device: ") + hipGetErrorString(e) +
                         " (the engine has no CPU fallback)";
        return COV_ERR_HIP;
    }
    if (cfg->device < 0 || cfg->device >= ndev) { g_create_error = "device ordinal out of range"; return COV_ERR_INVALID_ARG; }
    e = hipSetDevice(cfg->device);
    if (e != hipSuccess) { g_create_error = std::string("hipSetDevice: ") + hipGetErrorString(e); return COV_ERR_HIP; }
    cov_session *s = new cov_session();
    s->cfg = *cfg;
    {
        const char *mode = getenv("COVERM_PILEUP");      // "stream": k_pileup_stream over every tile (the second kernel behind k_pileup_fast, alone: tests)
        if (mode && !strcmp(mode, "stream")) s->use_fast = false;
        s->tile = STREAM_TW;
        stamp("hipSetDevice");
        int cus = 0;      // (hipGetDeviceProperties fills a kilobyte of fields from many driver queries; one attribute is all that is needed)
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, cfg->device) == hipSuccess && cus > 0) s->n_cus = cus;
        stamp("device attribute");
    }
    if (cfg->want & COV_WANT_INGEST) s->ing.prep = std::async(std::launch::async, [s] { return ingest_prepare_(s); });
    if (const char *el = getenv("COVERM_EST_LANES")) s->est_lanes = atoi(el) ? 1 : 0;
    if (const char *ft = getenv("COVERM_FAST_TABLES")) s->fast_tables = atoi(ft) == 2 ? 2 : 1;
    if (const char *pk = getenv("COVERM_PREP_KERNEL")) s->prep_kernel = atoi(pk) == 7 ? 7 : 0;
    if (const char *im = getenv("COVERM_IDENTITY")) s->id_mode = strcmp(im, "serial") ? 1 : 0;
    { long long v; if (covknob::get("store_cap_records", v) && v >= 1) s->cap_records = std::min<uint64_t>((uint64_t)v, 0xfffffff0ull); }
    { long long v; if (covknob::get("store_cap_cigar", v) && v >= 1) s->cap_cigar = std::min<uint64_t>((uint64_t)v, 0xfffffff0ull); }
    { long long v; if (covknob::get("pileup_chunk_tiles", v) && v >= 1 && v <= 64) s->chunk_tiles = s->chunk_tiles_listed = (int)v; }
    { long long v; if (covknob::get("pileup_deep_min", v) && v >= 0 && v <= 0x7fffffffll) s->deep_min = (uint32_t)v; }
    { long long v; if (covknob::get("depth_chunk_bases", v) && v >= 4) s->dr.chunk_bases = (uint64_t)v; }
    // (every stream costs ~6 ms to create and as much again when the process ends, tools/ubench/exit_probe: the side stream of the
    // identity kernels is created by the first cov_finish that wants it, and borrows the ingest's second stream when there is one)
    e = hipEventCreateWithFlags(&s->ev_prep_done, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&s->ev_side_done, hipEventDisableTiming);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { g_create_error = std::string("hipStreamCreate: ") + hipGetErrorString(e); (void)ingest_prep_wait(s); delete s; return COV_ERR_HIP; }
    stamp("streams and events");      // (the kernels' timing events are created by the first cov_finish: a run that ingests a file needs them half a second later)
    e = bind_result_block(s, 1);
    if (e != hipSuccess) { g_create_error = std::string("hipMalloc: ") + hipGetErrorString(e); cov_destroy(s); return COV_ERR_HIP; }
    stamp("first hipMalloc");
    *out = s;
    return COV_OK;
}

static void ingest_free_buffers(cov_session *s) {
    s->ing.free_buffers();
    for (auto &b : s->m_text) b.release();      // (the SAM text ingest's window: text, masks, line arrays)
    s->m_nl.release(); s->m_tab.release(); s->m_line_end.release(); s->m_cnt.release(); s->m_rec_idx.release(); s->m_cig_idx.release();
}

void cov_destroy(cov_session *s) {
    if (!s) return;
    (void)ingest_prep_wait(s);
    (void)hipSetDevice(s->cfg.device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    s->d_tlen.release(); s->d_tile_contig.release(); s->d_tile_start.release(); s->d_mask.release();
    s->d_grow.release(); s->d_gtids.release(); s->d_gseg_genome.release(); s->d_gseg_start.release(); s->d_genomes.release(); s->d_ghist.release(); s->d_ghist_top.release(); s->d_order.release();
    s->d_sgid.release(); s->d_sblk.release(); s->d_sent_pos.release(); s->d_stop_last1.release(); s->d_stop_first.release(); s->d_scounts.release(); s->d_scode.release();
    s->d_stop_cnt.release(); s->d_stop_seg.release(); s->d_sent.release();
    s->d_gout.release(); if (s->h_gout) (void)hipHostFree(s->h_gout); s->h_gout = nullptr;
    s->d_tile_first.release(); s->d_tcnt.release(); s->d_fov.release(); s->d_tscan.release(); s->d_ttop.release(); s->d_slow_list.release(); s->d_deep_list.release();
    s->dr.release(); s->d_ctg_scratch.release(); s->d_depth_all.release(); s->d_depth_off.release(); s->d_iv.release(); s->d_ivst.release(); s->d_ivhist.release();
    s->gr_code.release(); s->gr_mism.release(); s->gr_trec.release(); s->gr_pprim.release(); s->gr_tids.release(); s->gr_ttid.release(); s->gr_tpos.release(); s->gr_ident.release();
    s->gr_tident.release(); s->gr_ck.release(); s->gr_bcnt.release(); s->gr_bmism.release(); s->gr_pmism.release(); s->gr_glob.release(); s->gr_iv.release(); s->gr_out.release(); s->gr_bounds.release();
    s->d_cx_list.release(); s->d_cx_cnt.release(); s->d_cx_cur.release(); s->d_cx_scan.release(); s->d_cx_top.release(); s->d_cx_runs.release();
    if (s->side) {     // before ing.aux goes: `side` may be that very stream (stage_identity_side borrows the idle ingest stream)
        (void)hipStreamSynchronize(s->side);
        if (s->side_owned) (void)hipStreamDestroy(s->side);
        s->side = nullptr; s->side_owned = false;
    }
    s->ing.destroy();
    for (hipEvent_t e : s->sam_buf_free) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : s->sam_ev) if (e) (void)hipEventDestroy(e);
    for (auto &b : s->m_text) b.release();
    s->m_blob.release(); s->m_nl.release(); s->m_tab.release(); s->m_res.release(); s->m_noff.release(); s->m_line_end.release(); s->m_cnt.release();
    s->m_rec_idx.release(); s->m_cig_idx.release(); s->m_slots.release(); for (auto &b : s->m_bsum) b.release();
    s->d_res.release(); s->d_ctg.p = nullptr; s->d_glob.p = nullptr; s->d_desc.release(); s->d_gather.release();
    if (s->h_gather) (void)hipHostFree(s->h_gather);
    s->h_gather = nullptr;
    result_host_take(s);
    if (s->h_res) (void)hipHostFree(s->h_res);
    s->h_res = nullptr; s->h_res_cap = 0; s->h_ctg = nullptr;
    if (s->h_chist) (void)hipHostFree(s->h_chist);
    s->h_chist = nullptr; s->h_chist_cap = 0;
    s->h_estf = nullptr; s->store.release();
    s->d_runs.release(); s->d_part.release(); s->d_prep_args.release(); s->d_gen_list.release(); s->d_hist_top.release(); s->d_ident.release(); s->d_identp.release(); s->d_idch.release();
    if (s->ev_prep_done) (void)hipEventDestroy(s->ev_prep_done);
    if (s->ev_side_done) (void)hipEventDestroy(s->ev_side_done); s->d_arena.release(); s->d_chist.release(); s->d_depth.release();
    for (int k = 0; k < COV_K_COUNT; k++)
        for (int j = 0; j < 2; j++) if (s->ev[k][j]) (void)hipEventDestroy(s->ev[k][j]);
    if (s->stream) (void)hipStreamDestroy(s->stream);
    delete s;
}

// Genomes off.  Estimators that were valid for genome entries only (ANIr over the not-supplementary identity sum: the per-contig
// k_estimate reads the primary-read sum, which such a session never computes) are dropped with them: set them again.
static void genomes_off(cov_session *s) {
    if (s->have_genomes && (s->cfg.want & COV_WANT_IDENTITY_NONSUPP_ONLY))
        for (uint32_t k = 0; k < s->est.n; k++)
            if (s->est.e[k].kind == COV_EST_ANIR) { s->est = EstParams{}; s->est_valid = false; break; }
    s->have_genomes = false; s->have_runs = false; s->gen_valid = false;
}
cov_status cov_set_targets(cov_session *s, uint32_t n_targets, const uint64_t *target_len) {
    if (!s || (!target_len && n_targets)) return COV_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(s->cfg.device));
    s->n_targets = n_targets;
    s->h_tlen.resize(n_targets);
    s->h_tile_first.assign((size_t)n_targets + 1, 0);
    uint64_t nt = 0;
    for (uint32_t c = 0; c < n_targets; c++) {
        if (target_len[c] > 0x7fffffffull) { s->err = "target length exceeds BAM's i32 range"; return COV_ERR_INVALID_ARG; }
        s->h_tlen[c] = (uint32_t)target_len[c];
        s->h_tile_first[c] = (uint32_t)nt;
        nt += (target_len[c] + (uint64_t)s->tile - 1) / (uint64_t)s->tile;
    }
    if (nt >= 0x7fffffffull) { s->err = "too many tiles"; return COV_ERR_INVALID_ARG; }
    s->h_tile_first[n_targets] = (uint32_t)nt;
    s->n_tiles = (uint32_t)nt;
    std::vector<u32> tc(nt), ts(nt);
    for (uint32_t c = 0; c < n_targets; c++) {
        u32 k = s->h_tile_first[c];
        for (uint64_t p = 0; p < target_len[c]; p += (uint64_t)s->tile, k++) { tc[k] = c; ts[k] = (u32)p; }
    }
    HIPCHK(s->d_tlen.reserve(std::max<size_t>(1, n_targets), s->stream));
    HIPCHK(s->d_tile_contig.reserve(std::max<size_t>(1, nt), s->stream));
    HIPCHK(s->d_tile_start.reserve(std::max<size_t>(1, nt), s->stream));
    HIPCHK(s->d_desc.reserve(std::max<size_t>(2, 2 * nt), s->stream));
    HIPCHK(s->d_tile_first.reserve((size_t)n_targets + 1, s->stream));
    HIPCHK(s->d_tcnt.reserve(std::max<size_t>(1, nt), s->stream)); HIPCHK(s->d_fov.reserve(std::max<size_t>(1, nt), s->stream));
    HIPCHK(s->d_tscan.reserve(std::max<size_t>(1, nt), s->stream)); HIPCHK(s->d_ttop.reserve(nt / 1024 + 2, s->stream));
    HIPCHK(s->d_slow_list.reserve(std::max<size_t>(1, nt), s->stream));
    HIPCHK(s->d_deep_list.reserve(std::max<size_t>(1, nt), s->stream));
    HIPCHK(s->d_cx_cnt.reserve(std::max<size_t>(1, nt), s->stream)); HIPCHK(s->d_cx_cur.reserve(std::max<size_t>(1, nt), s->stream));
    HIPCHK(s->d_cx_scan.reserve(std::max<size_t>(1, nt), s->stream)); HIPCHK(s->d_cx_top.reserve(nt / 1024 + 2, s->stream));
    HIPCHK(hipMemcpyAsync(s->d_tile_first.p, s->h_tile_first.data(), ((size_t)n_targets + 1) * 4, hipMemcpyHostToDevice, s->stream));
    s->tile_shift = 0;
    while ((1u << s->tile_shift) < (uint32_t)s->tile) s->tile_shift++;
    HIPCHK(bind_result_block(s, n_targets));
    if (n_targets) HIPCHK(hipMemcpyAsync(s->d_tlen.p, s->h_tlen.data(), (size_t)n_targets * 4, hipMemcpyHostToDevice, s->stream));
    if (nt) {
        HIPCHK(hipMemcpyAsync(s->d_tile_contig.p, tc.data(), nt * 4, hipMemcpyHostToDevice, s->stream));
        HIPCHK(hipMemcpyAsync(s->d_tile_start.p, ts.data(), nt * 4, hipMemcpyHostToDevice, s->stream));
    }
    HIPCHK(hipStreamSynchronize(s->stream));
    s->have_mask = false;
    genomes_off(s);
    s->finished = false;
    s->dr.h_reg.clear(); s->dr.h_reg_input.clear(); s->dr.h_reg_first.clear(); s->dr.have_regions = false; s->dr.regs_valid = false;      // the regions were validated against the targets before
    if (n_targets >= 65536u && !s->h_res_prep.valid() && result_host_bytes(s, n_targets) > s->h_res_cap) {
        const size_t need = result_host_bytes(s, n_targets);
        const int dev = s->cfg.device;
        s->h_res_prep = std::async(std::launch::async, [need, dev]() -> std::pair<uint8_t *, size_t> {
            uint8_t *p = nullptr;
            if (hipSetDevice(dev) != hipSuccess || hipHostMalloc((void **)&p, need, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return {nullptr, 0}; }
            return {p, need};
        });
    }
    return COV_OK;
}

static cov_status set_target_mask_(cov_session *s, const uint8_t *mask);
cov_status cov_set_target_mask(cov_session *s, const uint8_t *mask) {
    if (!s) return COV_ERR_INVALID_ARG;
    genomes_off(s);
    return set_target_mask_(s, mask);
}
static cov_status set_target_mask_(cov_session *s, const uint8_t *mask) {
    HIPCHK(hipSetDevice(s->cfg.device));
    s->gen_valid = false;
    if (!mask) { s->have_mask = false; s->h_mask.clear(); return COV_OK; }
    s->h_mask.assign(mask, mask + s->n_targets);
    HIPCHK(s->d_mask.reserve(std::max<size_t>(1, s->n_targets), s->stream));
    if (s->n_targets) HIPCHK(hipMemcpyAsync(s->d_mask.p, mask, s->n_targets, hipMemcpyHostToDevice, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    s->have_mask = true;
    s->finished = false;
    return COV_OK;
}

// The table genome -> targets: a counting sort of the targets by genome (stable, so a row holds ascending tids), rows cut into segments.
// Built on the host at every call (cov_set_targets drops it, so once per sample in the CLI), like the tile tables of cov_set_targets, and
// kept on the device.
cov_status cov_set_genomes(cov_session *s, const int32_t *genome_of_tid, uint32_t n_genomes) {
    if (!s) return COV_ERR_INVALID_ARG;
    if (!genome_of_tid || n_genomes == 0) return cov_set_target_mask(s, nullptr);
    const u32 nT = s->n_targets;
    for (uint32_t k = 0; k < s->est.n; k++)
        if (s->est.e[k].kind == COV_EST_ANIR && (s->cfg.want & COV_WANT_IDENTITY_PRIMARY_ONLY)) {
            s->err = "cov_set_genomes: ANIr of a genome needs COV_WANT_IDENTITY with the not-supplementary sum (genome.rs:220)"; return COV_ERR_INVALID_ARG;
        }
    std::vector<uint8_t> mask(nT);
    std::vector<u32> row((size_t)n_genomes + 1, 0);
    for (u32 t = 0; t < nT; t++) {
        const int32_t g = genome_of_tid[t];
        if (g < -1 || (g >= 0 && (uint32_t)g >= n_genomes)) { s->err = "cov_set_genomes: genome index outside [-1, n_genomes)"; return COV_ERR_INVALID_ARG; }
        mask[t] = g >= 0;
        if (g >= 0) row[(size_t)g + 1]++;
    }
    for (uint32_t g = 0; g < n_genomes; g++) row[g + 1] += row[g];
    std::vector<u32> tids(std::max<u32>(row[n_genomes], 1u)), cur(row.begin(), row.end() - 1), seg_genome, seg_start;
    for (u32 t = 0; t < nT; t++) if (genome_of_tid[t] >= 0) tids[cur[genome_of_tid[t]]++] = t;
    for (uint32_t g = 0; g < n_genomes; g++)
        for (u32 i = row[g]; i < row[g + 1]; i += GENOME_SEG) { seg_genome.push_back(g); seg_start.push_back(i); }
    s->have_runs = false;
    const cov_status m = set_target_mask_(s, mask.data());
    if (m != COV_OK) return m;
    const size_t n_seg = seg_genome.size();
    hipStream_t st = s->stream;
    HIPCHK(s->d_grow.reserve(row.size(), st)); HIPCHK(s->d_gtids.reserve(tids.size(), st));
    HIPCHK(s->d_gseg_genome.reserve(std::max<size_t>(1, n_seg), st)); HIPCHK(s->d_gseg_start.reserve(std::max<size_t>(1, n_seg), st));
    HIPCHK(s->d_genomes.reserve(n_genomes, st));
    HIPCHK(s->d_ghist_top.reserve((size_t)(n_genomes + 1023u) / 1024u + 1, st));
    HIPCHK(s->d_gout.reserve((size_t)n_genomes * (sizeof(cov_genome_stats) + COV_EST_MAX * sizeof(float)), st));
    HIPCHK(hipMemcpyAsync(s->d_grow.p, row.data(), row.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(s->d_gtids.p, tids.data(), tids.size() * 4, hipMemcpyHostToDevice, st));
    if (n_seg) {
        HIPCHK(hipMemcpyAsync(s->d_gseg_genome.p, seg_genome.data(), n_seg * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(s->d_gseg_start.p, seg_start.data(), n_seg * 4, hipMemcpyHostToDevice, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    const size_t need = (size_t)n_genomes * (sizeof(cov_genome_stats) + COV_EST_MAX * sizeof(float));
    if (need > s->h_gout_cap) HIPCHK(pinned_grow(s->h_gout, s->h_gout_cap, need));
    s->n_genomes = n_genomes; s->n_gseg = (uint32_t)n_seg;
    s->have_genomes = true;
    return COV_OK;
}

// The header's part of the separator scan: gid[] and blk[] (first tid of each maximal run of equal gid), and every buffer the per-finish
// table and its results can need — an entry starts in a run of its own, so the runs bound the entries — so that no finish allocates a
// k_sep_* or per-entry buffer (the merged histogram, sized by the records, still grows with the sample as for cov_set_genomes).
cov_status cov_set_genome_runs(cov_session *s, const int32_t *gid_of_tid, uint32_t n_gids) {
    if (!s) return COV_ERR_INVALID_ARG;
    if (!gid_of_tid || n_gids == 0) return cov_set_target_mask(s, nullptr);
    const u32 nT = s->n_targets;
    std::vector<u32> blk(std::max<u32>(nT, 1u));
    u32 n_runs = 0;
    for (u32 t = 0; t < nT; t++) {
        if (gid_of_tid[t] < 0 || (uint32_t)gid_of_tid[t] >= n_gids) { s->err = "cov_set_genome_runs: genome id outside [0, n_gids)"; return COV_ERR_INVALID_ARG; }
        if (t != 0 && gid_of_tid[t] == gid_of_tid[t - 1]) blk[t] = blk[t - 1]; else { blk[t] = t; n_runs++; }
    }
    genomes_off(s);
    const cov_status m = set_target_mask_(s, nullptr);
    if (m != COV_OK) return m;
    hipStream_t st = s->stream;
    const size_t nT1 = std::max<size_t>(nT, 1), ent_cap = std::max<u32>(n_runs, 1u), seg_cap = ent_cap + nT / GENOME_SEG + 1, nb = (nT1 + SEP_TILE - 1) / SEP_TILE;
    HIPCHK(s->d_sgid.reserve(nT1, st)); HIPCHK(s->d_sblk.reserve(nT1, st)); HIPCHK(s->d_scode.reserve(nT1, st)); HIPCHK(s->d_sent_pos.reserve(nT1, st));
    HIPCHK(s->d_gtids.reserve(nT1, st)); HIPCHK(s->d_grow.reserve(ent_cap + 1, st)); HIPCHK(s->d_sent.reserve(ent_cap, st));
    HIPCHK(s->d_gseg_genome.reserve(seg_cap, st)); HIPCHK(s->d_gseg_start.reserve(seg_cap, st));
    HIPCHK(s->d_stop_last1.reserve(nb, st)); HIPCHK(s->d_stop_first.reserve(nb, st)); HIPCHK(s->d_stop_cnt.reserve(nb, st));
    HIPCHK(s->d_stop_seg.reserve((ent_cap + SEP_TILE - 1) / SEP_TILE, st)); HIPCHK(s->d_scounts.reserve(SEP_N_COUNTS, st));
    HIPCHK(s->d_genomes.reserve(ent_cap, st)); HIPCHK(s->d_order.reserve((nT1 + 1023) / 1024 + 2, st));
    HIPCHK(s->d_ghist_top.reserve((ent_cap + 1023u) / 1024u + 1, st));
    const size_t per = sizeof(cov_genome_stats) + COV_EST_MAX * sizeof(float) + sizeof(SepEntry), need = ent_cap * per + 16;
    HIPCHK(s->d_gout.reserve(ent_cap * per, st));
    if (nT) {
        HIPCHK(hipMemcpyAsync(s->d_sgid.p, gid_of_tid, (size_t)nT * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(s->d_sblk.p, blk.data(), (size_t)nT * 4, hipMemcpyHostToDevice, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    if (need > s->h_gout_cap) HIPCHK(pinned_grow(s->h_gout, s->h_gout_cap, need));
    s->finished = false;
    s->n_gids = n_gids; s->sep_ent_cap = (uint32_t)ent_cap; s->sep_seg_cap = (uint32_t)seg_cap; s->n_genomes = 0;
    s->have_runs = true;
    return COV_OK;
}

cov_status cov_push_batch(cov_session *s, const cov_batch *b) {
    if (!s || !b) return COV_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(s->cfg.device));
    if (s->ing.active) { const cov_status a = cov_ingest_abort(s); if (a != COV_OK) return a; }   // an ingest left open: its queued work may still write the store
    { const cov_status st = materialise_adopted(s); if (st) return st; }
    return append(s, b, false);
}

cov_status cov_push_batch_device(cov_session *s, const cov_batch *b) {
    if (!s || !b) return COV_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(s->cfg.device));
    if (s->store.n_records == 0 && !s->adopted) {
        if (b->n_records >= 0xfffffff0ull) { s->err = "more than 2^32 records in one session"; return COV_ERR_INVALID_ARG; }
        u32 o0 = 0, o1 = 0;
        if (b->n_records) {
            HIPCHK(hipMemcpy(&o0, b->cigar_off, 4, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(&o1, b->cigar_off + b->n_records, 4, hipMemcpyDeviceToHost));
        }
        s->adopted = true; s->adopted_batch = *b; s->store.n_records = b->n_records;
        s->adopted_ncig = (uint64_t)o1 - o0;
        s->adopted_cig_end = o1;
        s->finished = false;
        return COV_OK;
    }
    { const cov_status st = materialise_adopted(s); if (st) return st; }
    return append(s, b, true);
}

// Abandons an ingest between cov_ingest_begin and cov_ingest_end: everything queued on the ingest streams (uploads, inflate
// rounds, boundary search, extraction) is waited for, then the session is as if the ingest had never begun — the record
// store holds what it held before (extraction only ever writes behind n_records) and may be pushed to again.
cov_status cov_ingest_abort(cov_session *s) {
    if (!s) return COV_ERR_INVALID_ARG;
    if (!s->ing.active) return COV_OK;
    HIPCHK(hipSetDevice(s->cfg.device));
    s->ing.active = false; s->sam_active = false;
    for (hipStream_t st : {s->ing.copy, s->stream, s->ing.aux, s->ing.parse, s->ing.ext})
        if (st) HIPCHK(hipStreamSynchronize(st));
    s->ing.reset_for_file(IngestState::Reset::ABORT);
    if (s->ing.rec_spilled) {     // the store no longer holds what it held before the ingest: only cov_reset brings the session back
        s->ing.rec_spilled = 0;
        s->err = "cov_ingest_abort: part of the file had already left the bounded record store; cov_reset the session";
        return COV_ERR_STATE;
    }
    return COV_OK;
}

cov_status cov_reset(cov_session *s) {
    if (!s) return COV_ERR_INVALID_ARG;
    if (s->ing.active) {
        // an ingest that had already spilled part of its file: the abort drains the device and says "cov_reset the session" (COV_ERR_STATE) —
        // this IS that reset, so the status is expected here and everything below still has to be cleared
        const bool spilled = s->ing.rec_spilled != 0;
        const cov_status a = cov_ingest_abort(s);
        if (a != COV_OK && !(spilled && a == COV_ERR_STATE)) return a;
        if (a != COV_OK) s->err.clear();
    }
    s->adopted = false; s->store.n_records = 0; s->store.n_cigar = 0; s->finished = false; s->depth_all_valid = false; s->dr.drop(); s->store.mates_valid = 0; s->ing.was_span = false;
    s->spill.clear(); s->merged_valid = false; s->merged_hist.clear(); s->ing.rec_spilled = 0; s->spill_retry_at = 0; s->spill_est.clear(); s->est_valid = false; s->gen_valid = false;
    return COV_OK;
}

// The verdicts of a finished pipeline in their precedence: internal error, the order rule when it breaks no later than the first erroring
// record (the reference panics at the first offending record, in file order), that record's error.  unsorted_at = ~0: the order holds.
static cov_status record_verdict(cov_session *s, const DevGlobal &G, uint64_t unsorted_at, uint64_t rec_base) {
    if (G.internal_error) { s->err = "internal error: depth or histogram size exceeded its proven bound"; return COV_ERR_STATE; }
    uint64_t err_rec = ~0ull; int err_code = 0;
    if (G.first_error != ~0ull) { err_rec = G.first_error >> 8; err_code = (int)(G.first_error & 0xff); }
    if (unsorted_at != ~0ull && unsorted_at <= err_rec) {
        s->err = "BAM file appears to be unsorted. Input BAM files must be sorted by reference (i.e. by samtools sort)";
        return COV_ERR_UNSORTED;
    }
    if (err_code) {
        char b[256];
        const char *what = err_code == 2 ? "Mapping record encountered that does not have an 'NM' auxiliary tag in the SAM/BAM format"
                         : err_code == 3 ? "Unexpected data type of NM aux tag"
                         : err_code == 4 ? "aligned block starts at or beyond the end of its reference sequence"
                         : err_code == 7 ? "record refers to a reference id outside the header (Corrupt BAM file?)"
                                         : "invalid CIGAR operation";
        snprintf(b, sizeof b, "%s (record %llu)", what, (unsigned long long)(err_rec + rec_base));
        s->err = b;
        return (cov_status)err_code;
    }
    return COV_OK;
}
static void summary_of(const DevGlobal &G, uint64_t n_records, uint64_t hist_total, cov_summary *summary) {
    uint64_t prim = 0, cons = 0;
    for (u32 k = 0; k < COUNTER_SLOTS * 8; k++) { prim += G.prim_slots[k]; cons += G.cons_slots[k]; }
    summary->num_detected_primary_alignments = prim; summary->n_records = n_records; summary->n_considered = cons; summary->hist_total = hist_total;
}

// Host side of a finished pipeline: error checks in file order, sortedness, DevContig -> cov_contig_stats.  Used for the
// session's own results and for the blocks cov_gather collected from other ranks.
// `min_ok_tid` / `rec_base`: the session's own results after a spill (bounded record store) — a considered contig below the contig that
// was in flight at the last spill breaks the reference's order rule exactly like an interleaving inside one pass, and record indices
// count from the first record of the sample, not of the store.
static cov_status convert_results(cov_session *s, const DevGlobal &G, const DevContig *ctg, uint64_t n_records, cov_contig_stats *stats,
                                  cov_summary *summary, int64_t min_ok_tid = -1, uint64_t rec_base = 0) {
    const u32 nT = s->n_targets;
    const bool want_hist = s->cfg.want & COV_WANT_HIST;
    if (G.internal_error) return record_verdict(s, G, ~0ull, rec_base);
    // The two passes below walk every contig; above 64 k contigs (assemblies: 10^5 - 10^7 of them) they run on a few threads — each chunk
    // first leaves what the chunks behind it need from it (its largest last record, its histogram bins), then every chunk runs the
    // serial loop from the prefix of the chunks in front of it.  (One thread until round 6: 2 M contigs cost ~50 ms per finish.)
    const u32 n_chunks = nT >= 65536u ? std::min<u32>(8u, std::max<u32>(1u, std::thread::hardware_concurrency())) : 1u;
    const u32 per_chunk = (nT + n_chunks - 1) / std::max<u32>(n_chunks, 1u);
    auto chunked = [&](auto fn) {
        if (n_chunks <= 1) { fn(0u, 0u, nT); return; }
        std::vector<std::thread> th;
        for (u32 k = 1; k < n_chunks; k++) th.emplace_back([&, k] { fn(k, std::min(nT, k * per_chunk), std::min(nT, (k + 1) * per_chunk)); });
        fn(0u, 0u, std::min(nT, per_chunk));
        for (auto &t : th) t.join();
    };
    const bool want_hist_bins = want_hist;
    const u64 excl = s->cfg.contig_end_exclusion;
    std::vector<uint64_t> ch_last(n_chunks, 0), ch_bins(n_chunks, 0), ch_unsorted(n_chunks, ~0ull);
    std::vector<uint8_t> ch_any(n_chunks, 0);
    if (n_chunks > 1)
        chunked([&](u32 k, u32 lo, u32 hi) {
            uint64_t last = 0, bins = 0; bool any = false;
            for (u32 c = lo; c < hi; c++) {
                const DevContig &C = ctg[c];
                if (C.n_pass == 0) continue;
                last = any ? std::max<uint64_t>(last, C.last_rec) : C.last_rec; any = true;
                if (want_hist_bins) {
                    const u64 L = s->h_tlen[c];
                    if (2 * excl < L && (!s->have_mask || s->h_mask[c])) bins += C.max_d + 1u;
                }
            }
            ch_last[k] = last; ch_bins[k] = bins; ch_any[k] = any;
        });
    // sortedness: the considered records of successive touched contigs must not interleave
    // (contig.rs:129-132 panics when a considered record has tid < the previous considered tid)
    {
        chunked([&](u32 k, u32 lo, u32 hi) {
            uint64_t prev_last = 0; bool any = false; uint64_t unsorted_at = ~0ull;
            for (u32 j = 0; j < k; j++) if (ch_any[j]) { prev_last = any ? std::max(prev_last, ch_last[j]) : ch_last[j]; any = true; }
            for (u32 c = lo; c < hi; c++) {
                const DevContig &C = ctg[c];
                if (C.n_pass == 0) continue;
                if ((int64_t)c < min_ok_tid) unsorted_at = std::min<uint64_t>(unsorted_at, C.first_rec);      // tid < last_tid across a spill (contig.rs:129-132)
                if (any && C.first_rec < prev_last) unsorted_at = std::min<uint64_t>(unsorted_at, std::max<uint64_t>(C.first_rec, 0));
                prev_last = any ? std::max<uint64_t>(prev_last, C.last_rec) : C.last_rec;
                any = true;
            }
            ch_unsorted[k] = unsorted_at;
        });
        uint64_t unsorted_at = ~0ull;
        for (u32 k = 0; k < n_chunks; k++) unsorted_at = std::min(unsorted_at, ch_unsorted[k]);
        const cov_status v = record_verdict(s, G, unsorted_at, rec_base);
        if (v != COV_OK) return v;
    }
    uint64_t hist_total = 0;
    std::vector<uint64_t> ch_total(n_chunks, 0);
    chunked([&](u32 k, u32 lo, u32 hi) {
        uint64_t hist_run = 0;
        for (u32 j = 0; j < k; j++) hist_run += ch_bins[j];
        for (u32 c = lo; c < hi; c++) {
            const DevContig &C = ctg[c];
            cov_contig_stats &o = stats[c];
            memset(&o, 0, sizeof o);
            o.n_primary = C.n_primary; o.n_pass = C.n_pass; o.n_nonsupp = C.n_nonsupp;
            o.sum_nm = C.sum_nm; o.sum_indel = C.sum_indel;
            o.sum_identity_primary = C.id_primary; o.sum_identity_nonsupp = C.id_nonsupp;
            o.win_sum_d = C.sum_d; o.win_sum_d2 = C.sum_d2; o.win_covered = C.cov_win; o.full_covered = C.cov_full;
            o.first_record = C.first_rec; o.last_record = C.last_rec;
            if (C.n_pass) { o.first_record += rec_base; o.last_record += rec_base; }
            const u64 L = s->h_tlen[c];
            const u64 win_len = 2 * excl < L ? L - 2 * excl : 0;
            if (C.n_pass && win_len) {
                o.win_max_d = C.max_d;
                o.win_min_d = (C.proc_win < win_len || C.min_d == 0xffffffffu) ? 0u : C.min_d;
            }
            if (want_hist) {      // the compact histogram's layout (what k_hist_off<1> computes on the device when the bins are compacted there)
                const bool live = C.n_pass != 0 && (!s->have_mask || s->h_mask[c]);
                o.hist_len = (live && win_len) ? C.max_d + 1u : 0u; o.hist_off = hist_run; hist_run += o.hist_len;
            }
        }
        ch_total[k] = hist_run;
    });
    hist_total = ch_total[n_chunks - 1];
    if (summary) summary_of(G, n_records, hist_total, summary);
    return COV_OK;
}

// convert_results without the per-contig block (cov_finish_genomes): the same verdicts in the same precedence — internal error, the order
// rule when it breaks no later than the first erroring record, that record's error — from DevGlobal and k_order_check's word.
static cov_status verdict_results(cov_session *s, const DevGlobal &G, uint64_t unsorted_at, uint64_t n_records, cov_summary *summary) {
    const cov_status v = record_verdict(s, G, unsorted_at, 0);
    if (v == COV_OK && summary) summary_of(G, n_records, 0, summary);
    return v;
}

static cov_status finish_once(cov_session *s, cov_contig_stats *stats, cov_summary *summary, bool &again);

// The pipeline over what the store holds.  The buckets of long-CIGAR records are sized optimistically: a pass that finds them too
// small has already computed the exact need, grows the buffer and runs once more (at most once per growth of the workload).
static cov_status finish_store(cov_session *s, cov_contig_stats *stats, cov_summary *summary) {
    bool again = false;
    cov_status st = finish_once(s, stats, summary, again);
    if (s) s->last_passes = 1;
    if (st == COV_OK && again) { st = finish_once(s, stats, summary, again); s->last_passes = 2; }
    if (st == COV_OK && again) { s->err = "internal error: bucket sizing did not converge"; return COV_ERR_STATE; }
    return st;
}

static cov_status merge_spilled(cov_session *s, cov_contig_stats *stats, cov_summary *summary);

cov_status cov_finish(cov_session *s, cov_contig_stats *stats, cov_summary *summary) {
    covr::Range rr("cov_finish");
    if (s) s->merged_valid = false;
    cov_summary local;
    cov_status st = finish_store(s, stats, (s && s->spill.active && !summary) ? &local : summary);
    if (st == COV_OK && s->spill.active) st = merge_spilled(s, stats, summary ? summary : &local);
    return st;
}

cov_status cov_finish_genomes(cov_session *s, cov_summary *summary) {
    covr::Range rr("cov_finish_genomes");
    if (!s) return COV_ERR_INVALID_ARG;
    s->merged_valid = false;
    if (s->spill.active) { s->err = "cov_finish_genomes: part of the sample's contigs left the bounded record store: cov_finish, and aggregate on the host"; return COV_ERR_STATE; }
    s->lean_finish = true;
    const cov_status st = finish_store(s, nullptr, summary);
    s->lean_finish = false;
    return st;
}

// ---- one pass of the device pipeline over what the store holds.  Its decisions are taken once (finish_plan_core.h), its device views are
// built once (PassViews), and finish_once below is the list of its stages in stream order.
static finplan::Facts finish_facts(const cov_session *s) {
    finplan::Facts f;
    f.R = (u32)s->store.n_records; f.nT = s->n_targets; f.n_tiles = s->n_tiles;
    f.ncig = s->adopted ? s->adopted_ncig : s->store.n_cigar;
    f.want = s->cfg.want; f.est_n = s->est.n; f.est_lanes_knob = s->est_lanes; f.prep_kernel = s->prep_kernel; f.n_cus = s->n_cus;
    f.have_mask = s->have_mask; f.have_runs = s->have_runs; f.have_genomes = s->have_genomes;
    f.spill_active = s->spill.active; f.in_spill = s->in_spill; f.lean_finish = s->lean_finish; f.hist_fetch_seen = s->hist_fetch_seen;
    return f;
}

static FilterCfg filter_of(const cov_config &c) {
    FilterCfg f{};
    f.include_improper_pairs = c.include_improper_pairs; f.include_supplementary = c.include_supplementary;
    f.include_secondary = c.include_secondary; f.filter_single = c.filter_single;
    f.min_mapq = c.min_mapq; f.min_aligned_length = c.min_aligned_length;
    f.min_percent_identity = c.min_percent_identity; f.min_aligned_percent = c.min_aligned_percent;
    return f;
}

// k_prep_lean's arguments (k_init writes them to device memory for its rare branches and for k_prep_generic), from the views filled so far
static PrepArgs prep_args_of(const cov_session *s, const FinishPlan &p, const PassViews &v) {
    PrepArgs pa{};
    const Records &r = v.r; const FilterCfg &f = v.f;
    PrepHot &ph = pa.hot;
    ph.tid = r.tid; ph.pos = r.pos; ph.flag = r.flag; ph.nmk = r.nm_kind; ph.nm = r.nm; ph.coff = r.cigar_off; ph.cigar = r.cigar; ph.mapq = r.mapq; ph.lseq = r.l_seq;
    ph.runs = s->d_runs.p; ph.tcnt = v.ti.tcnt; ph.fov = v.ti.fov; ph.identp = v.idp; ph.identn = v.idn;
    ph.n = r.n; ph.cigar_end = r.cigar_end; ph.n_targets = v.nT; ph.shift = v.ti.shift; ph.steps = p.prep_chunk / 256u;
    ph.gate_mask = 0x4u | (f.include_secondary ? 0u : 0x100u) | (f.include_supplementary ? 0u : 0x800u) | (f.include_improper_pairs ? 0u : 0x2u);
    ph.p1_mask = 0x4u | (f.include_secondary ? 0u : 0x100u) | (f.include_supplementary ? 0u : 0x800u);
    ph.min_mapq = f.min_mapq; ph.min_aligned_length = f.min_aligned_length; ph.min_percent_identity = f.min_percent_identity; ph.min_aligned_percent = f.min_aligned_percent;
    PrepCold &pc = pa.cold;
    pc.ctg = s->d_ctg.p; pc.g = s->d_glob.p; pc.part = s->d_part.p; pc.cx_list = v.cx.list; pc.mask = v.mask; pc.tlen = s->d_tlen.p; pc.tile_first = s->d_tile_first.p;
    pc.cx_list_cap = v.cx.list_cap; pc.gen_list = s->d_gen_list.p;
    return pa;
}

// Stage 1: the session's state of a pass, the buffers sized by the records, the views, k_init.
static cov_status stage_begin(cov_session *s, const FinishPlan &p, PassViews &v) {
    s->depth_all_valid = false; s->dr.drop();
    HIPCHK(hipSetDevice(s->cfg.device));
    timing_events(s);
    for (int k = 0; k < COV_K_COUNT; k++) { s->k_launches[k] = 0; s->k_ms[k] = 0.f; }
    s->est_valid = false; s->gen_valid = false;
    s->ev_fresh = -1;      // a new pass: no group's end event is the last thing on the stream
    hipStream_t st = v.st = s->stream;
    const u32 R = v.R = (u32)s->store.n_records, nT = v.nT = s->n_targets;
    HIPCHK(s->d_runs.reserve(std::max<size_t>(1, R), st));
    HIPCHK(s->d_part.reserve((size_t)p.prep_grid + 2, st));
    if (p.id_nonsupp) HIPCHK(s->d_ident.reserve(std::max<size_t>(1, R), st));
    if (p.id_primary) HIPCHK(s->d_identp.reserve(std::max<size_t>(1, R), st));
    if (p.want_id) HIPCHK(s->d_idch.reserve((size_t)R / ID_CH + 2, st));
    if (p.want_hist) HIPCHK(s->d_arena.reserve((size_t)R + nT + 1, st));
    HIPCHK(s->d_cx_list.reserve((size_t)(p.ncig / CX_MIN_OPS) + 64, st));
    HIPCHK(s->d_prep_args.reserve(1, st));
    HIPCHK(s->d_gen_list.reserve((size_t)R / 64 + 2, st));

    v.ti.tile_first = s->d_tile_first.p; v.ti.tcnt = s->d_tcnt.p; v.ti.fov = s->d_fov.p; v.ti.shift = s->tile_shift; v.ti.n_tiles = s->n_tiles;
    v.cx.list = s->d_cx_list.p; v.cx.list_cap = (u32)std::min<uint64_t>(p.ncig / CX_MIN_OPS + 64, 0xffffffffull);
    v.cx.cnt = s->d_cx_cnt.p; v.cx.cur = s->d_cx_cur.p; v.cx.cscan = s->d_cx_scan.p; v.cx.ctop = s->d_cx_top.p;
    v.cx.runs = s->d_cx_runs.p; v.cx.runs_cap = s->d_cx_runs.cap;
    v.r = records_of(s);
    v.mask = device_mask(s); v.excl = (u64)s->cfg.contig_end_exclusion;
    v.f = filter_of(s->cfg);
    v.idp = p.id_primary ? s->d_identp.p : nullptr;
    v.idn = p.id_nonsupp ? s->d_ident.p : nullptr;
    v.pa = prep_args_of(s, p, v);
    v.block = result_block_bytes(nT);
    hipLaunchKernelGGL(k_init, dim3((std::max(std::max(nT, COUNTER_SLOTS * 8), s->n_tiles) + 255) / 256), dim3(256), 0, st, s->d_ctg.p,
                       nT, s->d_glob.p, v.ti, v.cx, s->d_prep_args.p, v.pa);
    HIPCHK(hipGetLastError());
    return COV_OK;
}

// Stage 2 (there are records): filter, CIGAR summary, run words, tile index, per-contig counters.
static cov_status stage_prep(cov_session *s, const FinishPlan &p, const PassViews &v) {
    time_begin(s, COV_K_PREP);
    s->last_gen_all = p.gen_all;
    launch_prep_key((p.want_id ? 4 : 0) | (s->cfg.filter_single ? 2 : 0) | (v.mask != nullptr ? 1 : 0), s, p, v);
    if (v.nT) {   // what depends on k_prep alone, one launch: the workgroups' partial counters to their contigs (the identity kernels read them),
                  // and the long-CIGAR bucket counts per tile (waves stride over the RW_BUCKET list; nothing to do for short reads)
        const u32 n_red = p.gen_all ? 0u : (v.nT + 3u) / 4u, cx_grid0 = (u32)s->n_cus * 8u;
        hipLaunchKernelGGL(k_post_prep, dim3(n_red + cx_grid0), dim3(256), 0, v.st, v.r, s->d_tlen.p, s->d_glob.p, v.cx, v.ti, s->d_ctg.p, v.nT, (const PrepPartial *)s->d_part.p,
                           p.prep_grid, p.prep_chunk, n_red);
    }
    time_end(s, COV_K_PREP);
    HIPCHK(hipGetLastError());
    return COV_OK;
}

// Stage 3 (identity wanted, records and targets): the identity sums depend only on k_prep and run beside k_ranges / k_pileup on the side stream.
static cov_status stage_identity_side(cov_session *s, const PassViews &v) {
    const u32 R = v.R, nT = v.nT;
    if (!s->side) {
        (void)ingest_prep_wait(s);
        if (s->ing.aux && !s->ing.active) s->side = s->ing.aux;      // idle since cov_ingest_end
        else { HIPCHK(hipStreamCreateWithFlags(&s->side, hipStreamNonBlocking)); s->side_owned = true; }
    }
    HIPCHK(hipEventRecord(s->ev_prep_done, v.st));
    HIPCHK(hipStreamWaitEvent(s->side, s->ev_prep_done, 0));
    (void)hipEventRecord(s->ev[COV_K_IDENTITY][0], s->side);
    if (s->id_mode) {
        const u32 nch = (R + ID_CH - 1) / ID_CH;
        hipLaunchKernelGGL(k_id_approx, dim3(nch), dim3(256), 0, s->side, v.idp, v.idn, R, s->d_idch.p);
        hipLaunchKernelGGL(k_id_predict, dim3(nT), dim3(64), 0, s->side, s->d_ctg.p, nT, v.idp, v.idn, s->d_idch.p);
        hipLaunchKernelGGL(k_id_exact, dim3(nch), dim3(256), 0, s->side, v.idp, v.idn, R, s->d_idch.p);
        hipLaunchKernelGGL(k_id_combine, dim3(nT), dim3(64), 0, s->side, s->d_ctg.p, nT, v.idp, v.idn, v.r.tid, s->d_idch.p);
    } else
        hipLaunchKernelGGL(k_identity, dim3(nT), dim3(64), 0, s->side, s->d_ctg.p, nT, v.idp, v.idn, v.r.tid);
    (void)hipEventRecord(s->ev[COV_K_IDENTITY][1], s->side);
    s->k_launches[COV_K_IDENTITY]++;
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s->ev_side_done, s->side));   // joined just before the results are copied back (stage_join_side)
    s->ev_fresh = -1;      // the host worked between the groups (a stream created on first use, five launches on it): the next group's
                           // time starts at its own event, not at k_prep's end (smoke() used to print k_ranges 7.8 ms for 80 k records)
    return COV_OK;
}

// Stage 4 (records and tiles): prefix sums of the tile index and of the bucket counts, the buckets' fill, the tiles' candidate ranges.
static cov_status stage_ranges(cov_session *s, const FinishPlan &p, const PassViews &v) {
    time_begin(s, COV_K_RANGES);
    const u32 n_blocks = (s->n_tiles + 1023u) / 1024u;
    const u32 cx_grid = (u32)s->n_cus * 8u;     // waves stride over the RW_BUCKET list; nothing to do for short reads
    ScanPair sp{};
    sp.cnt[0] = s->d_tcnt.p; sp.scan[0] = s->d_tscan.p; sp.top[0] = s->d_ttop.p; sp.total[0] = nullptr;
    sp.cnt[1] = s->d_cx_cnt.p; sp.scan[1] = s->d_cx_scan.p; sp.top[1] = s->d_cx_top.p; sp.total[1] = &s->d_glob.p->cx_total;
    hipLaunchKernelGGL(k_tile_scan1, dim3(2u * n_blocks), dim3(1024), 0, v.st, sp, s->n_tiles, n_blocks);
    hipLaunchKernelGGL(k_tile_scan2, dim3(2), dim3(1024), 0, v.st, sp, n_blocks);
    hipLaunchKernelGGL((k_cx_expand<true>), dim3(cx_grid), dim3(256), 0, v.st, v.r, s->d_tlen.p, s->d_glob.p, v.cx, v.ti);
    u32 *slow_list = s->use_fast ? s->d_slow_list.p : nullptr;
    u32 *deep_list = const_cast<u32 *>(pileup_deep_list(s));
    const auto ranges = p.want_hist ? &k_ranges<true> : &k_ranges<false>;
    hipLaunchKernelGGL(ranges, dim3((s->n_tiles + 255) / 256), dim3(256), 0, v.st, s->d_tile_contig.p, s->d_tile_start.p, s->n_tiles, s->d_tlen.p,
                       v.mask, s->d_ctg.p, s->d_desc.p, v.ti, s->d_tscan.p, s->d_ttop.p, v.cx, s->d_glob.p, slow_list, deep_list, s->deep_min);
    time_end(s, COV_K_RANGES);
    HIPCHK(hipGetLastError());
    return COV_OK;
}

// Stage 5 (histogram wanted): the arena's layout from the bounds k_ranges left, and its zero fill.
static cov_status stage_hist_layout(cov_session *s, const PassViews &v) {
    time_begin(s, COV_K_HIST);
    const u32 hb = (v.nT + 1023u) / 1024u;
    HIPCHK(s->d_hist_top.reserve(hb, v.st));
    hipLaunchKernelGGL((k_hist_sum<0>), dim3(hb), dim3(1024), 0, v.st, (const DevContig *)s->d_ctg.p, v.nT, s->d_tlen.p, v.mask, v.excl, s->d_hist_top.p);
    hipLaunchKernelGGL((k_hist_off<0>), dim3(hb), dim3(1024), 0, v.st, s->d_ctg.p, v.nT, s->d_tlen.p, v.mask, v.excl, (const u64 *)s->d_hist_top.p, s->d_glob.p);
    hipLaunchKernelGGL(k_zero_u32, dim3(2048), dim3(256), 0, v.st, s->d_arena.p, &s->d_glob.p->hist_cap_total);
    time_end(s, COV_K_HIST);
    HIPCHK(hipGetLastError());
    return COV_OK;
}

// Stage 6: the pileup, and k_hist_stats inside its bracket when the estimator kernel is not the first reader of the window statistics.
static cov_status stage_pileup(cov_session *s, const FinishPlan &p, const PassViews &v) {
    const PileupArgs a = pileup_args(s);
    time_begin(s, COV_K_PILEUP);
    if (p.want_hist) launch_any_pileup<true, false>(s, a, s->n_tiles);
    else launch_any_pileup<false, false>(s, a, s->n_tiles);
    if (p.hist_stats_launch) {
        const auto hist_stats = p.est_lanes ? &k_hist_stats<true> : &k_hist_stats<false>;
        hipLaunchKernelGGL(hist_stats, dim3(p.est_lanes ? (v.nT + 255) / 256 : (v.nT + 3) / 4), dim3(256), 0, v.st, s->d_ctg.p, v.nT, (const u32 *)s->d_tlen.p,
                           v.mask, v.excl, (const u32 *)s->d_arena.p);
    }
    time_end(s, COV_K_PILEUP);
    HIPCHK(hipGetLastError());
    return COV_OK;
}

// Stage 7 (histogram wanted): the compact histogram, when this pass builds it, and the start of its way to the host.
static cov_status stage_hist_compact(cov_session *s, const FinishPlan &p, const PassViews &v) {
    s->hist_prefetched = 0;
    if (p.compacted) {
        HIPCHK(s->d_chist.reserve((size_t)v.R + v.nT + 1, v.st));
        time_begin(s, COV_K_HIST_COMPACT);
        launch_hist_compact(s, v.mask, v.excl);
        time_end(s, COV_K_HIST_COMPACT);
        HIPCHK(hipGetLastError());
        // (only for a caller that fetched the histogram after the finish before this one: a caller that never does pays no copy)
        const u64 guess = p.hist_prefetch ? std::min<u64>({s->last_chist_total + s->last_chist_total / 16, (u64)v.R + v.nT + 1, (u64)(64u << 20) / 8}) : 0;
        if (guess) {
            if (guess > s->h_chist_cap) HIPCHK(pinned_grow(s->h_chist, s->h_chist_cap, guess));
            HIPCHK(hipMemcpyAsync(s->h_chist, s->d_chist.p, (size_t)guess * 8, hipMemcpyDeviceToHost, v.st));
            s->hist_prefetched = guess;
        }
    }
    s->hist_fetch_seen = false;
    return COV_OK;
}

// The page-locked staging of the results: what cov_set_targets' helper thread obtained, or grown here.
static cov_status result_host_bind(cov_session *s, const FinishPlan &p, const PassViews &v) {
    result_host_take(s);
    const size_t need = p.lean ? sizeof(DevGlobal) + sizeof(DevContig) : result_host_bytes(s, v.nT);      // (lean: DevGlobal + the order word)
    if (need > s->h_res_cap) HIPCHK(pinned_grow(s->h_res, s->h_res_cap, need < ((size_t)64 << 20) ? need + need / 2 : need));      // (room to grow for small blocks only)
    s->h_ctg = (DevContig *)(s->h_res + sizeof(DevGlobal));
    s->h_estf = reinterpret_cast<float *>(s->h_res + v.block);
    return COV_OK;
}

// The side stream's identity sums are in the contigs' accumulators from here on.
static cov_status stage_join_side(cov_session *s, const PassViews &v) {
    HIPCHK(hipStreamWaitEvent(v.st, s->ev_side_done, 0));
    s->ev_fresh = -1;      // the stream waited here: the wait is not the next group's time
    return COV_OK;
}

// Stage 8 (per-contig floats wanted): CoverageEstimator::calculate_coverage of every contig (k_init left n_pass = 0 everywhere when nothing
// ran: rows of zeros).
static cov_status stage_estimate(cov_session *s, const FinishPlan &p, const PassViews &v) {
    time_begin(s, COV_K_ESTIMATE);
    const auto estimate = p.est_lanes ? &k_estimate_lanes : &k_estimate;
    hipLaunchKernelGGL(estimate, dim3(p.est_lanes ? (v.nT + 255) / 256 : (v.nT + 3) / 4), dim3(256), 0, v.st, s->d_ctg.p, v.nT, (const u32 *)s->d_tlen.p, v.excl,
                       (const u32 *)s->d_arena.p, s->est, reinterpret_cast<float *>(s->d_res.p + v.block), p.derive_in_est ? 1u : 0u);
    time_end(s, COV_K_ESTIMATE);
    HIPCHK(hipGetLastError());
    return COV_OK;
}

// Stage 9 (cov_set_genome_runs): separator / single-genome entries — which targets form an entry depends on where the reads fell: the
// table of this finish (sep_kernels.hip.h), then its counts on the host: the genome kernels' launches are sized by them.
static cov_status stage_sep_table(cov_session *s, const PassViews &v) {
    hipStream_t st = v.st; const u32 nT = v.nT;
    const u32 nb = (std::max(nT, 1u) + SEP_TILE - 1u) / SEP_TILE, eb = (s->sep_ent_cap + SEP_TILE - 1u) / SEP_TILE, cap = s->sep_ent_cap;
    time_begin(s, COV_K_SEP);
    hipLaunchKernelGGL(k_sep_obs_top, dim3(nb), dim3(SEP_TILE), 0, st, (const DevContig *)s->d_ctg.p, nT, s->d_stop_last1.p, s->d_stop_first.p);
    hipLaunchKernelGGL(k_sep_flags, dim3(nb), dim3(SEP_TILE), 0, st, (const DevContig *)s->d_ctg.p, nT, (const int32_t *)s->d_sgid.p, (const u32 *)s->d_sblk.p,
                       (const u32 *)s->d_stop_last1.p, (const u32 *)s->d_stop_first.p, s->d_scode.p, s->d_stop_cnt.p);
    hipLaunchKernelGGL(k_sep_compact, dim3(nb), dim3(SEP_TILE), 0, st, nT, (const int32_t *)s->d_sgid.p, (const u32 *)s->d_sblk.p, (const uint8_t *)s->d_scode.p,
                       (const u64 *)s->d_stop_cnt.p, s->d_gtids.p, s->d_sent_pos.p, s->d_sent.p, cap, s->d_scounts.p, s->d_glob.p);
    hipLaunchKernelGGL(k_sep_rows, dim3((std::max(nT, 1u) + 255u) / 256u), dim3(256), 0, st, (const u32 *)s->d_scounts.p, (const u32 *)s->d_sent_pos.p, s->d_grow.p, cap);
    hipLaunchKernelGGL(k_sep_seg_sum, dim3(eb), dim3(SEP_TILE), 0, st, (const u32 *)s->d_scounts.p, (const u32 *)s->d_grow.p, s->d_stop_seg.p);
    hipLaunchKernelGGL(k_sep_seg_write, dim3(eb), dim3(SEP_TILE), 0, st, s->d_scounts.p, (const u32 *)s->d_grow.p, (const u64 *)s->d_stop_seg.p, s->d_gseg_genome.p,
                       s->d_gseg_start.p, s->sep_seg_cap);
    time_end(s, COV_K_SEP);
    HIPCHK(hipGetLastError());
    u32 sep_counts[SEP_N_COUNTS] = {0, 0, 0, 0};
    uint8_t *hc = s->h_gout + s->h_gout_cap - 16;
    HIPCHK(hipMemcpyAsync(hc, s->d_scounts.p, SEP_N_COUNTS * sizeof(u32), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    memcpy(sep_counts, hc, sizeof sep_counts);
    s->ev_fresh = -1;      // the host waited here: the wait is not the next group's time
    s->n_genomes = sep_counts[SEP_N_ENTRIES]; s->n_gseg = sep_counts[SEP_N_SEG];
    return COV_OK;
}

// Stage 10 (genome entries, and at least one): reduce the contigs' accumulators over each genome's row, merge their histograms, evaluate,
// and start the entries' way to the host.  (runs and no target with a considered record: no entry, nothing to reduce.)
static cov_status stage_genomes(cov_session *s, const FinishPlan &p, const PassViews &v) {
    hipStream_t st = v.st;
    const u32 nG = s->n_genomes, n_seg = s->n_gseg, sep = p.runs ? 1u : 0u;
    GenomeTable gt{s->d_grow.p, s->d_gtids.p, s->d_gseg_genome.p, s->d_gseg_start.p, nG, n_seg};
    const u64 excl = v.excl;
    const u64 ghist_cap = (u64)v.R + v.nT + 1;      // the genomes' bins are at most the contigs' (every genome bin is some contig's bin)
    if (p.want_hist) HIPCHK(s->d_ghist.reserve((size_t)ghist_cap, st));
    time_begin(s, COV_K_GENOME);
    hipLaunchKernelGGL(k_genome_init, dim3((nG + 255u) / 256u), dim3(256), 0, st, s->d_genomes.p, nG);
    if (n_seg) hipLaunchKernelGGL(k_genome_reduce, dim3((n_seg + 3u) / 4u), dim3(256), 0, st, (const DevContig *)s->d_ctg.p, (const u32 *)s->d_tlen.p, excl, gt, s->d_genomes.p, sep);
    if (p.genome_identity) hipLaunchKernelGGL(k_genome_identity, dim3(nG), dim3(64), 0, st, (const DevContig *)s->d_ctg.p, gt, s->d_genomes.p, sep);
    if (p.want_hist) {
        const u32 gb = (nG + 1023u) / 1024u;
        u64 *total = s->d_ghist_top.p + gb;
        hipLaunchKernelGGL(k_genome_hist_sum, dim3(gb), dim3(1024), 0, st, (const DevGenome *)s->d_genomes.p, nG, s->d_ghist_top.p);
        hipLaunchKernelGGL(k_genome_hist_off, dim3(gb), dim3(1024), 0, st, s->d_genomes.p, nG, (const u64 *)s->d_ghist_top.p, total, ghist_cap, s->d_glob.p);
        hipLaunchKernelGGL(k_zero_u64, dim3(1024), dim3(256), 0, st, s->d_ghist.p, (const u64 *)total, ghist_cap);
        if (n_seg && p.run_pileup)
            hipLaunchKernelGGL(k_genome_hist_merge, dim3((n_seg + 3u) / 4u), dim3(256), 0, st, (const DevContig *)s->d_ctg.p, (const u32 *)s->d_tlen.p, excl,
                               (const u32 *)s->d_arena.p, gt, (const DevGenome *)s->d_genomes.p, s->d_ghist.p, ghist_cap);
    }
    DevGenomeStats *gstats = reinterpret_cast<DevGenomeStats *>(s->d_gout.p);
    float *gest = reinterpret_cast<float *>(s->d_gout.p + (size_t)nG * sizeof(DevGenomeStats));
    const bool lanes = nG >= p.genome_lanes_from;      // a lane per genome, as for the contigs of an assembly
    const auto estimate = lanes ? &k_genome_estimate_lanes : &k_genome_estimate;
    hipLaunchKernelGGL(estimate, dim3(lanes ? (nG + 255u) / 256u : (nG + 3u) / 4u), dim3(256), 0, st, (const DevGenome *)s->d_genomes.p, nG, (const u64 *)s->d_ghist.p, s->est, gest, gstats);
    time_end(s, COV_K_GENOME);
    HIPCHK(hipGetLastError());
    const size_t rows = (size_t)nG * (sizeof(DevGenomeStats) + s->est.n * sizeof(float));
    HIPCHK(hipMemcpyAsync(s->h_gout, s->d_gout.p, rows, hipMemcpyDeviceToHost, st));
    if (p.runs) HIPCHK(hipMemcpyAsync(s->h_gout + rows, s->d_sent.p, (size_t)nG * sizeof(SepEntry), hipMemcpyDeviceToHost, st));
    return COV_OK;
}

// Stage 11: the results' way to the host.  Lean (cov_finish_genomes): DevGlobal and the order rule of convert_results evaluated on the
// device — the first considered record of a seen contig must not lie before the last one of any seen contig in front of it
// (contig.rs:129-132); the verdict is one word behind DevGlobal.  Else one copy: the result block and, behind it, the estimators' floats.
static cov_status stage_result_copy(cov_session *s, const FinishPlan &p, const PassViews &v) {
    hipStream_t st = v.st; const u32 nT = v.nT;
    if (!p.lean) {
        HIPCHK(hipMemcpyAsync(s->h_res, s->d_res.p, sizeof(DevGlobal) + (size_t)nT * sizeof(DevContig) + (p.nf ? (v.block - sizeof(DevGlobal) - (size_t)nT * sizeof(DevContig)) + p.nf * sizeof(float) : 0),
                              hipMemcpyDeviceToHost, st));
        return COV_OK;
    }
    const u32 ob = (nT + 1023u) / 1024u;
    HIPCHK(s->d_order.reserve((size_t)ob + 2, st));
    hipLaunchKernelGGL(k_order_max, dim3(std::max(ob, 1u)), dim3(1024), 0, st, (const DevContig *)s->d_ctg.p, nT, s->d_order.p);
    hipLaunchKernelGGL(k_order_check, dim3(std::max(ob, 1u)), dim3(1024), 0, st, (const DevContig *)s->d_ctg.p, nT, s->d_order.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(s->h_res, s->d_res.p, sizeof(DevGlobal), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(s->h_res + sizeof(DevGlobal), s->d_order.p, 8, hipMemcpyDeviceToHost, st));
    return COV_OK;
}

// Stage 12a: the end of the pass.  A finish is a millisecond: the host looks for its end itself for a while before it asks to be woken.
static cov_status stage_wait(cov_session *s, const PassViews &v) {
    const auto t_spin = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t q = hipStreamQuery(v.st);
        if (q == hipSuccess) break;
        if (q != hipErrorNotReady) { (void)hipGetLastError(); break; }
        (void)hipGetLastError();
        if (std::chrono::steady_clock::now() - t_spin > std::chrono::milliseconds(4)) break;
        __builtin_ia32_pause();
    }
    HIPCHK(hipStreamSynchronize(v.st));
    memcpy(&s->h_glob, s->h_res, sizeof(DevGlobal));
    return COV_OK;
}

// Stage 12b: the groups' times, the algorithmic bytes, and the verdict on what came back.
static cov_status stage_verdict(cov_session *s, const FinishPlan &p, const PassViews &v, cov_contig_stats *stats, cov_summary *summary) {
    for (int k = 0; k < COV_K_COUNT; k++)
        if (s->k_launches[k]) (void)hipEventElapsedTime(&s->k_ms[k], k == COV_K_IDENTITY ? s->ev[k][0] : s->ev_begin[k], s->ev[k][1]);
    // algorithmic bytes: each record's SoA fields and CIGAR words are needed once; results written once
    s->algo_bytes = (uint64_t)v.R * 24 + p.ncig * 4 + (uint64_t)v.nT * sizeof(DevContig);
    if (p.lean) {
        u64 unsorted_at; memcpy(&unsorted_at, s->h_res + sizeof(DevGlobal), 8);
        const cov_status cst = verdict_results(s, s->h_glob, unsorted_at, v.R, summary);
        if (cst != COV_OK) return cst;
        s->last_chist_total = 0; s->hist_compacted = false; s->est_valid = false; s->gen_valid = true; s->finished = true;
        return COV_OK;
    }
    const cov_status cst = convert_results(s, s->h_glob, s->h_ctg, v.R, stats, summary, s->spill.inflight, s->spill.records);
    if (cst != COV_OK) return cst;
    s->last_chist_total = 0;
    if (p.want_hist) for (u32 c = 0; c < v.nT; c++) s->last_chist_total += stats[c].hist_len;      // (the host laid the compact histogram out: convert_results)
    s->hist_compacted = p.compacted;
    s->est_valid = s->est.n != 0 && !s->have_mask && !s->have_runs;
    s->gen_valid = p.genomes;
    s->finished = true;
    return COV_OK;
}

// The stages in stream order; every condition is a field of the plan.
static cov_status finish_once(cov_session *s, cov_contig_stats *stats, cov_summary *summary, bool &again) {
    again = false;
    if (!s || (!stats && s->n_targets && !s->lean_finish)) return COV_ERR_INVALID_ARG;
    const FinishPlan p = finplan::plan(finish_facts(s));
    PassViews v;
    cov_status rc = stage_begin(s, p, v);
    if (rc == COV_OK && p.run_prep) rc = stage_prep(s, p, v);
    if (rc == COV_OK && p.identity_side) rc = stage_identity_side(s, v);
    if (rc == COV_OK && p.run_pileup) rc = stage_ranges(s, p, v);
    if (rc == COV_OK && p.run_pileup && p.want_hist) rc = stage_hist_layout(s, v);
    if (rc == COV_OK && p.run_pileup) rc = stage_pileup(s, p, v);
    if (rc == COV_OK && p.run_pileup && p.want_hist) rc = stage_hist_compact(s, p, v);
    if (rc == COV_OK) rc = result_host_bind(s, p, v);
    if (rc == COV_OK && p.identity_side) rc = stage_join_side(s, v);
    if (rc == COV_OK && p.nf) rc = stage_estimate(s, p, v);
    if (rc == COV_OK && p.lean_without_genomes) {      // (refused here, where the pass always refused: what it leaves the next pass stays as it was)
        s->err = "cov_finish_genomes: cov_set_genomes or cov_set_genome_runs, and cov_set_estimators, first, and no spill of the bounded record store (cov_finish then)";
        rc = COV_ERR_STATE;
    }
    if (rc == COV_OK && p.runs) rc = stage_sep_table(s, v);
    if (rc == COV_OK && p.genomes && s->n_genomes != 0) rc = stage_genomes(s, p, v);
    if (rc == COV_OK) rc = stage_result_copy(s, p, v);
    if (rc == COV_OK) rc = stage_wait(s, v);
    if (rc != COV_OK) return rc;
    if (s->h_glob.cx_total > s->d_cx_runs.cap) {      // the long-CIGAR buckets were too small: the pass computed the exact need, and runs once more
        const uint64_t need = s->h_glob.cx_total + s->h_glob.cx_total / 8 + 1024;
        s->d_cx_runs.release();
        HIPCHK(s->d_cx_runs.reserve((size_t)need, v.st));
        again = true;
        return COV_OK;
    }
    return stage_verdict(s, p, v, stats, summary);
}


// ---- bounded record store: spill and merge (see cov_session::spill)
static cov_status fetch_chunk_hist(cov_session *s, uint64_t *hist);

// Runs the pipeline over the store, keeps every contig but the one in flight, moves the records from that contig's first considered
// record onwards to the front.  The contig in flight = the last considered contig (after the order check: the highest tid with a
// considered record); every considered record behind its first one is its own (anything else would have failed the order check),
// so the contigs in front of it are complete — the reference would have flushed them at the tid change (contig.rs:128-155).
// progress = false: nothing could leave (one contig fills the store, or the store is an adopted batch / carries mate columns).
static cov_status spill_store(cov_session *s, bool &progress) {
    progress = false;
    if (s->adopted || s->store.n_records == 0 || s->want_mates || s->n_targets == 0) return COV_OK;
    covr::Range rr("bounded store: spill");
    const u32 nT = s->n_targets;
    const bool want_hist = s->cfg.want & COV_WANT_HIST;
    std::vector<cov_contig_stats> st(nT);
    cov_summary sm{};
    s->in_spill = true;
    const bool lean_was = s->lean_finish; s->lean_finish = false;
    cov_status rc = finish_store(s, st.data(), &sm);
    s->in_spill = false; s->lean_finish = lean_was;
    if (rc != COV_OK) return rc;
    const u64 R = s->store.n_records;
    cov_session::Spill &S = s->spill;
    int64_t cstar = -1; u64 best = 0;
    for (u32 c = 0; c < nT; c++)
        if (st[c].n_pass && (cstar < 0 || st[c].last_record >= best)) { cstar = c; best = st[c].last_record; }
    const u64 keep_from = cstar >= 0 ? st[cstar].first_record - S.records : R;      // (record indices come back counted from the sample's first record)
    if (keep_from == 0) { s->finished = false; return COV_OK; }
    if (!S.active) { S.stats.assign(nT, cov_contig_stats{}); S.ctg.assign(nT, DevContig{}); S.have.assign(nT, 0); S.active = true; }
    std::vector<uint64_t> h;
    if (want_hist && sm.hist_total) { h.resize(sm.hist_total); rc = fetch_chunk_hist(s, h.data()); if (rc != COV_OK) return rc; }
    for (u32 c = 0; c < nT; c++) {
        if ((int64_t)c == cstar || !st[c].n_pass) continue;
        if (S.have[c]) { s->err = "BAM file appears to be unsorted. Input BAM files must be sorted by reference (i.e. by samtools sort)"; return COV_ERR_UNSORTED; }
        S.stats[c] = st[c]; S.ctg[c] = s->h_ctg[c]; S.have[c] = 1;
        if (s->est.n && !s->have_mask && !s->have_runs) {
            if (s->spill_est.size() != (size_t)nT * s->est.n) s->spill_est.assign((size_t)nT * s->est.n, 0.0f);
            memcpy(&s->spill_est[(size_t)c * s->est.n], s->h_estf + (size_t)c * s->est.n, s->est.n * sizeof(float));
        }
        if (want_hist && st[c].hist_len) {
            S.stats[c].hist_off = S.hist.size();
            S.hist.insert(S.hist.end(), h.begin() + st[c].hist_off, h.begin() + st[c].hist_off + st[c].hist_len);
        }
    }
    hipStream_t q = s->stream;
    u64 prim_keep = 0;
    u32 c0 = (u32)s->store.n_cigar;
    if (keep_from < R) {
        unsigned long long *ctr = reinterpret_cast<unsigned long long *>(&s->d_glob.p->pad2[1]);
        HIPCHK(hipMemsetAsync(ctr, 0, 8, q));
        hipLaunchKernelGGL(k_count_primary, dim3((u32)std::min<u64>((R - keep_from + 255) / 256, (u64)s->n_cus * 8)), dim3(256), 0, q, (const uint16_t *)s->store.flag.p, (u32)keep_from, (u32)R, ctr);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&prim_keep, ctr, 8, hipMemcpyDeviceToHost, q));
        HIPCHK(hipMemcpyAsync(&c0, s->store.cigar_off.p + keep_from, 4, hipMemcpyDeviceToHost, q));
        HIPCHK(hipStreamSynchronize(q));
    }
    S.prim += sm.num_detected_primary_alignments - prim_keep;
    S.cons += sm.n_considered - (cstar >= 0 ? st[cstar].n_pass : 0);
    S.records += keep_from;
    if (cstar > S.inflight) S.inflight = cstar;
    S.count++;
    const u64 n_keep = R - keep_from, cig_keep = s->store.n_cigar - c0;
    HIPCHK(s->store.move_front(keep_from, c0, q));
    if (n_keep && c0) {
        hipLaunchKernelGGL(k_rebase_offsets, dim3((u32)((n_keep + 1 + 255) / 256)), dim3(256), 0, q, s->store.cigar_off.p, (u32)(n_keep + 1), c0, 0u);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(q));
    s->store.n_records = n_keep; s->store.n_cigar = cig_keep;
    s->finished = false; s->depth_all_valid = false; s->dr.drop();
    if (cov_timing_on())
        fprintf(stderr, "[covermhip] bounded store: spill %u, %llu records left the store (%llu stay: contig %lld in flight), %llu since the sample began\n", S.count,
                (unsigned long long)keep_from, (unsigned long long)n_keep, (long long)cstar, (unsigned long long)S.records);
    progress = true;
    return COV_OK;
}

// cov_finish after one or more spills: `stats` / `summary` hold the pass over what the store still held; the contigs that left
// earlier come back from the host, the histogram is re-based into one array (cov_fetch_hist serves it), and the device's result
// block is rewritten as the merged one so that cov_gather sends the whole sample.
static cov_status merge_spilled(cov_session *s, cov_contig_stats *stats, cov_summary *summary) {
    cov_session::Spill &S = s->spill;
    const u32 nT = s->n_targets;
    const bool want_hist = s->cfg.want & COV_WANT_HIST;
    std::vector<uint64_t> h;
    if (want_hist && summary->hist_total) { h.resize(summary->hist_total); const cov_status rc = fetch_chunk_hist(s, h.data()); if (rc != COV_OK) return rc; }
    s->merged_hist = S.hist;
    std::vector<DevContig> m(nT);
    u32 rank = 0;
    for (u32 c = 0; c < nT; c++) {
        if (S.have[c]) {
            if (stats[c].n_pass) { s->err = "BAM file appears to be unsorted. Input BAM files must be sorted by reference (i.e. by samtools sort)"; return COV_ERR_UNSORTED; }
            stats[c] = S.stats[c]; m[c] = S.ctg[c];
            if (s->est.n && s->est_valid && s->spill_est.size() == (size_t)nT * s->est.n)
                memcpy(s->h_estf + (size_t)c * s->est.n, &s->spill_est[(size_t)c * s->est.n], s->est.n * sizeof(float));
        } else {
            m[c] = s->h_ctg[c];
            if (want_hist && stats[c].hist_len) {
                const u64 off = s->merged_hist.size();
                s->merged_hist.insert(s->merged_hist.end(), h.begin() + stats[c].hist_off, h.begin() + stats[c].hist_off + stats[c].hist_len);
                stats[c].hist_off = off;
            }
        }
        m[c].chist_off = stats[c].hist_off; m[c].hist_len = stats[c].hist_len;
        // the block a peer converts (cov_gathered) judges the order from first_rec / last_rec: the merged block carries the contigs' ranks
        if (m[c].n_pass) { m[c].first_rec = m[c].last_rec = rank++; }
    }
    summary->num_detected_primary_alignments += S.prim; summary->n_records += S.records; summary->n_considered += S.cons;
    summary->hist_total = s->merged_hist.size();
    s->merged_valid = true; s->merged_records = summary->n_records;
    DevGlobal g = s->h_glob;
    g.prim_slots[0] += S.prim; g.cons_slots[0] += S.cons; g.chist_total = s->merged_hist.size();
    HIPCHK(hipSetDevice(s->cfg.device));
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(hipMemcpy(s->d_res.p, &g, sizeof g, hipMemcpyHostToDevice));
    if (nT) HIPCHK(hipMemcpy(s->d_res.p + sizeof(DevGlobal), m.data(), (size_t)nT * sizeof(DevContig), hipMemcpyHostToDevice));
    return COV_OK;
}


cov_status cov_reserve(cov_session *s, uint64_t n_records, uint64_t n_cigar) {
    if (!s) return COV_ERR_INVALID_ARG;
    if (n_records >= 0xfffffff0ull || n_cigar >= 0xfffffff0ull) { s->err = "more than 2^32 records in one session"; return COV_ERR_INVALID_ARG; }
    HIPCHK(hipSetDevice(s->cfg.device));
    const uint64_t R = s->adopted ? 0 : s->store.n_records, C = s->adopted ? 0 : s->store.n_cigar;
    HIPCHK(s->store.reserve(n_records, n_cigar + 1, s->stream, R, C, false));
    return COV_OK;
}

// ---- cov_gather: ONE RCCL gather of every rank's result block to the root rank's device (north star: "a single RCCL gather
// of per-contig results over xGMI").  librccl is bound at run time (dlopen), so single-GPU users need no RCCL at all.
namespace {
struct Rccl {
    typedef int (*init_all_t)(void **, int, const int *);
    typedef int (*gather_t)(const void *, void *, size_t, int, int, void *, hipStream_t);
    typedef int (*grp_t)();
    typedef const char *(*errstr_t)(int);
    init_all_t init_all = nullptr; gather_t gather = nullptr; grp_t group_start = nullptr, group_end = nullptr; errstr_t errstr = nullptr;
    bool ok = false;
    Rccl() {
        void *h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
        if (!h) return;
        init_all = (init_all_t)dlsym(h, "ncclCommInitAll"); gather = (gather_t)dlsym(h, "ncclGather");
        group_start = (grp_t)dlsym(h, "ncclGroupStart"); group_end = (grp_t)dlsym(h, "ncclGroupEnd");
        errstr = (errstr_t)dlsym(h, "ncclGetErrorString");
        ok = init_all && gather && group_start && group_end;
    }
};
Rccl *rccl_lib() { static Rccl r; return &r; }
std::mutex g_comm_mutex;
std::map<std::vector<int>, std::vector<void *>> g_comms;   // communicators per device list, kept for the process lifetime
}  // namespace

cov_status cov_gather(cov_session *const *sessions, uint32_t n, uint32_t root) {
    if (!sessions || n == 0 || root >= n) return COV_ERR_INVALID_ARG;
    cov_session *s = sessions[root];
    const u32 nT = s->n_targets;
    std::vector<int> devs(n);
    bool distinct = true;
    for (u32 i = 0; i < n; i++) {
        if (!sessions[i] || !sessions[i]->finished || sessions[i]->n_targets != nT) { s->err = "cov_gather: every session must be finished over the same targets"; return COV_ERR_STATE; }
        devs[i] = sessions[i]->cfg.device;
        for (u32 j = 0; j < i; j++) if (devs[j] == devs[i]) distinct = false;
    }
    const size_t block = result_block_bytes(nT);
    HIPCHK(hipSetDevice(s->cfg.device));
    HIPCHK(s->d_gather.reserve((size_t)n * block, s->stream));
    if ((size_t)n * block > s->h_gather_cap) HIPCHK(pinned_grow(s->h_gather, s->h_gather_cap, (size_t)n * block));
    for (u32 i = 0; i < n; i++) {   // the record count of each rank travels in its block (a padding word of DevGlobal)
        HIPCHK(hipSetDevice(devs[i]));
        const u64 nr = sessions[i]->merged_valid ? sessions[i]->merged_records : sessions[i]->store.n_records;
        HIPCHK(hipMemcpyAsync(&sessions[i]->d_glob.p->pad2[0], &nr, 8, hipMemcpyHostToDevice, sessions[i]->stream));
        HIPCHK(hipStreamSynchronize(sessions[i]->stream));
    }
    if (distinct && (n > 1 || getenv("COVERM_FORCE_RCCL") != nullptr)) {
        Rccl &R = *rccl_lib();
        if (!R.ok) { s->err = "cov_gather: librccl.so.1 not available"; return COV_ERR_HIP; }
        std::vector<void *> comms;
        {
            std::lock_guard<std::mutex> lk(g_comm_mutex);
            auto it = g_comms.find(devs);
            if (it == g_comms.end()) {
                std::vector<void *> c(n, nullptr);
                const int rc = R.init_all(c.data(), (int)n, devs.data());
                if (rc != 0) { s->err = std::string("ncclCommInitAll: ") + (R.errstr ? R.errstr(rc) : "error"); return COV_ERR_HIP; }
                it = g_comms.emplace(devs, c).first;
            }
            comms = it->second;
        }
        int rc = R.group_start();
        for (u32 i = 0; i < n && rc == 0; i++) {
            (void)hipSetDevice(devs[i]);
            rc = R.gather(sessions[i]->d_res.p, i == root ? s->d_gather.p : nullptr, block, /* ncclUint8 */ 1, (int)root, comms[i], sessions[i]->stream);
        }
        const int rc2 = R.group_end();
        if (rc != 0 || rc2 != 0) { s->err = std::string("ncclGather: ") + (R.errstr ? R.errstr(rc ? rc : rc2) : "error"); return COV_ERR_HIP; }
        for (u32 i = 0; i < n; i++) { HIPCHK(hipSetDevice(devs[i])); HIPCHK(hipStreamSynchronize(sessions[i]->stream)); }
    } else {
        // one device given more than once (functional checks on a single-GPU box): RCCL refuses two ranks on one device,
        // so the blocks move by plain device copies instead
        for (u32 i = 0; i < n; i++) {
            HIPCHK(hipSetDevice(devs[i]));
            HIPCHK(hipStreamSynchronize(sessions[i]->stream));
        }
        HIPCHK(hipSetDevice(s->cfg.device));
        for (u32 i = 0; i < n; i++)    // on the root's stream: ordered before the copy to the host below (a device-to-device hipMemcpyPeer may return early)
            HIPCHK(hipMemcpyPeerAsync(s->d_gather.p + (size_t)i * block, s->cfg.device, sessions[i]->d_res.p, devs[i], block, s->stream));
    }
    HIPCHK(hipSetDevice(s->cfg.device));
    HIPCHK(hipMemcpyAsync(s->h_gather, s->d_gather.p, (size_t)n * block, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    s->gather_n = n; s->gather_block = block;
    return COV_OK;
}

cov_status cov_gathered(cov_session *root, uint32_t rank, cov_contig_stats *stats, cov_summary *summary) {
    if (!root || !root->h_gather || rank >= root->gather_n || (!stats && root->n_targets)) return COV_ERR_INVALID_ARG;
    const uint8_t *blk = root->h_gather + (size_t)rank * root->gather_block;
    DevGlobal G; memcpy(&G, blk, sizeof G);
    return convert_results(root, G, reinterpret_cast<const DevContig *>(blk + sizeof(DevGlobal)), G.pad2[0], stats, summary);
}


// ---------------------------------------------------------------------------------------------- device ingest (covermhip.h cov_ingest_*)
static_assert(sizeof(cov_bgzf_block) == sizeof(covi::BgzfBlock) && offsetof(cov_bgzf_block, in_len) == offsetof(covi::BgzfBlock, in_len) &&
              offsetof(cov_bgzf_block, out_off) == offsetof(covi::BgzfBlock, out_off), "cov_bgzf_block mirrors the device struct");

constexpr int INF1_LB = 7, INF1_DB = 6;       // k_inflate's primary tables: 7 + 6 bits = 28 KiB per wave, five waves per CU (the fastest measured)
// Blocks per k_inflate_wave round = per window.  81 920 from round 3 to the middle of round 6 (round 4's sweep: smaller windows lost to the fixed
// host cost per window); with the feed at the link's rate and round 5-6's faster kernels the sweep was repeated at 200 M reads,
// alternating: ingest 0.478-0.485 s with 61 440 blocks against 0.487-0.494 s with 81 920, 0.484-0.494 s with 40 960, 0.496-0.505 s with 122 880
// (profiles/r06_round_blocks_ab_200M.json) — what the device still has to do when the last byte has arrived is about one window's
// processing, 32 ms instead of 44.  61 440 is also exactly 15 launches' worth of resident waves on 256 CUs (16 per CU).
constexpr u32 WAVE_ROUND_BLOCKS = 61440;
// Decided once per ingest (cov_ingest_begin) and kept in the session: the switches are read there, never in a launch path.
static InflateKernel choose_inflate_kernel(cov_session *s) {
    InflateKernel K;
    const char *ve = getenv("COVERM_INFLATE_V");
    K.version = ve && atoi(ve) == 1 ? 1 : 3;
    if (const char *lz = getenv("COVERM_LZ_V")) K.lz_version = atoi(lz) == 1 ? 1 : 2;      // 1: k_lz_resolve (rounds through global memory), 2: k_lz_stage (batches staged in LDS)
    if (K.version == 1) {
        int per_cu = 0;
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&covi::k_inflate<INF1_LB, INF1_DB, false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)covi::inflate_smem_bytes(INF1_LB, INF1_DB));
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, covi::k_inflate<INF1_LB, INF1_DB, false>, 64, covi::inflate_smem_bytes(INF1_LB, INF1_DB));
        if (per_cu <= 0) per_cu = 2;
        K.round_blocks = (u32)s->n_cus * (u32)per_cu * 64u;
    } else K.round_blocks = WAVE_ROUND_BLOCKS;
    { long long v; if (covknob::get("ingest_round_blocks", v) && v >= 64) K.round_blocks = (u32)v / 64u * 64u; }   // tests: many small windows
    { long long v; if (covknob::get("ingest_carry_kb", v) && v >= 1) K.carry = (u64)v << 10; }
    K.carry = (K.carry + 63u) & ~63ull;
    // compressed bytes one round may span: 32 KiB per block on average (BGZF blocks of BAM files compress to 15-25 KiB); a round of
    // less compressible blocks simply closes earlier
    K.cwin = std::max<u64>((u64)K.round_blocks * 32768u, 1ull << 20);
    { long long v; if (covknob::get("ingest_cwin_kb", v) && v >= 256) K.cwin = (u64)v << 10; }
    return K;
}

cov_status cov_ingest_begin(cov_session *s, uint64_t compressed_bytes, uint64_t first_record_offset, int check_crc) {
    if (!s) return COV_ERR_INVALID_ARG;
    if (s->sam_active) { s->err = "cov_ingest_begin: a SAM text ingest is open (cov_sam_end or cov_ingest_abort first)"; return COV_ERR_STATE; }
    covr::Range rr("ingest: buffers, streams, events (cov_ingest_begin)");
    HIPCHK(hipSetDevice(s->cfg.device));
    HIPCHK(ingest_prep_wait(s));
    if (!s->ing.copy) HIPCHK(ingest_prepare_(s));
    { const cov_status a = materialise_adopted(s); if (a) return a; }
    HIPCHK(hipStreamSynchronize(s->stream));     // the record store is about to be written from the parse stream
    IngestState &I = s->ing;
    I.reset_for_file(IngestState::Reset::BGZF_FILE);
    I.K = choose_inflate_kernel(s);      // (also sets the kernel's dynamic-LDS limit on this session's device)
    I.first_record = first_record_offset;
    I.check_crc = check_crc ? 1 : 0;
    HIPCHK(I.g_result.reserve(ingplan::G_WORDS, s->stream));
    HIPCHK(I.g_carry.reserve(I.K.carry, s->stream));
    if (!I.g_crc_tab.p) {      // (cov_ingest_release between two files gave the tables back with the buffers)
        std::vector<u32> t(covi::crcw::TABLE_WORDS);
        covi::crcw::build_tables(t.data());
        HIPCHK(I.g_crc_tab.reserve(covi::crcw::TABLE_WORDS, s->stream));
        HIPCHK(hipMemcpy(I.g_crc_tab.p, t.data(), covi::crcw::TABLE_WORDS * sizeof(u32), hipMemcpyHostToDevice));
    }
    HIPCHK(I.g_blocks.reserve(compressed_bytes / 8192 + 1024, s->stream));
    HIPCHK(I.g_status.reserve(compressed_bytes / 8192 + 1024, s->stream));
    if (compressed_bytes / 16384 + 1024 > I.h_blocks_cap) {     // page-locked mirror of the block table: sized once for ordinary ~20 KB blocks (it grows if they are smaller)
        if (I.h_blocks) { (void)hipHostFree(I.h_blocks); I.h_blocks = nullptr; I.h_blocks_cap = 0; }
        const size_t nc = compressed_bytes / 16384 + 1024;
        HIPCHK(hipHostMalloc((void **)&I.h_blocks, nc * sizeof(covi::BgzfBlock), hipHostMallocDefault));
        I.h_blocks_cap = nc;
    }
    HIPCHK(hipMemsetAsync(I.g_result.p, 0, ingplan::G_WORDS * sizeof(u64), s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    I.comp = compressed_bytes; I.span_hi = compressed_bytes;
    I.ccap = std::min<u64>(I.K.cwin, compressed_bytes + 65536u + 128u);     // a small file is one buffer: the byte rule never fires
    I.active = true;
    return COV_OK;
}

cov_status cov_ingest_span(cov_session *s, int64_t key_lo, int64_t key_hi, int search_first_record, int open_end, uint64_t file_lo, uint64_t file_hi) {
    if (!s || !s->ing.active || s->ing.feed.fed_any || key_lo < 0 || key_hi < key_lo || file_hi < file_lo || file_hi > s->ing.comp) return COV_ERR_INVALID_ARG;
    s->ing.key_lo = key_lo; s->ing.key_hi = key_hi; s->ing.search_first = search_first_record != 0; s->ing.open_end = open_end != 0;
    s->ing.span_lo = file_lo; s->ing.span_hi = file_hi;
    if (s->ing.is_span()) s->ing.was_span = true;
    return COV_OK;
}

// One window of a running ingest, BGZF or SAM text — nrec records, ncig CIGAR words — asks for room behind what the store holds and what the
// ingest has extracted so far (ing_rec_total / ing_cig_total: in the columns, not committed before the ingest ends).  `wr`: the stream that
// writes the store in this ingest; scale > 0: the first of several windows, the whole file being `scale` times this one (store_plan_core.h).
// Bounded store: if the window would pass a cap, what has been extracted becomes the store's content, the pipeline runs over it, the complete
// contigs leave for the host and the contig in flight moves to the front; this window's records follow it.  past_limit: the window does not
// fit 32-bit indices (the caller's to report); room: the columns take its records from R and its CIGAR words from Cg on.
struct PartTimer { double &acc; std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now(); ~PartTimer() { acc += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); } };
struct Admitted { u64 R = 0, Cg = 0; bool past_limit = false, room = false; };
static cov_status admit_window(cov_session *s, u64 nrec, u64 ncig, hipStream_t wr, double scale, Admitted &a) {
    RecordStore &S = s->store;
    a = Admitted{};
    u64 R = S.n_records + s->ing.rec_total, Cg = S.n_cigar + s->ing.cig_total;
    if (nrec && stplan::spill_first(R == 0, s->want_mates, s->ing.fail != 0, R + nrec > s->cap_records, Cg + ncig > s->cap_cigar)) {
        if (wr != s->stream) HIPCHK(hipStreamSynchronize(wr));
        HIPCHK(S.seal(R, Cg, s->stream));
        s->ing.rec_spilled += s->ing.rec_total; s->ing.rec_total = 0; s->ing.cig_total = 0;
        bool progress = false; const cov_status sp = spill_store(s, progress);
        if (sp != COV_OK) return sp;
        R = S.n_records; Cg = S.n_cigar;
    }
    a.R = R; a.Cg = Cg; a.past_limit = !s->ing.fail && (stplan::past_limit(R, nrec) || stplan::past_limit(Cg, ncig));
    if (s->ing.fail || a.past_limit || !nrec) return COV_OK;
    const u64 Nn = scale > 0 ? stplan::first_window_size(R, nrec, 0, scale, s->cap_records) : R + nrec;
    const u64 Cn = scale > 0 ? stplan::first_window_size(Cg, ncig, 1, scale, s->cap_cigar) : Cg + ncig + 1;
    PartTimer alloc{s->ing.s_alloc};
    HIPCHK(S.reserve(Nn, Cn, wr, R, Cg, s->want_mates));
    a.room = true;
    return COV_OK;
}

// The end of an ingest: what it extracted becomes the store's content.
static cov_status ingest_commit(cov_session *s) {
    if (!s->ing.rec_total) return COV_OK;
    RecordStore &S = s->store;
    const u64 Nn = S.n_records + s->ing.rec_total;
    const bool mates_cover = s->want_mates && S.mates_valid == S.n_records;      // the columns cover the whole store as long as every file came through here
    HIPCHK(S.seal(Nn, S.n_cigar + s->ing.cig_total, s->stream));
    if (mates_cover) S.mates_valid = Nn;
    s->finished = false;
    return COV_OK;
}

// What the parse kernels are told about window w: N bytes behind the start of its buffer, carry area included.
static covi::BamScan window_scan(const cov_session *s, u32 w, u64 N, int final, int search_first) {
    const IngestState &I = s->ing;
    covi::BamScan S{};
    S.u = I.g_win[ingplan::win_slot(w)].p; S.N = N; S.p0 = I.g_result.p + ingplan::G_P0; S.seg_bytes = ingplan::SEG_BYTES; S.n_seg = (u32)((S.N + S.seg_bytes - 1) / S.seg_bytes);
    S.n_ref = (int)s->n_targets; S.ref_len = s->d_tlen.p; S.final = final; S.key_lo = I.key_lo; S.key_hi = I.key_hi; S.search_first = search_first;
    S.walk_cap = I.K.carry;
    return S;
}

// ---- the drain: records of the windows whose boundaries are verified go into the store — all windows up to `must_upto` (waiting for
// their k_bam_verify if need be), later ones only if their result is already here.  Per window: take its result, admit it, extract it.
struct WindowResult { u64 nrec = 0, ncig = 0, nlong = 0; };

// The result block of verified window w (page-locked; the host has seen ver_done): statistics, the tail's key, the sticky failure.
static WindowResult take_window_result(cov_session *s, u32 w) {
    IngestState &I = s->ing;
    const u32 q = ingplan::parse_slot(w);
    const u64 *res = I.h_winres + ingplan::WIN_RESULT_WORDS * q;
    cov_ingest_stats &T = I.stats;
    T.windows++; T.segments += I.win[q].n_seg; T.segments_with_start += res[ingplan::W_LIVE_SEGS]; T.records += res[ingplan::W_RECORDS];
    T.max_hop_records = std::max<u64>(T.max_hop_records, res[ingplan::W_MAX_HOP]); T.repaired_starts += res[ingplan::W_REPAIRED];
    u32 st = (u32)res[ingplan::W_STATUS];
    I.tail_key = res[ingplan::W_TAIL_KEY];
    if (!I.is_span() && (!s->want_mates || s->want_grouping)) st &= ~(u32)ingplan::ST_DISORDER;       // whole file: cov_finish reports disorder in file order, beside the other per-record errors
    if (st && !I.fail) { I.fail = st; I.fail_dbg[0] = res[ingplan::W_BAD_SEG]; I.fail_dbg[1] = res[ingplan::W_BAD_START]; I.fail_dbg[2] = res[ingplan::W_BAD_LANDED]; }
    WindowResult r; r.nrec = res[ingplan::W_RECORDS]; r.ncig = res[ingplan::W_CIGAR]; r.nlong = res[ingplan::W_LONG];
    return r;
}

// The records of admitted window w go into the store from (a.R, a.Cg) on, on the extraction stream.
static cov_status extract_window(cov_session *s, u32 w, const Admitted &a, const WindowResult &r) {
    IngestState &I = s->ing;
    hipStream_t ps = I.ext;
    const u32 q = ingplan::parse_slot(w);
    covi::RecStore RS{};
    s->store.view(RS); RS.rec0 = a.R; RS.cig0 = a.Cg;
    if (s->want_mates) s->store.view_mates(RS);
    const covi::BamScan S = window_scan(s, w, I.win[q].N, 0, 0);
    u32 *n_long = reinterpret_cast<u32 *>(I.g_result.p + ingplan::G_LONG);
    if (r.nlong) {      // (sized by the window's own count; the buffer only ever grows)
        PartTimer alloc{I.s_alloc};
        HIPCHK(I.g_long.reserve((size_t)r.nlong, ps));
        HIPCHK(hipMemsetAsync(n_long, 0, sizeof(u32), ps));
    }
    hipLaunchKernelGGL(covi::k_bam_extract, dim3((S.n_seg * I.K.ext_parts + 63) / 64), dim3(64), 0, ps, S, (const covi::SegInfo *)I.g_seg[q].p, (const u64 *)I.g_recbase[q].p,
                       (const u64 *)I.g_cigbase[q].p, RS, reinterpret_cast<u32 *>(I.g_result.p + ingplan::G_FAILURES) + ingplan::FAIL_EXTRACT, I.K.ext_parts,
                       I.g_long.p, n_long, (u32)r.nlong);
    if (r.nlong) {
        hipLaunchKernelGGL(covi::k_bam_extract_long, dim3((u32)((r.nlong + 3) / 4)), dim3(256), 0, ps, S, (const covi::LongRec *)I.g_long.p, (u32)r.nlong, RS);
        I.stats.long_records += r.nlong;
    }
    HIPCHK(hipGetLastError());
    I.rec_total += r.nrec; I.cig_total += r.ncig;
    return COV_OK;
}

static cov_status ingest_drain_(cov_session *s, int64_t must_upto) {
    IngestState &I = s->ing;
    hipStream_t ps = I.ext;     // the host has seen the window's verification finish: nothing on the device to wait for
    while (I.extracted < I.batch) {
        const u32 w = I.extracted, q = ingplan::parse_slot(w);
        if ((int64_t)w > must_upto) { if (hipEventQuery(I.ver_done[q]) != hipSuccess) { (void)hipGetLastError(); break; } }   // not ready is not an error
        else { PartTimer pt{I.s_part[3]}; HIPCHK(hipEventSynchronize(I.ver_done[q])); }
        const WindowResult r = take_window_result(s, w);
        const double scale = w == 0 ? ingplan::first_window_scale(I.win[0].comp_end, I.span_lo, I.span_hi) : 0;
        Admitted a; { const cov_status ad = admit_window(s, r.nrec, r.ncig, ps, scale, a); if (ad != COV_OK) return ad; }
        if (a.past_limit) I.fail = ingplan::ST_PAST_LIMIT;
        if (a.room) { const cov_status e = extract_window(s, w, a, r); if (e != COV_OK) return e; }
        HIPCHK(hipEventRecord(I.ext_done[ingplan::win_slot(w)], ps));
        I.extracted++;
    }
    return COV_OK;
}
static cov_status ingest_drain(cov_session *s, int64_t must_upto) { PartTimer t{s->ing.s_part[0]}; covr::Range rr("ingest: verify + extract windows"); return ingest_drain_(s, must_upto); }

// ---- one round = one window: k_inflate over the next `n` blocks fed but not yet launched (main stream), k_lz_resolve + k_crc32
// behind it (aux stream, beside the next round's k_inflate), then the window's record boundaries (parse stream).
// A lane decodes a whole block serially and every block takes about the same time T, so a launch costs T per started ROUND
// of resident waves: launches are cut to exactly the number of blocks the device holds at once (a launch of 1.05 rounds
// costs 2 T — measured: 46 ms per launch of ~51 k blocks against 23.5 ms per round of 49 152).
// Windows bound the memory: the inflated stream of a 200 M-read BAM is 62 GB, and device allocations cost ~30 ms per GB.
struct Round {
    u32 w = 0, n = 0;             // window, its blocks
    u64 b0 = 0;                   // first of them in the block table
    u64 origin = 0;               // file offset of the first byte of its compressed buffer (from the feed plan's launch step)
    bool final = false;
    u64 wbytes = 0;               // inflated bytes of the blocks
    uint8_t *out_bias = nullptr;  // blocks carry absolute offsets of the inflated stream
    u64 header_left = 0;          // bytes of the BAM header in front of the window's first record (0 once the header has ended)
};

// The round's buffers, sized by ingplan::window_geometry (a process that starts right after another one has given tens of GB back waits
// for the driver in its large allocations: 0.06 s in a 2 M-read run, tools/r06/call43.sh).
static cov_status size_round_buffers(cov_session *s, const Round &R) {
    IngestState &I = s->ing;
    const u32 q = ingplan::parse_slot(R.w), tb = ingplan::tok_slot(R.w);
    DevBuf<uint8_t> &win = I.g_win[ingplan::win_slot(R.w)];
    const ingplan::WindowGeometry g = ingplan::window_geometry(I.span_lo, I.span_hi, R.n, I.K.round_blocks, I.K.carry, covi::INF_SCRATCH_BYTES, covi::INF_TOK_CAP);
    // A buffer that has to GROW may still be in use: drain the device first.  First-time allocations need no such thing —
    // and must not wait, or the first four windows (three window buffers, four parse-state sets) would run one after the other.
    auto grows = [](size_t need, size_t cap) { return cap != 0 && need > cap; };
    if (grows(g.tok_cap, I.g_tok[tb].cap) || grows(g.full, I.g_ntok[tb].cap) || grows(g.scratch_bytes, I.g_scratch.cap) || grows(g.win_bytes, win.cap) ||
        grows(g.seg_cap, I.g_seg[q].cap)) {
        HIPCHK(hipStreamSynchronize(I.aux)); HIPCHK(hipStreamSynchronize(I.parse)); HIPCHK(hipStreamSynchronize(I.ext)); HIPCHK(hipStreamSynchronize(s->stream));
    }
    PartTimer alloc{I.s_alloc};
    HIPCHK(I.g_scratch.reserve(g.scratch_bytes, s->stream));
    HIPCHK(I.g_tok[tb].reserve(g.tok_cap, s->stream));
    HIPCHK(I.g_ntok[tb].reserve(g.full, s->stream));
    HIPCHK(win.reserve(g.win_bytes, s->stream));
    HIPCHK(I.g_seg[q].reserve(g.seg_cap, s->stream)); HIPCHK(I.g_recbase[q].reserve(g.seg_cap, s->stream)); HIPCHK(I.g_cigbase[q].reserve(g.seg_cap, s->stream));
    return COV_OK;
}

// k_inflate on the main stream, LZ and CRC-32 on the aux stream; the parse stream is told when the window's bytes are final.
static cov_status launch_inflate(cov_session *s, const Round &R) {
    IngestState &I = s->ing;
    const InflateKernel &K = I.K;
    const u32 n = R.n, tb = ingplan::tok_slot(R.w), cs = ingplan::cwin_slot(R.w);
    const covi::BgzfBlock *blocks = I.g_blocks.p + R.b0;
    u32 *status = I.g_status.p + R.b0, *n_failed = reinterpret_cast<u32 *>(I.g_result.p + ingplan::G_FAILURES) + ingplan::FAIL_INFLATE;
    covi::tokpos_t *tok = I.g_tok[tb].p; u32 *ntok = I.g_ntok[tb].p;
    HIPCHK(hipStreamWaitEvent(s->stream, I.fed, 0));
    // token buffers alternate: this k_inflate may not start before the k_lz_resolve that read the same buffer two rounds ago is done;
    // the window buffer is free once the extraction of the window three rounds ago is done
    if (ingplan::tok_reused(R.w)) HIPCHK(hipStreamWaitEvent(s->stream, I.lz_done[tb], 0));
    if (ingplan::win_reused(R.w)) HIPCHK(hipStreamWaitEvent(s->stream, I.ext_done[ingplan::win_slot(R.w)], 0));
    const uint8_t *comp_bias = I.g_cwin[cs].p - R.origin;     // blocks carry absolute file offsets
    if (K.version == 3)
        hipLaunchKernelGGL(covi::k_inflate_wave, dim3(n), dim3(64), 0, s->stream, comp_bias, blocks, n, R.out_bias, tok, ntok, status, n_failed, 0u);
    else
        hipLaunchKernelGGL((covi::k_inflate<INF1_LB, INF1_DB, false>), dim3((n + 63u) / 64u), dim3(64), covi::inflate_smem_bytes(INF1_LB, INF1_DB), s->stream, comp_bias,
                           blocks, n, R.out_bias, I.g_scratch.p, tok, ntok, status, n_failed);
    HIPCHK(hipEventRecord(I.inf_done[tb], s->stream));
    HIPCHK(hipEventRecord(I.cdone[cs], s->stream));      // this round's compressed buffer may be overwritten (three rounds on)
    HIPCHK(hipStreamWaitEvent(I.aux, I.inf_done[tb], 0));
    if (K.lz_version == 1)
        hipLaunchKernelGGL(covi::k_lz_resolve, dim3((n + 3u) / 4u), dim3(256), 0, I.aux, blocks, n, R.out_bias, (const covi::tokpos_t *)tok, (const u32 *)ntok);
    else
        hipLaunchKernelGGL(covi::k_lz_stage, dim3((n + 3u) / 4u), dim3(256), 0, I.aux, blocks, n, R.out_bias, (const covi::tokpos_t *)tok, (const u32 *)ntok);
    // the window's bytes are final once the matches are resolved: the boundary search (parse stream) starts here, beside the
    // CRC-32 pass, whose verdict is only looked at in cov_ingest_end (the aux stream is in order, so CRC(w) is done before LZ(w + 1)
    // and with it before anything may overwrite window w)
    HIPCHK(hipEventRecord(I.lz_done[tb], I.aux));
    if (I.check_crc) {
        if (K.version == 3)      // a wave per block, coalesced; resident workgroups stride over the window's blocks
            hipLaunchKernelGGL(covi::k_crc32_wave, dim3(std::min<u32>((n + 7u) / 8u, (u32)s->n_cus * 4u)), dim3(512), 0, I.aux,
                               blocks, n, (const uint8_t *)R.out_bias, status, n_failed, (const u32 *)I.g_crc_tab.p);
        else                     // the lane-per-block combination keeps the lane-per-block CRC
            hipLaunchKernelGGL(covi::k_crc32, dim3((n + 255u) / 256u), dim3(256), 0, I.aux, blocks, n, (const uint8_t *)R.out_bias, status, n_failed);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamWaitEvent(I.parse, I.lz_done[tb], 0));
    return COV_OK;
}

// The window's records on the parse stream: tail of the previous window in front, boundaries, counts, the new tail; its result block
// follows to the host.
static cov_status launch_parse(cov_session *s, const Round &R) {
    IngestState &I = s->ing;
    const u32 w = R.w, q = ingplan::parse_slot(w);
    const covi::BamScan S = window_scan(s, w, I.K.carry + R.wbytes, (R.final && !I.open_end) ? 1 : 0, (w == 0 && I.search_first) ? 1 : 0);
    const covi::BgzfBlock *last = R.n ? &I.h_blocks[R.b0 + R.n - 1] : nullptr;
    I.win[q].N = S.N; I.win[q].n_seg = S.n_seg; I.win[q].comp_end = last ? last->in_off + last->in_len + 8 : I.comp;
    hipStream_t ps = I.parse;
    u64 *G = I.g_result.p, *res = G + ingplan::win_result_at(w);
    uint8_t *win = I.g_win[ingplan::win_slot(w)].p;
    if (ingplan::win_reused(w)) HIPCHK(hipStreamWaitEvent(ps, I.ext_done[ingplan::win_slot(w)], 0));     // the carried tail goes in front of a buffer whose records must be out
    hipLaunchKernelGGL(covi::k_carry_in, dim3(1), dim3(1024), 0, ps, win, I.K.carry, (const uint8_t *)I.g_carry.p, (const u64 *)(G + ingplan::G_CARRY_LEN),
                       R.header_left, G + ingplan::G_P0);
    hipLaunchKernelGGL(covi::k_bam_find, dim3((S.n_seg + 3) / 4), dim3(256), 0, ps, S, I.g_seg[q].p);
    hipLaunchKernelGGL(covi::k_bam_hop, dim3((S.n_seg + 63) / 64), dim3(64), 0, ps, S, I.g_seg[q].p);
    hipLaunchKernelGGL(covi::k_bam_verify, dim3(1), dim3(1024), 0, ps, S, I.g_seg[q].p, I.g_recbase[q].p, I.g_cigbase[q].p, res,
                       I.g_carry.p, (u64)I.K.carry, G + ingplan::G_CARRY_LEN, G + ingplan::G_PREV_KEY);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(I.h_winres + ingplan::WIN_RESULT_WORDS * q, res, ingplan::WIN_RESULT_WORDS * sizeof(u64), hipMemcpyDeviceToHost, ps));
    HIPCHK(hipEventRecord(I.ver_done[q], ps));
    return COV_OK;
}

// The next `n64` blocks fed but not launched become window ing.batch; `origin`: where the round's compressed buffer starts in the file.
static cov_status launch_round_(cov_session *s, uint64_t n64, uint64_t origin, bool final) {
    IngestState &I = s->ing;
    Round R;
    R.b0 = I.launched; R.n = (u32)std::min<uint64_t>(n64, I.feed.blocks - R.b0); R.w = I.batch; R.origin = origin; R.final = final;
    if (ingplan::win_reused(R.w)) {      // this window's buffer and parse state are free again
        const cov_status d = ingest_drain(s, ingplan::extracted_before_launch(R.w)); if (d != COV_OK) return d;
    }
    { const cov_status b = size_round_buffers(s, R); if (b != COV_OK) return b; }
    const covi::BgzfBlock *first = R.n ? &I.h_blocks[R.b0] : nullptr, *last = R.n ? &I.h_blocks[R.b0 + R.n - 1] : nullptr;
    const u64 out_off0 = first ? first->out_off : I.feed.infl;
    R.wbytes = last ? last->out_off + last->isize - out_off0 : 0;
    R.out_bias = I.g_win[ingplan::win_slot(R.w)].p + I.K.carry - out_off0;
    // The BAM header may run over the first windows: such a window parses to no record and no tail (p0 lies behind its end), and the next one
    // is told how much of the header is left.  Only a header that does not end inside the stream's last window is a failure.
    R.header_left = ingplan::header_left(I.first_record, out_off0);
    if (R.final && R.header_left > R.wbytes && !I.fail) I.fail = ingplan::ST_HEADER_LONG;
    if (R.n) { const cov_status c = launch_inflate(s, R); if (c != COV_OK) return c; }
    { const cov_status c = launch_parse(s, R); if (c != COV_OK) return c; }
    I.launched += R.n;
    I.batch++;
    return ingest_drain(s, -1);      // whatever is verified already
}
static cov_status launch_round(cov_session *s, uint64_t n64, uint64_t origin, bool final) { PartTimer t{s->ing.s_part[1]}; covr::Range rr("ingest: inflate round launch"); return launch_round_(s, n64, origin, final); }

cov_status cov_ingest_slot_wait(cov_session *s, int slot) {
    if (!s || slot < 0 || slot >= COV_INGEST_SLOTS || !s->ing.ev[slot]) return COV_ERR_INVALID_ARG;      // (also valid after cov_ingest_end: the slot's last upload)
    HIPCHK(hipSetDevice(s->cfg.device));
    HIPCHK(hipEventSynchronize(s->ing.ev[slot]));
    return COV_OK;
}

// ---- the feed: ingplan::feed_plan says which bytes and table entries of a piece go where and which rounds they complete; the three
// functions below execute its steps.
// Bytes [a, b) of the file (present in the staging piece that starts at file offset `piece_off`) go to the compressed buffer of
// round r, whose first byte is file offset `origin`.
static cov_status ingest_copy_range(cov_session *s, u32 r, u64 origin, u64 a, u64 b, const uint8_t *piece, u64 piece_off) {
    IngestState &I = s->ing;
    PartTimer pt{I.s_part[2]};
    DevBuf<uint8_t> &cw = I.g_cwin[ingplan::cwin_slot(r)];
    const size_t need = (size_t)ingplan::cwin_bytes(I.ccap);
    if (cw.cap < need) {
        if (cw.cap) { HIPCHK(hipStreamSynchronize(I.copy)); HIPCHK(hipStreamSynchronize(s->stream)); }      // replaced while possibly in use
        PartTimer alloc{I.s_alloc};
        HIPCHK(cw.reserve(need, s->stream));
    }
    if ((int64_t)r > I.copy_cleared) {     // first bytes of this round: the k_inflate that read this buffer three rounds ago must be done
        if (ingplan::cwin_reused(r)) HIPCHK(hipStreamWaitEvent(I.copy, I.cdone[ingplan::cwin_slot(r)], 0));
        I.copy_cleared = (int64_t)r;
    }
    if (a < origin || b - origin > cw.cap) { s->err = "cov_ingest_feed: internal error, bytes outside their round's buffer"; return COV_ERR_STATE; }
    HIPCHK(hipMemcpyAsync(cw.p + (a - origin), piece + (a - piece_off), b - a, hipMemcpyHostToDevice, I.copy));
    return COV_OK;
}

// Table entries [from, to) follow the bytes on the copy stream; ing.fed marks "everything fed so far is on the device"
// (recorded even without new entries: the bytes in front of it may complete a round).
static cov_status ingest_upload_table(cov_session *s, u64 from, u64 to) {
    if (from < to)
        HIPCHK(hipMemcpyAsync(s->ing.g_blocks.p + from, s->ing.h_blocks + from, (size_t)(to - from) * sizeof(covi::BgzfBlock), hipMemcpyHostToDevice, s->ing.copy));
    HIPCHK(hipEventRecord(s->ing.fed, s->ing.copy));
    return COV_OK;
}

static cov_status ingest_run_step(cov_session *s, const ingplan::Step &st, const uint8_t *piece, u64 piece_off) {
    switch (st.kind) {
    case ingplan::Step::COPY: return ingest_copy_range(s, st.round, st.origin, st.a, st.b, piece, piece_off);
    case ingplan::Step::UPLOAD: return ingest_upload_table(s, st.a, st.b);
    default: return launch_round(s, st.n, st.origin, false);
    }
}

// Room for `n_blocks` more table entries: the page-locked mirror (the async uploads read it later) and the device copy with its status words.
static cov_status ingest_grow_tables(cov_session *s, uint32_t n_blocks) {
    IngestState &I = s->ing;
    const u64 need = I.feed.blocks + n_blocks;
    if (need > I.h_blocks_cap) {
        const size_t nc = std::max<size_t>(need, I.h_blocks_cap * 2 + 4096);
        covi::BgzfBlock *nb = nullptr;
        HIPCHK(hipHostMalloc((void **)&nb, nc * sizeof(covi::BgzfBlock), hipHostMallocDefault));
        HIPCHK(hipStreamSynchronize(I.copy));      // earlier uploads still read the old mirror
        if (I.h_blocks) { memcpy(nb, I.h_blocks, I.feed.blocks * sizeof(covi::BgzfBlock)); (void)hipHostFree(I.h_blocks); }
        I.h_blocks = nb; I.h_blocks_cap = nc;
    }
    if (need > I.g_blocks.cap || need > I.g_status.cap) {
        HIPCHK(hipStreamSynchronize(I.copy)); HIPCHK(hipStreamSynchronize(I.aux)); HIPCHK(hipStreamSynchronize(s->stream));
        HIPCHK(I.g_blocks.reserve(need, s->stream, I.feed.blocks));
        HIPCHK(I.g_status.reserve(need, s->stream, I.feed.blocks));
    }
    return COV_OK;
}

cov_status cov_ingest_feed(cov_session *s, int slot, const void *host_bytes, uint64_t file_offset, uint64_t n_bytes,
                           const cov_bgzf_block *blocks, uint32_t n_blocks) {
    if (!s || !s->ing.active || slot < 0 || slot >= COV_INGEST_SLOTS || (n_bytes && !host_bytes) || (n_blocks && !blocks)) return COV_ERR_INVALID_ARG;
    if (s->sam_active) { s->err = "cov_ingest_feed: a SAM text ingest is open (cov_sam_feed / cov_sam_end)"; return COV_ERR_STATE; }
    if (file_offset + n_bytes > s->ing.comp) { s->err = "cov_ingest_feed: bytes beyond the size given to cov_ingest_begin"; return COV_ERR_INVALID_ARG; }
    covr::Range rr("ingest: window upload (cov_ingest_feed)");
    HIPCHK(hipSetDevice(s->cfg.device));
    { const cov_status d = ingest_drain(s, -1); if (d != COV_OK) return d; }      // extraction of whatever got verified meanwhile
    { const cov_status g = ingest_grow_tables(s, n_blocks); if (g != COV_OK) return g; }
    IngestState &I = s->ing;
    // (Short first rounds — an eighth, a quarter, half a window, so that the device starts on 0.2 GB instead of 1.8 — were measured on one box,
    // alternating: ingest 0.726 s against 0.677 s with full rounds from the start, profiles/r04_ramp_ab_200M.log.  Removed.)
    // (Short LAST rounds — a quarter of the blocks over the file's last 450 / 900 / 1800 MB, to shorten what the device still has to do when the
    // last byte has arrived — measured in round 6: ingest 0.498 / 0.505 / 0.500 s against 0.494 s with full rounds to the end; the device is
    // only just faster than the link, so the lag behind the feed does not shrink with the rounds and their launches wait for the drains.
    // profiles/r06_tail_rounds_ab_200M.json.  Removed.)
    const u64 blocks0 = I.feed.blocks;
    I.steps.clear();
    const bool blocks_ok = ingplan::feed_plan(I.feed, ingplan::FeedRule{I.K.round_blocks, I.ccap}, I.batch, file_offset, n_bytes, blocks, n_blocks,
                                              [&I](const ingplan::Step &st) { I.steps.push_back(st); });
    for (u64 i = blocks0; i < I.feed.blocks; i++) {      // the accepted entries, in the mirror before any step uploads them
        const cov_bgzf_block &b = blocks[i - blocks0];
        covi::BgzfBlock d; d.in_off = b.in_off; d.out_off = b.out_off; d.in_len = b.in_len; d.isize = b.isize; d.crc = b.crc; d.pad = 0;
        I.h_blocks[i] = d;
    }
    for (const ingplan::Step &st : I.steps) { const cov_status c = ingest_run_step(s, st, (const uint8_t *)host_bytes, file_offset); if (c != COV_OK) return c; }
    if (!blocks_ok) {      // (the rounds completed by the blocks in front of the offending one have been launched, as ever)
        s->err = "cov_ingest_feed: block outside the bytes fed so far, out of order, or not contiguous in the inflated stream"; return COV_ERR_INVALID_ARG;
    }
    HIPCHK(hipEventRecord(I.ev[slot], I.copy));
    return COV_OK;
}

cov_status cov_ingest_last_stats(const cov_session *s, cov_ingest_stats *out) {
    if (!s || !out) return COV_ERR_INVALID_ARG;
    *out = s->ing.stats_last;
    return COV_OK;
}

// ---- the end: last round, drain, the ingest's own result words, the verdict (ingplan::outcome) and its text.
static cov_status ingest_read_globals(cov_session *s, u64 (&glob)[ingplan::G_WINDOWS]) {
    IngestState &I = s->ing;
    HIPCHK(hipStreamSynchronize(I.ext));
    HIPCHK(hipStreamSynchronize(I.aux));        // the CRC pass of the last window runs beside its boundary search: its failure count is read below
    HIPCHK(hipMemcpyAsync(glob, I.g_result.p, sizeof glob, hipMemcpyDeviceToHost, I.parse));
    HIPCHK(hipStreamSynchronize(I.parse));
    HIPCHK(hipStreamSynchronize(s->stream));
    return COV_OK;
}

static std::string outcome_text(const IngestState &I, ingplan::Outcome o, u32 inflate_failures) {
    switch (o) {
    case ingplan::INFLATE_FAILED: return "device ingest: " + std::to_string(inflate_failures) + " BGZF blocks failed to inflate or their CRC-32 (handing the file to the CPU reader)";
    // only looked at because mates were asked for: the device pair filter takes "same tid" for "same run of one reference"
    case ingplan::DISORDER_FILE: return "device ingest: record keys (tid) decrease somewhere in the file; the pair filter of such a file runs on the host (handing the file to the CPU reader)";
    // contig.rs:129-132: the reference stops at the first record whose tid is lower than its predecessor's
    case ingplan::UNSORTED: return "BAM file appears to be unsorted. Input BAM files must be sorted by reference (i.e. by samtools sort)";
    case ingplan::PAST_LIMIT: return "more than 2^32 records or CIGAR words of one reference in the record store";
    case ingplan::HEADER_LONG: return "device ingest: the BAM header is longer than the first window of the inflated stream (handing the file to the CPU reader)";
    case ingplan::CG_CIGAR: return "device ingest: a record keeps its CIGAR in CG:B,I (handing the file to the CPU reader)";
    case ingplan::TAIL_LARGE: return "device ingest: a record larger than the carry buffer between windows (handing the file to the CPU reader)";
    case ingplan::TRUNCATED: return "device ingest: truncated BAM record";
    case ingplan::CHAIN: return "device ingest: record boundaries did not verify at segment " + std::to_string(I.fail_dbg[0]) + " (start " + std::to_string(I.fail_dbg[1]) +
                                ", landed " + std::to_string(I.fail_dbg[2]) + "; handing the file to the CPU reader)";
    case ingplan::CORRUPT_RECORD: return "device ingest: corrupt BAM record";
    case ingplan::SPAN_CUTS_RECORD: return "device ingest: the bytes fed for this span end inside one of its own records (handing the span to the CPU reader)";
    case ingplan::SPAN_END_UNSEEN: return "device ingest: the bytes fed for this span end before a record of the next span (handing the span to the CPU reader)";
    default: return std::string();
    }
}

cov_status cov_ingest_end(cov_session *s, uint64_t *n_records_out) {
    if (!s || !s->ing.active) return COV_ERR_INVALID_ARG;
    if (s->sam_active) { s->err = "cov_ingest_end: a SAM text ingest is open (cov_sam_end)"; return COV_ERR_STATE; }
    covr::Range rr("ingest: last rounds + parse (cov_ingest_end)");
    IngestState &I = s->ing;
    I.active = false;
    HIPCHK(hipSetDevice(s->cfg.device));
    if (n_records_out) *n_records_out = 0;
    { const cov_status lrc = launch_round(s, I.feed.round_n, I.feed.round_start, true); if (lrc != COV_OK) return lrc; }     // the last round: whatever the open one holds
    { const cov_status d = ingest_drain(s, (int64_t)I.batch); if (d != COV_OK) return d; }
    u64 glob[ingplan::G_WINDOWS];
    { const cov_status g = ingest_read_globals(s, glob); if (g != COV_OK) return g; }
    I.stats_last = I.stats;
    if (cov_timing_on())
        fprintf(stderr, "[covermhip] ingest: %llu blocks in %u windows of %u, device allocations %.3fs; host time in drain %.3fs (waiting for a verification %.3fs), in launches %.3fs (drains inside included), in upload calls %.3fs\n",
                (unsigned long long)I.feed.blocks, I.batch, I.K.round_blocks, I.s_alloc, I.s_part[0], I.s_part[3], I.s_part[1], I.s_part[2]);
    ingplan::EndFacts f;
    f.fail = I.fail; f.inflate_failures = ingplan::inflate_failures(glob[ingplan::G_FAILURES]); f.extract_failures = ingplan::extract_failures(glob[ingplan::G_FAILURES]);
    f.span = I.is_span(); f.open_end = I.open_end; f.tail_key = I.tail_key; f.prev_key = glob[ingplan::G_PREV_KEY]; f.key_hi = I.key_hi; f.spilled = I.rec_spilled != 0;
    const ingplan::Outcome o = ingplan::outcome(f);
    switch (ingplan::ending(o, f.spilled)) {
    case ingplan::END_OK: break;
    case ingplan::END_UNSORTED: s->err = outcome_text(I, o, f.inflate_failures); return COV_ERR_UNSORTED;
    case ingplan::END_INVALID: s->err = outcome_text(I, o, f.inflate_failures); return COV_ERR_INVALID_ARG;
    case ingplan::END_HAND_BACK: s->err = outcome_text(I, o, f.inflate_failures); return COV_ERR_INGEST_FALLBACK;
    case ingplan::END_LOST:      // "nothing was appended" no longer holds: part of the file is already in the spilled results
        s->err = outcome_text(I, o, f.inflate_failures) + " (after part of the file had left the bounded record store: it cannot be handed to the CPU reader on this session any more)";
        return COV_ERR_STATE;
    }
    { const cov_status c = ingest_commit(s); if (c != COV_OK) return c; }
    if (n_records_out) *n_records_out = I.rec_total + I.rec_spilled;
    return COV_OK;
}

// ---------------------------------------------------------------------------------------------- SAM text ingest (covermhip.h cov_sam_*, sam_kernels.hip.h)
// One window = one cov_sam_feed: upload on the copy stream, then on the session stream masks -> line scan -> (the host learns the number of
// lines) -> per-line counts -> two scans -> (the host learns records, CIGAR words and the first error) -> decode into the store.  The host
// waits twice per window; the upload of the next window runs beside the decode of this one (two text buffers).
static cov_status sam_fail(cov_session *s) {
    const u32 e = s->sam_err; const u64 line = s->sam_err_line;
    (void)cov_ingest_abort(s);      // drains the device, appends nothing, leaves the session ready for cov_push_batch
    const std::string at = " (line " + std::to_string(line) + ")";
    switch (e) {
    case samc::ERR_MALFORMED: s->err = "malformed SAM line" + at; return COV_ERR_INVALID_ARG;
    case samc::ERR_CIGAR_OPS: s->err = "SAM line with a CIGAR of more than 65535 operations" + at; return COV_ERR_INVALID_ARG;
    case samc::ERR_LINE_LONG: s->err = "SAM line longer than the decode window of " + std::to_string(s->sam_window) + " bytes" + at; return COV_ERR_INVALID_ARG;
    default: s->err = "SAM text: a header line (@) behind the first alignment line" + at + " (handing the file to the CPU reader)"; return COV_ERR_INGEST_FALLBACK;
    }
}
constexpr u32 SAM_ERR_AT_LINE = 4u;

uint64_t cov_sam_window_bytes(const cov_session *s) { return s ? s->sam_window : 0; }

cov_status cov_sam_begin(cov_session *s, const char *names_blob, const uint64_t *name_off, uint32_t n_names, uint64_t expected_bytes) {
    if (!s || (n_names && (!names_blob || !name_off))) return COV_ERR_INVALID_ARG;
    if (s->ing.active) { s->err = "cov_sam_begin: an ingest is still open (cov_ingest_end / cov_sam_end or cov_ingest_abort first)"; return COV_ERR_STATE; }
    HIPCHK(hipSetDevice(s->cfg.device));
    HIPCHK(ingest_prep_wait(s));
    if (!s->ing.copy) HIPCHK(ingest_prepare_(s));
    { const cov_status a = materialise_adopted(s); if (a) return a; }
    hipStream_t st = s->stream;
    HIPCHK(hipStreamSynchronize(st));
    u64 W = 32ull << 20;
    { long long v; if (covknob::get("sam_window_bytes", v) && v >= 256) W = (u64)v; }      // tests: many small windows
    W = std::min<u64>(W, 1ull << 30);
    s->sam_window = W;
    const size_t text_cap = (size_t)((W + 1 + samc::MASK_WG_BYTES - 1) / samc::MASK_WG_BYTES * samc::MASK_WG_BYTES), n_words = (size_t)((W + 1 + 63) / 64);
    for (int j = 0; j < 2; j++) {
        HIPCHK(s->m_text[j].reserve(text_cap, st));
        if (!s->sam_buf_free[j]) HIPCHK(hipEventCreateWithFlags(&s->sam_buf_free[j], hipEventDisableTiming));
    }
    for (hipEvent_t &e : s->sam_ev) if (!e) HIPCHK(hipEventCreate(&e));
    HIPCHK(s->m_nl.reserve(n_words, st)); HIPCHK(s->m_tab.reserve(n_words, st)); HIPCHK(s->m_res.reserve(covs::RES_WORDS, st));
    HIPCHK(s->m_bsum[0].reserve((size_t)scan_blocks((u32)n_words) + 1, st));
    // the reference names: blob, offsets, and the open-addressing table over them (sam_parse_core.h)
    s->m_names = samc::Table{nullptr, 0u, nullptr, nullptr};
    if (n_names) {
        const u64 blob_bytes = name_off[n_names];
        const u32 slots = samc::table_size(n_names);
        std::vector<u32> h_slots(slots, 0u);
        for (u32 i = 0; i < n_names; i++) samc::table_insert(h_slots.data(), slots - 1u, (const uint8_t *)names_blob, (const u64 *)name_off, i);
        HIPCHK(s->m_blob.reserve((size_t)blob_bytes + 8, st)); HIPCHK(s->m_noff.reserve((size_t)n_names + 1, st)); HIPCHK(s->m_slots.reserve(slots, st));
        if (blob_bytes) HIPCHK(hipMemcpyAsync(s->m_blob.p, names_blob, blob_bytes, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(s->m_noff.p, name_off, ((size_t)n_names + 1) * sizeof(u64), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(s->m_slots.p, h_slots.data(), (size_t)slots * sizeof(u32), hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
        s->m_names = samc::Table{s->m_slots.p, slots - 1u, s->m_blob.p, s->m_noff.p};
    }
    s->ing.reset_for_file(IngestState::Reset::SAM_FILE);
    s->sam_expected = expected_bytes; s->sam_lines = 0; s->sam_bytes = 0; s->sam_err = 0; s->sam_err_line = 0; s->sam_k = 0;
    s->sam_seen_record = false; s->sam_decode_timed = false; s->sam_ms = 0.f; s->sam_launches = 0;
    s->ing.active = true; s->sam_active = true;
    return COV_OK;
}

cov_status cov_sam_slot_wait(cov_session *s, int slot) { return cov_ingest_slot_wait(s, slot); }

static float sam_elapsed(hipEvent_t a, hipEvent_t b) { float ms = 0.f; return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : 0.f; }

cov_status cov_sam_feed(cov_session *s, int slot, const void *host_bytes, uint64_t n_bytes) {
    if (!s || slot < 0 || slot >= COV_INGEST_SLOTS || (n_bytes && !host_bytes)) return COV_ERR_INVALID_ARG;
    if (!s->sam_active) { s->err = "cov_sam_feed: no SAM text ingest is open (cov_sam_begin)"; return COV_ERR_STATE; }
    if (n_bytes == 0) return COV_OK;
    covr::Range rr("sam: window upload + decode (cov_sam_feed)");
    HIPCHK(hipSetDevice(s->cfg.device));
    const u64 W = s->sam_window;
    if (n_bytes > W) { s->err = "cov_sam_feed: a piece larger than the window (cov_sam_window_bytes)"; return COV_ERR_INVALID_ARG; }
    const uint8_t *hb = (const uint8_t *)host_bytes;
    const bool open_end = hb[n_bytes - 1] != '\n';
    if (open_end && n_bytes == W && !memchr(hb, '\n', n_bytes)) {      // a whole window without a line end
        s->sam_err = samc::ERR_LINE_LONG; s->sam_err_line = s->sam_lines + 1;
        return sam_fail(s);
    }
    const u32 j = s->sam_k & 1u;
    uint8_t *text = s->m_text[j].p;
    hipStream_t st = s->stream, cp = s->ing.copy;
    if (s->sam_k >= 2) HIPCHK(hipStreamWaitEvent(cp, s->sam_buf_free[j], 0));      // the decode of window k - 2 has read this buffer
    HIPCHK(hipMemcpyAsync(text, hb, n_bytes, hipMemcpyHostToDevice, cp));
    u64 n = n_bytes;
    if (open_end) { HIPCHK(hipMemsetAsync(text + n, '\n', 1, cp)); n++; }      // a last line without its line end is a record
    HIPCHK(hipEventRecord(s->ing.ev[slot], cp));
    HIPCHK(hipStreamWaitEvent(st, s->ing.ev[slot], 0));
    u64 *res = s->m_res.p;
    HIPCHK(hipMemsetAsync(res, 0xff, covs::RES_WORDS * sizeof(u64), st));
    HIPCHK(hipMemsetAsync(res + covs::RES_LAST_AT, 0, sizeof(u64), st));
    HIPCHK(hipEventRecord(s->sam_ev[0], st));
    const u32 n_words = (u32)((n + 63) / 64);
    hipLaunchKernelGGL(covs::k_sam_masks, dim3((u32)((n + samc::MASK_WG_BYTES - 1) / samc::MASK_WG_BYTES)), dim3(256), 0, st, (const uint8_t *)text, n, s->m_nl.p, s->m_tab.p);
    const covs::NlPop nlp{s->m_nl.p};
    scan_offsets(st, nlp, n_words, s->m_bsum[0].p, res + covs::RES_LINES);
    HIPCHK(hipGetLastError());
    u64 *h = s->ing.h_winres;
    HIPCHK(hipMemcpyAsync(h, res, covs::RES_WORDS * sizeof(u64), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const u32 n_lines = (u32)h[covs::RES_LINES], nbl = scan_blocks(n_lines);
    HIPCHK(s->m_line_end.reserve(n_lines, st)); HIPCHK(s->m_cnt.reserve(n_lines, st)); HIPCHK(s->m_rec_idx.reserve(n_lines, st)); HIPCHK(s->m_cig_idx.reserve(n_lines, st));
    HIPCHK(s->m_bsum[1].reserve((size_t)nbl + 1, st)); HIPCHK(s->m_bsum[2].reserve((size_t)nbl + 1, st));
    const covs::Lines L{text, s->m_tab.p, s->m_line_end.p, n_lines};
    scan_apply(st, nlp, covs::LineEmit{s->m_nl.p, s->m_line_end.p}, n_words, s->m_bsum[0].p);
    hipLaunchKernelGGL(covs::k_sam_count, dim3((n_lines + 255u) / 256u), dim3(256), 0, st, L, s->m_cnt.p, res);
    const covs::IsRec isr{s->m_cnt.p}; const covs::NCig ncg{s->m_cnt.p};
    scan_offsets(st, isr, n_lines, s->m_bsum[1].p, res + covs::RES_RECORDS);
    scan_apply(st, isr, covs::Put{s->m_rec_idx.p}, n_lines, s->m_bsum[1].p);
    scan_offsets(st, ncg, n_lines, s->m_bsum[2].p, res + covs::RES_CIGAR);
    scan_apply(st, ncg, covs::Put{s->m_cig_idx.p}, n_lines, s->m_bsum[2].p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s->sam_ev[1], st));
    HIPCHK(hipMemcpyAsync(h, res, covs::RES_WORDS * sizeof(u64), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    s->sam_ms += sam_elapsed(s->sam_ev[0], s->sam_ev[1]); s->sam_launches += 11;
    if (s->sam_decode_timed) { s->sam_ms += sam_elapsed(s->sam_ev[2], s->sam_ev[3]); s->sam_decode_timed = false; }      // the previous window's decode
    const u64 nrec = h[covs::RES_RECORDS], ncig = h[covs::RES_CIGAR], err = h[covs::RES_ERR], first_rec = h[covs::RES_FIRST_REC], last_at = h[covs::RES_LAST_AT];
    {   // the first offending line in file order: a malformed record, or a header line behind a record
        u64 bad_line = ~0ull; u32 bad = 0;
        if (err != ~0ull) { bad_line = err >> 8; bad = (u32)(err & 0xffu); }
        if (last_at && (s->sam_seen_record || (first_rec != ~0ull && last_at - 1 > first_rec)) && last_at - 1 < bad_line) { bad_line = last_at - 1; bad = SAM_ERR_AT_LINE; }
        // (last_at is the LAST header line of the window: the verdict is right, the line named may be a later one of several)
        if (bad) { s->sam_err = bad; s->sam_err_line = s->sam_lines + bad_line + 1; return sam_fail(s); }
    }
    if (nrec) s->sam_seen_record = true;
    s->sam_lines += n_lines; s->sam_bytes += n_bytes;
    // first of several windows of a file whose size is known: the store is sized once
    const double scale = s->sam_k == 0 && s->sam_expected > n_bytes ? (double)s->sam_expected / (double)n_bytes * 1.1 : 0;
    Admitted a; { const cov_status ad = admit_window(s, nrec, ncig, st, scale, a); if (ad != COV_OK) return ad; }
    if (a.past_limit) {
        (void)cov_ingest_abort(s);
        s->err = "more than 2^32 records or CIGAR words of one reference in the record store"; return COV_ERR_INVALID_ARG;
    }
    if (a.room) {
        covs::Out O{};
        s->store.view(O); O.rec0 = a.R; O.cig0 = a.Cg;
        if (s->want_mates) s->store.view_mates(O);
        HIPCHK(hipEventRecord(s->sam_ev[2], st));
        hipLaunchKernelGGL(covs::k_sam_decode, dim3((n_lines + 255u) / 256u), dim3(256), 0, st, L, (const u32 *)s->m_cnt.p, (const u32 *)s->m_rec_idx.p, (const u32 *)s->m_cig_idx.p, s->m_names, O);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(s->sam_ev[3], st));
        s->sam_decode_timed = true; s->sam_launches++;
        s->ing.rec_total += nrec; s->ing.cig_total += ncig;
    }
    HIPCHK(hipEventRecord(s->sam_buf_free[j], st));
    s->sam_k++;
    return COV_OK;
}

cov_status cov_sam_end(cov_session *s, uint64_t *n_records_out) {
    if (!s) return COV_ERR_INVALID_ARG;
    if (n_records_out) *n_records_out = 0;
    if (!s->sam_active) { s->err = "cov_sam_end: no SAM text ingest is open (cov_sam_begin)"; return COV_ERR_STATE; }
    HIPCHK(hipSetDevice(s->cfg.device));
    s->ing.active = false; s->sam_active = false;
    HIPCHK(hipStreamSynchronize(s->ing.copy));
    HIPCHK(hipStreamSynchronize(s->stream));
    if (s->sam_decode_timed) { s->sam_ms += sam_elapsed(s->sam_ev[2], s->sam_ev[3]); s->sam_decode_timed = false; }
    if (cov_timing_on())
        fprintf(stderr, "[covermhip] sam: device SAM decode: %llu bytes in %u windows of %llu, %llu lines, %llu records, kernels %.3f ms\n", (unsigned long long)s->sam_bytes, s->sam_k,
                (unsigned long long)s->sam_window, (unsigned long long)s->sam_lines, (unsigned long long)(s->ing.rec_total + s->ing.rec_spilled), s->sam_ms);
    { const cov_status c = ingest_commit(s); if (c != COV_OK) return c; }
    if (n_records_out) *n_records_out = s->ing.rec_total + s->ing.rec_spilled;
    return COV_OK;
}

cov_status cov_ingest_want_mates(cov_session *s, int on) {
    if (!s || s->ing.active) return COV_ERR_INVALID_ARG;
    s->want_mates = on != 0;
    return COV_OK;
}

cov_status cov_ingest_want_grouping(cov_session *s, int on) {
    if (!s || s->ing.active) return COV_ERR_INVALID_ARG;
    s->want_grouping = on != 0;
    return COV_OK;
}

// ---------------------------------------------------------------------------------------------- reader-stage pair filter (pair_kernels.hip.h)
static_assert(sizeof(cov_pair_filter) == sizeof(covp::PairFilter) && offsetof(cov_pair_filter, min_aligned_length_pair) == offsetof(covp::PairFilter, min_aligned_length_pair) &&
              offsetof(cov_pair_filter, min_mapq) == offsetof(covp::PairFilter, min_mapq), "cov_pair_filter mirrors the device struct");

// The store replaced by its records order[0 .. S) (order[new] = old): CIGAR offsets by a scan over the selected records' CIGAR lengths, whose
// consumer moves the fixed fields and the CIGAR words (pair_kernels.hip.h); with_mates: the three mate columns travel along.
static cov_status gather_store(cov_session *s, const u32 *order, u32 S, bool with_mates) {
    hipStream_t st = s->stream;
    DevBuf<u32> d_bsum; DevBuf<u64> d_tot;
    struct Rel { DevBuf<u32> &a; DevBuf<u64> &b; ~Rel() { a.release(); b.release(); } } rel{d_bsum, d_tot};
    RecordStore sel;      // (after the swap below: the old store, which goes with it)
    HIPCHK(d_bsum.reserve((size_t)scan_blocks(S) + 1, st)); HIPCHK(d_tot.reserve(1, st));
    const covp::SelCigarLen clen{order, s->store.cigar_off.p};
    scan_offsets(st, clen, S, d_bsum.p, d_tot.p);
    HIPCHK(hipGetLastError());
    u64 n_cig_sel = 0;
    HIPCHK(hipMemcpyAsync(&n_cig_sel, d_tot.p, sizeof n_cig_sel, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(sel.reserve(S, (size_t)n_cig_sel + 1, st, 0, 0, with_mates));
    covp::SelGather G{}; G.order = order; s->store.view(G.src); sel.view(G.dst);
    scan_apply(st, clen, G, S, d_bsum.p);
    HIPCHK(hipGetLastError());
    if (with_mates) {
        hipLaunchKernelGGL(covg::k_group_gather_mates, dim3((S + 255u) / 256u), dim3(256), 0, st, order, S, (const int32_t *)s->store.mtid.p, (const u64 *)s->store.qh1.p, (const u32 *)s->store.qh2.p,
                           sel.mtid.p, sel.qh1.p, sel.qh2.p);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(sel.seal(S, n_cig_sel, st));
    s->store.swap(sel, with_mates);
    return COV_OK;
}

cov_status cov_pair_filter_apply(cov_session *s, const cov_pair_filter *f, uint64_t *n_selected, uint64_t *n_primary) {
    if (!s || !f) return COV_ERR_INVALID_ARG;
    covr::Range rr("pair filter (cov_pair_filter_apply)");
    if (s->adopted || s->ing.active) { s->err = "cov_pair_filter_apply: needs the session's own record store, filled by the device ingest"; return COV_ERR_STATE; }
    if (s->spill.active) { s->err = "cov_pair_filter_apply: part of the sample's records already left the bounded record store"; return COV_ERR_STATE; }
    if (s->store.mates_valid != s->store.n_records) { s->err = "cov_pair_filter_apply: the store holds records without mate columns (cov_ingest_want_mates before every ingest, no cov_push_batch)"; return COV_ERR_STATE; }
    HIPCHK(hipSetDevice(s->cfg.device));
    hipStream_t st = s->stream;
    const u32 R = (u32)s->store.n_records;
    if (n_selected) *n_selected = 0;
    if (n_primary) *n_primary = 0;
    s->finished = false; s->depth_all_valid = false; s->dr.drop();
    if (R == 0) return COV_OK;
    covp::PairCols C{};
    s->store.view_unplaced(C); s->store.view_mates(C);
    covp::PairFilter F; memcpy(&F, f, sizeof F);
    // chunks of whole references (a pair never spans two), about T records each: the table of a chunk stays small enough for the
    // last-level cache, where the scattered atomics of the join are served
    u32 T = 4u << 20;
    { long long v; if (covknob::get("pair_chunk", v) && v >= 1024) T = (u32)std::min<long long>(v, 1ll << 30); }
    const u32 n_chunks = (u32)(((u64)R + T - 1) / T);
    DevBuf<u32> d_cuts, d_partner, d_bsum, d_order, d_cnt;       // d_cnt: [0] members listed by k_pair_collect, [1] table overflow, [2 + c] entries of chunk c with more than two records
    DevBuf<u64> d_w;        // [0] primaries, [1] first error, [2] selected slots, [3] selected CIGAR words
    DevBuf<covp::PairEntry> d_tab;
    struct Rel { DevBuf<u32> &a, &b, &c, &d, &e; DevBuf<u64> &w; DevBuf<covp::PairEntry> &t; ~Rel() { a.release(); b.release(); c.release(); d.release(); e.release(); w.release(); t.release(); } }
        rel{d_cuts, d_partner, d_bsum, d_order, d_cnt, d_w, d_tab};
    HIPCHK(d_cuts.reserve((size_t)n_chunks + 1, st)); HIPCHK(d_w.reserve(4, st)); HIPCHK(d_cnt.reserve((size_t)n_chunks + 2, st));
    if (d_partner.reserve(R, st) != hipSuccess) { (void)hipGetLastError(); s->err = "device pair filter: no device memory for the partner column (handing the file to the CPU reader)"; return COV_ERR_INGEST_FALLBACK; }
    const u64 w_init[4] = {0ull, ~0ull, 0ull, 0ull};
    HIPCHK(hipMemcpyAsync(d_w.p, w_init, sizeof w_init, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_cnt.p, 0, ((size_t)n_chunks + 2) * sizeof(u32), st));
    HIPCHK(hipMemsetAsync(d_partner.p, 0xff, (size_t)R * sizeof(u32), st));
    hipLaunchKernelGGL(covp::k_count_primary, dim3(std::min<u32>((R + 255u) / 256u, 4096u)), dim3(256), 0, st, (const uint16_t *)s->store.flag.p, R, d_w.p);
    hipLaunchKernelGGL(covp::k_pair_cuts, dim3((n_chunks + 1 + 255) / 256), dim3(256), 0, st, (const int32_t *)s->store.tid.p, R, T, n_chunks, d_cuts.p);
    HIPCHK(hipGetLastError());
    std::vector<u32> cuts((size_t)n_chunks + 1);
    HIPCHK(hipMemcpyAsync(cuts.data(), d_cuts.p, cuts.size() * sizeof(u32), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    u32 biggest = 0;
    for (u32 c = 0; c < n_chunks; c++) biggest = std::max(biggest, cuts[c + 1] > cuts[c] ? cuts[c + 1] - cuts[c] : 0u);
    const u64 cap = pkey::table_size(biggest);
    // (the kernels carry the table size as 32 bits: a table of 2^32 entries would read as 0.)  A reference with that many records, or a
    // table that does not fit the device beside the store, goes to the host's pair filter: the store is still untouched here.
    auto too_big = [&](const char *what) {
        (void)hipGetLastError();
        s->err = std::string("device pair filter: ") + what + " (handing the file to the CPU reader)";
        return COV_ERR_INGEST_FALLBACK;
    };
    if (cap > (1ull << 31)) return too_big("more than 2^30 records of one reference");
    if (d_tab.reserve((size_t)cap, st) != hipSuccess) return too_big("the join table of the largest reference does not fit the device's memory");
    auto chunk_table = [&](u32 r0, u32 r1) -> u64 {        // this chunk's table (a prefix of the buffer) built: its size
        const u64 cc = pkey::table_size(r1 - r0);
        (void)hipMemsetAsync(d_tab.p, 0, (size_t)cc * sizeof(covp::PairEntry), st);
        hipLaunchKernelGGL(covp::k_pair_insert, dim3((r1 - r0 + 255u) / 256u), dim3(256), 0, st, C, r0, r1, d_tab.p, (u32)(cc - 1), d_cnt.p);
        return cc;
    };
    for (u32 c = 0; c < n_chunks; c++) {
        const u32 r0 = cuts[c], r1 = cuts[c + 1];
        if (r1 <= r0) continue;
        const u64 cc = chunk_table(r0, r1);
        hipLaunchKernelGGL(covp::k_pair_resolve, dim3((u32)((cc + 255) / 256)), dim3(256), 0, st, C, (const covp::PairEntry *)d_tab.p, (u32)cc, F, d_partner.p, d_cnt.p + 2 + c,
                           d_w.p + 1, (u32)COV_ERR_NM_MISSING, (u32)COV_ERR_NM_BADTYPE);
    }
    HIPCHK(hipGetLastError());
    {   // read names that occur more than twice among the eligible records of a reference: the reference's serial sequence, replayed
        std::vector<u32> hcnt((size_t)n_chunks + 2);
        HIPCHK(hipMemcpyAsync(hcnt.data(), d_cnt.p, hcnt.size() * sizeof(u32), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (hcnt[1]) { s->err = "cov_pair_filter_apply: internal error, hash table overflow"; return COV_ERR_STATE; }
        u32 CAP = 1u << 20;        // listed records of one chunk; knob pair_multi_cap (tests reach the decline without a million records)
        { long long v; if (covknob::get("pair_multi_cap", v)) CAP = (u32)std::min<long long>(std::max<long long>(v, 16), 1ll << 20); }      // a value below 16 is 16
        DevBuf<covp::MultiRec> d_list; DevBuf<uint2> d_pairs;
        struct Rel2 { DevBuf<covp::MultiRec> &a; DevBuf<uint2> &b; ~Rel2() { a.release(); b.release(); } } rel2{d_list, d_pairs};
        for (u32 c = 0; c < n_chunks; c++) {
            if (!hcnt[2 + c]) continue;
            const u32 r0 = cuts[c], r1 = cuts[c + 1];
            HIPCHK(d_list.reserve(CAP, st));
            HIPCHK(hipMemsetAsync(d_cnt.p, 0, sizeof(u32), st));
            const u64 cc = chunk_table(r0, r1);
            hipLaunchKernelGGL(covp::k_pair_collect, dim3((r1 - r0 + 255u) / 256u), dim3(256), 0, st, C, r0, r1, (const covp::PairEntry *)d_tab.p, (u32)(cc - 1), d_list.p, CAP, d_cnt.p);
            HIPCHK(hipGetLastError());
            u32 n_list = 0;
            HIPCHK(hipMemcpyAsync(&n_list, d_cnt.p, sizeof n_list, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            if (n_list > CAP) {
                s->err = "pair filter: more than " + (CAP == 1u << 20 ? std::string("2^20") : std::to_string(CAP)) +
                         " records carry a read name that occurs more than twice among the primary proper-pair records of one reference "
                         "(handing the file to the CPU reader)";
                return COV_ERR_INGEST_FALLBACK;
            }
            std::vector<covp::MultiRec> list(n_list);
            HIPCHK(hipMemcpyAsync(list.data(), d_list.p, (size_t)n_list * sizeof(covp::MultiRec), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            std::sort(list.begin(), list.end(), [](const covp::MultiRec &x, const covp::MultiRec &y) { return x.entry != y.entry ? x.entry < y.entry : x.i < y.i; });
            std::vector<uint2> pairs;
            for (size_t a = 0; a < list.size();) {       // filter.rs:163-187 over one name's records, in file order
                size_t b = a; bool parked = false; u32 first = 0;
                for (; b < list.size() && list[b].entry == list[a].entry; b++) {
                    if (parked) { pairs.push_back(make_uint2(first, list[b].i)); parked = false; }
                    else if (list[b].parks) { parked = true; first = list[b].i; }
                }
                a = b;
            }
            if (!pairs.empty()) {
                HIPCHK(d_pairs.reserve(pairs.size(), st));
                HIPCHK(hipMemcpyAsync(d_pairs.p, pairs.data(), pairs.size() * sizeof(uint2), hipMemcpyHostToDevice, st));
                hipLaunchKernelGGL(covp::k_pair_judge_list, dim3((u32)((pairs.size() + 255) / 256)), dim3(256), 0, st, C, (const uint2 *)d_pairs.p, (u32)pairs.size(), F, d_partner.p,
                                   d_w.p + 1, (u32)COV_ERR_NM_MISSING, (u32)COV_ERR_NM_BADTYPE);
                HIPCHK(hipGetLastError());
                HIPCHK(hipStreamSynchronize(st));          // `pairs` is read by the copy until here
            }
        }
    }
    // ---- the reference's output order: pairs by their second record, first record then second
    HIPCHK(d_bsum.reserve((size_t)scan_blocks(R) + 1, st));
    const covp::PairSlots slots{d_partner.p};
    scan_offsets(st, slots, R, d_bsum.p, d_w.p + 2);
    HIPCHK(hipGetLastError());
    u64 hw[4];
    HIPCHK(hipMemcpyAsync(hw, d_w.p, sizeof hw, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (hw[1] != ~0ull) {
        const u32 code = (u32)(hw[1] & 0xffu);
        s->err = code == (u32)COV_ERR_NM_MISSING ? "Mapping record encountered that does not have an 'NM' auxiliary tag in the SAM/BAM format" : "Unexpected data type of NM aux tag";
        return (cov_status)code;
    }
    const u64 n_sel = hw[2];
    if (n_primary) *n_primary = hw[0];
    if (n_selected) *n_selected = n_sel;
    if (n_sel == 0) { s->store.n_records = 0; s->store.n_cigar = 0; s->store.mates_valid = 0; return COV_OK; }
    const u32 S = (u32)n_sel;
    HIPCHK(d_order.reserve(S, st));
    const covp::PairEmit emit{d_partner.p, d_order.p};
    scan_apply(st, slots, emit, R, d_bsum.p);
    // ---- the selected store: CIGAR offsets by a second scan, whose consumer moves the records
    HIPCHK(hipGetLastError());
    { const cov_status g = gather_store(s, d_order.p, S, false); if (g != COV_OK) return g; }
    s->store.mates_valid = 0;      // the mate columns still describe the unselected store: spent
    return COV_OK;
}

// ---------------------------------------------------------------------------------------------- records grouped by reference (group_kernels.hip.h)
cov_status cov_group_records(cov_session *s, uint64_t *n_moved) {
    if (!s) return COV_ERR_INVALID_ARG;
    covr::Range rr("group records by reference (cov_group_records)");
    if (n_moved) *n_moved = 0;
    if (s->ing.active) { s->err = "cov_group_records: a device ingest is still open (cov_ingest_end first)"; return COV_ERR_STATE; }
    if (s->adopted) { s->err = "cov_group_records: needs the session's own record store, not an adopted device batch (cov_push_batch_device)"; return COV_ERR_STATE; }
    if (s->ing.was_span) { s->err = "cov_group_records: the store holds one tid span of a file (cov_ingest_span), which is cut where a file sorted by reference changes tid"; return COV_ERR_STATE; }
    if (s->spill.active) { s->err = "cov_group_records: a sample that is not sorted by reference must fit the record store (part of it already left the bounded store, judged in file order)"; return COV_ERR_STATE; }
    HIPCHK(hipSetDevice(s->cfg.device));
    timing_events(s);
    hipStream_t st = s->stream;
    const u32 R = (u32)s->store.n_records, nT = s->n_targets;
    for (float &m : s->grp_ms) m = 0.f;
    s->grp_launches = 0;
    if (R < 2) return COV_OK;
    const bool mates = s->store.mates_valid == s->store.n_records && s->store.mates_valid != 0;
    hipEvent_t *ev = s->ev[COV_K_GROUP];      // [0] begin, [1] end; the split: events of its own (a few per sample)
    hipEvent_t ev_mid[2] = {nullptr, nullptr};
    DevBuf<u32> d_flag, d_hist, d_key[2], d_idx[2]; DevBuf<u64> d_cnt;
    struct Rel { std::function<void()> f; ~Rel() { f(); } } rel{[&] {
        d_flag.release(); d_hist.release(); d_key[0].release(); d_key[1].release(); d_idx[0].release(); d_idx[1].release(); d_cnt.release();
        for (hipEvent_t e : ev_mid) if (e) (void)hipEventDestroy(e); }};
    for (hipEvent_t &e : ev_mid) HIPCHK(hipEventCreate(&e));
    auto elapsed = [&](hipEvent_t a, hipEvent_t b) { float ms = 0.f; (void)hipEventElapsedTime(&ms, a, b); return ms; };

    // ---- keys never decrease: the store is grouped already
    HIPCHK(d_flag.reserve(1, st));
    HIPCHK(hipMemsetAsync(d_flag.p, 0, sizeof(u32), st));
    HIPCHK(hipEventRecord(ev[0], st));
    hipLaunchKernelGGL(covg::k_group_check, dim3(std::min<u32>((R + 255u) / 256u, 8192u)), dim3(256), 0, st, (const int32_t *)s->store.tid.p, R, nT, d_flag.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev_mid[0], st));
    s->grp_launches++;
    u32 decreasing = 0;
    HIPCHK(hipMemcpyAsync(&decreasing, d_flag.p, sizeof decreasing, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    s->grp_ms[1] = elapsed(ev[0], ev_mid[0]);
    if (!decreasing) { s->grp_ms[0] = s->grp_ms[1]; return COV_OK; }

    // ---- stable LSD radix sort of the record indices
    const u32 P = grpk::n_passes(nT), n_wg = grpk::n_tiles(R), n_hist = n_wg * grpk::RADIX;
    DevBuf<u32> d_bsum;
    struct Rel1 { DevBuf<u32> &a; ~Rel1() { a.release(); } } rel1{d_bsum};
    HIPCHK(d_hist.reserve(n_hist, st)); HIPCHK(d_bsum.reserve((size_t)scan_blocks(n_hist) + 1, st)); HIPCHK(d_cnt.reserve(2, st));
    HIPCHK(d_idx[0].reserve(R, st));
    if (P > 1) { HIPCHK(d_key[0].reserve(R, st)); HIPCHK(d_idx[1].reserve(R, st)); }
    if (P > 2) HIPCHK(d_key[1].reserve(R, st));
    HIPCHK(hipMemsetAsync(d_cnt.p, 0, 2 * sizeof(u64), st));
    const int32_t *tid = s->store.tid.p;
    for (u32 p = 0; p < P; p++) {
        const bool first = p == 0, last = p + 1 == P;
        const u32 *key_in = first ? nullptr : d_key[(p - 1) & 1u].p, *idx_in = first ? nullptr : d_idx[(p - 1) & 1u].p;
        u32 *key_out = last ? nullptr : d_key[p & 1u].p, *idx_out = d_idx[p & 1u].p;
        if (first) hipLaunchKernelGGL(covg::k_group_hist<true>, dim3(n_wg), dim3(256), 0, st, tid, key_in, R, nT, p, d_hist.p, n_wg);
        else hipLaunchKernelGGL(covg::k_group_hist<false>, dim3(n_wg), dim3(256), 0, st, tid, key_in, R, nT, p, d_hist.p, n_wg);
        const covg::HistVal hv{d_hist.p}; const covg::HistPut hp{d_hist.p};      // in place: a thread of the scan writes the items it read itself
        scan_offsets(st, hv, n_hist, d_bsum.p, d_cnt.p + 1);
        scan_apply(st, hv, hp, n_hist, d_bsum.p);
        const dim3 g(n_wg), b(256);
        if (first && last) hipLaunchKernelGGL((covg::k_group_scatter<true, true>), g, b, 0, st, tid, key_in, idx_in, key_out, idx_out, R, nT, p, (const u32 *)d_hist.p, n_wg);
        else if (first) hipLaunchKernelGGL((covg::k_group_scatter<true, false>), g, b, 0, st, tid, key_in, idx_in, key_out, idx_out, R, nT, p, (const u32 *)d_hist.p, n_wg);
        else if (last) hipLaunchKernelGGL((covg::k_group_scatter<false, true>), g, b, 0, st, tid, key_in, idx_in, key_out, idx_out, R, nT, p, (const u32 *)d_hist.p, n_wg);
        else hipLaunchKernelGGL((covg::k_group_scatter<false, false>), g, b, 0, st, tid, key_in, idx_in, key_out, idx_out, R, nT, p, (const u32 *)d_hist.p, n_wg);
        HIPCHK(hipGetLastError());
        s->grp_launches += 5;
    }
    const u32 *order = d_idx[(P - 1) & 1u].p;
    hipLaunchKernelGGL(covg::k_group_moved, dim3(std::min<u32>((R + 255u) / 256u, 4096u)), dim3(256), 0, st, order, R, d_cnt.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev_mid[1], st));
    s->grp_launches++;
    // ---- ONE gather of the store (and of the mate columns, which stay valid for cov_pair_filter_apply)
    { const cov_status g = gather_store(s, order, R, mates); if (g != COV_OK) return g; }
    HIPCHK(hipEventRecord(ev[1], st));
    s->grp_launches += mates ? 4 : 3;
    u64 moved = 0;
    HIPCHK(hipMemcpyAsync(&moved, d_cnt.p, sizeof moved, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    s->grp_ms[0] = elapsed(ev[0], ev[1]); s->grp_ms[2] = elapsed(ev_mid[0], ev_mid[1]); s->grp_ms[3] = elapsed(ev_mid[1], ev[1]);
    if (cov_timing_on())
        fprintf(stderr, "[covermhip] group: %u records, %u passes, %llu moved; order check %.3f ms, sort %.3f ms, gather %.3f ms\n", R, P, (unsigned long long)moved, s->grp_ms[1], s->grp_ms[2],
                s->grp_ms[3]);
    if (n_moved) *n_moved = moved;
    s->finished = false; s->depth_all_valid = false; s->dr.drop(); s->ev_fresh = -1;
    return COV_OK;
}

// Test hook: the owned record store copied back to host arrays (cov_batch of writable pointers sized by the caller:
// n_records entries, n_records + 1 cigar offsets, n_cigar words; *n_cigar receives the word count when words are not wanted).
cov_status cov_copy_records(cov_session *s, const cov_batch *host, uint64_t *n_records, uint64_t *n_cigar) {
    if (!s || s->adopted) return COV_ERR_STATE;
    if (s->spill.active) { s->err = "cov_copy_records: part of the sample's records already left the bounded record store"; return COV_ERR_STATE; }
    HIPCHK(hipSetDevice(s->cfg.device));
    if (n_records) *n_records = s->store.n_records;
    if (n_cigar) *n_cigar = s->store.n_cigar;
    if (!host) return COV_OK;
    HIPCHK(s->store.copy_out(*host, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return COV_OK;
}

// Test hook: what an ingest with cov_ingest_want_mates kept per record (the mate's reference, the 96-bit read-name hash), n_records each.
cov_status cov_copy_mates(cov_session *s, int32_t *mtid, uint64_t *qh1, uint32_t *qh2) {
    if (!s || s->adopted || !mtid || !qh1 || !qh2) return COV_ERR_STATE;
    if (s->spill.active) { s->err = "cov_copy_mates: part of the sample's records already left the bounded record store"; return COV_ERR_STATE; }
    const uint64_t n = s->store.n_records;
    if (!s->want_mates || (n && !s->store.mtid.p)) { s->err = "cov_copy_mates: the records were not ingested with cov_ingest_want_mates"; return COV_ERR_STATE; }
    HIPCHK(hipSetDevice(s->cfg.device));
    HIPCHK(s->store.copy_mates_out(mtid, qh1, qh2, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return COV_OK;
}

// Test hook, the counterpart of cov_copy_mates: the mate columns of a store that has them, overwritten (n_records each).  Read names cannot
// be made to collide in 64 or 96 bits of their hash; keys written here can.
cov_status cov_set_mates(cov_session *s, const int32_t *mtid, const uint64_t *qh1, const uint32_t *qh2) {
    if (!s || s->adopted || !mtid || !qh1 || !qh2) return COV_ERR_STATE;
    if (s->spill.active) { s->err = "cov_set_mates: part of the sample's records already left the bounded record store"; return COV_ERR_STATE; }
    const uint64_t n = s->store.n_records;
    if (!s->want_mates || (n && !s->store.mtid.p)) { s->err = "cov_set_mates: the records were not ingested with cov_ingest_want_mates"; return COV_ERR_STATE; }
    if (s->store.mates_valid != n) { s->err = "cov_set_mates: the store holds records without mate columns"; return COV_ERR_STATE; }
    HIPCHK(hipSetDevice(s->cfg.device));
    HIPCHK(s->store.copy_mates_in(mtid, qh1, qh2, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return COV_OK;
}

cov_status cov_ingest_release(cov_session *s) {
    if (!s) return COV_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(s->cfg.device));
    HIPCHK(hipStreamSynchronize(s->stream));
    if (s->ing.aux) HIPCHK(hipStreamSynchronize(s->ing.aux));
    if (s->ing.parse) HIPCHK(hipStreamSynchronize(s->ing.parse));
    if (s->ing.ext) HIPCHK(hipStreamSynchronize(s->ing.ext));
    ingest_free_buffers(s);
    return COV_OK;
}

// Test hook: the inflated stream of the last ingest (bytes [offset, offset + n) copied to `out`) — kept only when the whole file
// was a single window.
cov_status cov_ingest_copy_inflated(cov_session *s, uint64_t offset, uint64_t n, void *out) {
    if (!s || offset + n > s->ing.feed.infl || (n && !out)) return COV_ERR_INVALID_ARG;
    if (s->ing.batch != 1) { s->err = "cov_ingest_copy_inflated: the file was parsed in several windows, the stream is gone"; return COV_ERR_STATE; }
    HIPCHK(hipSetDevice(s->cfg.device));
    HIPCHK(hipMemcpyAsync(out, s->ing.g_win[0].p + s->ing.K.carry + offset, n, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return COV_OK;
}

cov_status cov_fetch_hist(cov_session *s, uint64_t *hist) {
    if (!s || !s->finished || !(s->cfg.want & COV_WANT_HIST)) return COV_ERR_STATE;
    if (s->merged_valid) {      // a finish that merged spilled contigs (bounded record store): the bins were re-based on the host
        s->hist_fetch_seen = true;
        if (s->merged_hist.empty()) return COV_OK;
        if (!hist) return COV_ERR_INVALID_ARG;
        memcpy(hist, s->merged_hist.data(), s->merged_hist.size() * 8);
        return COV_OK;
    }
    return fetch_chunk_hist(s, hist);
}

// the compact histogram of the last pass over the store
static cov_status fetch_chunk_hist(cov_session *s, uint64_t *hist) {
    if (!s || !s->finished || !(s->cfg.want & COV_WANT_HIST)) return COV_ERR_STATE;
    HIPCHK(hipSetDevice(s->cfg.device));
    const uint64_t total = s->last_chist_total;
    s->hist_fetch_seen = true;
    if (total == 0) return COV_OK;
    if (!hist) return COV_ERR_INVALID_ARG;
    if (!s->hist_compacted) {      // the finish left the bins in the arena (its estimators were evaluated on the device): lay them out and compact them now
        HIPCHK(s->d_chist.reserve(total, s->stream));
        HIPCHK(s->d_hist_top.reserve((s->n_targets + 1023u) / 1024u, s->stream));
        launch_hist_compact(s, device_mask(s), (u64)s->cfg.contig_end_exclusion);
        HIPCHK(hipGetLastError());
        s->hist_prefetched = 0; s->hist_compacted = true;
    }
    const u64 have = std::min<u64>(total, s->hist_prefetched);      // arrived with cov_finish's own synchronisation
    if (have) memcpy(hist, s->h_chist, (size_t)have * 8);
    if (have < total) {
        HIPCHK(hipMemcpyAsync(hist + have, s->d_chist.p + have, (size_t)(total - have) * 8, hipMemcpyDeviceToHost, s->stream));
        HIPCHK(hipStreamSynchronize(s->stream));
    }
    return COV_OK;
}

cov_status cov_copy_depth(cov_session *s, uint32_t tid, int32_t *depth_out) {
    if (!s || !s->finished) return COV_ERR_STATE;
    if (s->spill.active) { s->err = "cov_copy_depth: part of the sample's records already left the bounded record store"; return COV_ERR_STATE; }
    if (tid >= s->n_targets || !depth_out) return COV_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(s->cfg.device));
    const u32 L = s->h_tlen[tid];
    if (L == 0) return COV_OK;
    HIPCHK(s->d_depth.reserve(L, s->stream));
    HIPCHK(hipMemsetAsync(s->d_depth.p, 0, (size_t)L * 4, s->stream));
    PileupArgs a = pileup_args(s);
    // depth materialisation must not disturb the accumulated statistics: run against a scratch copy
    DevBuf<DevContig> &scratch = s->d_ctg_scratch;   // kept for the next call: per-gene coverage asks for every contig
    HIPCHK(scratch.reserve(s->n_targets, s->stream));
    HIPCHK(hipMemcpyAsync(scratch.p, s->d_ctg.p, (size_t)s->n_targets * sizeof(DevContig), hipMemcpyDeviceToDevice, s->stream));
    a.ctg = scratch.p;
    a.depth_out = s->d_depth.p;
    a.tile_base = s->h_tile_first[tid];
    const u32 grid = s->h_tile_first[tid + 1] - s->h_tile_first[tid];
    launch_any_pileup<false, true>(s, a, grid);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(depth_out, s->d_depth.p, (size_t)L * 4, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return COV_OK;
}

cov_status cov_interval_stats_compute(cov_session *s, const cov_interval *iv, uint64_t n, uint64_t excl, int want_hist,
                                      cov_interval_stats *out, uint64_t *hist_total) {
    if (!s || !s->finished) return COV_ERR_STATE;
    if (s->spill.active) { s->err = "cov_interval_stats_compute: part of the sample's records already left the bounded record store (per-gene coverage needs them all: raise COVERM_STORE_CAP_*)"; return COV_ERR_STATE; }
    if ((n && (!iv || !out))) return COV_ERR_INVALID_ARG;
    if (hist_total) *hist_total = 0;
    s->ivhist_total = 0;
    if (n == 0) return COV_OK;
    for (uint64_t i = 0; i < n; i++)
        if (iv[i].tid >= s->n_targets || iv[i].start >= iv[i].end || iv[i].end > s->h_tlen[iv[i].tid]) {
            s->err = "interval outside its target"; return COV_ERR_INVALID_ARG;
        }
    HIPCHK(hipSetDevice(s->cfg.device));
    hipStream_t st = s->stream;
    if (!s->depth_all_valid) {   // depth of every target, once per finish
        std::vector<u64> off((size_t)s->n_targets + 1, 0);
        for (u32 c = 0; c < s->n_targets; c++) off[c + 1] = off[c] + s->h_tlen[c];
        HIPCHK(s->d_depth_off.reserve(off.size(), st));
        HIPCHK(hipMemcpyAsync(s->d_depth_off.p, off.data(), off.size() * 8, hipMemcpyHostToDevice, st));
        HIPCHK(s->d_depth_all.reserve(std::max<size_t>(1, off.back()), st));
        HIPCHK(hipMemsetAsync(s->d_depth_all.p, 0, (size_t)off.back() * 4, st));
        if (s->store.n_records && s->n_tiles) {
            PileupArgs a = pileup_args(s);
            HIPCHK(s->d_ctg_scratch.reserve(s->n_targets, st));   // the accumulated statistics must stay as they are
            HIPCHK(hipMemcpyAsync(s->d_ctg_scratch.p, s->d_ctg.p, (size_t)s->n_targets * sizeof(DevContig), hipMemcpyDeviceToDevice, st));
            a.ctg = s->d_ctg_scratch.p;
            a.depth_out = s->d_depth_all.p; a.depth_off = s->d_depth_off.p; a.tile_base = 0;
            launch_any_pileup<false, true>(s, a, s->n_tiles);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipStreamSynchronize(st));   // `off` is read by the copy above
        s->depth_all_valid = true;
    }
    static_assert(sizeof(DevInterval) == sizeof(cov_interval) && sizeof(DevIntervalStats) == sizeof(cov_interval_stats), "ABI structs mirror the device ones");
    HIPCHK(s->d_iv.reserve(n, st)); HIPCHK(s->d_ivst.reserve(n, st));
    HIPCHK(hipMemcpyAsync(s->d_iv.p, iv, n * sizeof(cov_interval), hipMemcpyHostToDevice, st));
    const u32 grid = (u32)std::max<uint64_t>(1, std::min<uint64_t>((n + 3) / 4, (uint64_t)s->n_cus * 16));
    hipLaunchKernelGGL(k_interval_stats, dim3(grid), dim3(256), 0, st, s->d_depth_all.p, s->d_depth_off.p, s->d_iv.p, n, excl, s->d_ivst.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, s->d_ivst.p, n * sizeof(cov_interval_stats), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    uint64_t tot = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (want_hist) { out[i].hist_off = tot; tot += out[i].hist_len; }
        else out[i].hist_len = 0;
    }
    if (want_hist && tot) {
        HIPCHK(s->d_ivhist.reserve(tot, st));
        HIPCHK(hipMemsetAsync(s->d_ivhist.p, 0, tot * 8, st));
        HIPCHK(hipMemcpyAsync(s->d_ivst.p, out, n * sizeof(cov_interval_stats), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_interval_hist, dim3(grid), dim3(256), 0, st, s->d_depth_all.p, s->d_depth_off.p, s->d_iv.p, n, excl, s->d_ivst.p,
                           s->d_ivhist.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));
    }
    s->ivhist_total = want_hist ? tot : 0;
    if (hist_total) *hist_total = s->ivhist_total;
    return COV_OK;
}

// ---------------------------------------------------------------------------------------------- per-interval read aggregates (gene_kernels.hip.h)
// What covh_gene_coverage's record pass computes from the records on the host, from the store itself: 32 bytes per interval come back.
cov_status cov_interval_reads_compute(cov_session *s, const cov_interval *iv, uint64_t n, int want_identity, cov_interval_reads *out,
                                      uint64_t *mapped_total, int *sorted_by_start) {
    if (!s) return COV_ERR_INVALID_ARG;
    if (s->ing.active) { s->err = "cov_interval_reads_compute: a device ingest is still open (cov_ingest_end first)"; return COV_ERR_STATE; }
    if (s->spill.active) { s->err = "cov_interval_reads_compute: part of the sample's records already left the bounded record store (per-gene coverage needs them all: raise COVERM_STORE_CAP_*)"; return COV_ERR_STATE; }
    if ((n && (!iv || !out)) || !sorted_by_start) return COV_ERR_INVALID_ARG;
    for (uint64_t i = 0; i < n; i++)
        if (iv[i].tid >= s->n_targets || iv[i].start >= iv[i].end || iv[i].end > s->h_tlen[iv[i].tid]) { s->err = "interval outside its target"; return COV_ERR_INVALID_ARG; }
    covr::Range rr("per-interval read aggregates (cov_interval_reads_compute)");
    *sorted_by_start = 0;
    if (mapped_total) *mapped_total = 0;
    s->gene_ms = 0.f; s->gene_launches = 0;
    HIPCHK(hipSetDevice(s->cfg.device));
    timing_events(s);
    hipStream_t st = s->stream;
    const Records r = records_of(s);
    const u32 R = r.n, nb = (R + covgn::TILE - 1) / covgn::TILE;
    const bool ident = want_identity != 0;
    // the contigs with intervals, ascending, and each interval's contig by its number among them (where its checkpoints lie)
    std::vector<u32> tids(n);
    for (uint64_t i = 0; i < n; i++) tids[i] = iv[i].tid;
    std::sort(tids.begin(), tids.end());
    tids.erase(std::unique(tids.begin(), tids.end()), tids.end());
    std::vector<gnrc::Interval> hiv(n);
    for (uint64_t i = 0; i < n; i++) {
        hiv[i].tid = iv[i].tid; hiv[i].start = iv[i].start; hiv[i].end = iv[i].end;
        hiv[i].pad = (u32)(std::lower_bound(tids.begin(), tids.end(), iv[i].tid) - tids.begin());
    }
    const u32 nC = (u32)tids.size();
    HIPCHK(s->gr_code.reserve(std::max<size_t>(R, 1), st)); HIPCHK(s->gr_mism.reserve(std::max<size_t>(R, 1), st));
    HIPCHK(s->gr_bcnt.reserve((size_t)nb + 1, st)); HIPCHK(s->gr_bmism.reserve((size_t)nb + 1, st));
    HIPCHK(s->gr_ttid.reserve(std::max<size_t>(R, 1), st)); HIPCHK(s->gr_tpos.reserve(std::max<size_t>(R, 1), st)); HIPCHK(s->gr_trec.reserve(std::max<size_t>(R, 1), st));
    HIPCHK(s->gr_pprim.reserve((size_t)R + 1, st)); HIPCHK(s->gr_pmism.reserve((size_t)R + 1, st)); HIPCHK(s->gr_glob.reserve(covgn::G_COUNT, st));
    if (ident) { HIPCHK(s->gr_ident.reserve(std::max<size_t>(R, 1), st)); HIPCHK(s->gr_tident.reserve(std::max<size_t>(R, 1), st)); HIPCHK(s->gr_ck.reserve((size_t)gnrc::ck_slots(R, nC), st)); }
    HIPCHK(s->gr_iv.reserve(std::max<size_t>(n, 1), st)); HIPCHK(s->gr_out.reserve(std::max<size_t>(n, 1), st)); HIPCHK(s->gr_bounds.reserve(std::max<size_t>(n, 1), st));
    HIPCHK(s->gr_tids.reserve(std::max<size_t>(nC, 1), st));
    covgn::Work w{};
    w.code = s->gr_code.p; w.mism = s->gr_mism.p; w.ident = ident ? s->gr_ident.p : nullptr; w.b_cnt = s->gr_bcnt.p; w.b_mism = s->gr_bmism.p;
    w.t_tid = s->gr_ttid.p; w.t_pos = s->gr_tpos.p; w.t_rec = s->gr_trec.p; w.pprim = s->gr_pprim.p; w.pmism = s->gr_pmism.p;
    w.t_ident = ident ? s->gr_tident.p : nullptr; w.glob = s->gr_glob.p;
    const FilterCfg fc = filter_of(s->cfg);
    gnrc::Filter f{};
    f.include_improper_pairs = fc.include_improper_pairs; f.include_supplementary = fc.include_supplementary; f.include_secondary = fc.include_secondary;
    f.filter_single = fc.filter_single; f.min_mapq = fc.min_mapq; f.min_aligned_length = fc.min_aligned_length;
    f.min_percent_identity = fc.min_percent_identity; f.min_aligned_percent = fc.min_aligned_percent;
    const u64 glob0[covgn::G_COUNT] = {gnrc::NO_VERDICT, 0, 0, 0};
    u64 glob[covgn::G_COUNT];
    hipEvent_t *ev = s->ev[COV_K_GENE_READS];      // events of its own: the call is not part of a finish
    HIPCHK(hipMemcpyAsync(s->gr_glob.p, glob0, sizeof glob0, hipMemcpyHostToDevice, st));
    if (n) HIPCHK(hipMemcpyAsync(s->gr_iv.p, hiv.data(), n * sizeof(gnrc::Interval), hipMemcpyHostToDevice, st));
    if (nC) HIPCHK(hipMemcpyAsync(s->gr_tids.p, tids.data(), (size_t)nC * sizeof(u32), hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(ev[0], st));
    if (nb) { hipLaunchKernelGGL(covgn::k_gene_classify, dim3(nb), dim3(256), 0, st, r, f, w); s->gene_launches++; }
    hipLaunchKernelGGL(covgn::k_gene_offsets, dim3(1), dim3(1024), 0, st, w, nb);
    if (nb) { hipLaunchKernelGGL(covgn::k_gene_scatter, dim3(nb), dim3(256), 0, st, r, w); s->gene_launches++; }
    hipLaunchKernelGGL(covgn::k_gene_order, dim3(std::max(1u, std::min(nb, (u32)s->n_cus * 8u))), dim3(256), 0, st, w, s->n_targets);
    s->gene_launches += 2;
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev[1], st));
    HIPCHK(hipMemcpyAsync(glob, s->gr_glob.p, sizeof glob, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, ev[0], ev[1]);
    s->gene_ms = ms; s->ev_fresh = -1;
    if (glob[covgn::G_VERDICT] != gnrc::NO_VERDICT) {      // the reference's panic at the first offending record in file order
        switch ((u32)(glob[covgn::G_VERDICT] & 3u)) {
        case gnrc::RULE_NM_MISSING: s->err = "Mapping record encountered that does not have an 'NM' auxiliary tag in the SAM/BAM format"; return COV_ERR_NM_MISSING;
        case gnrc::RULE_NM_BADTYPE: s->err = "Unexpected data type of NM aux tag"; return COV_ERR_NM_BADTYPE;
        case gnrc::RULE_UNSORTED: s->err = "BAM file appears to be unsorted. Input BAM files must be sorted by reference (i.e. by samtools sort)"; return COV_ERR_UNSORTED;
        default: s->err = "record refers to a reference id outside the header (Corrupt BAM file?)"; return COV_ERR_BAD_TID;
        }
    }
    if (mapped_total) *mapped_total = glob[covgn::G_MAPPED];
    if (glob[covgn::G_UNSORTED]) return COV_OK;      // lower_bound over unsorted starts is the host loop's own probe sequence: its path
    *sorted_by_start = 1;
    if (n == 0) return COV_OK;
    HIPCHK(hipEventRecord(ev[0], st));
    hipLaunchKernelGGL(covgn::k_gene_bounds, dim3((u32)std::min<uint64_t>((n + 255) / 256, (uint64_t)s->n_cus * 8)), dim3(256), 0, st, w, (const gnrc::Interval *)s->gr_iv.p, (u64)n, s->gr_out.p, s->gr_bounds.p);
    s->gene_launches++;
    if (ident) {
        if (n >= 0x7fffffffull) { s->err = "cov_interval_reads_compute: more than 2^31 intervals"; return COV_ERR_INVALID_ARG; }
        hipLaunchKernelGGL(covgn::k_gene_ckpt, dim3(nC), dim3(64), 0, st, w, (const u32 *)s->gr_tids.p, nC, s->gr_ck.p);
        hipLaunchKernelGGL(covgn::k_gene_ident, dim3((u32)n), dim3(64), 0, st, w, (const covgn::Bounds *)s->gr_bounds.p, (u64)n, (const double *)s->gr_ck.p, s->gr_out.p);
        s->gene_launches += 2;
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev[1], st));
    HIPCHK(hipMemcpyAsync(out, s->gr_out.p, n * sizeof(cov_interval_reads), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    (void)hipEventElapsedTime(&ms, ev[0], ev[1]);
    s->gene_ms += ms;
    if (cov_timing_on())
        fprintf(stderr, "[covermhip] interval reads: %u records, %llu taken, %llu intervals on %u contigs, identity %s; %u launches, %.3f ms\n", R,
                (unsigned long long)glob[covgn::G_TAKEN], (unsigned long long)n, nC, ident ? "on" : "off", s->gene_launches, s->gene_ms);
    return COV_OK;
}

// ---------------------------------------------------------------------------------------------- depth runs (depth_kernels.hip.h)
// One chunk of whole targets: the arena filled by the pileup against the scratch copy of the contig block, then marks, the rank scan over
// the start mask, count / scan / emit over the arena's words.  The one host wait in the middle reads the run count the emit's buffer needs.
//
// depth_arena_stage is what cov_depth_runs_compute, cov_depth_bins_compute and cov_depth_regions_compute share: the chunk's plan and layout, the buffers, the woff
// upload, the zero fill, k_depth_marks, the pileup against the scratch copy of the contig block (ev[0] .. ev[1]) and the rank scan.
struct DepthChunk { u32 t1, nT, words, mw; };
// Behind its refusal, which touches nothing, the arena is the caller's: what the other call left in it is dropped there, not earlier.
static cov_status depth_arena_stage(cov_session *s, const char *who, int party, uint32_t tid_lo, uint32_t tid_hi, hipEvent_t *ev, DepthChunk &c) {
    cov_session::DepthRuns &D = s->dr;
    hipStream_t st = s->stream;
    const u32 t1 = dprc::plan_chunk(s->h_tlen.data(), tid_lo, tid_hi, D.chunk_bases), nT = t1 - tid_lo;
    D.h_woff.resize((size_t)nT + 1);
    const u64 words64 = [&] { u64 w = 0; for (u32 k = 0; k < nT; k++) w += dprc::words_of(s->h_tlen[tid_lo + k]); return w; }();
    // (the scan's item indices and block sums are u32: a chunk stays at or below 2^32 arena entries, which one target always does)
    if (words64 > (1ull << 30)) { s->err = std::string(who) + ": a chunk of more than 2^32 arena entries (COVERM_KNOBS depth_chunk_bases)"; return COV_ERR_INVALID_ARG; }
    D.take_arena(party);      // the arena holds one chunk
    const u32 words = dprc::layout(s->h_tlen.data() + tid_lo, nT, D.h_woff.data()), mw = (words + 31u) >> 5;
    HIPCHK(D.arena.reserve(4ull * words, st)); HIPCHK(D.woff.reserve((size_t)nT + 1, st)); HIPCHK(D.mask.reserve(mw, st)); HIPCHK(D.rank.reserve(mw, st));
    HIPCHK(D.sums.reserve((size_t)scan_blocks(std::max(words, mw)) + 1, st)); HIPCHK(D.doff.reserve((size_t)s->n_targets + 1, st));
    HIPCHK(D.total.reserve(2, st));
    // ---- the arena: zero, then the pileup of the chunk's tiles (a tile without a record is skipped by the kernel: its depth is the zero fill)
    HIPCHK(hipMemcpyAsync(D.woff.p, D.h_woff.data(), ((size_t)nT + 1) * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(D.mask.p, 0, (size_t)mw * 4, st));
    HIPCHK(hipEventRecord(ev[0], st));
    HIPCHK(hipMemsetAsync(D.arena.p, 0, 16ull * words, st));
    hipLaunchKernelGGL(covdr::k_depth_marks, dim3((nT + 255u) / 256u), dim3(256), 0, st, D.arena.p, (const u32 *)D.woff.p, (const u32 *)s->d_tlen.p + tid_lo, nT, D.mask.p,
                       D.doff.p + tid_lo);
    const u32 tile0 = s->h_tile_first[tid_lo], n_tiles = s->h_tile_first[t1] - tile0;
    if (s->store.n_records && n_tiles) {
        PileupArgs a = pileup_args(s);
        HIPCHK(s->d_ctg_scratch.reserve(s->n_targets, st));   // the accumulated statistics must stay as they are
        HIPCHK(hipMemcpyAsync(s->d_ctg_scratch.p, s->d_ctg.p, (size_t)s->n_targets * sizeof(DevContig), hipMemcpyDeviceToDevice, st));
        a.ctg = s->d_ctg_scratch.p;
        a.depth_out = D.arena.p; a.depth_off = D.doff.p; a.tile_base = tile0;
        launch_any_pileup<false, true>(s, a, n_tiles);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev[1], st));
    // ---- the rank of every mask word: the shared scan over the start mask
    const covdr::RankCount rc{D.mask.p};
    const covdr::RankSink rs{D.rank.p};
    scan_offsets(st, rc, mw, D.sums.p, D.total.p + 1);
    scan_apply(st, rc, rs, mw, D.sums.p);
    c.t1 = t1; c.nT = nT; c.words = words; c.mw = mw;
    return COV_OK;
}

// `view`: dprc::Identity (cov_depth_runs_compute: runs of equal depth) or dclc::ClassView (cov_depth_class_runs_compute: runs of equal depth
// class); the chunk, the launches and what the fetch finds are the same.
extern "C++" template <class View>
static cov_status depth_runs_compute(cov_session *s, const char *who, const View &view, uint32_t tid_lo, uint32_t tid_hi, uint32_t *tid_next, uint64_t *n_runs) {
    if (s->ing.active) { s->err = std::string(who) + ": a device ingest is still open (cov_ingest_end first)"; return COV_ERR_STATE; }
    if (!s->finished) { s->err = std::string(who) + ": needs a cov_finish over the records"; return COV_ERR_STATE; }
    if (s->spill.active) { s->err = std::string(who) + ": part of the sample's records already left the bounded record store"; return COV_ERR_STATE; }
    if (!tid_next || !n_runs || tid_lo >= tid_hi || tid_hi > s->n_targets) return COV_ERR_INVALID_ARG;
    covr::Range rr(std::is_same<View, dprc::Identity>::value ? "depth runs of one chunk (cov_depth_runs_compute)" : "depth class runs of one chunk (cov_depth_class_runs_compute)");
    cov_session::DepthRuns &D = s->dr;
    HIPCHK(hipSetDevice(s->cfg.device));
    timing_events(s);
    hipStream_t st = s->stream;
    hipEvent_t *ev = s->ev[COV_K_DEPTH_RUNS];      // events of its own: the call is not part of a finish; ev_mid closes the run kernels in front of the host's wait
    if (!D.ev_mid) HIPCHK(hipEventCreate(&D.ev_mid));
    // ---- the arena and scan #1 (the rank of every mask word)
    DepthChunk ck;
    if (const cov_status rc = depth_arena_stage(s, who, cov_session::DepthRuns::RUNS, tid_lo, tid_hi, ev, ck)) return rc;
    const u32 t1 = ck.t1, nT = ck.nT, words = ck.words;
    HIPCHK(D.run_off.reserve((size_t)nT + 1, st));
    // ---- scan #2, first half: the words' run starts counted, the block offsets and the total
    const covdr::WordCountT<View> wc{view, D.arena.p, D.mask.p};
    scan_offsets(st, wc, words, D.sums.p, D.total.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(D.ev_mid, st));
    u64 total = 0;
    HIPCHK(hipMemcpyAsync(&total, D.total.p, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (total > 0xffffffffull) { s->err = std::string(who) + ": more than 2^32 runs in one chunk"; return COV_ERR_STATE; }      // (at most one run per entry: only a chunk of exactly 2^32 entries, every one a run, gets here)
    HIPCHK(D.runs.reserve(std::max<u64>(total, 1), st));
    // ---- scan #2, second half: every word's runs written at its exclusive prefix, a target's first word leaves its run offset
    const covdr::WordEmitT<View> we{view, D.arena.p, D.mask.p, D.rank.p, D.woff.p, D.runs.p, D.run_off.p};
    float ms_arena = 0.f, ms_a = 0.f, ms_b = 0.f;
    (void)hipEventElapsedTime(&ms_arena, ev[0], ev[1]);
    (void)hipEventElapsedTime(&ms_a, ev[1], D.ev_mid);
    HIPCHK(hipEventRecord(ev[0], st));
    scan_apply(st, wc, we, words, D.sums.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev[1], st));
    HIPCHK(hipStreamSynchronize(st));
    (void)hipEventElapsedTime(&ms_b, ev[0], ev[1]);
    s->ev_fresh = -1;
    D.arena_ms = ms_arena; D.runs_ms = ms_a + ms_b; D.launches = 7;
    D.lo = tid_lo; D.next = t1; D.n_runs = total; D.arena_bases = 4ull * words; D.valid = true;
    *tid_next = t1; *n_runs = total;
    if (cov_timing_on())
        fprintf(stderr, "[covermhip] %s: targets [%u, %u), %llu arena entries, %llu runs; arena %.3f ms, run kernels %.3f ms\n",
                std::is_same<View, dprc::Identity>::value ? "depth runs" : "depth class runs", tid_lo, t1, (unsigned long long)D.arena_bases, (unsigned long long)total,
                D.arena_ms, D.runs_ms);
    return COV_OK;
}

cov_status cov_depth_runs_compute(cov_session *s, uint32_t tid_lo, uint32_t tid_hi, uint32_t *tid_next, uint64_t *n_runs) {
    if (!s) return COV_ERR_INVALID_ARG;
    return depth_runs_compute(s, "cov_depth_runs_compute", dprc::Identity{}, tid_lo, tid_hi, tid_next, n_runs);
}

// The cut list of the quantised runs and the thresholds of the regions: one validator (csrc/depth_class_core.h), the first offending index named.
static cov_status depth_cuts_check(cov_session *s, const char *who, const int32_t *cuts, uint32_t n) {
    if (n && !cuts) return COV_ERR_INVALID_ARG;
    u32 at = 0;
    if (const char *what = dclc::validate(cuts, n, &at)) { s->err = std::string(who) + ": value " + std::to_string(at) + ": " + what; return COV_ERR_INVALID_ARG; }
    return COV_OK;
}

cov_status cov_depth_class_runs_compute(cov_session *s, const int32_t *cuts, uint32_t n_cuts, uint32_t tid_lo, uint32_t tid_hi, uint32_t *tid_next, uint64_t *n_runs) {
    if (!s) return COV_ERR_INVALID_ARG;
    if (const cov_status rc = depth_cuts_check(s, "cov_depth_class_runs_compute", cuts, n_cuts)) return rc;
    return depth_runs_compute(s, "cov_depth_class_runs_compute", dclc::ClassView{dclc::make(cuts, n_cuts)}, tid_lo, tid_hi, tid_next, n_runs);
}

cov_status cov_depth_runs_fetch(cov_session *s, uint64_t *run_off, cov_depth_run *runs) {
    if (!s) return COV_ERR_INVALID_ARG;
    if (s->ing.active) { s->err = "cov_depth_runs_fetch: a device ingest is still open (cov_ingest_end first)"; return COV_ERR_STATE; }
    if (s->spill.active) { s->err = "cov_depth_runs_fetch: part of the sample's records already left the bounded record store"; return COV_ERR_STATE; }
    if (s->finished && !s->dr.valid && s->dr.taker[cov_session::DepthRuns::RUNS]) { s->err = s->dr.lost(cov_session::DepthRuns::RUNS); return COV_ERR_STATE; }
    if (!s->finished || !s->dr.valid) { s->err = "cov_depth_runs_fetch: no chunk computed since the last finish (cov_depth_runs_compute)"; return COV_ERR_STATE; }
    if (!run_off || (s->dr.n_runs && !runs)) return COV_ERR_INVALID_ARG;
    static_assert(sizeof(cov_depth_run) == 8 && sizeof(cov_depth_run) == sizeof(dprc::Run) && offsetof(cov_depth_run, depth) == 4 && offsetof(dprc::Run, depth) == 4,
                  "cov_depth_run mirrors the device struct (numpy mirror in coverm_amd/native.py)");
    cov_session::DepthRuns &D = s->dr;
    const u32 nT = D.next - D.lo;
    HIPCHK(hipSetDevice(s->cfg.device));
    D.h_run_off.resize((size_t)nT + 1);
    HIPCHK(hipMemcpyAsync(D.h_run_off.data(), D.run_off.p, (size_t)nT * 4, hipMemcpyDeviceToHost, s->stream));
    if (D.n_runs) HIPCHK(hipMemcpyAsync(runs, D.runs.p, (size_t)D.n_runs * sizeof(cov_depth_run), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    for (u32 k = 0; k < nT; k++) run_off[k] = D.h_run_off[k];
    run_off[nT] = D.n_runs;
    return COV_OK;
}

cov_status cov_depth_runs_last(const cov_session *s, cov_depth_runs_info *out) {
    if (!s || !out) return COV_ERR_INVALID_ARG;
    const cov_session::DepthRuns &D = s->dr;
    out->arena_bases = D.arena_bases; out->n_runs = D.n_runs; out->arena_ms = D.arena_ms; out->runs_ms = D.runs_ms; out->tid_lo = D.lo; out->tid_next = D.next;
    return COV_OK;
}

// ---------------------------------------------------------------------------------------------- depth bins (depth_bins_kernels.hip.h)
// One chunk of whole targets: the arena stage of the depth runs, then every bin initialised and the arena reduced in one pass.  The bin
// offsets come from the lengths, which the host has: no count, no scan and no host wait in front of the reduction.
cov_status cov_depth_bins_compute(cov_session *s, uint32_t bin_size, uint32_t tid_lo, uint32_t tid_hi, uint32_t *tid_next, uint64_t *n_bins) {
    if (!s) return COV_ERR_INVALID_ARG;
    if (s->ing.active) { s->err = "cov_depth_bins_compute: a device ingest is still open (cov_ingest_end first)"; return COV_ERR_STATE; }
    if (!s->finished) { s->err = "cov_depth_bins_compute: needs a cov_finish over the records"; return COV_ERR_STATE; }
    if (s->spill.active) { s->err = "cov_depth_bins_compute: part of the sample's records already left the bounded record store"; return COV_ERR_STATE; }
    if (bin_size == 0 || bin_size > dbnc::MAX_BIN_SIZE) { s->err = "cov_depth_bins_compute: the bin size is 1 .. 2^31 - 1 bases"; return COV_ERR_INVALID_ARG; }
    if (!tid_next || !n_bins || tid_lo >= tid_hi || tid_hi > s->n_targets) return COV_ERR_INVALID_ARG;
    covr::Range rr("depth bins of one chunk (cov_depth_bins_compute)");
    cov_session::DepthRuns &D = s->dr;
    HIPCHK(hipSetDevice(s->cfg.device));
    timing_events(s);
    hipStream_t st = s->stream;
    // the chunk is the planner's whatever the bin size; its bins are known from the lengths alone
    const u32 t1 = dprc::plan_chunk(s->h_tlen.data(), tid_lo, tid_hi, D.chunk_bases), nT = t1 - tid_lo;
    const u64 total = [&] { u64 b = 0; for (u32 k = 0; k < nT; k++) b += dbnc::bins_of(s->h_tlen[tid_lo + k], bin_size); return b; }();
    // (a refusal leaves the chunk computed before, its offsets included, as it was)
    if (total > 0xffffffffull) { s->err = "cov_depth_bins_compute: more than 2^32 bins in one chunk"; return COV_ERR_STATE; }      // (at most one bin per entry, as for the runs)
    hipEvent_t *ev = s->ev[COV_K_DEPTH_BINS];      // events of its own: the call is not part of a finish; ev_mid closes the bin kernels
    if (!D.ev_mid) HIPCHK(hipEventCreate(&D.ev_mid));
    DepthChunk ck;
    if (const cov_status rc = depth_arena_stage(s, "cov_depth_bins_compute", cov_session::DepthRuns::BINS, tid_lo, tid_hi, ev, ck)) return rc;
    D.h_bin_off.resize((size_t)nT + 1); D.h_bin_off32.resize((size_t)nT + 1);
    (void)dbnc::bin_layout(s->h_tlen.data() + tid_lo, nT, bin_size, D.h_bin_off.data());
    for (u32 k = 0; k <= nT; k++) D.h_bin_off32[k] = (u32)D.h_bin_off[k];
    HIPCHK(D.bin_off.reserve((size_t)nT + 1, st)); HIPCHK(D.bins.reserve(std::max<u64>(total, 1), st));
    HIPCHK(hipMemcpyAsync(D.bin_off.p, D.h_bin_off32.data(), ((size_t)nT + 1) * 4, hipMemcpyHostToDevice, st));
    u32 launches = 4;      // k_depth_marks and the rank scan's three
    if (total) {
        hipLaunchKernelGGL(covdb::k_bins_init, dim3((u32)((total + 255ull) / 256ull)), dim3(256), 0, st, D.bins.p, total);
        const u32 waves = (ck.words + dbnc::STRETCH_WORDS - 1u) / dbnc::STRETCH_WORDS;
        hipLaunchKernelGGL(covdb::k_depth_bins, dim3((waves + 3u) / 4u), dim3(256), 0, st, (const int32_t *)D.arena.p, (const u32 *)D.mask.p, (const u32 *)D.rank.p,
                           (const u32 *)D.woff.p, (const u32 *)D.bin_off.p, ck.words, bin_size, D.bins.p, (u32)total);
        launches += 2;
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(D.ev_mid, st));
    HIPCHK(hipStreamSynchronize(st));
    float ms_arena = 0.f, ms_bins = 0.f;
    (void)hipEventElapsedTime(&ms_arena, ev[0], ev[1]);
    (void)hipEventElapsedTime(&ms_bins, ev[1], D.ev_mid);
    s->ev_fresh = -1;
    D.b_arena_ms = ms_arena; D.bins_ms = ms_bins; D.b_launches = launches;
    D.b_lo = tid_lo; D.b_next = t1; D.n_bins = total; D.b_arena_bases = 4ull * ck.words; D.bin_size = bin_size; D.bins_valid = true;
    *tid_next = t1; *n_bins = total;
    if (cov_timing_on())
        fprintf(stderr, "[covermhip] depth bins of %u: targets [%u, %u), %llu arena entries, %llu bins; arena %.3f ms, bin kernels %.3f ms\n", bin_size, tid_lo, t1,
                (unsigned long long)D.b_arena_bases, (unsigned long long)total, D.b_arena_ms, D.bins_ms);
    return COV_OK;
}

cov_status cov_depth_bins_fetch(cov_session *s, uint64_t *bin_off, cov_depth_bin *bins) {
    if (!s) return COV_ERR_INVALID_ARG;
    if (s->ing.active) { s->err = "cov_depth_bins_fetch: a device ingest is still open (cov_ingest_end first)"; return COV_ERR_STATE; }
    if (s->spill.active) { s->err = "cov_depth_bins_fetch: part of the sample's records already left the bounded record store"; return COV_ERR_STATE; }
    if (s->finished && !s->dr.bins_valid && s->dr.taker[cov_session::DepthRuns::BINS]) { s->err = s->dr.lost(cov_session::DepthRuns::BINS); return COV_ERR_STATE; }
    if (!s->finished || !s->dr.bins_valid) { s->err = "cov_depth_bins_fetch: no chunk computed since the last finish (cov_depth_bins_compute)"; return COV_ERR_STATE; }
    if (!bin_off || (s->dr.n_bins && !bins)) return COV_ERR_INVALID_ARG;
    cov_session::DepthRuns &D = s->dr;
    const u32 nT = D.b_next - D.b_lo;
    HIPCHK(hipSetDevice(s->cfg.device));
    if (D.n_bins) {
        HIPCHK(hipMemcpyAsync(bins, D.bins.p, (size_t)D.n_bins * sizeof(cov_depth_bin), hipMemcpyDeviceToHost, s->stream));
        HIPCHK(hipStreamSynchronize(s->stream));
    }
    for (u32 k = 0; k <= nT; k++) bin_off[k] = D.h_bin_off[k];
    return COV_OK;
}

cov_status cov_depth_bins_last(const cov_session *s, cov_depth_bins_info *out) {
    if (!s || !out) return COV_ERR_INVALID_ARG;
    const cov_session::DepthRuns &D = s->dr;
    out->arena_bases = D.b_arena_bases; out->n_bins = D.n_bins; out->arena_ms = D.b_arena_ms; out->bins_ms = D.bins_ms; out->tid_lo = D.b_lo; out->tid_next = D.b_next;
    out->bin_size = D.bin_size; out->reserved = 0;
    return COV_OK;
}

// ---------------------------------------------------------------------------------------------- depth regions (depth_regions_kernels.hip.h)
// The session's regions: validated, then kept in a stable order by tid with their positions in the caller's array.
cov_status cov_depth_regions_set(cov_session *s, const cov_depth_region *regions, uint64_t n) {
    if (!s || (n && !regions)) return COV_ERR_INVALID_ARG;
    if (s->h_tile_first.empty()) /* (cov_set_targets leaves n_targets + 1 entries) */ { s->err = "cov_depth_regions_set: needs cov_set_targets (the regions are validated against the targets)"; return COV_ERR_STATE; }
    if (n >= (1ull << 32)) { s->err = "cov_depth_regions_set: 2^32 regions or more (index 4294967296 is the first that does not fit)"; return COV_ERR_INVALID_ARG; }
    cov_session::DepthRuns &D = s->dr;
    for (uint64_t i = 0; i < n; i++) {
        const cov_depth_region &r = regions[i];
        const char *what = r.tid >= s->n_targets ? "its tid is not a target" : r.reserved != 0 ? "its reserved field is not 0" : r.start >= r.end ? "start >= end" :
                           r.end > s->h_tlen[r.tid] ? "its end lies behind the target's length" : nullptr;
        if (what) { s->err = "cov_depth_regions_set: region " + std::to_string(i) + ": " + what; return COV_ERR_INVALID_ARG; }
    }
    // counting sort by tid: stable, so the input order inside a target is kept
    std::vector<u32> first((size_t)s->n_targets + 1, 0u);
    for (uint64_t i = 0; i < n; i++) first[regions[i].tid + 1]++;
    for (u32 t = 0; t < s->n_targets; t++) first[t + 1] += first[t];
    std::vector<drgc::Region> reg((size_t)n);
    std::vector<u32> input((size_t)n), at(first.begin(), first.end() - 1);
    for (uint64_t i = 0; i < n; i++) {
        const u32 j = at[regions[i].tid]++;
        reg[j].tid = regions[i].tid; reg[j].start = regions[i].start; reg[j].end = regions[i].end; reg[j].reserved = 0u;
        input[j] = (u32)i;
    }
    D.h_reg.swap(reg); D.h_reg_input.swap(input); D.h_reg_first.swap(first);
    D.have_regions = n != 0;
    if (D.regs_valid) { D.regs_valid = false; D.taker[cov_session::DepthRuns::REGIONS] = 0; }      // the chunk computed for the regions before is not theirs
    return COV_OK;
}

// One chunk of whole targets: the arena stage of the depth runs, then the chunk's regions described from its woff[] on the host, every
// result initialised and one wave per piece of a region.  The piece offsets come from the regions alone: no count, no scan and no host wait
// in front of the reduction.
cov_status cov_depth_regions_compute(cov_session *s, uint32_t tid_lo, uint32_t tid_hi, uint32_t *tid_next, uint64_t *n_regions) {
    if (!s) return COV_ERR_INVALID_ARG;
    if (s->ing.active) { s->err = "cov_depth_regions_compute: a device ingest is still open (cov_ingest_end first)"; return COV_ERR_STATE; }
    if (!s->finished) { s->err = "cov_depth_regions_compute: needs a cov_finish over the records"; return COV_ERR_STATE; }
    if (s->spill.active) { s->err = "cov_depth_regions_compute: part of the sample's records already left the bounded record store"; return COV_ERR_STATE; }
    if (!s->dr.have_regions) { s->err = "cov_depth_regions_compute: no regions set (cov_depth_regions_set)"; return COV_ERR_STATE; }
    if (!tid_next || !n_regions || tid_lo >= tid_hi || tid_hi > s->n_targets) return COV_ERR_INVALID_ARG;
    covr::Range rr("depth regions of one chunk (cov_depth_regions_compute)");
    cov_session::DepthRuns &D = s->dr;
    HIPCHK(hipSetDevice(s->cfg.device));
    timing_events(s);
    hipStream_t st = s->stream;
    const u32 t1 = dprc::plan_chunk(s->h_tlen.data(), tid_lo, tid_hi, D.chunk_bases);
    const u32 r0 = D.h_reg_first[tid_lo], n = D.h_reg_first[t1] - r0;
    const u64 pieces = [&] { u64 p = 0; for (u32 r = 0; r < n; r++) p += drgc::pieces_of_region(D.h_reg[r0 + r].start, D.h_reg[r0 + r].end); return p; }();
    // (a refusal leaves the chunk computed before as it was)
    if (pieces > 0xffffffffull) { s->err = "cov_depth_regions_compute: more than 2^32 pieces in one chunk"; return COV_ERR_STATE; }
    hipEvent_t *ev = s->ev[COV_K_DEPTH_REGIONS];      // events of its own: the call is not part of a finish; ev_mid closes the region kernels
    if (!D.ev_mid) HIPCHK(hipEventCreate(&D.ev_mid));
    DepthChunk ck;
    if (const cov_status rc = depth_arena_stage(s, "cov_depth_regions_compute", cov_session::DepthRuns::REGIONS, tid_lo, tid_hi, ev, ck)) return rc;
    u32 launches = 4;      // k_depth_marks and the rank scan's three
    if (n) {
        D.h_reg_desc.resize(n); D.h_reg_piece_off.resize((size_t)n + 1);
        u32 p = 0;
        for (u32 r = 0; r < n; r++) {
            const drgc::Region &g = D.h_reg[r0 + r];
            D.h_reg_desc[r] = drgc::describe(D.h_woff[g.tid - tid_lo], g.start, g.end);
            D.h_reg_piece_off[r] = p; p += drgc::pieces_of(D.h_reg_desc[r]);
        }
        D.h_reg_piece_off[n] = p;
        HIPCHK(D.reg_desc.reserve(n, st)); HIPCHK(D.reg_piece_off.reserve((size_t)n + 1, st)); HIPCHK(D.regs.reserve(n, st));
        HIPCHK(hipMemcpyAsync(D.reg_desc.p, D.h_reg_desc.data(), (size_t)n * sizeof(drgc::Desc), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(D.reg_piece_off.p, D.h_reg_piece_off.data(), ((size_t)n + 1) * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(covdb::k_bins_init, dim3((n + 255u) / 256u), dim3(256), 0, st, D.regs.p, (u64)n);
        if (D.thr.n) {      // the threshold variant: the same launch, the counts beside the results (zeroed by a fill, which is no launch)
            HIPCHK(D.reg_counts.reserve((size_t)n * D.thr.n, st));
            HIPCHK(hipMemsetAsync(D.reg_counts.p, 0, (size_t)n * D.thr.n * 4, st));
            hipLaunchKernelGGL(covrg::k_depth_regions_thr, dim3((u32)((pieces + 3ull) / 4ull)), dim3(256), 0, st, (const int32_t *)D.arena.p, (const drgc::Desc *)D.reg_desc.p,
                               (const u32 *)D.reg_piece_off.p, n, (u32)pieces, D.regs.p, D.thr, D.reg_counts.p);
        } else
            hipLaunchKernelGGL(covrg::k_depth_regions, dim3((u32)((pieces + 3ull) / 4ull)), dim3(256), 0, st, (const int32_t *)D.arena.p, (const drgc::Desc *)D.reg_desc.p,
                               (const u32 *)D.reg_piece_off.p, n, (u32)pieces, D.regs.p);
        launches += 2;
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(D.ev_mid, st));
    HIPCHK(hipStreamSynchronize(st));
    float ms_arena = 0.f, ms_regs = 0.f;
    (void)hipEventElapsedTime(&ms_arena, ev[0], ev[1]);
    (void)hipEventElapsedTime(&ms_regs, ev[1], D.ev_mid);
    s->ev_fresh = -1;
    D.g_arena_ms = ms_arena; D.regs_ms = ms_regs; D.g_launches = launches;
    D.g_lo = tid_lo; D.g_next = t1; D.g_first = r0; D.n_regs = n; D.n_pieces = pieces; D.g_arena_bases = 4ull * ck.words; D.g_thr = D.thr.n; D.regs_valid = true;
    *tid_next = t1; *n_regions = n;
    if (cov_timing_on())
        fprintf(stderr, "[covermhip] depth regions: targets [%u, %u), %llu arena entries, %u regions in %llu pieces; arena %.3f ms, region kernels %.3f ms\n", tid_lo, t1,
                (unsigned long long)D.g_arena_bases, n, (unsigned long long)pieces, D.g_arena_ms, D.regs_ms);
    return COV_OK;
}

cov_status cov_depth_regions_fetch(cov_session *s, uint64_t *input_index, cov_depth_bin *out) {
    if (!s) return COV_ERR_INVALID_ARG;
    if (s->ing.active) { s->err = "cov_depth_regions_fetch: a device ingest is still open (cov_ingest_end first)"; return COV_ERR_STATE; }
    if (s->spill.active) { s->err = "cov_depth_regions_fetch: part of the sample's records already left the bounded record store"; return COV_ERR_STATE; }
    if (s->finished && !s->dr.regs_valid && s->dr.taker[cov_session::DepthRuns::REGIONS]) { s->err = s->dr.lost(cov_session::DepthRuns::REGIONS); return COV_ERR_STATE; }
    if (!s->finished || !s->dr.regs_valid) { s->err = "cov_depth_regions_fetch: no chunk computed since the last finish (cov_depth_regions_compute)"; return COV_ERR_STATE; }
    if (s->dr.n_regs && (!input_index || !out)) return COV_ERR_INVALID_ARG;
    cov_session::DepthRuns &D = s->dr;
    HIPCHK(hipSetDevice(s->cfg.device));
    if (D.n_regs) {
        HIPCHK(hipMemcpyAsync(out, D.regs.p, (size_t)D.n_regs * sizeof(cov_depth_bin), hipMemcpyDeviceToHost, s->stream));
        HIPCHK(hipStreamSynchronize(s->stream));
    }
    for (u64 i = 0; i < D.n_regs; i++) input_index[i] = D.h_reg_input[D.g_first + i];
    return COV_OK;
}

cov_status cov_depth_thresholds_set(cov_session *s, const int32_t *thr, uint32_t n) {
    if (!s) return COV_ERR_INVALID_ARG;
    cov_session::DepthRuns &D = s->dr;
    if (n) {
        if (const cov_status rc = depth_cuts_check(s, "cov_depth_thresholds_set", thr, n)) return rc;      // (the thresholds set before stay)
        D.thr = dclc::make(thr, n);
    } else
        D.thr = dclc::Cuts{};
    if (D.regs_valid) { D.regs_valid = false; D.taker[cov_session::DepthRuns::REGIONS] = 0; }      // the chunk computed under the thresholds before is not theirs
    return COV_OK;
}

cov_status cov_depth_regions_counts_fetch(cov_session *s, uint32_t *counts) {
    if (!s) return COV_ERR_INVALID_ARG;
    if (s->ing.active) { s->err = "cov_depth_regions_counts_fetch: a device ingest is still open (cov_ingest_end first)"; return COV_ERR_STATE; }
    if (s->spill.active) { s->err = "cov_depth_regions_counts_fetch: part of the sample's records already left the bounded record store"; return COV_ERR_STATE; }
    if (!s->dr.thr.n) { s->err = "cov_depth_regions_counts_fetch: no thresholds set (cov_depth_thresholds_set)"; return COV_ERR_STATE; }
    if (s->finished && !s->dr.regs_valid && s->dr.taker[cov_session::DepthRuns::REGIONS]) { s->err = s->dr.lost(cov_session::DepthRuns::REGIONS); return COV_ERR_STATE; }
    if (!s->finished || !s->dr.regs_valid) { s->err = "cov_depth_regions_counts_fetch: no chunk computed since the last finish (cov_depth_regions_compute)"; return COV_ERR_STATE; }
    cov_session::DepthRuns &D = s->dr;      // (a valid chunk was computed under the thresholds now set: setting them drops it)
    if (D.n_regs && !counts) return COV_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(s->cfg.device));
    if (D.n_regs) {
        HIPCHK(hipMemcpyAsync(counts, D.reg_counts.p, (size_t)D.n_regs * D.g_thr * 4, hipMemcpyDeviceToHost, s->stream));
        HIPCHK(hipStreamSynchronize(s->stream));
    }
    return COV_OK;
}

cov_status cov_depth_regions_last(const cov_session *s, cov_depth_regions_info *out) {
    if (!s || !out) return COV_ERR_INVALID_ARG;
    const cov_session::DepthRuns &D = s->dr;
    out->arena_bases = D.g_arena_bases; out->n_regions = D.n_regs; out->n_pieces = D.n_pieces; out->arena_ms = D.g_arena_ms; out->regions_ms = D.regs_ms;
    out->tid_lo = D.g_lo; out->tid_next = D.g_next;
    return COV_OK;
}

cov_status cov_fetch_interval_hist(cov_session *s, uint64_t *hist) {
    if (!s || !s->finished) return COV_ERR_STATE;
    if (s->ivhist_total == 0) return COV_OK;
    if (!hist) return COV_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(s->cfg.device));
    HIPCHK(hipMemcpyAsync(hist, s->d_ivhist.p, s->ivhist_total * 8, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return COV_OK;
}

cov_status cov_kernel_ms(const cov_session *s, cov_kernel_id k, double *ms_total, uint32_t *launches) {
    if (!s || k < 0 || k >= COV_K_COUNT) return COV_ERR_INVALID_ARG;
    if (k == COV_K_SAM) {        // not part of a finish: the decode kernels of the last cov_sam_* ingest, summed over its windows
        if (ms_total) *ms_total = s->sam_ms;
        if (launches) *launches = s->sam_launches;
        return COV_OK;
    }
    if (k == COV_K_GENE_READS) {      // not part of a finish: the last cov_interval_reads_compute
        if (ms_total) *ms_total = s->gene_ms;
        if (launches) *launches = s->gene_launches;
        return COV_OK;
    }
    if (k == COV_K_DEPTH_RUNS) {      // not part of a finish: the last cov_depth_runs_compute
        if (ms_total) *ms_total = s->dr.runs_ms;
        if (launches) *launches = s->dr.launches;
        return COV_OK;
    }
    if (k == COV_K_DEPTH_BINS) {      // not part of a finish: the last cov_depth_bins_compute
        if (ms_total) *ms_total = s->dr.bins_ms;
        if (launches) *launches = s->dr.b_launches;
        return COV_OK;
    }
    if (k == COV_K_DEPTH_REGIONS) {      // not part of a finish: the last cov_depth_regions_compute
        if (ms_total) *ms_total = s->dr.regs_ms;
        if (launches) *launches = s->dr.g_launches;
        return COV_OK;
    }
    if (k == COV_K_GROUP) {      // not part of a finish: the last cov_group_records
        if (ms_total) *ms_total = s->grp_ms[0];
        if (launches) *launches = s->grp_launches;
        return COV_OK;
    }
    if (ms_total) *ms_total = s->k_ms[k];
    if (launches) *launches = s->k_launches[k];
    return COV_OK;
}

cov_status cov_last_paths(const cov_session *s, cov_path_counts *out) {
    if (!s || !out) return COV_ERR_INVALID_ARG;
    out->listed_steps = s->h_glob.n_gen; out->generic_only = s->last_gen_all ? 1u : 0u;
    out->slow_tiles = s->h_glob.n_slow; out->bucket_records = s->h_glob.n_cx;
    out->bucket_entries = (uint32_t)std::min<uint64_t>(s->h_glob.cx_total, 0xffffffffull); out->passes = s->last_passes;
    return COV_OK;
}

cov_status cov_pileup_schedule(const cov_session *s, uint32_t out[4]) {
    if (!s || !out) return COV_ERR_INVALID_ARG;
    out[0] = s->h_glob.n_deep; out[1] = s->last_pileup_waves; out[2] = s->last_pileup_chunk; out[3] = s->deep_min;
    return COV_OK;
}

// Test hook: the run words the last finish's k_prep left, one per record of the store (x | y << 32, see "Run word" in pileup_kernels.hip.h).
cov_status cov_copy_run_words(const cov_session *cs, uint64_t *out) {
    cov_session *s = const_cast<cov_session *>(cs);      // (nothing of the session changes but the text of a HIP error)
    if (!s || !s->finished) return COV_ERR_STATE;
    // no run words for the whole store: part of it left in a spill, the records are an adopted device batch, or there are none
    if (s->spill.active || s->adopted || s->store.n_records == 0 || s->d_runs.cap < s->store.n_records) return COV_ERR_STATE;
    if (!out) return COV_ERR_INVALID_ARG;
    static_assert(sizeof(uint2) == sizeof(uint64_t), "a run word is eight bytes, x first");
    HIPCHK(hipSetDevice(s->cfg.device));
    HIPCHK(hipMemcpyAsync(out, s->d_runs.p, (size_t)s->store.n_records * sizeof(uint2), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return COV_OK;
}

uint32_t cov_store_spills(const cov_session *s) { return s ? s->spill.count : 0u; }

cov_status cov_set_estimators(cov_session *s, const cov_estimator *est, uint32_t n_est) {
    if (!s || (n_est && !est)) return COV_ERR_INVALID_ARG;
    if (n_est > COV_EST_MAX) { s->err = "cov_set_estimators: more than COV_EST_MAX estimators"; return COV_ERR_INVALID_ARG; }
    if (s->spill.active) { s->err = "cov_set_estimators: set them before the sample's first records (part of it already left the bounded record store)"; return COV_ERR_STATE; }
    for (uint32_t k = 0; k < n_est; k++) {
        const int kind = est[k].kind;
        if (kind < 0 || kind > COV_EST_ANIR || kind == COV_EST_TPM || kind == COV_EST_PILEUP_COUNTS) {
            s->err = "cov_set_estimators: this estimator is evaluated on the host (TPM: f64 exp / ln of the host's libm; coverage histogram: prints the histogram itself)";
            return COV_ERR_INVALID_ARG;
        }
        if (kind == COV_EST_TRIMMED_MEAN && !(s->cfg.want & COV_WANT_HIST)) { s->err = "cov_set_estimators: a trimmed mean needs COV_WANT_HIST"; return COV_ERR_INVALID_ARG; }
        if (kind == COV_EST_ANIR && s->have_genomes) {      // genome entries take the not-supplementary sum (genome.rs:220)
            if (!(s->cfg.want & COV_WANT_IDENTITY) || (s->cfg.want & COV_WANT_IDENTITY_PRIMARY_ONLY)) {
                s->err = "cov_set_estimators: ANIr of a genome needs COV_WANT_IDENTITY with the not-supplementary sum"; return COV_ERR_INVALID_ARG;
            }
        } else if (kind == COV_EST_ANIR && (!(s->cfg.want & COV_WANT_IDENTITY) || (s->cfg.want & COV_WANT_IDENTITY_NONSUPP_ONLY))) {
            s->err = "cov_set_estimators: ANIr needs COV_WANT_IDENTITY with the primary-read sum"; return COV_ERR_INVALID_ARG;
        }
    }
    s->est = EstParams{};
    for (uint32_t k = 0; k < n_est; k++) memcpy(&s->est.e[k], &est[k], sizeof(cov_estimator));
    s->est.n = n_est;
    s->est_valid = false; s->gen_valid = false;
    return COV_OK;
}

static cov_status genome_fetch_ready(cov_session *s, const char *what) {
    if (!s) return COV_ERR_INVALID_ARG;
    if (s->spill.active) { s->err = std::string(what) + ": part of the sample's contigs left the bounded record store: aggregate cov_finish's per-contig results on the host"; return COV_ERR_STATE; }
    if (!s->finished || !s->gen_valid) { s->err = std::string(what) + ": cov_set_genomes or cov_set_genome_runs, and cov_set_estimators, then cov_finish"; return COV_ERR_STATE; }
    return COV_OK;
}
cov_status cov_fetch_genome_estimates(cov_session *s, float *out) {
    const cov_status r = genome_fetch_ready(s, "cov_fetch_genome_estimates");
    if (r != COV_OK) return r;
    const size_t nf = (size_t)s->n_genomes * s->est.n;
    if (nf && !out) return COV_ERR_INVALID_ARG;
    if (nf) memcpy(out, s->h_gout + (size_t)s->n_genomes * sizeof(cov_genome_stats), nf * sizeof(float));
    return COV_OK;
}
cov_status cov_fetch_genome_stats(cov_session *s, cov_genome_stats *out) {
    const cov_status r = genome_fetch_ready(s, "cov_fetch_genome_stats");
    if (r != COV_OK) return r;
    if (!out) return COV_ERR_INVALID_ARG;
    memcpy(out, s->h_gout, (size_t)s->n_genomes * sizeof(cov_genome_stats));
    return COV_OK;
}

cov_status cov_genome_entry_count(cov_session *s, uint32_t *n_entries) {
    const cov_status r = genome_fetch_ready(s, "cov_genome_entry_count");
    if (r != COV_OK) return r;
    if (!s->have_runs) { s->err = "cov_genome_entry_count: cov_set_genome_runs first"; return COV_ERR_STATE; }
    if (!n_entries) return COV_ERR_INVALID_ARG;
    *n_entries = s->n_genomes;
    return COV_OK;
}
cov_status cov_fetch_genome_entries(cov_session *s, cov_genome_entry *out) {
    const cov_status r = genome_fetch_ready(s, "cov_fetch_genome_entries");
    if (r != COV_OK) return r;
    if (!s->have_runs) { s->err = "cov_fetch_genome_entries: cov_set_genome_runs first"; return COV_ERR_STATE; }
    const size_t n = s->n_genomes;
    if (n && !out) return COV_ERR_INVALID_ARG;
    const cov_genome_stats *gs = reinterpret_cast<const cov_genome_stats *>(s->h_gout);
    const SepEntry *se = reinterpret_cast<const SepEntry *>(s->h_gout + n * (sizeof(cov_genome_stats) + s->est.n * sizeof(float)));
    for (size_t e = 0; e < n; e++) {
        out[e].reads = gs[e].reads_in_genome; out[e].first_tid = se[e].first_tid; out[e].gid = se[e].gid;
        out[e].n_contigs_seen = gs[e].n_contigs_seen; out[e].any_nonzero = gs[e].any_nonzero;
    }
    return COV_OK;
}

cov_status cov_fetch_estimates(cov_session *s, float *out) {
    if (!s || !s->finished || !s->est_valid) { if (s) s->err = "cov_fetch_estimates: cov_set_estimators, then cov_finish"; return COV_ERR_STATE; }
    if (s->have_mask || s->have_runs) { s->err = "cov_fetch_estimates: with a target mask or genome runs the entries are genomes: aggregate on the host"; return COV_ERR_STATE; }
    const size_t nf = (size_t)s->n_targets * s->est.n;
    if (nf && !out) return COV_ERR_INVALID_ARG;
    if (nf) memcpy(out, s->h_estf, nf * sizeof(float));
    return COV_OK;
}

cov_status cov_algorithmic_bytes(const cov_session *s, uint64_t *bytes) {
    if (!s || !bytes) return COV_ERR_INVALID_ARG;
    *bytes = s->algo_bytes;
    return COV_OK;
}

// ---- pooled page-locked host memory (covermhip.h: cov_host_alloc / cov_host_free / cov_host_trim)
namespace {
struct HostPool {
    std::mutex m;
    std::map<void *, size_t> live;          // handed out: ptr -> block size
    std::multimap<size_t, void *> parked;   // free blocks by size
    static size_t round_up(size_t b) { const size_t g = (size_t)16 << 20; return b < g ? g : (b + g - 1) / g * g; }
};
HostPool g_host_pool;
}  // namespace

void *cov_host_alloc(size_t bytes) {
    const size_t want = HostPool::round_up(bytes);
    {
        std::lock_guard<std::mutex> lk(g_host_pool.m);
        auto it = g_host_pool.parked.lower_bound(want);
        if (it != g_host_pool.parked.end() && it->first <= 2 * want) {
            void *p = it->second; const size_t sz = it->first;
            g_host_pool.parked.erase(it);
            g_host_pool.live[p] = sz;
            return p;
        }
    }
    void *p = nullptr;
    if (hipHostMalloc(&p, want, hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    std::lock_guard<std::mutex> lk(g_host_pool.m);
    g_host_pool.live[p] = want;
    return p;
}

int cov_host_free(void *p) {
    if (!p) return 0;
    std::lock_guard<std::mutex> lk(g_host_pool.m);
    auto it = g_host_pool.live.find(p);
    if (it == g_host_pool.live.end()) return 0;
    g_host_pool.parked.emplace(it->second, p);
    g_host_pool.live.erase(it);
    return 1;
}

// File pages mapped by the caller (mmap of the BAM) made readable by the session's device, so that the DMA engine takes the
// compressed bytes straight from the page cache: no staging copy by the CPU (measured on the lease box, tools/ubench/io_probe:
// 57 GB/s, the link's rate, against 42 GB/s through 64 MiB staging slots filled by 16 threads).
cov_status cov_host_register(cov_session *s, void *p, size_t bytes) {
    if (!s || !p || !bytes) return COV_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(s->cfg.device));
    const hipError_t e = hipHostRegister(p, bytes, hipHostRegisterDefault);
    if (e != hipSuccess) { (void)hipGetLastError(); s->err = std::string("hipHostRegister: ") + hipGetErrorString(e); return COV_ERR_HIP; }
    return COV_OK;
}
cov_status cov_host_unregister(cov_session *s, void *p) {
    if (!s || !p) return COV_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(s->cfg.device));
    const hipError_t e = hipHostUnregister(p);
    if (e != hipSuccess) { (void)hipGetLastError(); s->err = std::string("hipHostUnregister: ") + hipGetErrorString(e); return COV_ERR_HIP; }
    return COV_OK;
}

// The calling thread (and every thread it creates afterwards: readers, pools) runs on the CPUs of the NUMA node the device hangs
// off, so that staging buffers, the page-cache copies into them and the DMA reads stay on one memory controller (lease box, 200 M
// reads: 0.87-0.88 s on the device's node, 0.99-1.00 s on the other one, 0.90-0.93 s unbound; profiles/r03_reader_sweep_200M.log).
// Returns the node, or -1 when nothing was changed (one node, no sysfs entry, affinity not permitted, COVERM_NUMA_BIND=0).
int cov_bind_thread_to_device_node(int device) {
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, device) != hipSuccess) { (void)hipGetLastError(); return -1; }
    for (char *c = bus; *c; c++) if (*c >= 'A' && *c <= 'F') *c = (char)(*c - 'A' + 'a');
    char path[256];
    snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bus);
    FILE *f = fopen(path, "r");
    if (!f) return -1;
    int node = -1;
    if (fscanf(f, "%d", &node) != 1) node = -1;
    fclose(f);
    if (node < 0) return -1;
    snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", node);
    f = fopen(path, "r");
    if (!f) return -1;
    char list[4096] = {0};
    const bool got = fgets(list, sizeof list, f) != nullptr;
    fclose(f);
    if (!got) return -1;
    cpu_set_t want, have;
    CPU_ZERO(&want);
    for (char *p = list; *p;) {          // "0-63,128-191"
        char *end = nullptr;
        const long a = strtol(p, &end, 10);
        if (end == p) break;
        long b = a;
        if (*end == '-') { p = end + 1; b = strtol(p, &end, 10); }
        for (long c = a; c <= b && c < CPU_SETSIZE; c++) CPU_SET((int)c, &want);
        p = (*end == ',') ? end + 1 : end;
        if (*end != ',') break;
    }
    if (sched_getaffinity(0, sizeof have, &have) != 0) return -1;
    cpu_set_t both;
    CPU_AND(&both, &want, &have);
    if (CPU_COUNT(&both) == 0 || CPU_COUNT(&both) == CPU_COUNT(&have)) return -1;      // nothing to narrow
    if (sched_setaffinity(0, sizeof both, &both) != 0) return -1;
    return node;
}

void cov_host_trim(void) {
    std::multimap<size_t, void *> drop;
    { std::lock_guard<std::mutex> lk(g_host_pool.m); drop.swap(g_host_pool.parked); }
    for (auto &kv : drop) (void)hipHostFree(kv.second);
}

}  // extern "C"

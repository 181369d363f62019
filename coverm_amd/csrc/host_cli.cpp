// covh_cli_main — `coverm contig` / `coverm genome` over --bam-files on the MI355X engine (the body of the coverm-amd binary).
//
// Mirrors the reference orchestrator for this path (src/bin/coverm.rs): FilterParameters::generate_from_clap
// :1659-1678 + doing_filtering :1695-1703, EstimatorsAndTaker::generate_from_clap :1315-1504, print_headers
// :1506-1519, run_contig :2088-2131, run_genome :1539-1628, parse_percentage :1296-1312, parse_separator
// :1522-1537; flag names and defaults from src/cli.rs (contig :2264-2582, genome :1669-2263).
// Everything else the reference binary does (mapping, indexing, filter/make/cluster subcommands) is out of scope.
//
// Ingest: a BAM is STREAMED (covh_bam_stream_*: windows of BGZF blocks inflated, parsed into page-locked SoA batches and
// pushed to HBM while later windows are still being inflated; host memory bounded) unless pair-mode filtering, --gff or SAM
// text input need the whole file on the host (covh_bam_open).  Each BAM brings its own header (contig.rs:29-32); only the
// cached taker insists that entry names agree between BAMs (coverage_takers.rs:140-148).
//
// Multi-GPU (--devices a,b,...; one process, one thread + session + stream reader per device):
//   * at least as many BAMs as devices: samples are dealt to devices (config 4 shape);
//   * fewer BAMs than devices: every BAM is cut into tid spans, one per device, each device inflating only its span
//     (config 5 shape); the per-contig result blocks meet on the first device through ONE RCCL gather (cov_gather).
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <future>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <cerrno>
#include <sys/stat.h>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/coverm_host.h"
#include "cli_route.h"
#include "knobs.h"

namespace {

std::atomic<bool> g_skip_teardown{false};   // covh_cli_set_fast_exit: a process about to exit need not hand ~100 GB of HBM back allocation by allocation

struct Fatal : std::runtime_error { using std::runtime_error::runtime_error; };
struct SpanUnsorted : Fatal { using Fatal::Fatal; };      // a tid span met keys that decrease (covh_bam_gpu_ingest_span -2, the CPU span reader's same rule)
[[noreturn]] void die(const std::string &m) { throw Fatal(m); }

// clap's typed value parsers (u8 / u16 / u32 / u64 / f32 arguments of coverm.rs / cli.rs): a value that is not a number of the argument's
// type ends the run, it is not read as 0
uint64_t parse_uint(const std::string &opt, const char *v, uint64_t max) {
    char *end = nullptr;
    errno = 0;
    const unsigned long long x = (v && *v >= '0' && *v <= '9') ? strtoull(v, &end, 10) : 0ull;
    if (!end || *end || errno || x > max) die(std::string("invalid value '") + (v ? v : "") + "' for '" + opt + "'");
    return x;
}
float parse_f32(const std::string &opt, const char *v) {
    char *end = nullptr;
    const float x = (v && *v) ? strtof(v, &end) : 0.0f;
    if (!end || *end || end == v) die(std::string("invalid value '") + (v ? v : "") + "' for '" + opt + "'");
    return x;
}

float parse_percentage(const char *v, const char *opt = "percentage") {   // coverm.rs:1296-1312
    if (!v) return 0.0f;
    float p = parse_f32(opt, v);
    if (p >= 1.0f && p <= 100.0f) p /= 100.0f;
    else if (!(p >= 0.0f && p <= 100.0f)) die(std::string("Invalid alignment percentage: '") + v + "'");
    return p;
}

// The reader-filter flags of contig, genome and filter (cli.rs) as given: the percentages still as text
struct FilterArgs {
    bool proper_pairs_only = false, exclude_supplementary = false, include_secondary = false;
    uint32_t len_single = 0, len_pair = 0;
    const char *pid_single = nullptr, *pct_single = nullptr, *pid_pair = nullptr, *pct_pair = nullptr;
    int mapq = 255;
};

// Takes `k` (and its value, through val()) when it is one of those flags
template <class Val> bool parse_filter_flag(const std::string &k, Val &&val, FilterArgs &fa) {
    if (k == "--proper-pairs-only") fa.proper_pairs_only = true;
    else if (k == "--exclude-supplementary") fa.exclude_supplementary = true;
    else if (k == "--include-secondary") fa.include_secondary = true;
    else if (k == "--min-read-aligned-length") fa.len_single = (uint32_t)parse_uint(k, val(), 0xffffffffull);
    else if (k == "--min-read-percent-identity") fa.pid_single = val();
    else if (k == "--min-read-aligned-percent") fa.pct_single = val();
    else if (k == "--min-read-aligned-length-pair") fa.len_pair = (uint32_t)parse_uint(k, val(), 0xffffffffull);
    else if (k == "--min-read-percent-identity-pair") fa.pid_pair = val();
    else if (k == "--min-read-aligned-percent-pair") fa.pct_pair = val();
    else if (k == "--min-mapq") fa.mapq = (int)parse_uint(k, val(), 255);
    else return false;
    return true;
}

struct Args {
    std::string mode;
    std::vector<std::string> bams, methods;
    const char *min_covered_fraction = nullptr, *trim_min = "5", *trim_max = "95";
    uint64_t contig_end_exclusion = 75;
    std::string output_format = "dense", output_file, genome_definition, gff, gff_feature_type;
    std::vector<std::string> genome_fasta_files;                       // genome mode: -f, -d (+ -x), --genome-fasta-list
    std::string genome_fasta_directory, genome_fasta_list, genome_fasta_extension = "fna";
    bool have_fasta_files = false, have_fasta_directory = false, have_fasta_list = false, use_full_contig_names = false;
    bool have_gff_feature_type = false;
    bool no_zeros = false;
    FilterArgs filter;
    bool single_genome = false, have_separator = false, no_stream = false;
    bool unsorted = false, verbose = false;      // --unsorted: the files need not be sorted by reference, records are grouped on the device (cov_group_records)
    char separator = '~';
    int threads = 1;
    std::vector<int> devices;
};

struct Filter {   // FilterParameters, coverm.rs:1648-1657
    bool improper = true, supp = true, sec = false;
    uint32_t len_single = 0, len_pair = 0;
    float pid_single = 0, pct_single = 0, pid_pair = 0, pct_pair = 0;
    int mapq = 255;
    bool doing_filtering() const {
        return pid_single > 0 || pid_pair > 0 || pct_single > 0 || mapq < 255 || pct_pair > 0 || len_single > 0 || len_pair > 0;
    }
    void mode(bool &fs, bool &fp) const {   // filter.rs:48-61
        const bool fs0 = len_single > 0 || pid_single > 0 || pct_single > 0;
        const bool fp0 = len_pair > 0 || pid_pair > 0 || pct_pair > 0;
        fs = fs0 || (!fp0 && mapq != 255);
        fp = fp0 || ((!fs || !improper) && mapq != 255);
    }
};

Filter resolve_filter(const FilterArgs &fa) {   // FilterParameters::generate_from_clap, coverm.rs:1659-1678
    Filter f;
    f.improper = !fa.proper_pairs_only; f.supp = !fa.exclude_supplementary; f.sec = fa.include_secondary;
    f.len_single = fa.len_single; f.len_pair = fa.len_pair; f.mapq = fa.mapq;
    f.pid_single = parse_percentage(fa.pid_single, "--min-read-percent-identity"); f.pct_single = parse_percentage(fa.pct_single, "--min-read-aligned-percent");
    f.pid_pair = parse_percentage(fa.pid_pair, "--min-read-percent-identity-pair"); f.pct_pair = parse_percentage(fa.pct_pair, "--min-read-aligned-percent-pair");
    return f;
}

// One BAM's results plus the header they refer to.
struct Sample {
    std::string stoit, path;
    std::string names_blob; std::vector<uint32_t> name_off; std::vector<uint64_t> tlen;
    std::vector<int32_t> genome_of_tid;
    std::vector<cov_contig_stats> stats;
    std::vector<uint64_t> hist;
    std::vector<float> estimates;      // calculate_coverage of every contig, evaluated on the device (Run::dev_est): n_targets x estimators
    // Run::dev_genome: the genomes aggregated and evaluated on the device — n_genomes x estimators floats and one cov_genome_stats per genome
    std::vector<float> genome_estimates; std::vector<cov_genome_stats> genome_stats; bool genome_dev = false, any_seen = false;
    // Run::dev_sep: the entries of the separator / single-genome scan from the device (their floats in genome_estimates); sep_set: this
    // sample's header went to the device (every name holds the separator), sep_dev: its results came back (no spill, some contig observed)
    std::vector<cov_genome_entry> sep_entries; bool sep_set = false, sep_dev = false;
    uint64_t prim = 0, n_records = 0;
    covh_reads_mapped gene_rm{0, 0};
    double t_open = 0, t_ingest = 0, t_finish = 0; uint64_t peak_bytes = 0; bool streamed = false, device_ingest = false;
    covh_header header() const { covh_header h; h.n_targets = (uint32_t)tlen.size(); h.names = names_blob.c_str(); h.name_off = name_off.data(); h.target_len = tlen.data(); return h; }
    std::string target_name(uint32_t t) const { return names_blob.substr(name_off[t], name_off[t + 1] - name_off[t]); }
};

double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
bool timing_on() { return covh_timing_on() != 0; }
// COVERM_NO_GPU_INGEST: every file through the CPU readers (tests compare the two paths); COVERM_PAIR_ON_HOST: the pair-mode reader filter on the host;
// COVERM_SAM_ON_HOST: a SAM file whole on the host; COVERM_GENES_DECODE_ON_HOST: --gff over the host's whole-file decode.  Facts of cli_route.h.
bool no_gpu_ingest() { static const bool v = getenv("COVERM_NO_GPU_INGEST") != nullptr; return v; }
bool pair_on_host() { static const bool v = getenv("COVERM_PAIR_ON_HOST") != nullptr; return v; }
bool sam_on_host() { static const bool v = getenv("COVERM_SAM_ON_HOST") != nullptr; return v; }
bool genes_decode_on_host() { static const bool v = getenv("COVERM_GENES_DECODE_ON_HOST") != nullptr; return v; }

struct HeaderAhead { covh_bam_header *hd = nullptr; std::string err; };

struct Run {
    std::mutex hdr_mutex;
    std::map<std::string, covh_sam *> sam_ahead;      // pipes, opened (and their format told) before the sessions exist
    std::map<std::string, std::future<HeaderAhead>> hdr_ahead;   // headers of the first BAM files, read beside the runtime's start-up
    Args a;
    Filter f;
    bool contig = true, by_names = false, per_gene = false, fs = false, fp = false;
    std::vector<covh_estimator> est;
    bool dev_est = false;      // `coverm contig` with estimators the device evaluates (cov_set_estimators): no per-contig finalisation, no histogram fetch on the host
    // contig-names genome scan with estimators the device evaluates (cov_set_genomes): no host pass over the contigs, no histogram fetch
    bool dev_genome = false;
    // separator / single-genome scan with estimators the device evaluates (cov_set_genome_runs): the same, per entry of the scan.  The
    // genome ids of a header are built once and kept for the samples that share it.
    bool dev_sep = false;
    std::mutex sep_mutex; std::string sep_names; std::vector<uint32_t> sep_name_off; std::vector<int32_t> sep_gid; uint32_t sep_n_gids = 0; bool sep_cached = false;
    uint32_t want = 0;
    cov_config cfg{};
    std::vector<std::string> genomes;
    std::unordered_map<std::string, int32_t> c2g;
    covh_genes *genes = nullptr;
    covh_taker *taker = nullptr;
    std::mutex taker_mutex;   // --gff writes entries while the sample is resident: one sample at a time
};

void check(cov_session *s, cov_status st) { if (st != COV_OK) die(cov_last_error(s)); }

// "-" (standard input), a FIFO or a character device: a stream that can be read once, with read() alone
bool input_is_pipe(const std::string &path) {
    if (path == "-") return true;
    struct stat sb;
    return stat(path.c_str(), &sb) == 0 && (S_ISFIFO(sb.st_mode) || S_ISCHR(sb.st_mode));
}

std::string stoit_of(const std::string &path) {   // file stem, bam_generator.rs:358-365
    if (path == "-") return "stdin";
    std::string p = path;
    const size_t sl = p.find_last_of('/');
    if (sl != std::string::npos) p = p.substr(sl + 1);
    const size_t dot = p.find_last_of('.');
    return dot == std::string::npos ? p : p.substr(0, dot);
}

void set_header(Sample &S, uint32_t nt, const std::function<const char *(uint32_t)> &name, const std::function<uint64_t(uint32_t)> &len) {
    S.names_blob.clear(); S.name_off.assign(1, 0); S.tlen.clear();
    for (uint32_t t = 0; t < nt; t++) { S.names_blob += name(t); S.name_off.push_back((uint32_t)S.names_blob.size()); S.tlen.push_back(len(t)); }
}

// tid -> genome table and participation mask of one BAM (genome.rs:51-67)
void genome_table(const Run &R, Sample &S, std::vector<uint8_t> &mask) {
    const uint32_t nt = (uint32_t)S.tlen.size();
    S.genome_of_tid.assign(nt, -1); mask.assign(nt, 0);
    uint32_t in = 0;
    for (uint32_t t = 0; t < nt; t++) {
        auto it = R.c2g.find(S.target_name(t));
        if (it != R.c2g.end()) { S.genome_of_tid[t] = it->second; mask[t] = 1; in++; }
    }
    if (!in) die("Error: There are no found reference sequences that are a part of a genome");
}

// The contig-names scan's participation of one BAM's references: the genome table for the device (Run::dev_genome), else the mask alone
void set_genomes_or_mask(Run &R, cov_session *s, const Sample &S, const std::vector<uint8_t> &mask) {
    if (!R.dev_genome) { check(s, cov_set_target_mask(s, mask.data())); return; }
    const double t0 = now();
    check(s, cov_set_genomes(s, S.genome_of_tid.data(), (uint32_t)R.genomes.size()));
    check(s, cov_set_estimators(s, reinterpret_cast<const cov_estimator *>(R.est.data()), (uint32_t)R.est.size()));
    if (timing_on()) fprintf(stderr, "[coverm-amd] %s: genome table to the device (cov_set_genomes) %.4fs\n", S.stoit.c_str(), now() - t0);
}

// The separator / single-genome scan on the device (Run::dev_sep): the genome ids of the sample's header, when every name holds the
// separator (a header with a name that does not stays with the host scan, which raises its error only for the names it touches).
void set_genome_runs(Run &R, cov_session *s, Sample &S) {
    const double t0 = now();
    S.sep_set = false;
    uint32_t n_gids;
    {
        // (the ids are handed over under the lock — the call only reads them —, so a sample takes no copy of a table of millions; the
        // offsets are compared first: two headers of equal offsets and different names are rare, two of different offsets are told at once)
        std::lock_guard<std::mutex> lk(R.sep_mutex);
        if (!R.sep_cached || R.sep_name_off != S.name_off || R.sep_names != S.names_blob) {
            const covh_header h = S.header();
            R.sep_gid.assign(S.tlen.size(), 0);
            R.sep_n_gids = covh_genome_separator_ids(&h, (uint8_t)R.a.separator, R.a.single_genome ? 1 : 0, R.sep_gid.data());
            R.sep_names = S.names_blob; R.sep_name_off = S.name_off; R.sep_cached = true;
        }
        n_gids = R.sep_n_gids;
        if (n_gids == 0 || S.tlen.empty()) return;
        check(s, cov_set_genome_runs(s, R.sep_gid.data(), n_gids));
    }
    check(s, cov_set_estimators(s, reinterpret_cast<const cov_estimator *>(R.est.data()), (uint32_t)R.est.size()));
    S.sep_set = true;
    if (timing_on()) fprintf(stderr, "[coverm-amd] %s: genome ids to the device (cov_set_genome_runs) %u ids, %.4fs\n", S.stoit.c_str(), n_gids, now() - t0);
}

// Genomes from FASTA files (-f / -d -x / --genome-fasta-list; genome_parsing.rs:10-70) into R.genomes / R.c2g, the table
// --genome-definition fills.  Returns the error message, or "" when resolved.
std::string resolve_fasta_genomes(Run &R) {
    const Args &a = R.a;
    char err[1024] = {0};
    std::vector<std::string> paths = a.genome_fasta_files;
    if (a.have_fasta_directory || a.have_fasta_list) {
        covh_path_list *l = covh_genome_fasta_paths(a.have_fasta_directory ? a.genome_fasta_directory.c_str() : nullptr, a.genome_fasta_extension.c_str(),
                                                    a.have_fasta_list ? a.genome_fasta_list.c_str() : nullptr, err, sizeof err);
        if (!l) return err;
        for (size_t i = 0; i < covh_path_list_count(l); i++) paths.push_back(covh_path_list_get(l, i));
        covh_path_list_free(l);
    }
    std::vector<const char *> pp;
    for (auto &p : paths) pp.push_back(p.c_str());
    const double t0 = now();
    covh_genome_set *gs = covh_genome_set_from_fasta(pp.data(), pp.size(), a.use_full_contig_names ? 1 : 0, std::max(1, a.threads), err, sizeof err);
    if (!gs) return err;
    const double t1 = now();
    for (size_t g = 0; g < covh_genome_set_n_genomes(gs); g++) R.genomes.push_back(covh_genome_set_genome_name(gs, g));
    const size_t nc = covh_genome_set_n_contigs(gs);
    R.c2g.reserve(nc);
    for (size_t i = 0; i < nc; i++) {
        const char *name; int32_t g;
        covh_genome_set_contig(gs, i, &name, &g);
        R.c2g.emplace(name, g);
    }
    covh_genome_set_free(gs);
    if (timing_on())
        fprintf(stderr, "[coverm-amd] genomes from FASTA: %zu files, %zu contigs, read %.3fs, table %.3fs\n", paths.size(), nc, t1 - t0, now() - t1);
    return "";
}

bool is_bgzf(const std::string &path) {
    if (input_is_pipe(path)) return false;      // (a pipe's format is told from the bytes read, covh_sam_open)
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    unsigned char m[2] = {0, 0};
    const size_t n = fread(m, 1, 2, f);
    fclose(f);
    return n == 2 && m[0] == 0x1f && m[1] == 0x8b;
}

// device ingests that run at once: every device in span mode (nb < nd) and with at least as many files as devices
size_t span_mode_feeders(size_t nb, size_t nd) { return nb < nd ? nd : std::min(nb, nd); }

// What the host keeps of a finished session: the estimators' floats when the device evaluated them, else the histogram bins the host's
// calculate_coverage needs.
void fetch_results(Run &R, cov_session *s, Sample &S, const cov_summary &summ) {
    if (R.dev_est) {
        S.estimates.resize(S.tlen.size() * R.est.size());
        check(s, cov_fetch_estimates(s, S.estimates.data()));
        return;
    }
    if (R.dev_genome && cov_store_spills(s) == 0) {
        S.genome_estimates.resize(R.genomes.size() * R.est.size()); S.genome_stats.resize(R.genomes.size());
        check(s, cov_fetch_genome_estimates(s, S.genome_estimates.data()));
        check(s, cov_fetch_genome_stats(s, S.genome_stats.data()));
        S.genome_dev = true; S.any_seen = summ.n_considered != 0;
        if (timing_on())
            fprintf(stderr, "[coverm-amd] %s: genome results from the device: %zu genomes x %zu estimators, %zu bytes\n", S.stoit.c_str(), R.genomes.size(), R.est.size(),
                    S.genome_estimates.size() * sizeof(float) + S.genome_stats.size() * sizeof(cov_genome_stats));
        return;
    }
    if (S.sep_set && cov_store_spills(s) == 0) {
        uint32_t ne = 0;
        check(s, cov_genome_entry_count(s, &ne));
        if (ne == 0) { S.stats.assign(S.tlen.size(), cov_contig_stats{}); S.hist.clear(); }      // no contig observed: nothing to aggregate, the host scan prints its zero rows
        else {
            S.sep_entries.resize(ne); S.genome_estimates.resize((size_t)ne * R.est.size());
            check(s, cov_fetch_genome_entries(s, S.sep_entries.data()));
            check(s, cov_fetch_genome_estimates(s, S.genome_estimates.data()));
            S.sep_dev = true;
        }
        if (timing_on())
            fprintf(stderr, "[coverm-amd] %s: separator entries from the device (cov_set_genome_runs): %u entries x %zu estimators, %zu bytes\n", S.stoit.c_str(), ne, R.est.size(),
                    S.genome_estimates.size() * sizeof(float) + S.sep_entries.size() * sizeof(cov_genome_entry));
        return;
    }
    // (Run::dev_genome / dev_sep after a spill of the bounded record store: finished contigs are on the host, and so is the aggregation)
    if (R.want & COV_WANT_HIST) {
        S.hist.resize(summ.hist_total); check(s, cov_fetch_hist(s, S.hist.data()));
        if (timing_on()) fprintf(stderr, "[coverm-amd] %s: histogram fetch: %llu bins, %llu bytes\n", S.stoit.c_str(), (unsigned long long)summ.hist_total, (unsigned long long)summ.hist_total * 8ull);
    }
}

// cov_finish of one sample.  Run::dev_genome: the genome results are all the host takes, so the per-contig block stays on the device
// (cov_finish_genomes) — unless the bounded record store spilled: finished contigs are on the host then, and so is the aggregation.
void finish_sample(Run &R, cov_session *s, Sample &S, cov_summary &summ) {
    if ((R.dev_genome || S.sep_set) && cov_store_spills(s) == 0) { check(s, cov_finish_genomes(s, &summ)); return; }
    S.stats.resize(S.tlen.size());
    check(s, cov_finish(s, S.stats.data(), &summ));
}

// --unsorted: the records of the sample grouped by reference on the device, between the last record's arrival and the pair filter / finish
void group_sample(Run &R, cov_session *s, const Sample &S) {
    if (!R.a.unsorted) return;
    uint64_t moved = 0;
    check(s, cov_group_records(s, &moved));
    if (R.a.verbose || timing_on()) {
        double ms = 0; uint32_t launches = 0;
        (void)cov_kernel_ms(s, COV_K_GROUP, &ms, &launches);
        fprintf(stderr, "[coverm-amd] %s: --unsorted: %llu records moved while grouping by reference, %.3f ms on the device\n", S.stoit.c_str(), (unsigned long long)moved, ms);
    }
}

// ---- one sample from its path into a finished session.  cli_route.h decides which reader takes it (and which one takes it next when
// a device reader hands it back); what a reader does is written once below: open + header, prepare_session, feed, after_ingest.

using cli_route::Decision;
using cli_route::Route;
using cli_route::RouteFacts;

template <auto Free> struct FreeWith { template <class T> void operator()(T *p) const { Free(p); } };
using BamHeader = std::unique_ptr<covh_bam_header, FreeWith<covh_bam_header_free>>;
using BamStream = std::unique_ptr<covh_bam_stream, FreeWith<covh_bam_stream_close>>;
using SamText = std::unique_ptr<covh_sam, FreeWith<covh_sam_close>>;
using BamWhole = std::unique_ptr<covh_bam, FreeWith<covh_bam_close>>;
struct OwnedBatch {      // a batch covh_batch_select filled
    cov_batch b;
    OwnedBatch() { memset(&b, 0, sizeof b); }
    OwnedBatch(const OwnedBatch &) = delete;
    OwnedBatch &operator=(const OwnedBatch &) = delete;
    ~OwnedBatch() { if (b.tid) covh_batch_free(&b); }
};

RouteFacts route_facts(const Run &R, const std::string &path, uint32_t span_count) {
    RouteFacts f;
    f.bgzf = is_bgzf(path); f.piped = input_is_pipe(path); f.no_stream = R.a.no_stream; f.per_gene = R.per_gene; f.pair_filter = R.fp; f.span_count = span_count;
    f.no_gpu_ingest = no_gpu_ingest(); f.pair_on_host = pair_on_host(); f.sam_on_host = sam_on_host(); f.genes_decode_on_host = genes_decode_on_host();
    return f;
}

// The thresholds of the reader-stage pair filter, for the device's filter (cov_pair_filter) and the host's (covh_pair_filter)
template <class PairFilter> PairFilter pair_thresholds(const Filter &f, bool fs) {
    PairFilter pf; memset(&pf, 0, sizeof pf);
    pf.filter_single = fs; pf.min_mapq = (uint8_t)f.mapq; pf.min_aligned_length_single = f.len_single;
    pf.min_percent_identity_single = f.pid_single; pf.min_aligned_percent_single = f.pct_single;
    pf.min_aligned_length_pair = f.len_pair; pf.min_percent_identity_pair = f.pid_pair; pf.min_aligned_percent_pair = f.pct_pair;
    return pf;
}

// ---- open + header: one function per reader; each sets the sample's header and returns the handle that owns the reader
BamHeader open_bam_header(Run &R, Sample &S) {
    char err[512] = {0};
    BamHeader hd;
    {   // the first files' headers were read while the HIP runtime came up
        std::unique_lock<std::mutex> lk(R.hdr_mutex);
        auto it = R.hdr_ahead.find(S.path);
        if (it != R.hdr_ahead.end()) {
            std::future<HeaderAhead> fut = std::move(it->second);
            R.hdr_ahead.erase(it);
            lk.unlock();
            HeaderAhead ha = fut.get();
            hd.reset(ha.hd);
            if (!hd && !ha.err.empty()) die(ha.err);
        }
    }
    if (!hd) hd.reset(covh_bam_read_header(S.path.c_str(), err, sizeof err));
    if (!hd) die(err);
    set_header(S, covh_bam_header_n_targets(hd.get()), [&](uint32_t t) { return covh_bam_header_target_name(hd.get(), t); },
               [&](uint32_t t) { return covh_bam_header_target_len(hd.get(), t); });
    return hd;
}

BamStream open_bam_stream(Sample &S, int threads, uint32_t span_index, uint32_t span_count) {
    char err[512] = {0};
    BamStream st(covh_bam_stream_open(S.path.c_str(), threads, span_index, span_count, err, sizeof err));
    if (!st) die(err);
    set_header(S, covh_bam_stream_n_targets(st.get()), [&](uint32_t t) { return covh_bam_stream_target_name(st.get(), t); },
               [&](uint32_t t) { return covh_bam_stream_target_len(st.get(), t); });
    return st;
}

// (the header only when the bytes are text: covh_sam_kind says so)
SamText open_sam(Run &R, Sample &S) {
    char err[512] = {0};
    SamText h;
    {   // a pipe was opened before the sessions existed; ingest() runs in one thread per device: the map is shared, as hdr_ahead is
        std::lock_guard<std::mutex> lk(R.hdr_mutex);
        auto it = R.sam_ahead.find(S.path);
        if (it != R.sam_ahead.end()) { h.reset(it->second); R.sam_ahead.erase(it); }
    }
    if (!h) h.reset(covh_sam_open(S.path.c_str(), err, sizeof err));
    if (!h) die(err);
    if (covh_sam_kind(h.get()) == 0)
        set_header(S, covh_sam_n_targets(h.get()), [&](uint32_t t) { return covh_sam_target_name(h.get(), t); }, [&](uint32_t t) { return covh_sam_target_len(h.get(), t); });
    return h;
}

BamWhole open_bam_whole(Run &R, Sample &S, int threads) {
    char err[512] = {0};
    BamWhole bam(covh_bam_open(S.path.c_str(), threads, R.fp ? 1 : 0, err, sizeof err));
    if (!bam) die(err);
    set_header(S, covh_bam_n_targets(bam.get()), [&](uint32_t t) { return covh_bam_target_name(bam.get(), t); }, [&](uint32_t t) { return covh_bam_target_len(bam.get(), t); });
    return bam;
}

// The session takes the sample's references (and, for the contig-names genome scan, their genomes); a device reader is told what to keep.
// `mask`: the genome table's participation mask when the caller has built the table already (the whole-file reader, before its host work).
void prepare_session(Run &R, cov_session *s, Sample &S, double t0, bool device_reader, std::vector<uint8_t> mask = {}) {
    check(s, cov_set_targets(s, (uint32_t)S.tlen.size(), S.tlen.data()));
    if (R.by_names) { if (mask.empty()) genome_table(R, S, mask); set_genomes_or_mask(R, s, S, mask); }
    if (R.dev_sep) set_genome_runs(R, s, S);
    S.t_open = now() - t0;
    if (!device_reader) return;
    check(s, cov_ingest_want_mates(s, R.fp ? 1 : 0));
    check(s, cov_ingest_want_grouping(s, R.a.unsorted ? 1 : 0));
}

// What a reader left behind: the reason when it hands the file back, else what the tail and the timing lines need
struct Fed {
    bool declined = false; std::string why;
    uint64_t nrec = 0;
    uint64_t prim = 0; bool have_prim = false;      // a pair-mode filter counts every primary record of the input itself (filter.rs:129-131)
    double tm[8] = {0, 0, 0, 0, 0, 0, 0, 0}; bool from_pipe = false;
};

// ---- feed, device ingest: the compressed file goes to HBM, the GPU inflates, finds the records and fills its own store
Fed feed_device_bgzf(Run &R, cov_session *s, Sample &S, const covh_bam_header *hd, int threads, uint32_t span_index, uint32_t span_count) {
    Fed fed; char err[512] = {0};
    // (an assembly's statistics are 128 B x millions of contigs: the array is obtained and touched beside the ingest, not behind it;
    // a std::async future joins in its destructor, so every way out of this function waits for the thread)
    std::future<void> stats_ahead;
    if (S.tlen.size() >= 65536 && !R.dev_genome && !S.sep_set && !R.per_gene) stats_ahead = std::async(std::launch::async, [&S] { S.stats.resize(S.tlen.size()); });
    const int rc = covh_bam_gpu_ingest_span(S.path.c_str(), threads, s, hd, 1, span_index, span_count, &fed.nrec, fed.tm, err, sizeof err);
    if (stats_ahead.valid()) stats_ahead.get();
    if (rc == -2 && span_count > 1) throw SpanUnsorted(err);
    if (rc < 0) die(err);
    if (rc) { fed.declined = true; fed.why = err; }
    return fed;
}

// ---- feed, streamed CPU reader: windows of BGZF blocks inflated and parsed on the host, pushed batch by batch
void feed_cpu_stream(cov_session *s, Sample &S, covh_bam_stream *st, uint32_t span_index, uint32_t span_count) {
    cov_batch b;
    int rc;
    while ((rc = covh_bam_stream_next(st, &b)) == 1) check(s, cov_push_batch(s, &b));
    if (rc == -2 && span_count > 1) throw SpanUnsorted(covh_bam_stream_error(st));
    if (rc < 0) die(covh_bam_stream_error(st));
    S.n_records = covh_bam_stream_n_records(st);
    S.peak_bytes = covh_bam_stream_peak_bytes(st);
    if (timing_on()) {
        double t[5]; covh_bam_stream_timing(st, t);
        fprintf(stderr, "[coverm-amd] %s span %u/%u: stream read %.3fs inflate %.3fs parse %.3fs (coordinator waits: inflate %.3fs parse %.3fs), %llu records, buffers %.0f MB\n",
                S.stoit.c_str(), span_index, span_count, t[0], t[1], t[2], t[3], t[4], (unsigned long long)S.n_records, S.peak_bytes / 1e6);
    }
}

// ---- feed, SAM text (a file or a pipe): decoded on the device window by window as it is read (cov_sam_*)
Fed feed_device_sam(cov_session *s, covh_sam *h, int threads) {
    Fed fed; char err[512] = {0};
    fed.from_pipe = covh_sam_is_pipe(h) != 0;
    const int rc = covh_sam_gpu_ingest(h, threads, s, &fed.nrec, fed.tm, err, sizeof err);
    if (rc < 0) die(err);
    if (rc) { fed.declined = true; fed.why = err; }
    return fed;
}

// ---- whole file on the host: SAM text, files the device ingest declined, --no-stream.  `batch` ends as the records to push — the
// file's, grouped by reference for --unsorted, selected by the host's pair filter — which the gene driver walks afterwards.
struct WholeFile { BamWhole bam; OwnedBatch selected, grouped; };

void select_on_host(Run &R, Sample &S, int threads, WholeFile &whole, cov_batch &batch, Fed &fed) {
    const Args &a = R.a;
    covh_bam *bam = whole.bam.get();
    covh_bam_batch(bam, &batch);
    S.n_records = batch.n_records;
    const int32_t *mtid = covh_bam_mtid(bam); const uint32_t *qoff = covh_bam_qname_off(bam); const char *qnames = covh_bam_qnames(bam);
    std::vector<int32_t> g_mtid; std::vector<uint32_t> g_qoff; std::string g_qnames;
    if (a.unsorted && (R.fp || R.per_gene)) {
        // the host's pair filter and the gene driver walk the whole-file arrays themselves: they see the sequence the device's grouping gives
        uint64_t *order = nullptr, moved = 0;
        if (covh_group_by_reference(batch.tid, batch.n_records, (uint32_t)S.tlen.size(), &order, &moved) != COV_OK) die("--unsorted: grouping the records on the host failed");
        if (moved) {
            const uint64_t n = batch.n_records;
            const int src = covh_batch_select(&batch, order, n, threads, &whole.grouped.b);
            if (src != COV_OK) { covh_free(order); die("--unsorted: grouping the records on the host failed"); }
            if (R.fp && qoff) {
                g_mtid.resize(n); g_qoff.resize(n + 1); g_qoff[0] = 0;
                for (uint64_t j = 0; j < n; j++) { g_mtid[j] = mtid[order[j]]; g_qoff[j + 1] = g_qoff[j] + (qoff[order[j] + 1] - qoff[order[j]]); }
                g_qnames.resize(g_qoff[n]);
                for (uint64_t j = 0; j < n; j++) memcpy(&g_qnames[g_qoff[j]], qnames + qoff[order[j]], g_qoff[j + 1] - g_qoff[j]);
                mtid = g_mtid.data(); qoff = g_qoff.data(); qnames = g_qnames.data();
            }
            batch = whole.grouped.b;
        }
        covh_free(order);
        if (a.verbose || timing_on()) fprintf(stderr, "[coverm-amd] %s: --unsorted: %llu records moved while grouping by reference on the host\n", S.stoit.c_str(), (unsigned long long)moved);
    }
    if (R.fp) {      // the reader-stage pair filter, on the host (Run::fp is only ever set when a filter is on: Filter::doing_filtering)
        for (uint64_t i = 0; i < batch.n_records; i++) if (!(batch.flag[i] & 0x900)) fed.prim++;   // filter.rs:129-131
        fed.have_prim = true;
        const covh_pair_filter pf = pair_thresholds<covh_pair_filter>(R.f, R.fs);
        uint64_t *order = nullptr, n_order = 0;
        const int prc = covh_pair_mode_order(&batch, mtid, qoff, qnames, &pf, threads, &order, &n_order);
        if (prc == COV_ERR_NM_MISSING) die("Mapping record encountered that does not have an 'NM' auxiliary tag in the SAM/BAM format");
        if (prc != COV_OK) die(prc == COV_ERR_NM_BADTYPE ? "Unexpected data type of NM aux tag" : "pair filter failed");
        const int src = covh_batch_select(&batch, order, n_order, threads, &whole.selected.b);
        covh_free(order);
        if (src != COV_OK) die("pair filter: selection failed");
        batch = whole.selected.b;
    }
}

// ---- behind the last record of every reader: --unsorted grouping; behind a device reader, the reader-stage pair filter (filter.rs:117-228)
// on the device, over the mate reference + read-name hash the ingest kept per record.  It may hand the file back, as the ingest may.
void after_ingest(Run &R, cov_session *s, const Sample &S, Route route, Fed &fed) {
    group_sample(R, s, S);      // (nothing moves when the host grouped the arrays, or its pair filter selected from them)
    if (!R.fp || (route != Route::DeviceBgzf && route != Route::DeviceSam)) return;
    const double tp0 = now();
    const cov_pair_filter pf = pair_thresholds<cov_pair_filter>(R.f, R.fs);
    uint64_t nsel = 0;
    const cov_status prc = cov_pair_filter_apply(s, &pf, &nsel, &fed.prim);
    if (prc == COV_ERR_INGEST_FALLBACK) { fed.declined = true; fed.why = cov_last_error(s); return; }
    check(s, prc);
    fed.have_prim = true;
    if (timing_on() && route == Route::DeviceBgzf)
        fprintf(stderr, "[coverm-amd] %s: pair filter on the device: %llu of %llu records selected, %.3fs\n", S.stoit.c_str(), (unsigned long long)nsel, (unsigned long long)fed.nrec, now() - tp0);
}

void report_device_reader(cov_session *s, const Sample &S, Route route, const Fed &fed, uint32_t span_index, uint32_t span_count) {
    const double *tm = fed.tm;
    if (route == Route::DeviceBgzf) {
        cov_ingest_stats ist{};
        (void)cov_ingest_last_stats(s, &ist);
        fprintf(stderr, "[coverm-amd] %s span %u/%u: device ingest: first upload after %.3fs, file read %.3fs, staging waits %.3fs, header walk %.3fs, feed calls %.3fs, inflate tail + parse %.3fs, total %.3fs, %llu records, long records %llu, repaired starts %llu, longest hop %llu, bytes from %s\n",
                S.stoit.c_str(), span_index, span_count, tm[4], tm[0], tm[1], tm[5], tm[6], tm[2], tm[3], (unsigned long long)fed.nrec,
                (unsigned long long)ist.long_records, (unsigned long long)ist.repaired_starts, (unsigned long long)ist.max_hop_records,
                tm[7] == 2 ? "the mapped file (registered up front)" : tm[7] == 1 ? "the mapped file" : tm[7] == 3 ? "staging slots (copied from the mapping)" : "staging slots (pread)");
        return;
    }
    double ms = 0; uint32_t launches = 0;
    (void)cov_kernel_ms(s, COV_K_SAM, &ms, &launches);
    fprintf(stderr, "[coverm-amd] %s: device SAM decode from %s: read %.3fs, slot waits %.3fs, feed calls %.3fs, total %.3fs, %llu records, decode kernels %.3f ms\n",
            S.stoit.c_str(), fed.from_pipe ? "a pipe" : "the file", tm[0], tm[1], tm[2], tm[3], (unsigned long long)fed.nrec, ms);
}

// ---- --gff behind a device reader: the records the gene driver needs on the host (per-read vectors, genes.rs:182-344) come BACK from the
// session's store — 24 B per record + CIGAR words over PCIe instead of a whole-file decode on the host
struct HostRecords { std::vector<int32_t> tid, pos; std::vector<uint16_t> flag; std::vector<uint8_t> mapq, nmk; std::vector<uint32_t> nm, lseq, coff, cig; };

void records_back(cov_session *s, HostRecords &hr, cov_batch &batch) {
    uint64_t n = 0, nc = 0;
    check(s, cov_copy_records(s, nullptr, &n, &nc));
    hr.tid.resize(n); hr.pos.resize(n); hr.flag.resize(n); hr.mapq.resize(n); hr.nmk.resize(n); hr.nm.resize(n); hr.lseq.resize(n);
    hr.coff.resize(n + 1); hr.cig.resize(nc + 1);
    batch.tid = hr.tid.data(); batch.pos = hr.pos.data(); batch.flag = hr.flag.data(); batch.mapq = hr.mapq.data(); batch.nm = hr.nm.data();
    batch.nm_kind = hr.nmk.data(); batch.l_seq = hr.lseq.data(); batch.cigar_off = hr.coff.data(); batch.cigar = hr.cig.data(); batch.n_records = n;
    check(s, cov_copy_records(s, &batch, nullptr, nullptr));
    if (n == 0) hr.coff[0] = 0;
}

// COVERM_GENE_READS_ON_HOST: behind a device reader the records come back and the gene driver's record pass runs on the host, as it did
// before cov_interval_reads_compute — the cross-check of the device aggregates
bool gene_reads_on_host() { static const bool v = getenv("COVERM_GENE_READS_ON_HOST") != nullptr; return v; }

// genes.rs:182-344: per-gene reductions over this sample's depth, while the session holds it.  device_reads: the store holds the sample
// (a device reader filled it) and the per-read numbers of every gene come from there, 32 bytes per gene; the records come back only
// when their starts decrease inside a contig (--unsorted) or COVERM_GENE_READS_ON_HOST asks for it.
void gene_coverage(Run &R, cov_session *s, Sample &S, cov_batch &batch, HostRecords &hr, bool device_reads, bool report) {
    const Args &a = R.a;
    std::lock_guard<std::mutex> lk(R.taker_mutex);
    const covh_header gh = S.header();
    covh_genome_namer nm; memset(&nm, 0, sizeof nm);
    std::vector<const char *> gn;
    for (auto &g : R.genomes) gn.push_back(g.c_str());
    if (!R.contig) {
        nm.mode = a.single_genome ? 1 : a.have_separator ? 2 : 3;
        nm.separator = (uint8_t)a.separator;
        nm.genome_of_tid = S.genome_of_tid.data(); nm.genome_names = gn.data();
    }
    auto depth_cb = [](void *ctx, uint32_t tid, int32_t *out) -> int { return (int)cov_copy_depth((cov_session *)ctx, tid, out); };
    cov_session *const reductions = getenv("COVERM_GENES_ON_HOST") ? nullptr : s;
    if (device_reads) {
        const char *why = "COVERM_GENE_READS_ON_HOST";
        if (!gene_reads_on_host()) {
            int sorted = 0;
            const int grc = covh_gene_coverage_reads(&gh, R.genes, &nm, S.stoit.c_str(), covh_session_interval_reads, s, reductions, depth_cb, s, S.prim, R.taker,
                                                     R.est.data(), R.est.size(), !a.no_zeros, &S.gene_rm, &sorted);
            if (grc == COV_ERR_HIP || grc == COV_ERR_STATE) die(cov_last_error(s));
            if (grc == COV_ERR_NM_MISSING || grc == COV_ERR_NM_BADTYPE) die(cov_last_error(s));
            if (grc != COV_OK) die(covh_last_error());
            if (sorted) {
                if (report) {
                    double ms = 0; uint32_t launches = 0;
                    (void)cov_kernel_ms(s, COV_K_GENE_READS, &ms, &launches);
                    fprintf(stderr, "[coverm-amd] %s: --gff over the device ingest: per-gene read aggregates on the device (%zu genes, %.3f kernels ms)\n", S.stoit.c_str(),
                            covh_genes_count(R.genes), ms);
                }
                return;
            }
            why = "starts decrease inside a reference";      // nothing was written: the record pass takes the sample
        }
        records_back(s, hr, batch);
        if (report)
            fprintf(stderr, "[coverm-amd] %s: --gff over the device ingest: %llu records came back from the store (%s)\n", S.stoit.c_str(), (unsigned long long)batch.n_records, why);
    }
    const int grc = covh_gene_coverage(&gh, R.genes, &nm, S.stoit.c_str(), &batch, &R.cfg, reductions, depth_cb, s,
                                       S.prim, R.taker, R.est.data(), R.est.size(), !a.no_zeros, &S.gene_rm);
    if (grc == COV_ERR_HIP || grc == COV_ERR_STATE) die(cov_last_error(s));
    if (grc != COV_OK) die(covh_last_error());
}

// Decode + push + finish of one BAM (or one tid span of it) on one session.  Leaves the session finished.
void ingest(Run &R, cov_session *s, Sample &S, int threads, uint32_t span_index, uint32_t span_count) {
    const RouteFacts facts = route_facts(R, S.path, span_count);
    Decision d = cli_route::first_route(facts);
    S.stoit = stoit_of(S.path);
    const double t0 = now();
    WholeFile whole; HostRecords hr;
    cov_batch batch; memset(&batch, 0, sizeof batch);      // the sample's records on the host, for the gene driver
    Fed fed;
    for (;;) {
        if (d.refused()) die(d.refusal);
        check(s, cov_reset(s));
        fed = Fed(); S.streamed = d.route == Route::CpuStream;
        switch (d.route) {
        case Route::DeviceBgzf: {
            const BamHeader hd = open_bam_header(R, S);
            prepare_session(R, s, S, t0, true);
            fed = feed_device_bgzf(R, s, S, hd.get(), threads, span_index, span_count);
            break;
        }
        case Route::CpuStream: {
            const BamStream st = open_bam_stream(S, threads, span_index, span_count);
            prepare_session(R, s, S, t0, false);
            feed_cpu_stream(s, S, st.get(), span_index, span_count);
            break;
        }
        case Route::DeviceSam: {
            const SamText h = open_sam(R, S);
            if (covh_sam_kind(h.get()) != 0) { fed.declined = true; fed.why = "the file is not text (NUL bytes in its first piece)"; break; }
            prepare_session(R, s, S, t0, true);
            fed = feed_device_sam(s, h.get(), threads);
            break;
        }
        case Route::HostWhole: {
            whole.bam = open_bam_whole(R, S, threads);
            std::vector<uint8_t> mask;
            if (R.by_names) genome_table(R, S, mask);      // (its refusal comes before those of the host's pair filter)
            select_on_host(R, S, threads, whole, batch, fed);
            prepare_session(R, s, S, t0, false, std::move(mask));
            check(s, cov_push_batch(s, &batch));
            break;
        }
        }
        if (!fed.declined) after_ingest(R, s, S, d.route, fed);
        if (!fed.declined) break;
        // the reader handed the file back: the next one takes it, on the session as cov_reset leaves it
        const bool sam = d.route == Route::DeviceSam;
        if (!sam && timing_on()) fprintf(stderr, "[coverm-amd] %s: %s\n", S.stoit.c_str(), fed.why.c_str());
        d = cli_route::after_decline(d.route, facts, S.stoit, fed.why);
        if (sam && !d.refused() && (R.a.verbose || timing_on()))
            fprintf(stderr, "[coverm-amd] %s: SAM text handed to the host route (whole file): %s\n", S.stoit.c_str(), fed.why.c_str());
    }
    if (d.route == Route::DeviceBgzf || d.route == Route::DeviceSam) {
        S.n_records = fed.nrec; S.device_ingest = true;
        if (timing_on()) report_device_reader(s, S, d.route, fed, span_index, span_count);
    }
    S.t_ingest = now() - t0;
    cov_summary summ;
    finish_sample(R, s, S, summ);
    fetch_results(R, s, S, summ);
    S.prim = fed.have_prim ? fed.prim : summ.num_detected_primary_alignments;
    if (R.per_gene) gene_coverage(R, s, S, batch, hr, S.device_ingest, timing_on());
    S.t_finish = now() - t0 - S.t_ingest;
}

// --genome-definition: a genome name and a contig name per line, into R.genomes / R.c2g
void read_genome_definition(Run &R) {
    const Args &a = R.a;
    if (a.genome_definition.empty()) die("genome mode over BAM files needs --separator, --single-genome or --genome-definition");
    FILE *fh = fopen(a.genome_definition.c_str(), "r");
    if (!fh) die("cannot open " + a.genome_definition);
    struct FClose { FILE *f; ~FClose() { fclose(f); } } fclose_{fh};
    std::vector<char> linebuf(1 << 16);
    char *line = linebuf.data();
    std::unordered_map<std::string, int32_t> gi;
    auto is_ws = [](unsigned char ch) { return ch == ' ' || (ch >= 9 && ch <= 13); };
    while (fgets(line, (int)linebuf.size(), fh)) {   // read_genome_definition_file, genome_parsing.rs:71-141
        std::string l(line);
        if (!l.empty() && l.back() == '\n') l.pop_back();
        if (!l.empty() && l.back() == '\r') l.pop_back();
        const size_t t = l.find('\t');
        if (t == std::string::npos || l.find('\t', t + 1) != std::string::npos)   // blank lines included (:116-124)
            die("The line \"" + l + "\" in the genome definition file is not a genome name and contig name separated by a tab");
        std::string g = l.substr(0, t);
        { size_t x = 0, y = g.size(); while (x < y && is_ws((unsigned char)g[x])) x++; while (y > x && is_ws((unsigned char)g[y - 1])) y--; g = g.substr(x, y - x); }
        size_t x = t + 1;
        while (x < l.size() && is_ws((unsigned char)l[x])) x++;
        size_t y = x;
        while (y < l.size() && !is_ws((unsigned char)l[y])) y++;
        if (x == y) die("Failed to split contig name by whitespace in genome definition file");
        const std::string c = l.substr(x, y - x);                                  // first token: comments after it are dropped
        auto it = gi.find(g);
        if (it == gi.end()) { it = gi.emplace(g, (int32_t)R.genomes.size()).first; R.genomes.push_back(g); }
        auto cit = R.c2g.find(c);
        if (cit != R.c2g.end() && cit->second != it->second) die("The contig name '" + c + "' was assigned to multiple genomes");
        if (cit == R.c2g.end()) R.c2g[c] = it->second;
    }
}

// COVERM_CLI_TIMING: the resident set of the process and its largest mappings
void report_resident_set() {
    // where the resident set comes from (VmHWM = peak; RssShmem counts page-locked / device-visible mappings of the HIP runtime)
    if (FILE *ps = fopen("/proc/self/status", "r")) {
        char ln[256];
        while (fgets(ln, sizeof ln, ps))
            if (!strncmp(ln, "VmHWM", 5) || !strncmp(ln, "VmRSS", 5) || !strncmp(ln, "RssAnon", 7) || !strncmp(ln, "RssFile", 7) || !strncmp(ln, "RssShmem", 8)) {
                ln[strcspn(ln, "\n")] = 0;
                fprintf(stderr, "[coverm-amd] %s\n", ln);
            }
        fclose(ps);
    }
    // ... and its eight largest mappings (what the kernel has to take apart when the process ends)
    if (FILE *sm = fopen("/proc/self/smaps", "r")) {
        struct M { unsigned long long rss_kb, size_kb; std::string what; };
        std::vector<M> ms;
        char ln[512]; std::string cur; unsigned long long size_kb = 0;
        while (fgets(ln, sizeof ln, sm)) {
            unsigned long long a, b2, v;
            if (sscanf(ln, "%llx-%llx ", &a, &b2) == 2 && strchr(ln, '-') && strchr(ln, '-') < ln + 17) {
                ln[strcspn(ln, "\n")] = 0;
                const char *path = strchr(ln, '/'); const char *br = strchr(ln, '[');
                cur = path ? path : br ? br : "(anonymous)"; size_kb = (b2 - a) >> 10;
            } else if (sscanf(ln, "Rss: %llu kB", &v) == 1) ms.push_back({v, size_kb, cur});
        }
        fclose(sm);
        std::sort(ms.begin(), ms.end(), [](const M &x, const M &y) { return x.rss_kb > y.rss_kb; });
        for (size_t i = 0; i < ms.size() && i < 8; i++)
            fprintf(stderr, "[coverm-amd] mapping %zu: %llu MB resident of %llu MB, %s\n", i, ms[i].rss_kb >> 10, ms[i].size_kb >> 10, ms[i].what.c_str());
    }
}

// Span mode: the per-contig result blocks of one file's spans meet on the first device through one RCCL gather (cov_gather) and become one sample
void merge_spans(Run &R, std::vector<cov_session *> &sess, const std::vector<Sample> &part, Sample &S) {
    const size_t nd = part.size();
    const std::vector<covh_estimator> &est = R.est;
    S.stoit = part[0].stoit; S.names_blob = part[0].names_blob; S.name_off = part[0].name_off; S.tlen = part[0].tlen;
    S.genome_of_tid = part[0].genome_of_tid; S.streamed = true;
    const uint32_t nt = (uint32_t)S.tlen.size();
    check(sess[0], cov_gather(sess.data(), (uint32_t)nd, 0));
    S.stats.assign(nt, cov_contig_stats{});
    if (R.dev_est) S.estimates.assign((size_t)nt * est.size(), 0.0f);
    std::vector<cov_contig_stats> tmp(nt);
    for (size_t d = 0; d < nd; d++) {
        cov_summary summ;
        check(sess[0], cov_gathered(sess[0], (uint32_t)d, tmp.data(), &summ));
        S.prim += summ.num_detected_primary_alignments; S.n_records += summ.n_records;
        S.peak_bytes = std::max(S.peak_bytes, part[d].peak_bytes);
        S.t_ingest = std::max(S.t_ingest, part[d].t_ingest); S.t_finish = std::max(S.t_finish, part[d].t_finish);
        for (uint32_t t = 0; t < nt; t++) {
            if (tmp[t].n_pass == 0) continue;
            if (S.stats[t].n_pass != 0) die("internal error: contig " + S.target_name(t) + " was seen by two spans");
            S.stats[t] = tmp[t];
            if (R.dev_est) {                // the floats stay with the rank that evaluated them, like the histogram bins
                std::copy(part[d].estimates.begin() + (size_t)t * est.size(), part[d].estimates.begin() + (size_t)(t + 1) * est.size(), S.estimates.begin() + (size_t)t * est.size());
            } else if (R.want & COV_WANT_HIST) {   // histogram bins stay with the rank that built them: re-based into one array
                S.stats[t].hist_off = S.hist.size();
                S.hist.insert(S.hist.end(), part[d].hist.begin() + tmp[t].hist_off, part[d].hist.begin() + tmp[t].hist_off + tmp[t].hist_len);
            }
        }
    }
}

// `coverm filter` (bin/coverm.rs:408-472): every input BAM through ReferenceSortedBamFilter into its output BAM.  Host code in the
// reference and here: the work is rewriting a BAM (inflate, select, deflate), which no pass over coverage touches.  The thresholds
// are FilterParameters::generate_from_clap's (coverm.rs:1659-1678); filter_out = !--inverse.
int run_filter(int argc, char **argv) {
    std::vector<std::string> in, out;
    FilterArgs fa;
    bool inverse = false;
    int threads = 1;
    auto collect = [&](int &i, std::vector<std::string> &dst) { while (i + 1 < argc && argv[i + 1][0] != '-') dst.push_back(argv[++i]); };
    for (int i = 2; i < argc; i++) {
        const std::string k = argv[i];
        auto val = [&]() -> const char * { if (i + 1 >= argc) die("missing value for " + k); return argv[++i]; };
        if (k == "-b" || k == "--bam-files") collect(i, in);
        else if (k == "-o" || k == "--output-bam-files") collect(i, out);
        else if (k == "--inverse") inverse = true;
        else if (parse_filter_flag(k, val, fa)) {}
        else if (k == "-t" || k == "--threads") threads = (int)parse_uint(k, val(), 65535);
        else if (k == "-v" || k == "--verbose" || k == "-q" || k == "--quiet") {}
        else if (k == "--unsorted") die("filter does not take --unsorted: it streams its input in bounded memory and copies records byte for byte, in the input's order (sort the file by reference first)");
        else die("unknown argument " + k);
    }
    if (in.empty()) die("--bam-files is required");
    if (in.size() != out.size()) die("The number of input BAM files must be the same as the number output");     // coverm.rs:422-425
    const Filter f = resolve_filter(fa);
    bool fs = false, fp = false;
    f.mode(fs, fp);
    const covh_pair_filter pf = pair_thresholds<covh_pair_filter>(f, fs);
    for (size_t k = 0; k < in.size(); k++) {
        char err[512] = {0};
        uint64_t n_in = 0, n_out = 0;
        if (covh_bam_filter_file(in[k].c_str(), out[k].c_str(), &pf, fp ? 1 : 0, f.supp ? 1 : 0, f.sec ? 1 : 0, inverse ? 0 : 1, 6, std::max(1, threads), &n_in, &n_out, err,
                                 sizeof err) != 0)
            die(err);
        if (timing_on()) fprintf(stderr, "[coverm-amd] filter %s -> %s: %llu of %llu records\n", in[k].c_str(), out[k].c_str(), (unsigned long long)n_out, (unsigned long long)n_in);
    }
    return 0;
}

// coverm-amd depth: the per-base depth of every reference as a bedGraph, one track per sample.  The samples go through `contig`'s routes,
// prepare_session, ingest and after_ingest (ingest() above) on one device, one after the other; behind a sample's cov_finish its depth runs
// come from the device chunk by chunk (covh_depth_runs_write) and are written before the next sample's records replace the store.
int run_depth(int argc, char **argv) {
    const double t_main0 = now();
    Run R;
    Args &a = R.a;
    a.mode = "contig";
    uint32_t bin_size = 0;      // --bin-size: one line per fixed window (covh_depth_bins_write) instead of one per depth run
    int bin_value = COVH_BIN_MEAN;
    bool have_bin_value = false;
    std::string regions_path;      // --regions: one line per region of a BED file (covh_depth_regions_write)
    std::string quantize, thresholds;      // --quantize: one line per stretch of one depth class; --thresholds: per region or window, the bases at or above each
    int32_t cuts[COV_DEPTH_MAX_CUTS] = {0}, thr[COV_DEPTH_MAX_CUTS] = {0};
    uint32_t n_cuts = 0, n_thr = 0;
    int open_end = 0;
    auto collect = [&](int &i, std::vector<std::string> &dst) { while (i + 1 < argc && (argv[i + 1][0] != '-' || !argv[i + 1][1])) dst.push_back(argv[++i]); };
    static const char *const REFUSED[] = {"-m", "--methods", "--gff", "--gff-feature-type", "--devices", "--contig-end-exclusion", "--min-covered-fraction", "--trim-min", "--trim-max",
                                          "--output-format", "-s", "--separator", "--single-genome", "--genome-definition", "-f", "--genome-fasta-files", "-d",
                                          "--genome-fasta-directory", "-x", "--genome-fasta-extension", "--genome-fasta-list", "--use-full-contig-names"};
    for (int i = 2; i < argc; i++) {
        const std::string k = argv[i];
        auto val = [&]() -> const char * { if (i + 1 >= argc) die("missing value for " + k); return argv[++i]; };
        for (const char *r : REFUSED)
            if (k == r) {
                if (k == "--devices") die("the argument '--devices' cannot be used with 'depth': a sample's depth runs come from one device (--device N)");
                if (k == "--contig-end-exclusion") die("the argument '--contig-end-exclusion' cannot be used with 'depth': the track is the depth of every base, the exclusion belongs to the estimators");
                if (k == "-m" || k == "--methods") die("the argument '" + k + "' cannot be used with 'depth': it writes the per-base depth itself, not a method's value (coverm-amd contig -m ...)");
                if (k == "--gff" || k == "--gff-feature-type") die("the argument '" + k + "' cannot be used with 'depth' (per-gene coverage: coverm-amd contig --gff)");
                die("the argument '" + k + "' cannot be used with 'depth': it belongs to coverm-amd contig / genome (the track has one line per depth run of a reference)");
            }
        if (k == "-b" || k == "--bam-files") collect(i, a.bams);
        else if (k == "-o" || k == "--output-file") a.output_file = val();
        else if (k == "--no-zeros") a.no_zeros = true;
        else if (k == "--bin-size") {
            bin_size = (uint32_t)parse_uint(k, val(), 0x7fffffffull);
            if (bin_size == 0) die("invalid value '0' for '" + k + "'");
        } else if (k == "--regions") regions_path = val();
        else if (k == "--quantize") {
            quantize = val();
            if (covh_depth_quantize_parse(quantize.c_str(), cuts, &n_cuts, &open_end) != COV_OK) die("invalid value for '--quantize': " + std::string(covh_last_error()));
        } else if (k == "--thresholds") {
            thresholds = val();
            if (covh_depth_thresholds_parse(thresholds.c_str(), thr, &n_thr) != COV_OK) die("invalid value for '--thresholds': " + std::string(covh_last_error()));
        }
        else if (k == "--bin-value") {
            const std::string v = val();
            static const char *const KINDS[] = {"mean", "sum", "min", "max", "covered"};      // covh_bin_value
            bin_value = -1;
            for (int j = 0; j < 5; j++) if (v == KINDS[j]) bin_value = j;
            if (bin_value < 0) die("invalid value '" + v + "' for '" + k + "' (mean, sum, min, max or covered)");
            have_bin_value = true;
        }
        else if (parse_filter_flag(k, val, a.filter)) {}
        else if (k == "-t" || k == "--threads") a.threads = (int)parse_uint(k, val(), 65535);
        else if (k == "--device") a.devices.assign(1, (int)parse_uint(k, val(), 1023));
        else if (k == "--no-stream") a.no_stream = true;
        else if (k == "--unsorted") a.unsorted = true;
        else if (k == "-v" || k == "--verbose") a.verbose = true;
        else if (k == "-q" || k == "--quiet") {}
        else die("unknown argument " + k);
    }
    if (!regions_path.empty() && bin_size) die("the argument '--regions' cannot be used with '--bin-size': a line per region of the BED file, or a line per fixed window");
    if (n_cuts) {
        if (!regions_path.empty()) die("the argument '--quantize' cannot be used with '--regions': a line per stretch of one depth class, or a line per region of the BED file");
        if (bin_size) die("the argument '--quantize' cannot be used with '--bin-size': a line per stretch of one depth class, or a line per fixed window");
        if (have_bin_value) die("the argument '--quantize' cannot be used with '--bin-value': the track prints the class of a stretch, not a value of a window or region");
        if (n_thr) die("the argument '--quantize' cannot be used with '--thresholds': the thresholds count the bases of a region or window (--regions, --bin-size)");
        if (a.no_zeros) die("the argument '--quantize' cannot be used with '--no-zeros': leave the zero class out of the spec instead (--quantize 1:... prints no line for depth 0)");
    }
    if (n_thr && !bin_size && regions_path.empty())
        die("the argument '--thresholds' needs '--regions' or '--bin-size': it counts, per region or window, the bases at or above each threshold");
    if (n_thr && have_bin_value) die("the argument '--thresholds' cannot be used with '--bin-value': the counts are the value columns");
    if (have_bin_value && !bin_size && regions_path.empty())
        die("the argument '--bin-value' needs '--bin-size' or '--regions': it picks what is printed per bin or region (coverm-amd depth --bin-size N --bin-value ...)");
    if (a.bams.empty()) die("--bam-files is required (read mapping is out of scope for this engine)");
    if (a.devices.empty()) a.devices.push_back(0);
    {
        size_t n_stdin = 0, n_pipe = 0;
        for (auto &b : a.bams) { n_stdin += b == "-"; n_pipe += input_is_pipe(b); }
        if (n_stdin > 1) die("'-b -' (standard input) can be given once only");
        if (n_pipe && a.no_stream) die("--no-stream reads the whole file on the host, which a pipe ('-b -', a FIFO) does not allow: write the stream to a file first");
    }
    R.contig = true;
    Filter &f = R.f;
    f = resolve_filter(a.filter);
    if (f.doing_filtering()) f.mode(R.fs, R.fp);
    cov_config &cfg = R.cfg; memset(&cfg, 0, sizeof cfg);
    cfg.include_improper_pairs = f.improper; cfg.include_supplementary = f.supp;
    cfg.include_secondary = f.sec; cfg.min_mapq = 255; cfg.contig_end_exclusion = 0; cfg.want = 0;
    if (f.doing_filtering() && R.fs && !R.fp) {
        cfg.filter_single = 1; cfg.min_mapq = (uint8_t)f.mapq; cfg.min_aligned_length = f.len_single;
        cfg.min_percent_identity = f.pid_single; cfg.min_aligned_percent = f.pct_single;
    }
    for (auto &b : a.bams) {      // a pipe's format is told from its first bytes read, before any device work
        if (!input_is_pipe(b) || R.sam_ahead.count(b)) continue;
        char e[512] = {0};
        covh_sam *h = covh_sam_open(b.c_str(), e, sizeof e);
        if (!h) die(e);
        R.sam_ahead.emplace(b, h);
        if (covh_sam_kind(h) == 1) die("BAM from a pipe is not supported yet; SAM text is (e.g. `samtools view -h`), or pass the file's path");
        if (covh_sam_kind(h) == 2) die(stoit_of(b) + ": the stream is neither SAM text nor BAM (NUL bytes in its first piece)");
    }
    covh_bed *bed = nullptr;      // read and syntax-checked before any device work; resolved per sample, against its header
    struct BedFree { covh_bed *&b; ~BedFree() { covh_bed_free(b); } } bed_free{bed};
    if (!regions_path.empty() && !(bed = covh_bed_read(regions_path.c_str()))) die(covh_last_error());
    struct SamDrain { Run &R; ~SamDrain() { for (auto &kv : R.sam_ahead) covh_sam_close(kv.second); R.sam_ahead.clear(); } } sam_drain{R};
    FILE *out = a.output_file.empty() || a.output_file == "-" ? stdout : fopen(a.output_file.c_str(), "w");
    if (!out) die("Failed to create output file: " + a.output_file);
    struct OutClose { FILE *f; ~OutClose() { if (f != stdout) fclose(f); else fflush(stdout); } } out_close{out};
    std::vector<cov_session *> sess(1, nullptr);
    struct SessFree { std::vector<cov_session *> &v; ~SessFree() { if (!g_skip_teardown.load()) for (auto *s : v) if (s) cov_destroy(s); } } sess_free{sess};
    {
        cov_config c = cfg; c.device = a.devices[0];
        long long prep = 1;
        (void)covknob::get("ingest_prepare", prep);
        if (!no_gpu_ingest() && prep) c.want |= COV_WANT_INGEST;
        if (cov_create(&c, &sess[0]) != COV_OK) die(cov_last_error(nullptr));
    }
    cov_session *s = sess[0];
    covh_bam_set_pinned(1);
    covh_bam_set_release_staging(0);
    if (a.bams.size() > 1) covh_bam_set_buffer_cache(1);
    covh_bam_set_concurrent_feeders(1);
    (void)cov_bind_thread_to_device_node(a.devices[0]);
    const double t_sessions = now();
    for (auto &b : a.bams) {
        Sample S; S.path = b;
        ingest(R, s, S, std::max(1, a.threads), 0, 1);
        const double t_runs0 = now();
        if (n_cuts) fprintf(out, "track name=\"%s\" description=\"depth classes %s\"\n", S.stoit.c_str(), quantize.c_str());      // (the label column is not numeric: no bedGraph)
        else fprintf(out, "track type=bedGraph name=\"%s\"\n", S.stoit.c_str());
        if (n_thr) {
            fputs("#thresholds", out);
            for (uint32_t j = 0; j < n_thr; j++) fprintf(out, "\t%d", thr[j]);
            fputc('\n', out);
        }
        fflush(out);
        const covh_header hdr = S.header();
        if (n_cuts) {
            uint64_t n_runs = 0;
            if (covh_depth_class_runs_write(s, &hdr, cuts, n_cuts, open_end, std::max(1, a.threads), fileno(out), &n_runs) != COV_OK) die(covh_last_error());
            if (timing_on())
                fprintf(stderr, "[coverm-amd] sample %s: open %.3fs, ingest (decode+push) %.3fs, finish %.3fs, %llu records; depth classes %s: %llu runs computed, fetched and written in %.3fs\n",
                        S.stoit.c_str(), S.t_open, S.t_ingest, S.t_finish, (unsigned long long)S.n_records, quantize.c_str(), (unsigned long long)n_runs, now() - t_runs0);
            continue;
        }
        if (n_thr) {
            uint64_t n_lines = 0;
            const int rc = bed ? covh_depth_regions_counts_write(s, &hdr, bed, thr, n_thr, a.no_zeros ? 1 : 0, std::max(1, a.threads), fileno(out), &n_lines)
                               : covh_depth_bins_counts_write(s, &hdr, bin_size, thr, n_thr, a.no_zeros ? 1 : 0, std::max(1, a.threads), fileno(out), &n_lines);
            if (rc != COV_OK) die(covh_last_error());
            if (timing_on())
                fprintf(stderr, "[coverm-amd] sample %s: open %.3fs, ingest (decode+push) %.3fs, finish %.3fs, %llu records; depth thresholds %s: %llu %s computed, fetched and written in %.3fs\n",
                        S.stoit.c_str(), S.t_open, S.t_ingest, S.t_finish, (unsigned long long)S.n_records, thresholds.c_str(), (unsigned long long)n_lines, bed ? "regions" : "windows",
                        now() - t_runs0);
            continue;
        }
        if (bed) {
            uint64_t n_regions = 0;
            if (covh_depth_regions_write(s, &hdr, bed, bin_value, a.no_zeros ? 1 : 0, std::max(1, a.threads), fileno(out), &n_regions) != COV_OK) die(covh_last_error());
            if (timing_on())
                fprintf(stderr, "[coverm-amd] sample %s: open %.3fs, ingest (decode+push) %.3fs, finish %.3fs, %llu records; depth regions: %llu regions computed, fetched and written in %.3fs\n",
                        S.stoit.c_str(), S.t_open, S.t_ingest, S.t_finish, (unsigned long long)S.n_records, (unsigned long long)n_regions, now() - t_runs0);
            continue;
        }
        if (bin_size) {
            uint64_t n_bins = 0;
            if (covh_depth_bins_write(s, &hdr, bin_size, bin_value, a.no_zeros ? 1 : 0, std::max(1, a.threads), fileno(out), &n_bins) != COV_OK) die(covh_last_error());
            if (timing_on())
                fprintf(stderr, "[coverm-amd] sample %s: open %.3fs, ingest (decode+push) %.3fs, finish %.3fs, %llu records; depth bins of %u: %llu bins computed, fetched and written in %.3fs\n",
                        S.stoit.c_str(), S.t_open, S.t_ingest, S.t_finish, (unsigned long long)S.n_records, bin_size, (unsigned long long)n_bins, now() - t_runs0);
            continue;
        }
        uint64_t n_runs = 0;
        if (covh_depth_runs_write(s, &hdr, a.no_zeros ? 1 : 0, std::max(1, a.threads), fileno(out), &n_runs) != COV_OK) die(covh_last_error());
        if (timing_on())
            fprintf(stderr, "[coverm-amd] sample %s: open %.3fs, ingest (decode+push) %.3fs, finish %.3fs, %llu records; depth runs: %llu runs computed, fetched and written in %.3fs\n",
                    S.stoit.c_str(), S.t_open, S.t_ingest, S.t_finish, (unsigned long long)S.n_records, (unsigned long long)n_runs, now() - t_runs0);
    }
    if (timing_on()) fprintf(stderr, "[coverm-amd] main: arguments + device session %.3fs, samples %.3fs\n", t_sessions - t_main0, now() - t_sessions);
    return 0;
}

int run_cli(int argc, char **argv) {
    const double t_main0 = now();
    Run R;
    Args &a = R.a;
    if (argc >= 2 && !strcmp(argv[1], "filter")) return run_filter(argc, argv);
    if (argc >= 2 && !strcmp(argv[1], "depth")) return run_depth(argc, argv);
    if (argc < 2 || (strcmp(argv[1], "contig") && strcmp(argv[1], "genome"))) {
        fprintf(stderr, "usage: coverm-amd contig|genome -b <bam>... [-m <methods>...] [options]   (see src/cli.rs of CoverM for the flags; "
                        "engine flags: --device N | --devices a,b,..., --no-stream, --unsorted)\n"
                        "       --unsorted: the BAM / SAM files need not be sorted by reference (a mapper's output in read order).  The records of a file are\n"
                        "       grouped on the device: references in header order, records without a reference last, the file's order kept inside a\n"
                        "       reference.  The result is the result for the file with its records in that order: equal to the table of the\n"
                        "       `samtools sort`ed file for every method but anir (whose f64 sums follow the record order); per-record errors name the\n"
                        "       first offending record of that order.  The sample must fit the device's record store.  Not with filter, and not with\n"
                        "       --devices when there are fewer files than devices.\n"
                        "       -b takes BAM files and SAM text; `-b -` reads SAM text from standard input and a FIFO or character device is read as a\n"
                        "       pipe (e.g. minimap2 -a ref.fa reads.fq | coverm-amd contig -b - --unsorted -m mean; sample name `stdin`, or the path's stem).\n"
                        "       SAM text is decoded on the device as it streams in, in bounded memory; --no-stream or COVERM_SAM_ON_HOST=1 decode a SAM\n"
                        "       FILE whole on the host instead (the cross-check).  BAM from a pipe and gzip-compressed SAM are not supported.\n"
                        "       genome mode takes its genomes from -s, --single-genome, --genome-definition, -f <fasta>..., -d <dir> [-x fna]\n"
                        "       (a directory's files in bytewise name order) or --genome-fasta-list <file>; --use-full-contig-names\n"
                        "       coverm-amd filter -b <bam>... -o <bam>... [thresholds] [--inverse]\n"
                        "       coverm-amd depth -b <bam|sam|->... [-o FILE] [--no-zeros] [--bin-size N | --regions BED [--bin-value V | --thresholds T,..]] [--quantize SPEC] [--unsorted] [--device N] [-t N] [--no-stream] [flag and read filters]\n"
                        "       the per-base depth of every reference, under contig's filters, as a bedGraph: one `track` line per sample, then\n"
                        "       name<TAB>start<TAB>end<TAB>depth (0-based, half open) per stretch of equal depth; --no-zeros drops the stretches of depth 0\n"
                        "       --bin-size N [--bin-value mean|sum|min|max|covered]: one line per window of N bases instead (the last window of a reference\n"
                        "       is short; windows never cross references), reduced on the device; mean (the default) is printed with three decimals, the\n"
                        "       others as integers; --no-zeros then drops the windows without a covered base\n"
                        "       --regions BED [--bin-value ...]: one line per region of a BED file instead (chrom<TAB>start<TAB>end[<TAB>name], 0-based, half\n"
                        "       open; regions may overlap and come in any order), in the file's order, reduced on the device: chrom, start, end, the name when\n"
                        "       the line had one, then the value; a reference the sample's header does not have, or an end behind its length, is an error\n"
                        "       --thresholds T1,T2,.. (with --regions or --bin-size; 1 to 16 ascending depths): per region or window, the number of its bases\n"
                        "       with depth >= each threshold instead of a value, counted on the device; a line `#thresholds<TAB>T1<TAB>T2..` follows the track line\n"
                        "       --quantize C0:C1:..[:] (1 to 16 ascending cuts): one line per stretch of one depth CLASS instead, name<TAB>start<TAB>end<TAB>lo:hi for\n"
                        "       the classes [C0,C1), [C1,C2) .. and, when the spec ends in ':', lo:inf for [Clast,inf); an empty first field means 0; depths below C0\n"
                        "       (and at or above the last cut of a spec without the final ':') print no line; merged on the device, e.g. --quantize 0:1:5:150:\n");
        return 2;
    }
    a.mode = argv[1];
    auto collect = [&](int &i, std::vector<std::string> &dst) { while (i + 1 < argc && (argv[i + 1][0] != '-' || !argv[i + 1][1])) dst.push_back(argv[++i]); };      // ("-": standard input)
    for (int i = 2; i < argc; i++) {
        const std::string k = argv[i];
        auto val = [&]() -> const char * { if (i + 1 >= argc) die("missing value for " + k); return argv[++i]; };
        if (k == "-b" || k == "--bam-files") collect(i, a.bams);
        else if (k == "-m" || k == "--methods") collect(i, a.methods);
        else if (k == "--min-covered-fraction") a.min_covered_fraction = val();
        else if (k == "--contig-end-exclusion") a.contig_end_exclusion = parse_uint(k, val(), ~0ull);
        else if (k == "--trim-min") a.trim_min = val();
        else if (k == "--trim-max") a.trim_max = val();
        else if (k == "--output-format") a.output_format = val();
        else if (k == "-o" || k == "--output-file") a.output_file = val();
        else if (k == "--no-zeros") a.no_zeros = true;
        else if (parse_filter_flag(k, val, a.filter)) {}
        else if (k == "-s" || k == "--separator") { a.separator = val()[0]; a.have_separator = true; }
        else if (k == "--single-genome") a.single_genome = true;
        else if (k == "--genome-definition") a.genome_definition = val();
        else if (a.mode == "genome" && (k == "-f" || k == "--genome-fasta-files")) {
            a.have_fasta_files = true;
            const size_t n0 = a.genome_fasta_files.size();
            collect(i, a.genome_fasta_files);
            if (a.genome_fasta_files.size() == n0) die("missing value for " + k);
        }
        else if (a.mode == "genome" && (k == "-d" || k == "--genome-fasta-directory")) { a.genome_fasta_directory = val(); a.have_fasta_directory = true; }
        else if (a.mode == "genome" && (k == "-x" || k == "--genome-fasta-extension")) a.genome_fasta_extension = val();
        else if (a.mode == "genome" && k == "--genome-fasta-list") { a.genome_fasta_list = val(); a.have_fasta_list = true; }
        else if (a.mode == "genome" && k == "--use-full-contig-names") a.use_full_contig_names = true;
        else if (k == "--gff") a.gff = val();
        else if (k == "--gff-feature-type") { a.gff_feature_type = val(); a.have_gff_feature_type = true; }
        else if (k == "-t" || k == "--threads") a.threads = (int)parse_uint(k, val(), 65535);
        else if (k == "--device") { a.devices.assign(1, (int)parse_uint(k, val(), 1023)); }
        else if (k == "--devices") {   // 0,1,2 or 0-7
            a.devices.clear();
            std::string v = val();
            size_t p = 0;
            while (p < v.size()) {
                size_t c = v.find(',', p); if (c == std::string::npos) c = v.size();
                const std::string tok = v.substr(p, c - p);
                const size_t dash = tok.find('-');
                if (dash != std::string::npos && dash > 0) { for (int d = atoi(tok.substr(0, dash).c_str()); d <= atoi(tok.substr(dash + 1).c_str()); d++) a.devices.push_back(d); }
                else if (!tok.empty()) a.devices.push_back(atoi(tok.c_str()));
                p = c + 1;
            }
            if (a.devices.empty()) die("--devices needs a list such as 0,1,2,3 or 0-7");
        }
        else if (k == "--no-stream") a.no_stream = true;
        else if (k == "--unsorted") a.unsorted = true;
        else if (k == "-v" || k == "--verbose") a.verbose = true;      // (logging verbosity: only --unsorted has a line to print)
        else if (k == "-q" || k == "--quiet") {}
        else die("unknown argument " + k);
    }
    {   // clap's conflicts_with table for the genome sources (cli.rs:1878-1990); --genome-definition beside --genome-fasta-list is
        // allowed, and the definition wins (coverm.rs:1262-1294)
        const std::pair<bool, const char *> src[] = {{a.have_fasta_files, "--genome-fasta-files"}, {a.have_fasta_directory, "--genome-fasta-directory"},
                                                     {a.have_fasta_list, "--genome-fasta-list"}};
        const std::pair<bool, const char *> other[] = {{a.have_separator, "--separator"}, {a.single_genome, "--single-genome"}};
        auto conflict = [](const char *x, const char *y) { die(std::string("the argument '") + x + "' cannot be used with '" + y + "'"); };
        for (size_t i = 0; i < 3; i++) {
            if (!src[i].first) continue;
            for (size_t j = i + 1; j < 3; j++) if (src[j].first) conflict(src[i].second, src[j].second);
            for (auto &o : other) if (o.first) conflict(src[i].second, o.second);
            if (i < 2 && !a.genome_definition.empty()) conflict(src[i].second, "--genome-definition");
        }
    }
    if (a.bams.empty()) die("--bam-files is required (read mapping is out of scope for this engine)");
    if (a.devices.empty()) a.devices.push_back(0);
    if (a.unsorted && a.devices.size() > 1 && a.bams.size() < a.devices.size())
        die("--unsorted cannot be used with --devices when there are fewer BAM files than devices: a file would be cut into tid spans, which only a file sorted by reference has "
            "(give at least as many files as devices, or one device)");
    {   // SAM text and pipes: one stream is one sample on one device
        size_t n_stdin = 0, n_pipe = 0, n_text = 0;
        for (auto &b : a.bams) {
            const bool piped = input_is_pipe(b);
            n_stdin += b == "-"; n_pipe += piped;
            struct stat sb;
            n_text += piped || (stat(b.c_str(), &sb) == 0 && S_ISREG(sb.st_mode) && sb.st_size >= 2 && !is_bgzf(b));
        }
        if (n_stdin > 1) die("'-b -' (standard input) can be given once only");
        if (n_pipe && a.no_stream) die("--no-stream reads the whole file on the host, which a pipe ('-b -', a FIFO) does not allow: write the stream to a file first");
        if (n_text && a.devices.size() > 1 && a.bams.size() < a.devices.size())
            die("--devices with fewer files than devices needs BAM files: SAM text and pipes are decoded as one stream, a sample is one device's "
                "(give at least as many files as devices, or one device)");
    }
    R.contig = a.mode == "contig";
    const bool contig = R.contig;
    if (a.methods.empty()) a.methods.push_back(contig ? "mean" : "relative_abundance");   // cli.rs:2521, 2048
    if (!a.min_covered_fraction) a.min_covered_fraction = contig ? "0" : "10";            // cli.rs:2528, 2065

    // ---- EstimatorsAndTaker::generate_from_clap
    const float mcf = parse_percentage(a.min_covered_fraction, "--min-covered-fraction");
    const uint64_t excl = a.contig_end_exclusion;
    std::vector<covh_estimator> &est = R.est;
    std::vector<int64_t> norm;
    int64_t rpkm = -1, tpm = -1;
    int printer = 0, taker_kind = COVH_TAKER_STREAM;
    auto E = [&](int kind, float mf, uint64_t ex, float t0 = 0, float t1 = 0) {
        covh_estimator e; e.kind = kind; e.min_fraction_covered_bases = mf; e.contig_end_exclusion = ex;
        e.exclude_mismatches = 0; e.trim_min = t0; e.trim_max = t1; est.push_back(e);
    };
    Filter &f = R.f;
    f = resolve_filter(a.filter);
    const bool metabat = a.methods.size() == 1 && a.methods[0] == "metabat";
    for (auto &m : a.methods) if (m == "metabat" && a.methods.size() > 1) die("Cannot specify the metabat method with any other coverage methods");
    if (metabat) {
        E(COVH_LENGTH, 0, 0); E(COVH_MEAN, mcf, excl); E(COVH_VARIANCE, mcf, excl);
        taker_kind = COVH_TAKER_CACHED; printer = 3;
        f.pid_single = 0.97001f; f.improper = f.supp = f.sec = true;   // coverm.rs:1680-1693
    } else {
        for (size_t i = 0; i < a.methods.size(); i++) {
            const std::string &m = a.methods[i];
            if (m == "mean") E(COVH_MEAN, mcf, excl);
            else if (m == "coverage_histogram") E(COVH_PILEUP_COUNTS, mcf, excl);
            else if (m == "trimmed_mean") E(COVH_TRIMMED_MEAN, mcf, excl, parse_percentage(a.trim_min, "--trim-min"), parse_percentage(a.trim_max, "--trim-max"));
            else if (m == "covered_fraction") E(COVH_COVERED_FRACTION, mcf, 0);
            else if (m == "covered_bases") E(COVH_COVERED_BASES, mcf, 0);
            else if (m == "rpkm") { if (rpkm >= 0) die("The RPKM column cannot be specified more than once"); rpkm = (int64_t)i; E(COVH_RPKM, mcf, 0); }
            else if (m == "tpm") { if (tpm >= 0) die("The TPM column cannot be specified more than once"); tpm = (int64_t)i; E(COVH_TPM, mcf, 0); }
            else if (m == "variance") E(COVH_VARIANCE, mcf, excl);
            else if (m == "length") E(COVH_LENGTH, 0, 0);
            else if (m == "relative_abundance") { norm.push_back((int64_t)i); E(COVH_MEAN, mcf, excl); }
            else if (m == "count") E(COVH_READ_COUNT, 0, 0);
            else if (m == "reads_per_base") E(COVH_READS_PER_BASE, 0, 0);
            else if (m == "anir") E(COVH_ANIR, 0, 0);
            else die("unknown method " + m);
        }
        bool hist_method = false;
        for (auto &m : a.methods) hist_method |= m == "coverage_histogram";
        if (hist_method) {
            if (a.methods.size() > 1) die("Cannot specify the coverage_histogram method with any other coverage methods");
            taker_kind = COVH_TAKER_PILEUP; printer = 0;
        } else if (norm.empty() && rpkm < 0 && tpm < 0 && a.output_format == "sparse") { taker_kind = COVH_TAKER_STREAM; printer = 0; }
        else { taker_kind = COVH_TAKER_CACHED; printer = a.output_format == "sparse" ? 1 : 2; }
        if (mcf != 0.0f)
            for (auto &e : est)
                if (e.kind == COVH_READ_COUNT || e.kind == COVH_LENGTH || e.kind == COVH_READS_PER_BASE || e.kind == COVH_ANIR)
                    die("this coverage estimator cannot be used when --min-covered-fraction is > 0");
    }
    static const char *HDR[] = {"Mean", "Trimmed Mean", "Coverage\tBases", "Covered Fraction", "Covered Bases", "RPKM", "TPM",
                                "Variance", "Length", "Read Count", "Reads per base", "ANIr"};
    std::vector<std::string> headers;
    for (auto &e : est) {
        if (e.kind == COVH_PILEUP_COUNTS) { headers.push_back("Coverage"); headers.push_back("Bases"); }
        else headers.push_back(HDR[e.kind]);
    }
    for (int64_t i : norm) headers[(size_t)i] = "Relative Abundance (%)";
    std::vector<const char *> hptr;
    for (auto &h : headers) hptr.push_back(h.c_str());
    const char *entry_type = contig ? "Contig" : "Genome";
    R.per_gene = !a.gff.empty();                                    // coverm.rs:488-518, 1557-1590
    if (R.per_gene) entry_type = contig ? "Gene\tContig" : "Gene\tContig\tGenome";
    covh_taker *taker = R.taker = covh_taker_new(taker_kind, est.size());
    struct TakerFree { covh_taker *t; ~TakerFree() { covh_taker_free(t); } } taker_free{taker};
    covh_print_headers(taker, printer, entry_type, hptr.data(), hptr.size());

    if (R.per_gene) {
        if (a.methods.size() == 1 && a.methods[0] == "metabat") die("The metabat method cannot be used with --gff");
        char gerr[512] = {0};
        R.genes = covh_genes_read_gff(a.gff.c_str(), a.have_gff_feature_type ? a.gff_feature_type.c_str() : nullptr, gerr, sizeof gerr);
        if (!R.genes) die(gerr);
    }
    struct GenesFree { covh_genes *&g; ~GenesFree() { if (g) covh_genes_free(g); } } genes_free{R.genes};
    // ---- genome definition
    std::vector<std::string> &genomes = R.genomes;
    R.by_names = !contig && !a.have_separator && !a.single_genome;
    const bool fasta_genomes = R.by_names && a.genome_definition.empty() && (a.have_fasta_files || a.have_fasta_directory || a.have_fasta_list);
    if (R.by_names && !fasta_genomes) read_genome_definition(R);

    // ---- sessions: one per device, brought up in parallel
    R.want = covh_wants(est.data(), est.size());
    if (R.want & COV_WANT_IDENTITY)   // contig.rs:208 / genome.rs:724 use the primary-read sum, genome.rs:220 the not-supplementary one
        R.want |= R.by_names ? COV_WANT_IDENTITY_NONSUPP_ONLY : COV_WANT_IDENTITY_PRIMARY_ONLY;
    if (f.doing_filtering()) f.mode(R.fs, R.fp);
    cov_config &cfg = R.cfg; memset(&cfg, 0, sizeof cfg);
    cfg.include_improper_pairs = f.improper; cfg.include_supplementary = f.supp;
    cfg.include_secondary = f.sec; cfg.min_mapq = 255; cfg.contig_end_exclusion = excl; cfg.want = R.want;
    if (f.doing_filtering() && R.fs && !R.fp) {
        cfg.filter_single = 1; cfg.min_mapq = (uint8_t)f.mapq; cfg.min_aligned_length = f.len_single;
        cfg.min_percent_identity = f.pid_single; cfg.min_aligned_percent = f.pct_single;
    }
    const size_t nd = a.devices.size(), nb = a.bams.size();
    // genomes from FASTA files are resolved beside the sessions' start-up; the error of a failed resolution is the run's, before
    // any ingest, as if it had been resolved first
    std::future<std::string> fasta_ahead;
    if (fasta_genomes) fasta_ahead = std::async(std::launch::async, [&R] { return resolve_fasta_genomes(R); });
    if (!a.no_stream && !R.per_gene && !no_gpu_ingest())
        for (size_t i = 0; i < std::min<size_t>(nb, std::max<size_t>(nd, 2)); i++) {      // (the file type is checked by covh_bam_read_header itself)
            const std::string path = a.bams[i];
            if (R.hdr_ahead.count(path) || !is_bgzf(path)) continue;
            R.hdr_ahead.emplace(path, std::async(std::launch::async, [path] {
                HeaderAhead h; char e[512] = {0};
                h.hd = covh_bam_read_header(path.c_str(), e, sizeof e);
                if (!h.hd) h.err = e;
                return h;
            }));
        }
    // a pipe's format is told from its first bytes READ, before any device work: BAM from a pipe is refused here
    for (auto &b : a.bams) {
        if (!input_is_pipe(b) || R.sam_ahead.count(b)) continue;
        char e[512] = {0};
        covh_sam *h = covh_sam_open(b.c_str(), e, sizeof e);
        if (!h) die(e);
        R.sam_ahead.emplace(b, h);
        if (covh_sam_kind(h) == 1) die("BAM from a pipe is not supported yet; SAM text is (e.g. `samtools view -h`), or pass the file's path");
        if (covh_sam_kind(h) == 2) die(stoit_of(b) + ": the stream is neither SAM text nor BAM (NUL bytes in its first piece)");
    }
    struct SamDrain { Run &R; ~SamDrain() { for (auto &kv : R.sam_ahead) covh_sam_close(kv.second); R.sam_ahead.clear(); } } sam_drain{R};
    struct HdrDrain { Run &R; ~HdrDrain() { for (auto &kv : R.hdr_ahead) { HeaderAhead h = kv.second.get(); if (h.hd) covh_bam_header_free(h.hd); } } } hdr_drain{R};
    std::vector<cov_session *> sess(nd, nullptr);
    struct SessFree { std::vector<cov_session *> &v; ~SessFree() { if (!g_skip_teardown.load()) for (auto *s : v) if (s) cov_destroy(s); } } sess_free{sess};
    {
        std::vector<std::thread> th;
        std::vector<cov_status> rc(nd, COV_OK);
        std::vector<std::string> emsg(nd);
        std::mutex em;
        for (size_t d = 0; d < nd; d++)
            th.emplace_back([&, d] {
                cov_config c = cfg; c.device = a.devices[d];
                long long prep = 1;
                (void)covknob::get("ingest_prepare", prep);
                if (!no_gpu_ingest() && prep) c.want |= COV_WANT_INGEST;      // the ingest's streams and events come up beside the rest of the start-up
                rc[d] = cov_create(&c, &sess[d]);
                if (rc[d] != COV_OK) { std::lock_guard<std::mutex> lk(em); emsg[d] = cov_last_error(nullptr); }
            });
        for (auto &t : th) t.join();
        if (fasta_ahead.valid()) { const std::string e = fasta_ahead.get(); if (!e.empty()) die(e); }
        for (size_t d = 0; d < nd; d++) if (rc[d] != COV_OK) die(emsg[d]);
    }
    {
        // CoverageEstimator::calculate_coverage on the device for `coverm contig` (one entry per contig) when every estimator asked for is
        // one the device evaluates (all but TPM and the coverage histogram); COVERM_HOST_ESTIMATES=1 keeps the host's evaluation
        static_assert(sizeof(covh_estimator) == sizeof(cov_estimator) && offsetof(covh_estimator, trim_max) == offsetof(cov_estimator, trim_max), "estimator structs share one layout");
        bool ok = contig && !R.per_gene && !getenv("COVERM_HOST_ESTIMATES") && !est.empty() && est.size() <= COV_EST_MAX;
        for (const covh_estimator &e : est) ok = ok && e.kind != COVH_TPM && e.kind != COVH_PILEUP_COUNTS;
        R.dev_est = ok;
        if (ok) for (size_t d = 0; d < nd; d++) check(sess[d], cov_set_estimators(sess[d], reinterpret_cast<const cov_estimator *>(est.data()), (uint32_t)est.size()));
    }
    {
        // ... and for the contig-names genome scan (one entry per genome, cov_set_genomes) under the same conditions; not with --gff, not when
        // a file is cut into spans over several devices (each rank would hold a part of every genome).  The estimators are set per sample,
        // behind the genome table (ANIr takes the not-supplementary identity sum there).
        bool ok = R.by_names && !R.per_gene && !(nd > 1 && nb < nd) && !getenv("COVERM_HOST_ESTIMATES") && !est.empty() && est.size() <= COV_EST_MAX;
        for (const covh_estimator &e : est) ok = ok && e.kind != COVH_TPM && e.kind != COVH_PILEUP_COUNTS;
        R.dev_genome = ok;
        // ... and for the separator / single-genome scan (one entry per run of observed contigs of a genome, cov_set_genome_runs)
        bool sep = !contig && (a.have_separator || a.single_genome) && !R.per_gene && !(nd > 1 && nb < nd) && !getenv("COVERM_HOST_ESTIMATES") && !est.empty() && est.size() <= COV_EST_MAX;
        for (const covh_estimator &e : est) sep = sep && e.kind != COVH_TPM && e.kind != COVH_PILEUP_COUNTS;
        R.dev_sep = sep;
    }
    const double t_sessions = now();
    covh_bam_set_pinned(1);
    // (measured, profiles/r03_tail_variants.log: releasing the staging slots beside the last rounds shortens the exit by ~0.03 s and
    // lengthens the tail by as much — hipHostFree waits for the device — so it stays opt-in)
    covh_bam_set_release_staging(0);
    if (nb > 1) covh_bam_set_buffer_cache(1);
    covh_bam_set_concurrent_feeders((int)std::min(nd, span_mode_feeders(nb, nd)));      // > 2 at once: mapped files, registered up front (host memory traffic / 3)
    const bool timing = timing_on();
    std::vector<Sample> samples(nb);
    for (size_t i = 0; i < nb; i++) samples[i].path = a.bams[i];
    std::mutex err_mutex; std::string first_error;
    size_t n_errors = 0, n_span_unsorted = 0;      // a span-mode fallback is taken only when EVERY failed span failed on the order of its keys
    auto guarded = [&](auto fn) {
        try { fn(); }
        catch (const SpanUnsorted &e) { std::lock_guard<std::mutex> lk(err_mutex); n_errors++; n_span_unsorted++; if (first_error.empty()) first_error = e.what(); }
        catch (const Fatal &e) { std::lock_guard<std::mutex> lk(err_mutex); n_errors++; if (first_error.empty() || n_span_unsorted == n_errors - 1) first_error = e.what(); }
        catch (const std::exception &e) { std::lock_guard<std::mutex> lk(err_mutex); n_errors++; if (first_error.empty() || n_span_unsorted == n_errors - 1) first_error = e.what(); }
    };
    const bool span_mode = nd > 1 && nb < nd;
    if (!span_mode) {
        // samples dealt to devices; host threads shared between the concurrently decoded files
        const size_t lanes = std::min(nd, nb);
        // every device's reader gets at least six threads (four of them read): with -t divided evenly, eight devices under a 16-CPU
        // quota had two threads each and a reader that cannot fill its link; the readers block in pread and in slot waits most of
        // the time, so oversubscribing the CPUs costs less than starving a device
        const int thr = std::min(std::max(1, a.threads), std::max(6, a.threads / (int)lanes));
        std::atomic<size_t> next{0};
        std::vector<std::thread> th;
        for (size_t d = 0; d < lanes; d++)
            th.emplace_back([&, d] {
                (void)cov_bind_thread_to_device_node(a.devices[d]);
                guarded([&] {
                    for (;;) {
                        const size_t bi = next.fetch_add(1);
                        if (bi >= nb) break;
                        { std::lock_guard<std::mutex> lk(err_mutex); if (!first_error.empty()) break; }
                        ingest(R, sess[d], samples[bi], thr, 0, 1);
                    }
                });
            });
        for (auto &t : th) t.join();
        if (!first_error.empty()) die(first_error);
    } else {
        // every BAM cut into nd tid spans; the per-contig result blocks meet on device 0 through one RCCL gather
        const int thr = std::min(std::max(1, a.threads), std::max(6, a.threads / (int)nd));      // (as above)
        for (size_t bi = 0; bi < nb; bi++) {
            std::vector<Sample> part(nd);
            std::vector<std::thread> th;
            for (size_t d = 0; d < nd; d++) {
                part[d].path = a.bams[bi];
                th.emplace_back([&, d] { (void)cov_bind_thread_to_device_node(a.devices[d]); guarded([&] { ingest(R, sess[d], part[d], thr, (uint32_t)d, (uint32_t)nd); }); });
            }
            for (auto &t : th) t.join();
            if (!first_error.empty()) {
                // A span trusts the file's order and refuses a file whose keys decrease anywhere — any record, also one the scan would
                // skip.  The reference only compares the tids of mapped records that passed the flag filters (contig.rs:118-132), so a
                // file it accepts can be refused here: such a file goes through ONE device whole, where cov_finish judges its order with
                // the reference's rule (and ends in the same error if it really is unsorted).
                if (n_span_unsorted != n_errors) die(first_error);      // some span failed for another reason: that error is the run's (first_error holds it)
                first_error.clear(); n_errors = n_span_unsorted = 0;
                if (timing) fprintf(stderr, "[coverm-amd] %s: keys decrease inside a span; the file goes through one device whole\n", a.bams[bi].c_str());
                ingest(R, sess[0], samples[bi], a.threads, 0, 1);
                continue;
            }
            merge_spans(R, sess, part, samples[bi]);
        }
    }
    const double t_ingested = now();
    if (timing) report_resident_set();
    if (timing)
        for (auto &S : samples)
            fprintf(stderr, "[coverm-amd] sample %s: %s, open %.3fs, ingest (decode+push) %.3fs, finish+fetch %.3fs, %llu records, reader buffers %.0f MB\n", S.stoit.c_str(),
                    S.device_ingest ? "device ingest" : S.streamed ? "streamed" : "whole file", S.t_open, S.t_ingest, S.t_finish, (unsigned long long)S.n_records, S.peak_bytes / 1e6);

    // ---- scan drivers: one call per BAM, each with its own header (contig.rs:29-32)
    std::vector<covh_reads_mapped> rm(nb);
    for (size_t bi = 0; bi < nb; bi++) {
        const Sample &S = samples[bi];
        if (R.per_gene) { rm[bi] = S.gene_rm; continue; }
        const covh_header hdr = S.header();
        covh_sample hs; hs.stoit_name = S.stoit.c_str(); hs.stats = S.stats.data(); hs.hist = S.hist.empty() ? nullptr : S.hist.data();
        hs.num_detected_primary_alignments = S.prim;
        int rc;
        const float *ef = S.estimates.empty() ? nullptr : S.estimates.data();
        if (contig) rc = covh_contig_coverage_estimated(&hdr, &hs, 1, taker, est.data(), est.size(), !a.no_zeros, &rm[bi], R.dev_est ? &ef : nullptr);
        else if (S.sep_dev)
            rc = covh_genome_coverage_separator_estimated(&hdr, S.stoit.c_str(), S.prim, (uint8_t)(a.single_genome ? '0' : a.separator), a.single_genome, taker, !a.no_zeros, est.data(),
                                                          est.size(), S.sep_entries.data(), S.sep_entries.size(), S.genome_estimates.data(), &rm[bi]);
        else if (a.have_separator || a.single_genome)
            rc = covh_genome_coverage_separator(&hdr, &hs, 1, (uint8_t)(a.single_genome ? '0' : a.separator), taker, !a.no_zeros, est.data(), est.size(),
                                                a.single_genome, &rm[bi]);
        else if (S.genome_dev) {
            std::vector<const char *> gn;
            for (auto &g : genomes) gn.push_back(g.c_str());
            rc = covh_genome_coverage_estimated(S.stoit.c_str(), S.prim, S.any_seen, gn.data(), gn.size(), taker, !a.no_zeros, est.data(), est.size(), S.genome_estimates.data(),
                                                S.genome_stats.data(), &rm[bi]);
        } else {
            std::vector<const char *> gn;
            for (auto &g : genomes) gn.push_back(g.c_str());
            rc = covh_genome_coverage_with_contig_names(&hdr, &hs, 1, S.genome_of_tid.data(), gn.data(), gn.size(), taker, !a.no_zeros, est.data(),
                                                        est.size(), &rm[bi]);
        }
        if (rc != COV_OK) die(covh_last_error());
        if (covh_taker_names_mismatch(taker))   // coverage_takers.rs:140-148
            die("Found a difference amongst the reference sets used for mapping. For this (non-streaming) usage of CoverM, all BAM files must have the "
                "same set of reference sequences.");
    }
    for (size_t i = 0; i < nb; i++)   // contig.rs:233-240
        fprintf(stderr, "[coverm-amd] In sample '%s', found %llu reads mapped out of %llu total (%.2f%%)\n", samples[i].stoit.c_str(),
                (unsigned long long)rm[i].num_mapped_reads, (unsigned long long)rm[i].num_reads,
                (double)(rm[i].num_mapped_reads * 100) / (double)rm[i].num_reads);
    const double t_scanned = now();
    covh_finalise_printing(taker, printer, entry_type, hptr.data(), hptr.size(), rm.data(), rm.size(), norm.data(), norm.size(), rpkm, tpm);
    const double t_printed = now();
    size_t len = 0;
    const char *txt = covh_taker_text(taker, &len);
    FILE *out = a.output_file.empty() || a.output_file == "-" ? stdout : fopen(a.output_file.c_str(), "w");
    if (!out) die("Failed to create output file: " + a.output_file);
    fwrite(txt, 1, len, out);
    if (out != stdout) fclose(out); else fflush(stdout);
    if (timing)
        fprintf(stderr, "[coverm-amd] main: arguments + device sessions %.3fs, samples %.3fs, scan drivers + table %.3fs (scan drivers %.3fs, printer %.3fs, %zu bytes written in %.3fs; process start-up and exit are outside)\n",
                t_sessions - t_main0, t_ingested - t_sessions, now() - t_ingested, t_scanned - t_ingested, t_printed - t_scanned, len, now() - t_printed);
    return 0;
}

}  // namespace

extern "C" void covh_cli_set_fast_exit(int on) { g_skip_teardown.store(on != 0); }

extern "C" int covh_cli_main(int argc, char **argv) {
    try {
        return run_cli(argc, argv);
    } catch (const Fatal &e) {
        fprintf(stderr, "[coverm-amd] ERROR: %s\n", e.what());
        return 1;
    } catch (const std::exception &e) {
        fprintf(stderr, "[coverm-amd] ERROR: %s\n", e.what());
        return 1;
    }
}

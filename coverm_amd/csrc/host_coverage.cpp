// Host side above the covermhip ABI (include/coverm_host.h): estimator finalisation from integer
// statistics, the three scan drivers, CoverageTaker implementations and CoveragePrinter.
// Pure C++17, no HIP: this is where the reference's Rust `calculate_coverage` / takers / printers sit.
#include "../../include/coverm_host.h"
#include "knobs.h"
#include "sep_entry_core.h"
#include "depth_class_core.h"

#include <algorithm>
#include <cerrno>
#include <unistd.h>
#include <mutex>
#include <functional>
#include <condition_variable>
#include <atomic>
#include <charconv>
#include <cmath>
#include <cstring>
#include <limits>
#include <memory>
#include <optional>
#include <string>
#include <thread>
#include <string_view>
#include <unordered_map>
#include <vector>

typedef uint64_t u64;
typedef uint32_t u32;

namespace {

thread_local std::string g_err;

// ------------------------------------------------------------------ Rust float Display
template <typename F>
size_t fmt_float(F v, char *buf, size_t cap) {
    std::string s;
    if (std::isnan(v)) s = "NaN";
    else if (std::isinf(v)) s = v > 0 ? "inf" : "-inf";
    else if (v == 0) s = std::signbit(v) ? "-0" : "0";
    else {
        char tmp[512];
        auto r = std::to_chars(tmp, tmp + sizeof tmp, v, std::chars_format::fixed);  // shortest round-trip
        s.assign(tmp, r.ptr);
    }
    if (cap) {
        size_t n = std::min(cap - 1, s.size());
        memcpy(buf, s.data(), n);
        buf[n] = 0;
    }
    return s.size();
}
std::string f32s(float v) { char b[512]; fmt_float(v, b, sizeof b); return b; }
std::string f64s(double v) { char b[512]; fmt_float(v, b, sizeof b); return b; }
// the same digits appended in place (the printers' rows: no temporary strings)
template <typename F>
void put_float(std::string &o, F v) {
    if (std::isnan(v)) { o += "NaN"; return; }
    if (std::isinf(v)) { o += v > 0 ? "inf" : "-inf"; return; }
    if (v == 0) { o += std::signbit(v) ? "-0" : "0"; return; }
    char tmp[512];
    auto r = std::to_chars(tmp, tmp + sizeof tmp, v, std::chars_format::fixed);
    o.append(tmp, (size_t)(r.ptr - tmp));
}
// Rows of a table formatted on several threads when there are many (an assembly's table is millions of rows and several times as many
// numbers: 0.56 s of a 1.2 s run at 2 M contigs on one thread): `row(out, k)` appends row k to `out`; the pieces are joined in order.
template <typename Row>
void format_rows(std::string &o, size_t n_rows, size_t bytes_per_row, Row row) {
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const size_t T = std::min<size_t>({(size_t)8, (size_t)hw, n_rows / 32768 + 1});
    if (T <= 1) { for (size_t k = 0; k < n_rows; k++) row(o, k); return; }
    const size_t n_parts = T * 4, per = (n_rows + n_parts - 1) / n_parts;
    std::vector<std::string> parts(n_parts);
    std::atomic<size_t> next{0};
    std::vector<std::thread> th;
    for (size_t t = 0; t < T; t++)
        th.emplace_back([&] {
            for (;;) {
                const size_t p = next.fetch_add(1);
                if (p >= n_parts) break;
                const size_t lo = p * per, hi = std::min(n_rows, lo + per);
                if (hi > lo) parts[p].reserve((hi - lo) * bytes_per_row);
                for (size_t k = lo; k < hi; k++) row(parts[p], k);
            }
        });
    for (auto &x : th) x.join();
    size_t total = 0;
    for (auto &x : parts) total += x.size();
    o.reserve(o.size() + total);
    for (auto &x : parts) { o += x; std::string().swap(x); }
}

// Rust `x as usize` for f32: saturating, NaN -> 0
u64 f32_to_usize(float x) {
    if (!(x == x) || x <= 0.0f) return 0;
    if (x >= 18446744073709551616.0f) return std::numeric_limits<u64>::max();
    return (u64)x;
}

// ------------------------------------------------------------------ entry accumulator
// What the estimators of one entry (contig or genome) would hold after add_contig over its contigs
// (estimators.rs:366-528), expressed in the integer statistics the device returns.
struct EntryAcc {
    u64 win_len = 0, win_sum_d = 0, win_sum_d2 = 0, win_covered = 0;
    u64 full_len = 0, full_covered = 0, n_reads = 0, mismatches = 0;
    u32 win_min_d = 0xffffffffu;
    double sum_identity = 0.0;
    std::vector<u64> hist;  // merged counts; hist.size() == counts.len()
    // an entry made of ONE contig reads that contig's bins where they lie (no copy); a second contig materialises `hist`
    const u64 *hview = nullptr; size_t hview_n = 0;
    size_t hsize() const { return hview ? hview_n : hist.size(); }
    u64 hat(size_t i) const { return hview ? hview[i] : hist[i]; }
    void own_hist() { if (hview) { hist.assign(hview, hview + hview_n); hview = nullptr; hview_n = 0; } }
    void reset() {   // keeps hist's capacity: one reset per contig
        win_len = win_sum_d = win_sum_d2 = win_covered = full_len = full_covered = n_reads = mismatches = 0;
        win_min_d = 0xffffffffu; sum_identity = 0.0; hist.clear(); hview = nullptr; hview_n = 0; hist_len_only = 0;
    }
    void add_contig(const cov_contig_stats &s, u64 L, u64 excl, u64 n, double identity, const u64 *h) {
        n_reads += n;
        mismatches += s.sum_nm - s.sum_indel;   // total_edit_distance - total_indels (u64 wrapping, contig.rs:59)
        sum_identity += identity;
        full_len += L;
        full_covered += s.full_covered;
        if (2 * excl < L) {                      // estimators.rs:386-392, 436-445
            win_len += L - 2 * excl;
            win_sum_d += s.win_sum_d; win_sum_d2 += s.win_sum_d2; win_covered += s.win_covered;
            win_min_d = std::min(win_min_d, s.win_min_d);
            if (h && s.hist_len) {
                if (!hview && hist.empty()) { hview = h + s.hist_off; hview_n = s.hist_len; }
                else {
                    own_hist();
                    if (hist.size() < s.hist_len) hist.resize(s.hist_len, 0);
                    for (u32 d = 0; d < s.hist_len; d++) hist[d] += h[s.hist_off + d];
                }
            } else if (!h) {
                // no histogram requested: remember only how long counts would be
                if (hist_len_only < (u64)s.win_max_d + 1) hist_len_only = (u64)s.win_max_d + 1;
            }
        }
    }
    // same, from an explicit entry (unit tests)
    u64 hist_len_only = 0;
};

u64 unobserved_bases(const u64 *u, size_t n, u64 excl) {  // estimators.rs:226-242
    u64 s = 0, e = 2 * excl;
    for (size_t i = 0; i < n; i++) s += u[i] < e ? u[i] : u[i] - e;
    return s;
}
u64 sum_u64(const u64 *u, size_t n) { u64 s = 0; for (size_t i = 0; i < n; i++) s += u[i]; return s; }

// estimators.rs:530-839, every branch in the reference's operation order
float calculate(const covh_estimator &e, const EntryAcc &a, const u64 *unobs, size_t n_unobs) {
    const float minfrac = e.min_fraction_covered_bases;
    switch (e.kind) {
    case COVH_MEAN: {
        const u64 T = a.win_len + unobserved_bases(unobs, n_unobs, e.contig_end_exclusion);
        if (T == 0 || ((float)a.win_covered / (float)T) < minfrac) return 0.0f;
        const float num = e.exclude_mismatches ? (float)(a.win_sum_d - a.mismatches) : (float)a.win_sum_d;
        return num / (float)T;
    }
    case COVH_TRIMMED_MEAN: {
        const u64 U = unobserved_bases(unobs, n_unobs, e.contig_end_exclusion);
        const u64 T = a.win_len + U;
        if (T == 0) return 0.0f;
        if (((float)a.win_covered / (float)T) < minfrac) return 0.0f;
        const u64 min_index = f32_to_usize(std::floor(e.trim_min * (float)T));
        const u64 max_index = f32_to_usize(std::ceil(e.trim_max * (float)T));
        if (a.win_covered == 0) return 0.0f;
        u64 acc = 0, total = 0;
        bool started = false;
        for (size_t i = 0, nh = a.hsize(); i < nh; i++) {
            const u64 n = a.hat(i) + (i == 0 ? U : 0);  // counts[0] += unobserved (:596)
            acc += n;
            if (acc >= min_index) {
                if (started) {
                    if (acc > max_index) {
                        const u64 excess = acc - n;
                        total += (max_index >= excess ? max_index - excess + 1 : 0) * (u64)i;
                        break;
                    } else total += n * (u64)i;
                } else if (acc > max_index) { total = (max_index - min_index + 1) * (u64)i; started = true; }  // no break (:626-629)
                else if (acc < min_index) {}
                else { total = (acc - min_index + 1) * (u64)i; started = true; }
            }
        }
        return (float)total / (float)(max_index - min_index);
    }
    case COVH_PILEUP_COUNTS: {
        if (a.win_len == 0) return 0.0f;
        const u64 T = a.win_len + unobserved_bases(unobs, n_unobs, e.contig_end_exclusion);
        if (((float)a.win_covered / (float)T) < minfrac) return 0.0f;
        return (float)(T - a.win_covered + 1);
    }
    case COVH_COVERED_FRACTION: {
        const u64 T = a.full_len + sum_u64(unobs, n_unobs);
        if (T == 0 || ((float)a.full_covered / (float)T) < minfrac) return 0.0f;
        return (float)a.full_covered / (float)T;
    }
    case COVH_COVERED_BASES: {
        const u64 T = a.full_len + sum_u64(unobs, n_unobs);
        if (T == 0 || ((float)a.full_covered / (float)T) < minfrac) return 0.0f;
        return (float)a.full_covered;
    }
    case COVH_RPKM: {
        const u64 T = a.full_len + sum_u64(unobs, n_unobs);
        if (T == 0 || ((float)a.full_covered / (float)T) < minfrac) return 0.0f;
        return (float)(a.n_reads * 1000000000ull) / (float)T;
    }
    case COVH_TPM: {
        const u64 T = a.full_len + sum_u64(unobs, n_unobs);
        if (T == 0 || ((float)a.full_covered / (float)T) < minfrac) return 0.0f;
        return (float)std::exp(std::log((double)a.n_reads) - std::log((double)T));
    }
    case COVH_VARIANCE: {
        const u64 U = unobserved_bases(unobs, n_unobs, e.contig_end_exclusion);
        const u64 T = a.win_len + U;
        if (T == 0) return 0.0f;
        // counts.is_empty()  <=>  no contig contributed a window position  <=>  win_len == 0
        if (((float)a.win_covered / (float)T) < minfrac || T < 3 || a.win_len == 0) return 0.0f;
        // shifted sums: k = lowest occupied depth (0 as soon as unobserved bases land in counts[0]); the
        // reference's ex = sum (x-k) n and ex2 = sum (x-k)^2 n over the histogram are these integers
        const u64 k = U > 0 ? 0 : a.win_min_d;
        const u64 N = a.win_len + U;
        const u64 ex = a.win_sum_d - k * N;
        const u64 ex2 = a.win_sum_d2 - 2 * k * a.win_sum_d + k * k * N;
        return ((float)ex2 - (float)(ex * ex) / (float)T) / (float)(T - 1);
    }
    case COVH_LENGTH: return (float)(a.full_len + sum_u64(unobs, n_unobs));
    case COVH_READ_COUNT: return (float)a.n_reads;
    case COVH_READS_PER_BASE: return (float)a.n_reads / (float)(a.full_len + sum_u64(unobs, n_unobs));
    case COVH_ANIR: return a.n_reads == 0 ? 0.0f : (float)(a.sum_identity / (double)a.n_reads);
    }
    return 0.0f;
}

}  // namespace

// ------------------------------------------------------------------ takers (coverage_takers.rs)
struct covh_taker {
    int kind;
    size_t num_coverages;
    std::string text;
    std::string cur_stoit, cur_entry_name;
    // cached
    std::vector<std::string> stoit_names;
    // entry names live in one arena (a std::string per entry costs an allocation per contig per sample)
    struct NameRef { int64_t off = -1; uint32_t len = 0; explicit operator bool() const { return off >= 0; } };
    struct NameTable {
        std::string arena;
        std::vector<NameRef> refs;
        size_t size() const { return refs.size(); }
        void resize(size_t n) { refs.resize(n); }
        struct Entry {
            const NameTable *t; size_t i;
            explicit operator bool() const { return (bool)t->refs[i]; }
            std::string operator*() const { return std::string(t->arena.data() + t->refs[i].off, t->refs[i].len); }
            std::string_view view() const { return std::string_view(t->arena.data() + t->refs[i].off, t->refs[i].len); }
        };
        Entry operator[](size_t i) const { return Entry{this, i}; }
        void set(size_t i, std::string_view n) { refs[i].off = (int64_t)arena.size(); refs[i].len = (uint32_t)n.size(); arena.append(n); }
        struct Iter { const NameTable *t; size_t i; Entry operator*() const { return Entry{t, i}; } Iter &operator++() { ++i; return *this; } bool operator!=(const Iter &o) const { return i != o.i; } };
        Iter begin() const { return Iter{this, 0}; }
        Iter end() const { return Iter{this, refs.size()}; }
    } entry_names;
    std::vector<std::vector<std::pair<size_t, float>>> coverages;
    size_t cur_stoit_i = 0, cur_entry_i = 0;
    bool mismatch = false;

    void start_stoit(const std::string &n) {
        if (kind == COVH_TAKER_CACHED) { stoit_names.push_back(n); coverages.emplace_back(); cur_stoit_i = stoit_names.size() - 1; }
        else cur_stoit = n;
    }
    // capacity hint from the scan drivers: entries per sample, coverages per entry, bytes of all entry names
    void reserve(size_t entries, size_t per_entry, size_t name_bytes) {
        if (kind != COVH_TAKER_CACHED) { text.reserve(text.size() + entries * (per_entry * 12 + 24) + name_bytes); return; }
        if (!coverages.empty()) coverages.back().reserve(entries * per_entry);
        if (entry_names.refs.size() < entries) entry_names.refs.resize(entries);        // unset refs: ids arrive in any order, and not all of them
        if (entry_names.arena.capacity() < name_bytes) entry_names.arena.reserve(name_bytes);
    }
    // Cached taker, every target of a header an entry (zero rows printed): the name table in one pass.  True when the table now holds exactly
    // these names under ids 0 .. n - 1 (it was empty, or already held this very header); false: the caller goes entry by entry.
    bool names_bulk(const char *blob, const uint32_t *off, size_t n) {
        if (kind != COVH_TAKER_CACHED) return false;
        const size_t bytes = off[n] - off[0];
        if (entry_names.refs.empty() || (entry_names.arena.empty() && entry_names.refs.size() <= n)) {
            entry_names.arena.assign(blob + off[0], bytes);
            entry_names.refs.resize(n);
            for (size_t i = 0; i < n; i++) { entry_names.refs[i].off = (int64_t)(off[i] - off[0]); entry_names.refs[i].len = off[i + 1] - off[i]; }
            return true;
        }
        if (entry_names.refs.size() != n || entry_names.arena.size() != bytes || memcmp(entry_names.arena.data(), blob + off[0], bytes) != 0) return false;
        for (size_t i = 0; i < n; i++)
            if (entry_names.refs[i].off != (int64_t)(off[i] - off[0]) || entry_names.refs[i].len != off[i + 1] - off[i]) return false;
        return true;
    }
    void start_entry(size_t id, std::string_view name) {
        if (kind == COVH_TAKER_STREAM) { text += cur_stoit; text += '\t'; text.append(name); }
        else if (kind == COVH_TAKER_PILEUP) cur_entry_name.assign(name);
        else {
            if (id >= entry_names.size()) entry_names.resize(id + 1);
            if (!entry_names[id]) entry_names.set(id, name);
            else if (entry_names[id].view() != name) mismatch = true;  // coverage_takers.rs:140-148 (process::exit(1))
            cur_entry_i = id;
        }
    }
    void add_single_coverage(float c) {
        if (kind == COVH_TAKER_STREAM) { text += '\t'; text += (c == 0.0f) ? std::string("0") : f32s(c); }
        else if (kind == COVH_TAKER_CACHED) coverages[cur_stoit_i].emplace_back(cur_entry_i, c);
    }
    void add_coverage_entry(u64 num_reads, u64 num_bases) {
        if (kind == COVH_TAKER_PILEUP) {
            text += cur_stoit; text += '\t'; text += cur_entry_name; text += '\t';
            text += std::to_string(num_reads); text += '\t'; text += std::to_string(num_bases); text += '\n';
        }
    }
    void finish_entry() { if (kind == COVH_TAKER_STREAM) text += '\n'; }
};

namespace {

struct EntryAndCoverages { size_t entry_index, stoit_index; std::vector<float> coverages; };

// CoverageTakerTypeIterator, coverage_takers.rs:265-377
std::vector<EntryAndCoverages> iterate_cached(const covh_taker &t) {
    std::vector<EntryAndCoverages> out;
    const size_t ns = t.stoit_names.size(), nc = t.num_coverages;
    if (ns == 0) return out;
    std::vector<size_t> nxt(ns, 0);
    size_t cur = 0;
    std::optional<size_t> last;
    while (cur <= ns) {
        std::optional<size_t> lowest;
        for (size_t si = 0; si < ns; si++) {
            if (nxt[si] < t.coverages[si].size()) {
                const size_t ei = t.coverages[si][nxt[si]].first;
                if (!last || ei > *last) { if (!lowest || ei < *lowest) lowest = ei; }
            }
        }
        if (lowest) {
            const size_t chosen = nxt[cur];
            const auto &lst = t.coverages[cur];
            EntryAndCoverages e{*lowest, cur, {}};
            if (chosen >= lst.size() || lst[chosen].first != *lowest) e.coverages.assign(nc, 0.0f);
            else for (size_t k = 0; k < nc; k++) e.coverages.push_back(lst[chosen + k].second);
            for (size_t si = 0; si < ns; si++)
                if (t.coverages[si].size() > nxt[si] && t.coverages[si][nxt[si]].first == *lowest) nxt[si] += nc;
            last = *lowest;
            out.push_back(std::move(e));
        } else {
            cur++;
            if (cur >= ns) break;
            std::fill(nxt.begin(), nxt.end(), 0);
            last.reset();
        }
    }
    return out;
}

void print_coverage(const covh_estimator &e, const EntryAcc &a, float coverage, covh_taker &t) {  // estimators.rs:936-969
    if (e.kind != COVH_PILEUP_COUNTS) { t.add_single_coverage(coverage); return; }
    for (size_t i = 0, nh = a.hsize(); i < nh; i++) {
        u64 cov;
        if (i == 0) { const u64 c = f32_to_usize(std::floor(coverage)); cov = c == 0 ? 0 : c - 1; }
        else cov = a.hat(i);
        t.add_coverage_entry(i, cov);
    }
}
void print_zero_coverage(const covh_estimator &e, covh_taker &t, u64 entry_length) {  // estimators.rs:971-991
    if (e.kind == COVH_PILEUP_COUNTS) return;
    t.add_single_coverage(e.kind == COVH_LENGTH ? (float)entry_length : 0.0f);
}

std::string_view target_name(const covh_header *h, u32 tid) {
    return std::string_view(h->names + h->name_off[tid], h->name_off[tid + 1] - h->name_off[tid]);
}

bool check_excl(const covh_estimator *est, size_t n) {
    bool have = false; u64 x = 0;
    for (size_t i = 0; i < n; i++) {
        const int k = est[i].kind;
        if (k == COVH_MEAN || k == COVH_TRIMMED_MEAN || k == COVH_PILEUP_COUNTS || k == COVH_VARIANCE) {
            if (have && x != est[i].contig_end_exclusion) return false;
            have = true; x = est[i].contig_end_exclusion;
        }
    }
    return true;
}
u64 session_excl(const covh_estimator *est, size_t n) {
    for (size_t i = 0; i < n; i++) {
        const int k = est[i].kind;
        if (k == COVH_MEAN || k == COVH_TRIMMED_MEAN || k == COVH_PILEUP_COUNTS || k == COVH_VARIANCE)
            return est[i].contig_end_exclusion;
    }
    return 0;
}

}  // namespace

extern "C" {

const char *covh_last_error(void) { return g_err.c_str(); }
size_t covh_format_f32(float v, char *buf, size_t cap) { return fmt_float(v, buf, cap); }
size_t covh_format_f64(double v, char *buf, size_t cap) { return fmt_float(v, buf, cap); }

covh_taker *covh_taker_new(int kind, size_t num_coverages) {
    covh_taker *t = new covh_taker();
    t->kind = kind; t->num_coverages = num_coverages;
    return t;
}
void covh_taker_free(covh_taker *t) { delete t; }
const char *covh_taker_text(const covh_taker *t, size_t *len) { if (len) *len = t->text.size(); return t->text.c_str(); }
void covh_taker_clear_text(covh_taker *t) { t->text.clear(); }
size_t covh_taker_cached_coverages(const covh_taker *t, size_t stoit, float *out, size_t cap) {
    if (t->kind != COVH_TAKER_CACHED || stoit >= t->coverages.size()) return 0;
    const auto &v = t->coverages[stoit];
    for (size_t i = 0; i < v.size() && i < cap; i++) out[i] = v[i].second;
    return v.size();
}

uint32_t covh_wants(const covh_estimator *est, size_t n_est) {
    uint32_t w = 0;
    for (size_t i = 0; i < n_est; i++) {
        if (est[i].kind == COVH_TRIMMED_MEAN || est[i].kind == COVH_PILEUP_COUNTS) w |= COV_WANT_HIST;
        if (est[i].kind == COVH_ANIR) w |= COV_WANT_IDENTITY;
    }
    return w;
}

// ---- trait MosdepthGenomeCoverageEstimator (estimators.rs:245-265) over device results: the stateful face a Rust
// `impl MosdepthGenomeCoverageEstimator for GpuEstimator` forwards to, one call per trait method.
struct covh_estimator_state {
    covh_estimator e;
    EntryAcc acc;
    u64 num_mapped_reads = 0;     // what num_mapped_reads() reports (estimators.rs:993-1010)
};
covh_estimator_state *covh_estimator_new(const covh_estimator *e) {
    if (!e) return nullptr;
    covh_estimator_state *s = new covh_estimator_state();
    s->e = *e; s->acc.reset();
    return s;
}
void covh_estimator_free(covh_estimator_state *s) { delete s; }
void covh_estimator_setup(covh_estimator_state *s) { s->acc.reset(); s->num_mapped_reads = 0; }          /* fn setup(&mut self) */
/* fn add_contig(&mut self, ups_and_downs, num_mapped_reads, total_mismatches, sum_identity): the delta array is replaced by the
 * contig's integer statistics from cov_finish (+ its histogram slice); num_mapped_reads / sum_identity are the values the scan
 * loop would have passed (n_primary / n_pass / n_nonsupp and the matching identity sum, depending on the loop). */
void covh_estimator_add_contig_stats(covh_estimator_state *s, const cov_contig_stats *stats, uint64_t target_len, const uint64_t *hist,
                                     uint64_t num_mapped_reads, double sum_identity) {
    s->acc.add_contig(*stats, target_len, s->e.contig_end_exclusion, num_mapped_reads, sum_identity, hist);
    s->acc.own_hist();   // exported path: the caller's `hist` need not outlive this call (the in-tree scan drivers keep the zero-copy view)
    // Mean/ReadCount/... accumulate, the histogram family assigns (estimators.rs:434): EntryAcc keeps the sum, the assignment
    // only matters to num_mapped_reads()
    if (s->e.kind == COVH_TRIMMED_MEAN || s->e.kind == COVH_PILEUP_COUNTS || s->e.kind == COVH_VARIANCE) s->num_mapped_reads = num_mapped_reads;
    else s->num_mapped_reads += num_mapped_reads;
}
float covh_estimator_calculate_coverage(covh_estimator_state *s, const uint64_t *unobserved_contig_lengths, size_t n) {
    return calculate(s->e, s->acc, unobserved_contig_lengths, n);
}
void covh_estimator_print_coverage(const covh_estimator_state *s, float coverage, covh_taker *t) { print_coverage(s->e, s->acc, coverage, *t); }
void covh_estimator_print_zero_coverage(const covh_estimator_state *s, covh_taker *t, uint64_t entry_length) { print_zero_coverage(s->e, *t, entry_length); }
covh_estimator_state *covh_estimator_copy(const covh_estimator_state *s) { return covh_estimator_new(&s->e); }   /* fn copy(&self): fresh state, same parameters */
uint64_t covh_estimator_num_mapped_reads(const covh_estimator_state *s) { return s->num_mapped_reads; }

float covh_calculate_coverage(const covh_estimator *e, const covh_entry *en, const uint64_t *unobs, size_t n) {
    EntryAcc a;
    a.win_len = en->win_len; a.win_sum_d = en->win_sum_d; a.win_sum_d2 = en->win_sum_d2; a.win_covered = en->win_covered;
    a.full_len = en->full_len; a.full_covered = en->full_covered; a.n_reads = en->n_reads; a.mismatches = en->mismatches;
    a.win_min_d = en->win_min_d; a.sum_identity = en->sum_identity;
    if (en->hist) a.hist.assign(en->hist, en->hist + en->hist_len);
    return calculate(*e, a, unobs, n);
}

// ------------------------------------------------------------------ contig.rs:13-253
extern "C++" {
namespace {
// A few persistent workers for loops over contigs whose iterations are independent (the float expressions of calculate_coverage
// are pure functions of one contig's integer statistics): 5 000 contigs x 4 estimators are 0.33 ms on one thread, a third of the
// kernels' time at BASELINE config 2.  Threads are started on first use and sleep on a condition variable in between.
class ContigWorkers {
    std::vector<std::thread> th_;
    std::mutex m_;
    std::condition_variable cv_, done_;
    std::function<void(size_t, size_t)> fn_;
    size_t n_ = 0, parts_ = 0;
    std::atomic<size_t> next_{0};
    uint64_t gen_ = 0;
    int busy_ = 0;
    bool stop_ = false;
    void drain() {
        for (;;) {
            const size_t p = next_.fetch_add(1);
            if (p >= parts_) break;
            fn_(n_ * p / parts_, n_ * (p + 1) / parts_);
        }
    }
    void worker(uint64_t seen) {        // seen = the generation current when the thread was created: a thread added later must not replay it
        for (;;) {
            { std::unique_lock<std::mutex> lk(m_); cv_.wait(lk, [&] { return stop_ || gen_ != seen; }); if (stop_) return; seen = gen_; }
            drain();
            { std::lock_guard<std::mutex> lk(m_); if (--busy_ == 0) done_.notify_all(); }
        }
    }
public:
    ~ContigWorkers() { { std::lock_guard<std::mutex> lk(m_); stop_ = true; } cv_.notify_all(); for (auto &t : th_) t.join(); }
    // fn(lo, hi) over [0, n) in `parts` ranges; the caller works too.  One run at a time (run_m_ serialises callers).
    std::mutex run_m_;
    void run(size_t n, std::function<void(size_t, size_t)> fn) {
        const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
        size_t want = std::min<size_t>({(size_t)4, (size_t)hw, n / 512 + 1});
        { long long v; if (covknob::get("finalise_threads", v)) want = (size_t)std::max<long long>(1, v); }
        if (want <= 1) { fn(0, n); return; }
        std::lock_guard<std::mutex> rl(run_m_);
        while (th_.size() + 1 < want) { uint64_t g; { std::lock_guard<std::mutex> lk(m_); g = gen_; } th_.emplace_back([this, g] { worker(g); }); }
        { std::lock_guard<std::mutex> lk(m_); fn_ = std::move(fn); n_ = n; parts_ = want * 2; next_ = 0; busy_ = (int)th_.size(); gen_++; }
        cv_.notify_all();
        drain();
        std::unique_lock<std::mutex> lk(m_);
        done_.wait(lk, [&] { return busy_ == 0; });
    }
};
ContigWorkers &contig_workers() { static ContigWorkers w; return w; }
}  // namespace
}  // extern "C++"

int covh_contig_coverage(const covh_header *h, const covh_sample *samples, size_t n_samples, covh_taker *taker,
                         const covh_estimator *est, size_t n_est, int print_zero, covh_reads_mapped *rm_out) {
    return covh_contig_coverage_estimated(h, samples, n_samples, taker, est, n_est, print_zero, rm_out, nullptr);
}

// The same scan loop with calculate_coverage already done on the device for some or all samples (cov_set_estimators /
// cov_fetch_estimates: the same floats, bit for bit): what is left here is contig.rs:40-104's control flow — zero rows, ReadsMapped,
// the taker calls — in target order.
int covh_contig_coverage_estimated(const covh_header *h, const covh_sample *samples, size_t n_samples, covh_taker *taker,
                                   const covh_estimator *est, size_t n_est, int print_zero, covh_reads_mapped *rm_out,
                                   const float *const *estimates) {
    if (!check_excl(est, n_est)) { g_err = "estimators disagree on contig_end_exclusion"; return COV_ERR_INVALID_ARG; }
    if (estimates)
        for (size_t k = 0; k < n_est; k++)
            if (est[k].kind == COVH_PILEUP_COUNTS || est[k].kind == COVH_TPM) { g_err = "covh_contig_coverage_estimated: coverage histogram and TPM are evaluated on the host"; return COV_ERR_INVALID_ARG; }
    const u64 excl = session_excl(est, n_est);
    const u64 zero = 0;
    std::vector<float> cov(n_est);
    bool needs_acc_to_print = false;       // coverage_histogram prints the histogram itself: keeps the one-pass loop
    for (size_t k = 0; k < n_est; k++) needs_acc_to_print |= est[k].kind == COVH_PILEUP_COUNTS;
    std::vector<float> all;
    for (size_t si = 0; si < n_samples; si++) {
        const covh_sample &S = samples[si];
        taker->start_stoit(S.stoit_name);
        taker->reserve(h->n_targets, n_est, h->name_off[h->n_targets]);
        u64 mapped_total = 0;
        int64_t prev = -1;
        const float *ext = estimates ? estimates[si] : nullptr;
        if (ext || (!needs_acc_to_print && h->n_targets >= 1024)) {
            // phase 1 (contigs in parallel, or done on the device): the coverages; phase 2 (in order): zero rows, reads mapped, the taker
            if (!ext) all.resize((size_t)h->n_targets * n_est);
            if (!ext) contig_workers().run(h->n_targets, [&](size_t lo, size_t hi) {
                EntryAcc acc;
                for (size_t t = lo; t < hi; t++) {
                    const cov_contig_stats &s = S.stats[t];
                    if (s.n_pass == 0) continue;
                    acc.reset();
                    acc.add_contig(s, h->target_len[t], excl, s.n_primary, s.sum_identity_primary, S.hist);
                    for (size_t k = 0; k < n_est; k++) all[t * n_est + k] = calculate(est[k], acc, &zero, 1);
                }
            });
            auto zero_rows2 = [&](int64_t from, int64_t to) {
                for (int64_t t = from + 1; t < to; t++) {
                    taker->start_entry((size_t)t, target_name(h, (u32)t));
                    for (size_t k = 0; k < n_est; k++) print_zero_coverage(est[k], *taker, h->target_len[t]);
                    taker->finish_entry();
                }
            };
            if (print_zero && taker->names_bulk(h->names, h->name_off, h->n_targets)) {
                // every target is an entry of a cached taker: the (entry, coverage) pairs are written in place — the same pairs in the same
                // order as the calls below would append (zero rows through print_zero_coverage's values: the length for COVH_LENGTH, else 0)
                auto &v = taker->coverages[taker->cur_stoit_i];
                const size_t base = v.size();
                v.resize(base + (size_t)h->n_targets * n_est);
                std::pair<size_t, float> *o = v.data() + base;
                for (u32 t = 0; t < h->n_targets; t++, o += n_est) {
                    const cov_contig_stats &s = S.stats[t];
                    if (s.n_pass == 0) {
                        for (size_t k = 0; k < n_est; k++) o[k] = {t, est[k].kind == COVH_LENGTH ? (float)h->target_len[t] : 0.0f};
                        continue;
                    }
                    const float *c = ext ? ext + (size_t)t * n_est : &all[(size_t)t * n_est];
                    bool nonzero = false;
                    for (size_t k = 0; k < n_est; k++) { nonzero |= c[k] > 0.0f; o[k] = {t, c[k]}; }
                    if (nonzero) mapped_total += s.n_primary;           // :67-72
                }
                taker->cur_entry_i = h->n_targets ? h->n_targets - 1 : 0;
                if (rm_out) { rm_out[si].num_mapped_reads = mapped_total; rm_out[si].num_reads = S.num_detected_primary_alignments; }
                continue;
            }
            for (u32 t = 0; t < h->n_targets; t++) {
                const cov_contig_stats &s = S.stats[t];
                if (s.n_pass == 0) continue;
                if (print_zero) zero_rows2(prev, t);
                const float *c = ext ? ext + (size_t)t * n_est : &all[(size_t)t * n_est];
                bool nonzero = false;
                for (size_t k = 0; k < n_est; k++) nonzero |= c[k] > 0.0f;
                if (nonzero) mapped_total += s.n_primary;           // :67-72
                if (print_zero || nonzero) {
                    taker->start_entry(t, target_name(h, t));
                    for (size_t k = 0; k < n_est; k++) taker->add_single_coverage(c[k]);
                    taker->finish_entry();
                }
                prev = t;
            }
            if (print_zero) zero_rows2(prev, h->n_targets);
            if (rm_out) { rm_out[si].num_mapped_reads = mapped_total; rm_out[si].num_reads = S.num_detected_primary_alignments; }
            continue;
        }
        auto zero_rows = [&](int64_t from, int64_t to) {   // print_previous_zero_coverage_contigs, :255-277
            for (int64_t t = from + 1; t < to; t++) {
                taker->start_entry((size_t)t, target_name(h, (u32)t));
                for (size_t k = 0; k < n_est; k++) print_zero_coverage(est[k], *taker, h->target_len[t]);
                taker->finish_entry();
            }
        };
        EntryAcc acc;
        for (u32 t = 0; t < h->n_targets; t++) {
            const cov_contig_stats &s = S.stats[t];
            if (s.n_pass == 0) continue;   // no considered record: the scan never allocated this contig
            if (print_zero) zero_rows(prev, t);
            acc.reset();
            acc.add_contig(s, h->target_len[t], excl, s.n_primary, s.sum_identity_primary, S.hist);
            bool nonzero = false;
            for (size_t k = 0; k < n_est; k++) { cov[k] = calculate(est[k], acc, &zero, 1); nonzero |= cov[k] > 0.0f; }
            if (nonzero) mapped_total += s.n_primary;           // :67-72
            if (print_zero || nonzero) {
                taker->start_entry(t, target_name(h, t));
                for (size_t k = 0; k < n_est; k++) print_coverage(est[k], acc, cov[k], *taker);
                taker->finish_entry();
            }
            prev = t;
        }
        if (print_zero) zero_rows(prev, h->n_targets);
        if (rm_out) { rm_out[si].num_mapped_reads = mapped_total; rm_out[si].num_reads = S.num_detected_primary_alignments; }
    }
    return COV_OK;
}

// ------------------------------------------------------------------ genome.rs:17-322
int covh_genome_coverage_with_contig_names(const covh_header *h, const covh_sample *samples, size_t n_samples,
                                           const int32_t *genome_of_tid, const char *const *genome_names,
                                           size_t n_genomes, covh_taker *taker, int print_zero,
                                           const covh_estimator *est, size_t n_est, covh_reads_mapped *rm_out) {
    if (!check_excl(est, n_est)) { g_err = "estimators disagree on contig_end_exclusion"; return COV_ERR_INVALID_ARG; }
    const u64 excl = session_excl(est, n_est);
    std::vector<std::vector<u32>> refs(n_genomes);
    for (u32 t = 0; t < h->n_targets; t++) if (genome_of_tid[t] >= 0) refs[genome_of_tid[t]].push_back(t);
    std::vector<float> cov(n_est);
    for (size_t si = 0; si < n_samples; si++) {
        const covh_sample &S = samples[si];
        taker->start_stoit(S.stoit_name);
        std::vector<EntryAcc> acc(n_genomes);
        std::vector<u64> reads_in_genome(n_genomes, 0);
        bool any_seen = false;
        for (u32 t = 0; t < h->n_targets; t++) {
            const cov_contig_stats &s = S.stats[t];
            if (s.n_pass == 0) continue;
            any_seen = true;
            const int32_t g = genome_of_tid[t];
            if (g < 0) continue;                               // :170-171
            reads_in_genome[g] += s.n_pass;                    // :173-174 every record passing the flag filter
            acc[g].add_contig(s, h->target_len[t], excl, s.n_pass, s.sum_identity_nonsupp, S.hist);
        }
        u64 mapped_total = 0;
        if (!any_seen && S.num_detected_primary_alignments == 0) {
            // warn only (:230-234)
        } else {
            std::vector<u64> unobs;
            for (size_t gi = 0; gi < n_genomes; gi++) {
                unobs.clear();
                u64 genome_len = 0;
                for (u32 t : refs[gi]) { genome_len += h->target_len[t]; if (S.stats[t].n_pass == 0) unobs.push_back(h->target_len[t]); }
                bool nonzero = false;
                for (size_t k = 0; k < n_est; k++) { cov[k] = calculate(est[k], acc[gi], unobs.data(), unobs.size()); nonzero |= cov[k] > 0.0f; }
                if (nonzero) mapped_total += reads_in_genome[gi];
                if (print_zero || nonzero) {
                    taker->start_entry(gi, genome_names[gi]);
                    for (size_t k = 0; k < n_est; k++) {
                        if (cov[k] > 0.0f) print_coverage(est[k], acc[gi], cov[k], *taker);
                        else print_zero_coverage(est[k], *taker, genome_len);
                    }
                    taker->finish_entry();
                }
            }
        }
        if (rm_out) { rm_out[si].num_mapped_reads = mapped_total; rm_out[si].num_reads = S.num_detected_primary_alignments; }
    }
    return COV_OK;
}

// The same scan of one sample with the genomes aggregated and evaluated on the device (cov_set_genomes / cov_fetch_genome_estimates:
// the same floats, bit for bit): what is left is the loop over genomes above — zero rows, --no-zeros, ReadsMapped, the taker calls.
int covh_genome_coverage_estimated(const char *stoit_name, uint64_t num_detected_primary_alignments, int any_contig_seen,
                                   const char *const *genome_names, size_t n_genomes, covh_taker *taker, int print_zero,
                                   const covh_estimator *est, size_t n_est, const float *estimates, const cov_genome_stats *gstats,
                                   covh_reads_mapped *rm_out) {
    if (!check_excl(est, n_est)) { g_err = "estimators disagree on contig_end_exclusion"; return COV_ERR_INVALID_ARG; }
    for (size_t k = 0; k < n_est; k++)
        if (est[k].kind == COVH_PILEUP_COUNTS || est[k].kind == COVH_TPM) { g_err = "covh_genome_coverage_estimated: coverage histogram and TPM are evaluated on the host"; return COV_ERR_INVALID_ARG; }
    if (n_genomes && n_est && (!estimates || !gstats)) { g_err = "covh_genome_coverage_estimated: no estimates"; return COV_ERR_INVALID_ARG; }
    taker->start_stoit(stoit_name);
    u64 mapped_total = 0;
    if (!any_contig_seen && num_detected_primary_alignments == 0) {
        // warn only (:230-234)
    } else {
        for (size_t gi = 0; gi < n_genomes; gi++) {
            const float *c = estimates + gi * n_est;
            bool nonzero = false;
            for (size_t k = 0; k < n_est; k++) nonzero |= c[k] > 0.0f;
            if (nonzero) mapped_total += gstats[gi].reads_in_genome;
            if (print_zero || nonzero) {
                taker->start_entry(gi, genome_names[gi]);
                for (size_t k = 0; k < n_est; k++) {
                    if (c[k] > 0.0f) taker->add_single_coverage(c[k]);
                    else print_zero_coverage(est[k], *taker, gstats[gi].genome_len);
                }
                taker->finish_entry();
            }
        }
    }
    if (rm_out) { rm_out->num_mapped_reads = mapped_total; rm_out->num_reads = num_detected_primary_alignments; }
    return COV_OK;
}

// ------------------------------------------------------------------ genome.rs:419-929
namespace {
struct SepCtx {
    const covh_header *h; uint8_t split; bool single; bool err = false;
    std::string_view genome(u32 tid) {   // extract_genome, :799-805
        std::string_view n = target_name(h, tid);
        size_t p = n.find((char)split);
        if (p == std::string_view::npos) { err = true; return n; }
        return n.substr(0, p);
    }
};
struct Unobs { std::vector<u64> v; size_t first_tid = 0; };

void fill_backwards(SepCtx &c, u32 current_tid, std::string_view target, Unobs &u) {   // :807-853
    u.v.clear();
    if (current_tid == 0) { u.first_tid = 0; return; }
    u32 my = current_tid - 1;
    while (c.single || c.genome(my) == target) {
        u.v.push_back(c.h->target_len[my]);
        if (my == 0) { u.first_tid = 0; return; }
        my--;
    }
    u.first_tid = (size_t)my + 1;
}
void fill_backwards_to_last(SepCtx &c, u32 current_tid, u32 last_tid, std::string_view target, Unobs &u) {  // :477-499
    if (current_tid == 0) return;
    for (u32 my = last_tid + 1; my < current_tid; my++) {
        if (c.single || c.genome(my) == target) u.v.push_back(c.h->target_len[my]); else break;
    }
}
void fill_forwards(SepCtx &c, u32 current_tid, const std::optional<std::string_view> &target, Unobs &u) {   // :448-475
    if (!target) return;
    for (u32 my = current_tid + 1; my < c.h->n_targets; my++) {
        if (c.single || c.genome(my) == *target) u.v.push_back(c.h->target_len[my]); else break;
    }
}
// print_previous_zero_coverage_genomes2, :859-929
void zero_genomes2(SepCtx &c, const std::optional<std::string_view> &last_genome, std::string_view current_genome,
                   u32 current_tid, const covh_estimator *est, size_t n_est, covh_taker &t) {
    std::string_view my_current = current_genome;
    u32 tid = current_tid;
    std::vector<std::string_view> names; std::vector<size_t> first_tids; std::vector<u64> lens;
    u64 unobserved = 0;
    std::optional<u32> last_first;
    for (;;) {
        std::string_view g = c.genome(tid);
        if (last_genome && g == *last_genome) break;
        else if (g != my_current) {
            if (last_first) {
                if (!last_genome || g != *last_genome) { first_tids.push_back(*last_first); names.push_back(my_current); lens.push_back(unobserved); }
            }
            my_current = g; last_first = tid; unobserved = c.h->target_len[tid];
        } else if (g != current_genome) { last_first = tid; unobserved += c.h->target_len[tid]; }
        if (tid == 0) break;
        tid--;
    }
    if (last_first) { first_tids.push_back(*last_first); names.push_back(my_current); lens.push_back(unobserved); }
    for (size_t i = names.size(); i-- > 0;) {
        t.start_entry(first_tids[i], names[i]);
        for (size_t k = 0; k < n_est; k++) print_zero_coverage(est[k], t, lens[i]);
        t.finish_entry();
    }
}
}  // namespace

int covh_genome_coverage_separator(const covh_header *h, const covh_sample *samples, size_t n_samples,
                                   uint8_t split_char, covh_taker *taker, int print_zero,
                                   const covh_estimator *est, size_t n_est, int single_genome,
                                   covh_reads_mapped *rm_out) {
    if (!check_excl(est, n_est)) { g_err = "estimators disagree on contig_end_exclusion"; return COV_ERR_INVALID_ARG; }
    const u64 excl = session_excl(est, n_est);
    std::vector<float> cov(n_est);
    for (size_t si = 0; si < n_samples; si++) {
        const covh_sample &S = samples[si];
        taker->start_stoit(S.stoit_name);
        SepCtx cx{h, split_char, single_genome != 0};
        EntryAcc acc;
        Unobs u;
        bool doing_first = true;
        u32 last_tid = 0;
        std::optional<std::string_view> last_genome;
        u64 mapped_total = 0, n_in_genome = 0;
        auto add_last_contig = [&]() {
            // estimator.add_contig(&ups_and_downs, ...) for the contig the scan was in (last_tid); before the
            // first mapped record ups_and_downs is an empty Vec, which adds nothing
            if (doing_first) return;
            const cov_contig_stats &s = S.stats[last_tid];
            acc.add_contig(s, h->target_len[last_tid], excl, s.n_nonsupp, s.sum_identity_primary, S.hist);
        };
        // print_last_genomes, :331-416
        auto print_last_genomes = [&](std::string_view current_genome, u32 tid_to_print_zeros_to, bool had_contig) -> bool {
            if (had_contig) add_last_contig();
            bool positive = false;
            for (size_t k = 0; k < n_est; k++) { cov[k] = calculate(est[k], acc, u.v.data(), u.v.size()); positive |= cov[k] > 0.0f; }
            if ((print_zero || positive) && last_genome) {
                taker->start_entry(u.first_tid, *last_genome);
                for (size_t k = 0; k < n_est; k++) {
                    if (cov[k] > 0.0f) print_coverage(est[k], acc, cov[k], *taker);
                    else print_zero_coverage(est[k], *taker, 9);
                }
                taker->finish_entry();
            }
            acc.reset();
            if (print_zero && !cx.single) zero_genomes2(cx, last_genome, current_genome, tid_to_print_zeros_to, est, n_est, *taker);
            return positive;
        };
        for (u32 tid = 0; tid < h->n_targets; tid++) {
            const cov_contig_stats &s = S.stats[tid];
            if (s.n_pass == 0) continue;
            std::string_view current_genome = cx.single ? std::string_view() : cx.genome(tid);
            if (cx.err) { g_err = "Contig name does not contain split symbol, so cannot determine which genome it belongs to"; return COV_ERR_INVALID_ARG; }
            if (doing_first) {
                acc.reset();
                fill_backwards(cx, tid, current_genome, u);
                last_genome = current_genome;
                if (print_zero && !cx.single) zero_genomes2(cx, std::nullopt, current_genome, tid, est, n_est, *taker);
                doing_first = false;
            } else if (current_genome == *last_genome) {
                add_last_contig();
                fill_backwards_to_last(cx, tid, last_tid, current_genome, u);
            } else {
                fill_backwards_to_last(cx, tid, last_tid, *last_genome, u);
                if (print_last_genomes(current_genome, tid, true)) mapped_total += n_in_genome;
                n_in_genome = 0;
                last_genome = current_genome;
                fill_backwards(cx, tid, current_genome, u);
            }
            if (cx.err) { g_err = "Contig name does not contain split symbol, so cannot determine which genome it belongs to"; return COV_ERR_INVALID_ARG; }
            last_tid = tid;
            n_in_genome += s.n_nonsupp;    // :677-682
        }
        if (doing_first && S.num_detected_primary_alignments == 0) {
            // warn only (:731-735)
        } else {
            static const char g1[] = "genome1";
            const bool had_contig = !doing_first;
            if (cx.single) last_genome = std::string_view(g1, 7);   // :739-741
            fill_forwards(cx, last_tid, last_genome, u);
            if (print_last_genomes(std::string_view(), h->n_targets - 1, had_contig)) mapped_total += n_in_genome;
            if (cx.err) { g_err = "Contig name does not contain split symbol, so cannot determine which genome it belongs to"; return COV_ERR_INVALID_ARG; }
        }
        if (rm_out) { rm_out[si].num_mapped_reads = mapped_total; rm_out[si].num_reads = S.num_detected_primary_alignments; }
    }
    return COV_OK;
}

uint32_t covh_genome_separator_ids(const covh_header *h, uint8_t split_char, int single_genome, int32_t *gid_of_tid) {
    if (single_genome) { for (u32 t = 0; t < h->n_targets; t++) gid_of_tid[t] = 0; return 1; }
    std::unordered_map<std::string_view, int32_t> ids;
    std::string_view prev;
    for (u32 t = 0; t < h->n_targets; t++) {
        const std::string_view n = target_name(h, t);
        const size_t p = n.find((char)split_char);
        if (p == std::string_view::npos) return 0;
        const std::string_view g = n.substr(0, p);
        gid_of_tid[t] = (t != 0 && g == prev) ? gid_of_tid[t - 1] : ids.emplace(g, (int32_t)ids.size()).first->second;
        prev = g;
    }
    return (uint32_t)ids.size();
}

int covh_genome_separator_entries(const covh_header *h, const covh_sample *sample, const int32_t *gid_of_tid, const covh_estimator *est,
                                  size_t n_est, cov_genome_entry *entries, float *estimates, size_t *n_entries) {
    if (!check_excl(est, n_est)) { g_err = "estimators disagree on contig_end_exclusion"; return COV_ERR_INVALID_ARG; }
    const u64 excl = session_excl(est, n_est);
    const u32 n = h->n_targets;
    std::vector<uint8_t> obs(n);
    for (u32 t = 0; t < n; t++) obs[t] = sample->stats[t].n_pass != 0;
    std::vector<u32> blk(n), prev1(n), next(n), row((size_t)n + 1), tids(n), first(n);
    std::vector<int32_t> egid(n);
    const u32 ne = sepc::entries_cpu(gid_of_tid, obs.data(), n, blk.data(), prev1.data(), next.data(), row.data(), tids.data(), first.data(), egid.data());
    EntryAcc acc;
    std::vector<u64> unobs;
    for (u32 e = 0; e < ne; e++) {
        acc.reset(); unobs.clear();
        cov_genome_entry &o = entries[e];
        o.reads = 0; o.first_tid = first[e]; o.gid = egid[e]; o.n_contigs_seen = 0; o.any_nonzero = 0;
        for (u32 i = row[e]; i < row[e + 1]; i++) {
            const u32 t = tids[i];
            const cov_contig_stats &s = sample->stats[t];
            if (!obs[t]) { unobs.push_back(h->target_len[t]); continue; }
            acc.add_contig(s, h->target_len[t], excl, s.n_nonsupp, s.sum_identity_primary, sample->hist);      // host_coverage.cpp: add_last_contig
            o.reads += s.n_nonsupp; o.n_contigs_seen++;
        }
        for (size_t k = 0; k < n_est; k++) {
            const float c = calculate(est[k], acc, unobs.data(), unobs.size());
            estimates[(size_t)e * n_est + k] = c;
            if (c > 0.0f) o.any_nonzero = 1;
        }
    }
    *n_entries = ne;
    return COV_OK;
}

// covh_genome_coverage_separator's control flow over entries that exist already: print_last_genomes at every change of entry and at the
// end, zero_genomes2 in front of the first entry, between two entries and behind the last one.  zero_genomes2 walks down from the
// entry's first_tid instead of its first observed target: the targets between the two carry the entry's own name, which it passes over.
int covh_genome_coverage_separator_estimated(const covh_header *h, const char *stoit_name, uint64_t num_detected_primary_alignments,
                                             uint8_t split_char, int single_genome, covh_taker *taker, int print_zero,
                                             const covh_estimator *est, size_t n_est, const cov_genome_entry *entries, size_t n_entries,
                                             const float *estimates, covh_reads_mapped *rm_out) {
    if (!check_excl(est, n_est)) { g_err = "estimators disagree on contig_end_exclusion"; return COV_ERR_INVALID_ARG; }
    for (size_t k = 0; k < n_est; k++)
        if (est[k].kind == COVH_PILEUP_COUNTS || est[k].kind == COVH_TPM) { g_err = "covh_genome_coverage_separator_estimated: coverage histogram and TPM are evaluated on the host"; return COV_ERR_INVALID_ARG; }
    if (n_entries == 0 || !entries || (n_est && !estimates)) { g_err = "covh_genome_coverage_separator_estimated: no entries (a sample without an observed target runs covh_genome_coverage_separator)"; return COV_ERR_INVALID_ARG; }
    taker->start_stoit(stoit_name);
    SepCtx cx{h, split_char, single_genome != 0};
    static const char g1[] = "genome1";
    u64 mapped_total = 0;
    std::optional<std::string_view> last_genome;
    for (size_t e = 0; e <= n_entries; e++) {
        std::string_view current_genome;
        if (e < n_entries) {
            if (entries[e].first_tid >= h->n_targets) { g_err = "covh_genome_coverage_separator_estimated: first_tid outside the header"; return COV_ERR_INVALID_ARG; }
            if (!cx.single) current_genome = cx.genome(entries[e].first_tid);
        }
        if (e != 0) {      // print_last_genomes of entry e - 1
            const cov_genome_entry &E = entries[e - 1];
            const float *c = estimates + (e - 1) * n_est;
            bool positive = false;
            for (size_t k = 0; k < n_est; k++) positive |= c[k] > 0.0f;
            if (print_zero || positive) {
                taker->start_entry(E.first_tid, cx.single ? std::string_view(g1, 7) : *last_genome);
                for (size_t k = 0; k < n_est; k++) {
                    if (c[k] > 0.0f) taker->add_single_coverage(c[k]);
                    else print_zero_coverage(est[k], *taker, 9);
                }
                taker->finish_entry();
            }
            if (positive) mapped_total += E.reads;
        }
        if (print_zero && !cx.single)
            zero_genomes2(cx, last_genome, current_genome, e < n_entries ? entries[e].first_tid : h->n_targets - 1, est, n_est, *taker);
        if (cx.err) { g_err = "Contig name does not contain split symbol, so cannot determine which genome it belongs to"; return COV_ERR_INVALID_ARG; }
        last_genome = current_genome;
    }
    if (rm_out) { rm_out->num_mapped_reads = mapped_total; rm_out->num_reads = num_detected_primary_alignments; }
    return COV_OK;
}

// ------------------------------------------------------------------ coverage_printer.rs
void covh_print_headers(covh_taker *t, int printer, const char *entry_type, const char *const *headers, size_t n) {
    if (printer == 0 || printer == 1) {   // :130-137
        t->text += "Sample\t"; t->text += entry_type;
        for (size_t i = 0; i < n; i++) { t->text += '\t'; t->text += headers[i]; }
        t->text += '\n';
    }
}

namespace {
bool contains(const int64_t *v, size_t n, size_t x) { for (size_t i = 0; i < n; i++) if ((size_t)v[i] == x) return true; return false; }
static std::string rstrip_cr(const std::string &s) { size_t n = s.size(); while (n && s[n - 1] == '\r') n--; return s.substr(0, n); }
static void put_name(std::string &o, std::string_view v) { size_t n = v.size(); while (n && v[n - 1] == '\r') n--; o.append(v.data(), n); }
double round4(double v) { return std::round(v) / 10000.0; }  // (x * 10000.0).round() / 10000.0 with x*10000 passed in

void print_sparse(covh_taker &t, const covh_reads_mapped *rm, const int64_t *norm, size_t n_norm, int64_t rpkm_col, int64_t tpm_col) {
    const size_t nc = t.num_coverages;
    size_t extra_cols = 0;
    for (auto n : t.entry_names) if (n) { const std::string_view v = n.view(); extra_cols = std::count(v.begin(), v.end(), '\t'); break; }
    auto all = iterate_cached(t);
    std::string &o = t.text;
    auto print_previous = [&](const std::vector<const EntryAndCoverages *> &rows, size_t si) {
        std::vector<std::optional<float>> mult(nc), totals(nc);
        for (size_t k = 0; k < n_norm; k++) {
            const size_t i = (size_t)norm[k];
            float tot = 0.0f;
            for (auto r : rows) tot += r->coverages[i];
            totals[i] = tot;
            if (rm) mult[i] = (float)rm[si].num_mapped_reads / (float)rm[si].num_reads;
        }
        if (tpm_col >= 0) { float tot = 0.0f; for (auto r : rows) tot += r->coverages[tpm_col]; totals[tpm_col] = tot; }
        const std::string &stoit = t.stoit_names[si];
        if (n_norm) {
            o += stoit; o += "\tunmapped"; o.append(extra_cols, '\t');
            for (size_t k = 0; k < n_norm; k++) {
                const size_t col = (size_t)norm[k];
                const size_t lo = k == 0 ? 0 : (size_t)norm[k - 1] + 1;
                for (size_t j = lo; j < col; j++) o += "\tNA";
                o += '\t'; o += f32s(100.0f * (1.0f - *mult[col]));
            }
            for (size_t j = (size_t)norm[n_norm - 1] + 1; j < nc; j++) o += "\tNA";
            o += '\n';
        }
        format_rows(o, rows.size(), stoit.size() + 24 + 12 * nc, [&](std::string &o, size_t k) {
            const EntryAndCoverages *r = rows[k];
            o += stoit; o += '\t'; put_name(o, t.entry_names[r->entry_index].view());
            for (size_t i = 0; i < nc; i++) {
                o += '\t';
                const float c = r->coverages[i];
                if (contains(norm, n_norm, i)) put_float(o, c * 100.0f * *mult[i] / *totals[i]);          // :285-286
                else if (rpkm_col == (int64_t)i) { const u64 n = rm[si].num_mapped_reads; put_float(o, n == 0 ? 0.0f : c / (float)n); }
                else if (tpm_col == (int64_t)i) {
                    const u64 n = rm[si].num_mapped_reads;
                    if (n == 0) put_float(o, 0.0);
                    else put_float(o, (double)std::exp(std::log(c) - std::log(*totals[i])) * (double)1000000);   // :320-323
                } else put_float(o, c);
            }
            o += '\n';
        });
    };
    std::vector<const EntryAndCoverages *> rows;
    size_t cur = 0;
    for (auto &e : all) {
        if (cur != e.stoit_index) { print_previous(rows, cur); rows.clear(); cur = e.stoit_index; }
        rows.push_back(&e);
    }
    if (!t.stoit_names.empty()) print_previous(rows, cur);
}

void print_dense(covh_taker &t, const char *entry_type, const char *const *headers, size_t n_headers, const covh_reads_mapped *rm,
                 size_t n_samples, const int64_t *norm, size_t n_norm, int64_t rpkm_col, int64_t tpm_col) {
    const size_t nc = t.num_coverages;
    std::string &o = t.text;
    o += entry_type;
    for (auto &s : t.stoit_names) for (size_t i = 0; i < n_headers; i++) { o += '\t'; o += s; o += ' '; o += headers[i]; }
    o += '\n';
    std::vector<float> mult;
    if (rm) for (size_t i = 0; i < n_samples; i++) mult.push_back((float)rm[i].num_mapped_reads / (float)rm[i].num_reads);
    if (n_norm) {
        o += "unmapped";
        o.append(std::count(entry_type, entry_type + strlen(entry_type), '\t'), '\t');
        for (size_t si = 0; si < t.stoit_names.size(); si++) {
            for (size_t k = 0; k < n_norm; k++) {
                const size_t col = (size_t)norm[k];
                const size_t lo = k == 0 ? 0 : (size_t)norm[k - 1] + 1;
                for (size_t j = lo; j < col; j++) o += "\tNA";
                o += '\t'; o += f32s(100.0f * (1.0f - mult[si]));
            }
            for (size_t j = (size_t)norm[n_norm - 1] + 1; j < nc; j++) o += "\tNA";
        }
        o += '\n';
    }
    {   // The usual table — every sample lists the same entries, in increasing order (one entry per reference with zero rows printed, or
        // the same mapped references in every sample) — read where the taker keeps it: CoverageTakerTypeIterator's merge
        // (iterate_cached below) yields exactly these rows in this order, at the cost of a small vector per row.
        const size_t ns = t.stoit_names.size();
        bool plain = ns > 0 && nc > 0;
        const size_t len0 = plain ? t.coverages[0].size() : 0;
        plain = plain && len0 % nc == 0;
        for (size_t si = 1; plain && si < ns; si++) plain = t.coverages[si].size() == len0;
        const size_t n_rows = plain ? len0 / nc : 0;
        for (size_t k = 0; plain && k < n_rows; k++) {
            const size_t e = t.coverages[0][k * nc].first;
            if (k && e <= t.coverages[0][(k - 1) * nc].first) plain = false;
            for (size_t si = 1; plain && si < ns; si++) plain = t.coverages[si][k * nc].first == e;
        }
        long long use_plain = 1;
        (void)covknob::get("printer_plain", use_plain);      // tests: 0 = always through the merge below
        if (plain && n_rows >= 4096 && use_plain) {
            std::vector<std::vector<std::optional<float>>> totals(ns, std::vector<std::optional<float>>(nc));
            for (size_t si = 0; si < ns; si++) {       // the same additions in the same order as the merge's (entry by entry, sample by sample: a total is per sample)
                auto addt = [&](size_t i) { auto &x = totals[si][i]; for (size_t k = 0; k < n_rows; k++) { const float c = t.coverages[si][k * nc + i].second; x = x ? *x + c : c; } };
                for (size_t k = 0; k < n_norm; k++) addt((size_t)norm[k]);
                if (tpm_col >= 0) addt((size_t)tpm_col);
            }
            format_rows(o, n_rows, 24 + 12 * nc * ns, [&](std::string &o, size_t k) {
                put_name(o, t.entry_names[t.coverages[0][k * nc].first].view());
                for (size_t si = 0; si < ns; si++)
                    for (size_t i = 0; i < nc; i++) {
                        o += '\t';
                        const float c = t.coverages[si][k * nc + i].second;
                        if (contains(norm, n_norm, i)) put_float(o, c / *totals[si][i] * 100.0f * mult[si]);   // :496-502
                        else if (rpkm_col == (int64_t)i) { const u64 n = rm[si].num_mapped_reads; put_float(o, n == 0 ? 0.0f : c / (float)n); }
                        else if (tpm_col == (int64_t)i) {
                            const u64 n = rm[si].num_mapped_reads;
                            put_float(o, n == 0 ? 0.0f : std::exp(std::log(c) - std::log(*totals[si][i])) * (float)1000000);  // :536-539
                        } else put_float(o, c);
                    }
                o += '\n';
            });
            return;
        }
    }
    auto all = iterate_cached(t);
    std::vector<std::vector<std::optional<float>>> totals(t.stoit_names.size(), std::vector<std::optional<float>>(nc));
    std::vector<std::vector<const EntryAndCoverages *>> by_stoit;
    for (auto &e : all) {
        auto addt = [&](size_t i) { auto &x = totals[e.stoit_index][i]; x = x ? *x + e.coverages[i] : e.coverages[i]; };
        for (size_t k = 0; k < n_norm; k++) addt((size_t)norm[k]);
        if (tpm_col >= 0) addt((size_t)tpm_col);
        if (by_stoit.size() <= e.stoit_index) by_stoit.emplace_back();
        by_stoit[e.stoit_index].push_back(&e);
    }
    if (by_stoit.empty()) return;
    for (size_t k = 0; k < by_stoit[0].size(); k++) {
        o += rstrip_cr(*t.entry_names[by_stoit[0][k]->entry_index]);
        for (size_t si = 0; si < by_stoit.size(); si++) {
            const EntryAndCoverages *e = by_stoit[si][k];
            for (size_t i = 0; i < e->coverages.size(); i++) {
                o += '\t';
                const float c = e->coverages[i];
                if (contains(norm, n_norm, i)) o += f32s(c / *totals[e->stoit_index][i] * 100.0f * mult[si]);   // :496-502
                else if (rpkm_col == (int64_t)i) { const u64 n = rm[si].num_mapped_reads; o += f32s(n == 0 ? 0.0f : c / (float)n); }
                else if (tpm_col == (int64_t)i) {
                    const u64 n = rm[si].num_mapped_reads;
                    o += f32s(n == 0 ? 0.0f : std::exp(std::log(c) - std::log(*totals[e->stoit_index][i])) * (float)1000000);  // :536-539
                } else o += f32s(c);
            }
        }
        o += '\n';
    }
}

void print_metabat(covh_taker &t) {   // coverage_printer.rs:57-119
    std::string &o = t.text;
    o += "contigName\tcontigLen\ttotalAvgDepth";
    for (auto &s : t.stoit_names) { o += '\t'; o += s; o += ".bam\t"; o += s; o += ".bam-var"; }
    o += '\n';
    auto all = iterate_cached(t);
    std::vector<std::vector<const EntryAndCoverages *>> by_stoit;
    for (auto &e : all) { if (by_stoit.size() <= e.stoit_index) by_stoit.emplace_back(); by_stoit[e.stoit_index].push_back(&e); }
    if (by_stoit.empty()) return;
    for (size_t k = 0; k < by_stoit[0].size(); k++) {
        float total = 0.0f;
        for (auto &st : by_stoit) total += st[k]->coverages[1];
        o += *t.entry_names[k]; o += '\t'; o += f32s(by_stoit[0][k]->coverages[0]); o += '\t';
        o += f64s(round4((double)total * 10000.0 / (double)t.coverages.size()));
        for (auto &st : by_stoit) {
            o += '\t'; o += f64s(round4((double)st[k]->coverages[1] * 10000.0));
            o += '\t'; o += f64s(round4((double)st[k]->coverages[2] * 10000.0));
        }
        o += '\n';
    }
}
}  // namespace

// ---- trait CoverageTaker (coverage_takers.rs:29-38) as plain calls, for hosts that drive a taker themselves
void covh_taker_start_stoit(covh_taker *t, const char *stoit_name) { t->start_stoit(stoit_name); }
void covh_taker_start_entry(covh_taker *t, size_t entry_order_id, const char *entry_name) { t->start_entry(entry_order_id, entry_name); }
void covh_taker_add_single_coverage(covh_taker *t, float coverage) { t->add_single_coverage(coverage); }
void covh_taker_add_coverage_entry(covh_taker *t, uint64_t num_reads, uint64_t num_bases) { t->add_coverage_entry(num_reads, num_bases); }
void covh_taker_finish_entry(covh_taker *t) { t->finish_entry(); }
int covh_taker_names_mismatch(const covh_taker *t) { return t->mismatch ? 1 : 0; }
// CoverageTakerTypeIterator (coverage_takers.rs:265-377) flattened: returns the number of (entry, stoit) items and fills up to
// `cap` of them; coverages holds num_coverages floats per item.
size_t covh_taker_iterate(const covh_taker *t, uint64_t *entry_index, uint64_t *stoit_index, float *coverages, size_t cap) {
    const auto all = iterate_cached(*t);
    for (size_t i = 0; i < all.size() && i < cap; i++) {
        if (entry_index) entry_index[i] = all[i].entry_index;
        if (stoit_index) stoit_index[i] = all[i].stoit_index;
        if (coverages) for (size_t k = 0; k < all[i].coverages.size(); k++) coverages[i * t->num_coverages + k] = all[i].coverages[k];
    }
    return all.size();
}

void covh_finalise_printing(covh_taker *t, int printer, const char *entry_type, const char *const *headers,
                            size_t n_headers, const covh_reads_mapped *rm, size_t n_samples,
                            const int64_t *norm, size_t n_norm, int64_t rpkm_col, int64_t tpm_col) {
    if (printer == 1) print_sparse(*t, rm, norm, n_norm, rpkm_col, tpm_col);
    else if (printer == 2) print_dense(*t, entry_type, headers, n_headers, rm, n_samples, norm, n_norm, rpkm_col, tpm_col);
    else if (printer == 3) print_metabat(*t);
}

}  // extern "C"

// =====================================================================================================================
// Per-gene coverage (--gff): src/genes.rs.  The pileup stays on the device (the depth of a contig comes through a
// callback: cov_copy_depth in the product, the oracle's depth in CPU tests); what genes.rs adds on top of the contig
// scan — GFF parsing (:42-161), gene resolution against the header (:346-419), per-gene window statistics over the
// contig's depth (:508-535) and per-gene read aggregates by leftmost position (:521-526) — is this host code, feeding the
// same calculate() / print_coverage() as the contig scan.
namespace {

struct GeneDef { std::string id, contig; u64 start, end; };

bool parse_u64(const std::string &s, u64 &v) {   // Rust u64::from_str: optional '+', decimal digits, no overflow
    size_t i = 0;
    if (i < s.size() && s[i] == '+') i++;
    if (i >= s.size()) return false;
    u64 x = 0;
    for (; i < s.size(); i++) {
        if (s[i] < '0' || s[i] > '9') return false;
        const u64 d = (u64)(s[i] - '0');
        if (x > (0xffffffffffffffffull - d) / 10) return false;
        x = x * 10 + d;
    }
    v = x;
    return true;
}
std::string trim(const std::string &s) {
    size_t a = 0, b = s.size();
    auto ws = [](unsigned char c) { return c == ' ' || (c >= 9 && c <= 13); };
    while (a < b && ws((unsigned char)s[a])) a++;
    while (b > a && ws((unsigned char)s[b - 1])) b--;
    return s.substr(a, b - a);
}
bool gff_attribute(const std::string &attrs, const std::string &key, std::string &out) {   // genes.rs:144-161
    size_t p = 0;
    while (p <= attrs.size()) {
        size_t q = attrs.find(';', p);
        if (q == std::string::npos) q = attrs.size();
        const std::string entry = trim(attrs.substr(p, q - p));
        if (!entry.empty()) {
            if (entry.compare(0, key.size() + 1, key + "=") == 0) { out = trim(entry.substr(key.size() + 1)); return true; }
            if (entry.compare(0, key.size() + 1, key + " ") == 0) {
                std::string v = trim(entry.substr(key.size() + 1));
                size_t a = 0, b = v.size();
                while (a < b && v[a] == '"') a++;
                while (b > a && v[b - 1] == '"') b--;
                out = v.substr(a, b - a);
                return true;
            }
        }
        p = q + 1;
    }
    return false;
}

struct ResolvedGene { size_t entry_id; std::string name; u64 start, end; };

}  // namespace

struct covh_genes { std::vector<GeneDef> genes; };

extern "C" {

covh_genes *covh_genes_read_gff(const char *path, const char *feature_type, char *err, size_t errcap) {
    FILE *fh = fopen(path, "rb");
    if (!fh) {
        if (err && errcap) snprintf(err, errcap, "Failed to open GFF file %s", path);
        return nullptr;
    }
    std::string all;
    char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, fh)) > 0) all.append(buf, n);
    fclose(fh);
    covh_genes *g = new covh_genes();
    u64 auto_id = 0;
    size_t p = 0;
    while (p < all.size()) {
        size_t q = all.find('\n', p);
        if (q == std::string::npos) q = all.size();
        std::string line = all.substr(p, q - p);
        p = q + 1;
        {   // trim_end
            size_t b = line.size();
            while (b > 0 && (line[b - 1] == ' ' || ((unsigned char)line[b - 1] >= 9 && (unsigned char)line[b - 1] <= 13))) b--;
            line.resize(b);
        }
        if (line.empty() || line[0] == '#') continue;
        std::vector<std::string> f;
        for (size_t a = 0;;) {
            const size_t t = line.find('\t', a);
            if (t == std::string::npos) { f.push_back(line.substr(a)); break; }
            f.push_back(line.substr(a, t - a));
            a = t + 1;
        }
        if (f.size() < 8) continue;
        if (feature_type && f[2] != feature_type) continue;
        u64 s1, e1;
        if (!parse_u64(f[3], s1) || !parse_u64(f[4], e1)) continue;
        if (s1 == 0 || e1 < s1) continue;
        const std::string attrs = f.size() > 8 ? f[8] : std::string();
        std::string id;
        bool have = false;
        for (const char *k : {"ID", "locus_tag", "gene_id", "Name", "gene", "Parent"}) {
            std::string v;
            if (gff_attribute(attrs, k, v) && !v.empty()) { id = v; have = true; break; }
        }
        if (!have) { auto_id++; id = f[0] + "_gene_" + std::to_string(auto_id); }
        g->genes.push_back(GeneDef{id, f[0], s1 - 1, e1});
    }
    return g;
}

covh_genes *covh_genes_from_arrays(const char *const *ids, const char *const *contigs, const uint64_t *start,
                                   const uint64_t *end, size_t n) {
    covh_genes *g = new covh_genes();
    for (size_t i = 0; i < n; i++) g->genes.push_back(GeneDef{ids[i], contigs[i], start[i], end[i]});
    return g;
}
size_t covh_genes_count(const covh_genes *g) { return g ? g->genes.size() : 0; }
void covh_genes_get(const covh_genes *g, size_t i, const char **id, const char **contig, uint64_t *start, uint64_t *end) {
    const GeneDef &d = g->genes[i];
    if (id) *id = d.id.c_str();
    if (contig) *contig = d.contig.c_str();
    if (start) *start = d.start;
    if (end) *end = d.end;
}
void covh_genes_free(covh_genes *g) { delete g; }

}  // extern "C"

// The gene driver, one body for its two sources of the per-read numbers (n_reads / mismatches / sum_identity / "the scan saw this contig"):
// `rec` — the record pass below, over the sample's records on the host; or `reads_fn` — one cov_interval_reads per resolved gene, in
// entry order, from whoever holds the records (cov_interval_reads_compute in the product).
static int gene_coverage_body(const covh_header *h, const covh_genes *genes, const covh_genome_namer *namer, const char *stoit_name,
                              const cov_batch *rec, const cov_config *cfg, covh_interval_reads_fn reads_fn, void *reads_ctx, int *sorted_by_start,
                              cov_session *device_session, covh_depth_fn depth_fn,
                              void *depth_ctx, uint64_t num_detected_primary_alignments, covh_taker *taker, const covh_estimator *est,
                              size_t n_est, int print_zero, covh_reads_mapped *rm_out) {
    if (!h || !genes || (!rec && !reads_fn) || (rec && !cfg) || (!depth_fn && !device_session) || !taker || (!est && n_est)) return COV_ERR_INVALID_ARG;
    if (!check_excl(est, n_est)) { g_err = "estimators disagree on contig_end_exclusion"; return COV_ERR_INVALID_ARG; }
    const u64 excl = session_excl(est, n_est);
    const u64 zero = 0;
    const u32 nT = h->n_targets;

    // ---- resolve_genes_against_header, genes.rs:346-419
    std::vector<std::vector<ResolvedGene>> by_tid(nT);
    {
        std::unordered_map<std::string_view, u32> name_to_tid;
        name_to_tid.reserve(nT * 2);
        for (u32 t = 0; t < nT; t++) name_to_tid[target_name(h, t)] = t;      // a repeated name keeps the last tid
        for (const GeneDef &g : genes->genes) {
            auto it = name_to_tid.find(std::string_view(g.contig));
            if (it == name_to_tid.end()) continue;
            const u32 tid = it->second;
            const u64 L = h->target_len[tid];
            const u64 s = std::min(g.start, L), e = std::min(g.end, L);
            if (s >= e) continue;
            std::string name = g.id + "\t" + g.contig;
            if (namer && namer->mode != 0) {
                if (namer->mode == 1) name += "\tgenome1";
                else if (namer->mode == 2) {
                    const size_t sp = g.contig.find((char)namer->separator);
                    if (sp == std::string::npos) continue;
                    name += "\t" + g.contig.substr(0, sp);
                } else {
                    const int32_t gi = namer->genome_of_tid ? namer->genome_of_tid[tid] : -1;
                    if (gi < 0) continue;
                    name += std::string("\t") + namer->genome_names[gi];
                }
            }
            by_tid[tid].push_back(ResolvedGene{0, std::move(name), s, e});
        }
        size_t next_id = 0;
        for (auto &v : by_tid) {
            std::stable_sort(v.begin(), v.end(), [](const ResolvedGene &a, const ResolvedGene &b) { return a.start < b.start; });
            for (auto &g : v) g.entry_id = next_id++;
        }
    }

    // ---- device path: every resolved gene is one interval, reduced on the GPU over the materialised depth
    std::vector<cov_interval_stats> dstats;
    std::vector<uint64_t> dhist;
    std::vector<cov_interval> ivs;      // in entry order: ivs[g.entry_id] is gene g
    if (device_session || reads_fn)
        for (u32 t = 0; t < nT; t++)
            for (const ResolvedGene &g : by_tid[t]) { cov_interval iv; iv.tid = t; iv.pad = 0; iv.start = g.start; iv.end = g.end; ivs.push_back(iv); }
    // ---- the per-read numbers of every gene from the holder of the records.  Its verdicts are the record pass's own (the first offending
    // record in file order), returned before anything is written; starts that decrease inside a contig leave the work to the record pass.
    std::vector<cov_interval_reads> reads;
    u64 reads_mapped_total = 0;
    if (reads_fn) {
        bool want_identity = false;
        for (size_t k = 0; k < n_est; k++) want_identity |= est[k].kind == COVH_ANIR;
        reads.resize(ivs.size());
        int sorted = 0;
        const int rc = reads_fn(reads_ctx, ivs.data(), ivs.size(), want_identity ? 1 : 0, reads.data(), &reads_mapped_total, &sorted);
        if (rc == COV_ERR_UNSORTED) g_err = "BAM file appears to be unsorted. Input BAM files must be sorted by reference (i.e. by samtools sort)";
        else if (rc == COV_ERR_BAD_TID) g_err = "record refers to a reference id outside the header (Corrupt BAM file?)";
        else if (rc != COV_OK && rc != COV_ERR_NM_MISSING && rc != COV_ERR_NM_BADTYPE) g_err = "per-gene read aggregates failed";      // (the record pass leaves the text alone for the NM errors)
        if (rc != COV_OK) return rc;
        if (sorted_by_start) *sorted_by_start = sorted;
        if (!sorted) return COV_OK;
    }
    if (device_session) {
        bool want_hist = false;
        for (size_t k = 0; k < n_est; k++) want_hist |= est[k].kind == COVH_TRIMMED_MEAN || est[k].kind == COVH_PILEUP_COUNTS;
        dstats.resize(ivs.size());
        uint64_t htot = 0;
        int rc = (int)cov_interval_stats_compute(device_session, ivs.data(), ivs.size(), excl, want_hist, dstats.data(), &htot);
        if (rc == COV_OK && htot) { dhist.resize(htot); rc = (int)cov_fetch_interval_hist(device_session, dhist.data()); }
        if (rc != COV_OK) { g_err = cov_last_error(device_session); return rc; }
    }

    taker->start_stoit(stoit_name);
    auto zero_genes = [&](u32 tid) {   // emit_zero_coverage_genes, :554-567
        for (const ResolvedGene &g : by_tid[tid]) {
            taker->start_entry(g.entry_id, g.name);
            for (size_t k = 0; k < n_est; k++) print_zero_coverage(est[k], *taker, g.end - g.start);
            taker->finish_entry();
        }
    };

    std::vector<u64> starts, pprim, pmism;
    std::vector<double> pident;
    std::vector<int32_t> depth;
    std::vector<float> cov(n_est);
    EntryAcc acc;
    int rc_err = COV_OK;
    auto emit = [&](u32 tid) {   // emit_genes_for_contig, :462-552
        const auto &gl = by_tid[tid];
        if (gl.empty()) return;
        const u64 L = h->target_len[tid];
        if (!device_session) {
            depth.resize((size_t)L);
            const int rc = depth_fn(depth_ctx, tid, depth.data());
            if (rc != COV_OK) { if (!rc_err) rc_err = rc; return; }
        }
        for (const ResolvedGene &g : gl) {
            const u64 s = g.start, e = std::min(g.end, L);
            if (s >= e) continue;
            const u64 len = e - s;
            acc.reset();
            acc.full_len = len;
            if (device_session) {
                const cov_interval_stats &D = dstats[g.entry_id];
                acc.full_covered = D.full_covered;
                if (2 * excl < len) {
                    acc.win_len = len - 2 * excl;
                    acc.win_sum_d = D.win_sum_d; acc.win_sum_d2 = D.win_sum_d2; acc.win_covered = D.win_covered; acc.win_min_d = D.win_min_d;
                    if (D.hist_len && !dhist.empty()) acc.hist.assign(dhist.begin() + (ptrdiff_t)D.hist_off, dhist.begin() + (ptrdiff_t)(D.hist_off + D.hist_len));
                    else acc.hist_len_only = (u64)D.win_max_d + 1;
                }
            } else {
            for (u64 p = s; p < e; p++) acc.full_covered += depth[p] > 0;
            if (2 * excl < len) {                              // add_contig's window on the GENE's own array (:394-404)
                acc.win_len = len - 2 * excl;
                u32 mx = 0;
                for (u64 p = s + excl; p < e - excl; p++) {
                    const u32 d = (u32)depth[p];
                    acc.win_sum_d += d; acc.win_sum_d2 += (u64)d * d; acc.win_covered += d > 0;
                    acc.win_min_d = std::min(acc.win_min_d, d); mx = std::max(mx, d);
                }
                acc.hist.assign((size_t)mx + 1, 0);
                for (u64 p = s + excl; p < e - excl; p++) acc.hist[(u32)depth[p]]++;
            }
            }
            if (reads_fn) {
                const cov_interval_reads &Rd = reads[g.entry_id];
                acc.n_reads = Rd.n_reads; acc.mismatches = Rd.mismatches; acc.sum_identity = Rd.sum_identity;
            } else {
            const size_t lo = std::lower_bound(starts.begin(), starts.end(), s) - starts.begin();
            const size_t hi = std::lower_bound(starts.begin(), starts.end(), e) - starts.begin();
            acc.n_reads = pprim[hi] - pprim[lo];
            acc.mismatches = pmism[hi] - pmism[lo];
            acc.sum_identity = pident[hi] - pident[lo];       // difference of the running f64 prefix sums, as :526 does
            }
            bool nonzero = false;
            for (size_t k = 0; k < n_est; k++) { cov[k] = calculate(est[k], acc, &zero, 1); nonzero |= cov[k] > 0.0f; }
            if (print_zero || nonzero) {
                taker->start_entry(g.entry_id, g.name);
                for (size_t k = 0; k < n_est; k++) print_coverage(est[k], acc, cov[k], *taker);
                taker->finish_entry();
            }
        }
    };
    auto previous = [&](int64_t last, int64_t cur) {   // process_previous_genes, :421-460
        if (last != -2) emit((u32)last);
        if (print_zero) for (int64_t t = last == -2 ? 0 : last + 1; t < cur; t++) zero_genes((u32)t);
    };

    if (reads_fn) {
        // The record pass below calls previous() at every contig it sees, in tid order, and once behind the last: a contig with genes is
        // emitted when the scan saw it (contig_taken > 0, the same for all of its genes) and is a zero row otherwise; contigs without
        // genes write nothing either way.
        for (u32 t = 0; t < nT; t++) {
            if (by_tid[t].empty()) continue;
            if (reads[by_tid[t][0].entry_id].contig_taken > 0) emit(t);
            else if (print_zero) zero_genes(t);
            if (rc_err) return rc_err;
        }
        if (rm_out) { rm_out->num_mapped_reads = reads_mapped_total; rm_out->num_reads = num_detected_primary_alignments; }
        return COV_OK;
    }

    int64_t last_tid = -2;
    u64 mapped_total = 0;
    auto reset_contig = [&]() { starts.clear(); pprim.assign(1, 0); pmism.assign(1, 0); pident.assign(1, 0.0); };
    reset_contig();
    // Per-record work (filters, CIGAR walk, identity) is independent: blocks of records are classified by a few threads,
    // then consumed in file order (contig changes, prefix sums and emission are sequential, as in the reference).
    enum : uint8_t { SKIP = 0, TAKE = 1, NM_MISSING = 2, NM_BADTYPE = 3 };
    const u64 BLOCK = 1u << 20;
    std::vector<uint8_t> state(std::min<u64>(BLOCK, rec->n_records));
    std::vector<u64> mism(state.size());
    std::vector<double> ident(state.size());
    auto classify = [&](u64 i, u64 k) {
        const u32 flag = rec->flag[i];
        const bool supp = flag & 0x800u, sec = flag & 0x100u, unmapped = flag & 0x4u;
        state[k] = SKIP;
        u64 aligned = 0, indels = 0;
        auto walk = [&]() {
            for (u32 c = rec->cigar_off[i]; c < rec->cigar_off[i + 1]; c++) {
                const u32 op = rec->cigar[c] & 15u, len = rec->cigar[c] >> 4;
                if (op == 0 || op == 7 || op == 8) aligned += len;
                else if (op == 2 || op == 1) { aligned += len; indels += len; }
            }
        };
        bool walked = false;
        if (cfg->filter_single) {   // reader stage, single-read branch (filter.rs:88-116, 243-279), as k_prep applies it
            if (unmapped || (!cfg->include_supplementary && supp) || (!cfg->include_secondary && sec)) return;
            if (cfg->min_mapq != 255 && (rec->mapq[i] < cfg->min_mapq || rec->mapq[i] == 255)) return;
            if (rec->nm_kind[i] != COV_NM_UNSIGNED) { state[k] = rec->nm_kind[i] == COV_NM_ABSENT ? NM_MISSING : NM_BADTYPE; return; }
            walk(); walked = true;
            const u32 al = (u32)aligned;
            const float a = (float)al;
            if (!(al >= cfg->min_aligned_length && a / (float)rec->l_seq[i] >= cfg->min_aligned_percent &&
                  1.0f - (float)rec->nm[i] / a >= cfg->min_percent_identity)) return;
        }
        if ((!cfg->include_secondary && sec) || (!cfg->include_supplementary && supp) || (!cfg->include_improper_pairs && !(flag & 0x2u))) return;
        if (unmapped) return;
        if (!walked) walk();
        if (rec->nm_kind[i] != COV_NM_UNSIGNED) { state[k] = rec->nm_kind[i] == COV_NM_ABSENT ? NM_MISSING : NM_BADTYPE; return; }
        const u64 edit = rec->nm[i];
        const bool primary = !supp && !sec;
        state[k] = TAKE;
        mism[k] = edit > indels ? edit - indels : 0;                                   // saturating_sub, :296
        ident[k] = (primary && aligned > 0) ? ((double)aligned - (double)edit) / (double)aligned : 0.0;
    };
    const unsigned hw = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    for (u64 b0 = 0; b0 < rec->n_records; b0 += BLOCK) {
        const u64 nb = std::min<u64>(BLOCK, rec->n_records - b0);
        if (nb >= (1u << 16) && hw > 1) {
            std::vector<std::thread> pool;
            for (unsigned t = 0; t < hw; t++)
                pool.emplace_back([&, t]() { for (u64 k = nb * t / hw, e = nb * (t + 1) / hw; k < e; k++) classify(b0 + k, k); });
            for (auto &th : pool) th.join();
        } else {
            for (u64 k = 0; k < nb; k++) classify(b0 + k, k);
        }
        for (u64 k = 0; k < nb; k++) {
            const u64 i = b0 + k;
            // a record that fails the NM requirement before its contig is reached still ends the scan there, like the panic
            if (state[k] == SKIP) continue;
            if (state[k] != TAKE) {
                // single-read mode meets nm() inside the filter, before the flag filter; otherwise after it: classify()
                // already ordered those tests, so any error state is the reference's panic at this record
                return state[k] == NM_MISSING ? COV_ERR_NM_MISSING : COV_ERR_NM_BADTYPE;
            }
            const int64_t tid = rec->tid[i];
            if (tid != last_tid) {
                if (tid < last_tid) { g_err = "BAM file appears to be unsorted. Input BAM files must be sorted by reference (i.e. by samtools sort)"; return COV_ERR_UNSORTED; }
                if (tid < 0 || (u64)tid >= nT) { g_err = "record refers to a reference id outside the header (Corrupt BAM file?)"; return COV_ERR_BAD_TID; }
                previous(last_tid, tid);
                if (rc_err) return rc_err;
                last_tid = tid;
                reset_contig();
            }
            const bool primary = !(rec->flag[i] & 0x900u);
            mapped_total += primary;
            starts.push_back((u64)(int64_t)rec->pos[i]);
            pprim.push_back(pprim.back() + (primary ? 1 : 0));
            pmism.push_back(pmism.back() + mism[k]);
            pident.push_back(pident.back() + ident[k]);
        }
    }
    previous(last_tid, nT);
    if (rc_err) return rc_err;
    if (rm_out) { rm_out->num_mapped_reads = mapped_total; rm_out->num_reads = num_detected_primary_alignments; }
    return COV_OK;
}

extern "C" {

int covh_gene_coverage(const covh_header *h, const covh_genes *genes, const covh_genome_namer *namer, const char *stoit_name,
                       const cov_batch *rec, const cov_config *cfg, cov_session *device_session, covh_depth_fn depth_fn,
                       void *depth_ctx, uint64_t num_detected_primary_alignments, covh_taker *taker, const covh_estimator *est,
                       size_t n_est, int print_zero, covh_reads_mapped *rm_out) {
    if (!rec || !cfg) return COV_ERR_INVALID_ARG;
    return gene_coverage_body(h, genes, namer, stoit_name, rec, cfg, nullptr, nullptr, nullptr, device_session, depth_fn, depth_ctx, num_detected_primary_alignments, taker, est,
                              n_est, print_zero, rm_out);
}

int covh_gene_coverage_reads(const covh_header *h, const covh_genes *genes, const covh_genome_namer *namer, const char *stoit_name,
                             covh_interval_reads_fn reads, void *reads_ctx, cov_session *device_session, covh_depth_fn depth_fn,
                             void *depth_ctx, uint64_t num_detected_primary_alignments, covh_taker *taker, const covh_estimator *est,
                             size_t n_est, int print_zero, covh_reads_mapped *rm_out, int *sorted_by_start) {
    if (!reads || !sorted_by_start) return COV_ERR_INVALID_ARG;
    *sorted_by_start = 0;
    return gene_coverage_body(h, genes, namer, stoit_name, nullptr, nullptr, reads, reads_ctx, sorted_by_start, device_session, depth_fn, depth_ctx, num_detected_primary_alignments,
                              taker, est, n_est, print_zero, rm_out);
}

// covh_interval_reads_fn over a session: cov_interval_reads_compute (ctx = the cov_session holding the sample's records)
int covh_session_interval_reads(void *ctx, const cov_interval *iv, uint64_t n, int want_identity, cov_interval_reads *out, uint64_t *mapped_total, int *sorted_by_start) {
    return (int)cov_interval_reads_compute((cov_session *)ctx, iv, n, want_identity, out, mapped_total, sorted_by_start);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------- depth runs as a bedGraph (`coverm-amd depth`)
namespace {

bool write_all(int fd, const char *p, size_t n) {
    while (n) {
        const ssize_t w = ::write(fd, p, n);
        if (w < 0) { if (errno == EINTR) continue; return false; }
        p += w; n -= (size_t)w;
    }
    return true;
}

// runs [j0, j1) of the chunk as text; k = the target of run j0
void format_piece(const covh_header *h, uint32_t tid_lo, uint32_t n_targets, const uint64_t *run_off, const cov_depth_run *runs, bool no_zeros, uint64_t j0,
                  uint64_t j1, std::string &out) {
    out.clear();
    uint32_t k = (uint32_t)(std::upper_bound(run_off, run_off + n_targets + 1, j0) - run_off) - 1u;      // last target whose offset is <= j0: an empty one in front shares it
    char num[24];
    auto put = [&](uint64_t v) { const auto r = std::to_chars(num, num + sizeof num, v); out.append(num, (size_t)(r.ptr - num)); };
    for (uint64_t j = j0; j < j1; j++) {
        while (j >= run_off[k + 1]) k++;
        const cov_depth_run r = runs[j];
        if (no_zeros && r.depth == 0) continue;
        const uint32_t t = tid_lo + k;
        const uint64_t end = j + 1 < run_off[k + 1] ? runs[j + 1].start : h->target_len[t];
        out.append(h->names + h->name_off[t], h->name_off[t + 1] - h->name_off[t]);
        out.push_back('\t'); put(r.start); out.push_back('\t'); put(end); out.push_back('\t');
        if (r.depth < 0) { out.push_back('-'); put((uint64_t)(-(int64_t)r.depth)); } else put((uint64_t)r.depth);
        out.push_back('\n');
    }
}

}  // namespace

int covh_depth_runs_format(const covh_header *h, uint32_t tid_lo, uint32_t n_targets, const uint64_t *run_off, const cov_depth_run *runs, int no_zeros,
                           int threads, int out_fd) {
    if (!h || !run_off || (uint64_t)tid_lo + n_targets > h->n_targets) { g_err = "covh_depth_runs_format: targets outside the header"; return COV_ERR_INVALID_ARG; }
    const uint64_t n = run_off[n_targets];
    if (n && !runs) { g_err = "covh_depth_runs_format: no runs"; return COV_ERR_INVALID_ARG; }
    constexpr uint64_t PIECE = 1ull << 17;      // runs per piece: a few MB of text
    const unsigned T = (unsigned)std::max(1, std::min(threads, 64));
    std::vector<std::string> text(T);
    for (uint64_t base = 0; base < n; base += PIECE * T) {      // T pieces side by side, written in their order
        const unsigned np = (unsigned)std::min<uint64_t>(T, (n - base + PIECE - 1) / PIECE);
        auto piece = [&](unsigned i) { format_piece(h, tid_lo, n_targets, run_off, runs, no_zeros != 0, base + i * PIECE, std::min(n, base + (i + 1) * PIECE), text[i]); };
        std::vector<std::thread> th;
        for (unsigned i = 1; i < np; i++) th.emplace_back(piece, i);
        piece(0);
        for (auto &t : th) t.join();
        for (unsigned i = 0; i < np; i++)
            if (!write_all(out_fd, text[i].data(), text[i].size())) { g_err = "covh_depth_runs_format: write failed"; return COV_ERR_INVALID_ARG; }
    }
    return COV_OK;
}

int covh_depth_runs_write(cov_session *s, const covh_header *h, int no_zeros, int threads, int out_fd, uint64_t *n_runs_out) {
    if (!s || !h) { g_err = "covh_depth_runs_write: no session"; return COV_ERR_INVALID_ARG; }
    uint64_t total = 0;
    if (n_runs_out) *n_runs_out = 0;
    cov_depth_run *runs = nullptr; size_t cap = 0;      // page-locked, grown to the largest chunk
    struct Free { cov_depth_run *&p; ~Free() { if (p) cov_host_free(p); } } free_runs{runs};
    std::vector<uint64_t> run_off;
    for (uint32_t lo = 0; lo < h->n_targets;) {
        uint32_t next = 0; uint64_t n = 0;
        int rc = (int)cov_depth_runs_compute(s, lo, h->n_targets, &next, &n);
        if (rc != COV_OK) { g_err = cov_last_error(s); return rc; }
        if (n > cap) {
            if (runs) { cov_host_free(runs); runs = nullptr; }
            cap = (size_t)n;
            runs = static_cast<cov_depth_run *>(cov_host_alloc(cap * sizeof(cov_depth_run)));
            if (!runs) { g_err = "covh_depth_runs_write: no page-locked memory for a chunk's runs"; return COV_ERR_HIP; }
        }
        run_off.resize((size_t)(next - lo) + 1);
        rc = (int)cov_depth_runs_fetch(s, run_off.data(), runs);
        if (rc != COV_OK) { g_err = cov_last_error(s); return rc; }
        rc = covh_depth_runs_format(h, lo, next - lo, run_off.data(), runs, no_zeros, threads, out_fd);
        if (rc != COV_OK) return rc;
        total += n; lo = next;
    }
    if (n_runs_out) *n_runs_out = total;
    return COV_OK;
}

// ---------------------------------------------------------------------------------------------- depth bins as a bedGraph (`coverm-amd depth --bin-size`)
namespace {

// bins [j0, j1) of the chunk as text
void format_bins_piece(const covh_header *h, uint32_t tid_lo, uint32_t n_targets, uint32_t bin_size, const uint64_t *bin_off, const cov_depth_bin *bins, int value,
                       bool no_zeros, uint64_t j0, uint64_t j1, std::string &out) {
    out.clear();
    uint32_t k = (uint32_t)(std::upper_bound(bin_off, bin_off + n_targets + 1, j0) - bin_off) - 1u;      // last target whose offset is <= j0: an empty one in front shares it
    char num[40];
    auto put = [&](uint64_t v) { const auto r = std::to_chars(num, num + sizeof num, v); out.append(num, (size_t)(r.ptr - num)); };
    auto put_i = [&](int64_t v) { if (v < 0) { out.push_back('-'); put((uint64_t)(-v)); } else put((uint64_t)v); };
    for (uint64_t j = j0; j < j1; j++) {
        while (j >= bin_off[k + 1]) k++;
        const cov_depth_bin b = bins[j];
        if (no_zeros && b.max == 0) continue;
        const uint32_t t = tid_lo + k;
        const uint64_t start = (j - bin_off[k]) * bin_size, end = std::min<uint64_t>(start + bin_size, h->target_len[t]);
        out.append(h->names + h->name_off[t], h->name_off[t + 1] - h->name_off[t]);
        out.push_back('\t'); put(start); out.push_back('\t'); put(end); out.push_back('\t');
        switch (value) {
        case COVH_BIN_SUM: put(b.sum); break;
        case COVH_BIN_MIN: put_i(b.min); break;
        case COVH_BIN_MAX: put_i(b.max); break;
        case COVH_BIN_COVERED: put(b.covered); break;
        default: out.append(num, (size_t)snprintf(num, sizeof num, "%.3f", (double)b.sum / (double)(end - start))); break;
        }
        out.push_back('\n');
    }
}

}  // namespace

int covh_depth_bins_format(const covh_header *h, uint32_t tid_lo, uint32_t n_targets, uint32_t bin_size, const uint64_t *bin_off, const cov_depth_bin *bins, int value,
                           int no_zeros, int threads, int out_fd) {
    if (!h || !bin_off || (uint64_t)tid_lo + n_targets > h->n_targets) { g_err = "covh_depth_bins_format: targets outside the header"; return COV_ERR_INVALID_ARG; }
    if (bin_size == 0 || value < COVH_BIN_MEAN || value > COVH_BIN_COVERED) { g_err = "covh_depth_bins_format: bin size 0 or an unknown value kind"; return COV_ERR_INVALID_ARG; }
    const uint64_t n = bin_off[n_targets];
    if (n && !bins) { g_err = "covh_depth_bins_format: no bins"; return COV_ERR_INVALID_ARG; }
    constexpr uint64_t PIECE = 1ull << 17;      // bins per piece: a few MB of text
    const unsigned T = (unsigned)std::max(1, std::min(threads, 64));
    std::vector<std::string> text(T);
    for (uint64_t base = 0; base < n; base += PIECE * T) {      // T pieces side by side, written in their order
        const unsigned np = (unsigned)std::min<uint64_t>(T, (n - base + PIECE - 1) / PIECE);
        auto piece = [&](unsigned i) {
            format_bins_piece(h, tid_lo, n_targets, bin_size, bin_off, bins, value, no_zeros != 0, base + i * PIECE, std::min(n, base + (i + 1) * PIECE), text[i]);
        };
        std::vector<std::thread> th;
        for (unsigned i = 1; i < np; i++) th.emplace_back(piece, i);
        piece(0);
        for (auto &t : th) t.join();
        for (unsigned i = 0; i < np; i++)
            if (!write_all(out_fd, text[i].data(), text[i].size())) { g_err = "covh_depth_bins_format: write failed"; return COV_ERR_INVALID_ARG; }
    }
    return COV_OK;
}

int covh_depth_bins_write(cov_session *s, const covh_header *h, uint32_t bin_size, int value, int no_zeros, int threads, int out_fd, uint64_t *n_bins_out) {
    if (!s || !h) { g_err = "covh_depth_bins_write: no session"; return COV_ERR_INVALID_ARG; }
    uint64_t total = 0;
    if (n_bins_out) *n_bins_out = 0;
    cov_depth_bin *bins = nullptr; size_t cap = 0;      // page-locked, grown to the largest chunk
    struct Free { cov_depth_bin *&p; ~Free() { if (p) cov_host_free(p); } } free_bins{bins};
    std::vector<uint64_t> bin_off;
    for (uint32_t lo = 0; lo < h->n_targets;) {
        uint32_t next = 0; uint64_t n = 0;
        int rc = (int)cov_depth_bins_compute(s, bin_size, lo, h->n_targets, &next, &n);
        if (rc != COV_OK) { g_err = cov_last_error(s); return rc; }
        if (n > cap) {
            if (bins) { cov_host_free(bins); bins = nullptr; }
            cap = (size_t)n;
            bins = static_cast<cov_depth_bin *>(cov_host_alloc(cap * sizeof(cov_depth_bin)));
            if (!bins) { g_err = "covh_depth_bins_write: no page-locked memory for a chunk's bins"; return COV_ERR_HIP; }
        }
        bin_off.resize((size_t)(next - lo) + 1);
        rc = (int)cov_depth_bins_fetch(s, bin_off.data(), bins);
        if (rc != COV_OK) { g_err = cov_last_error(s); return rc; }
        rc = covh_depth_bins_format(h, lo, next - lo, bin_size, bin_off.data(), bins, value, no_zeros, threads, out_fd);
        if (rc != COV_OK) return rc;
        total += n; lo = next;
    }
    if (n_bins_out) *n_bins_out = total;
    return COV_OK;
}

// ---------------------------------------------------------------------------------------------- depth regions of a BED file (`coverm-amd depth --regions`)
struct covh_bed {
    struct Line { uint32_t chrom_off, chrom_len, name_off, name_len, start, end; uint64_t line_no; bool has_name; };
    std::string path, text;      // text: the chrom and name fields, back to back
    std::vector<Line> lines;
};

namespace {

// a decimal integer <= 2^31 - 1, digits only
bool bed_number(std::string_view f, uint32_t &v) {
    if (f.empty() || f.size() > 10) return false;
    uint64_t x = 0;
    for (char c : f) { if (c < '0' || c > '9') return false; x = x * 10 + (uint64_t)(c - '0'); }
    if (x > 0x7fffffffull) return false;
    v = (uint32_t)x;
    return true;
}

std::string bed_at(const covh_bed *b, uint64_t line_no) { return b->path + ":" + std::to_string(line_no) + ": "; }

// regions [j0, j1) of the file as text
void format_regions_piece(const covh_bed *b, const cov_depth_bin *res, int value, bool no_zeros, uint64_t j0, uint64_t j1, std::string &out) {
    out.clear();
    char num[40];
    auto put = [&](uint64_t v) { const auto r = std::to_chars(num, num + sizeof num, v); out.append(num, (size_t)(r.ptr - num)); };
    auto put_i = [&](int64_t v) { if (v < 0) { out.push_back('-'); put((uint64_t)(-v)); } else put((uint64_t)v); };
    for (uint64_t j = j0; j < j1; j++) {
        const covh_bed::Line &l = b->lines[j];
        const cov_depth_bin r = res[j];
        if (no_zeros && r.max == 0) continue;
        out.append(b->text, l.chrom_off, l.chrom_len);
        out.push_back('\t'); put(l.start); out.push_back('\t'); put(l.end); out.push_back('\t');
        if (l.has_name) { out.append(b->text, l.name_off, l.name_len); out.push_back('\t'); }
        switch (value) {
        case COVH_BIN_SUM: put(r.sum); break;
        case COVH_BIN_MIN: put_i(r.min); break;
        case COVH_BIN_MAX: put_i(r.max); break;
        case COVH_BIN_COVERED: put(r.covered); break;
        default: out.append(num, (size_t)snprintf(num, sizeof num, "%.3f", (double)r.sum / (double)(l.end - l.start))); break;
        }
        out.push_back('\n');
    }
}

}  // namespace

covh_bed *covh_bed_read(const char *path) {
    if (!path) { g_err = "covh_bed_read: no path"; return nullptr; }
    FILE *fh = fopen(path, "rb");
    if (!fh) { g_err = std::string(path) + ": " + strerror(errno); return nullptr; }
    std::string data;
    char buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, fh)) > 0) data.append(buf, got);
    const bool bad = ferror(fh) != 0;
    fclose(fh);
    if (bad) { g_err = std::string(path) + ": read failed"; return nullptr; }
    std::unique_ptr<covh_bed> b(new covh_bed);
    b->path = path;
    uint64_t line_no = 0;
    for (size_t at = 0; at < data.size();) {
        size_t nl = data.find('\n', at);
        if (nl == std::string::npos) nl = data.size();
        std::string_view line(data.data() + at, nl - at);
        at = nl + 1; line_no++;
        if (!line.empty() && line.back() == '\r') line.remove_suffix(1);
        if (line.empty() || line[0] == '#' || line.substr(0, 5) == "track" || line.substr(0, 7) == "browser") continue;
        std::string_view f[4];
        size_t nf = 0, p = 0;
        while (nf < 4) {
            const size_t t = line.find('\t', p);
            f[nf++] = line.substr(p, t == std::string_view::npos ? std::string_view::npos : t - p);
            if (t == std::string_view::npos) break;
            p = t + 1;
        }
        if (nf < 3) { g_err = bed_at(b.get(), line_no) + "expected chrom<TAB>start<TAB>end, found " + std::to_string(nf) + (nf == 1 ? " field" : " fields"); return nullptr; }
        if (f[0].empty()) { g_err = bed_at(b.get(), line_no) + "the reference name is empty"; return nullptr; }
        covh_bed::Line l{};
        if (!bed_number(f[1], l.start)) { g_err = bed_at(b.get(), line_no) + "start '" + std::string(f[1]) + "' is not a decimal integer of at most 2147483647"; return nullptr; }
        if (!bed_number(f[2], l.end)) { g_err = bed_at(b.get(), line_no) + "end '" + std::string(f[2]) + "' is not a decimal integer of at most 2147483647"; return nullptr; }
        if (l.start >= l.end) { g_err = bed_at(b.get(), line_no) + "start " + std::to_string(l.start) + " >= end " + std::to_string(l.end) + " (a region is [start, end), not empty)"; return nullptr; }
        if (b->text.size() + f[0].size() + f[3].size() > 0xffffffffull || b->lines.size() >= 0xffffffffull) { g_err = bed_at(b.get(), line_no) + "more than 2^32 regions or bytes of names"; return nullptr; }
        l.chrom_off = (uint32_t)b->text.size(); l.chrom_len = (uint32_t)f[0].size(); b->text.append(f[0]);
        l.has_name = nf >= 4;
        if (l.has_name) { l.name_off = (uint32_t)b->text.size(); l.name_len = (uint32_t)f[3].size(); b->text.append(f[3]); }
        l.line_no = line_no;
        b->lines.push_back(l);
    }
    return b.release();
}

void covh_bed_free(covh_bed *b) { delete b; }
uint64_t covh_bed_count(const covh_bed *b) { return b ? b->lines.size() : 0; }

int covh_bed_line(const covh_bed *b, uint64_t i, const char **chrom, uint32_t *chrom_len, uint32_t *start, uint32_t *end, const char **name, uint32_t *name_len, uint64_t *line_no) {
    if (!b || i >= b->lines.size()) { g_err = "covh_bed_line: no such region"; return COV_ERR_INVALID_ARG; }
    const covh_bed::Line &l = b->lines[i];
    if (chrom) *chrom = b->text.data() + l.chrom_off;
    if (chrom_len) *chrom_len = l.chrom_len;
    if (start) *start = l.start;
    if (end) *end = l.end;
    if (name) *name = l.has_name ? b->text.data() + l.name_off : nullptr;
    if (name_len) *name_len = l.has_name ? l.name_len : 0;
    if (line_no) *line_no = l.line_no;
    return COV_OK;
}

int covh_bed_resolve(const covh_bed *b, const covh_header *h, cov_depth_region *out) {
    if (!b || !h || (!out && !b->lines.empty())) { g_err = "covh_bed_resolve: no regions or no header"; return COV_ERR_INVALID_ARG; }
    std::unordered_map<std::string_view, uint32_t> tid_of;
    tid_of.reserve(h->n_targets);
    for (uint32_t t = 0; t < h->n_targets; t++) tid_of.emplace(std::string_view(h->names + h->name_off[t], h->name_off[t + 1] - h->name_off[t]), t);      // (the first of equal names)
    for (size_t i = 0; i < b->lines.size(); i++) {
        const covh_bed::Line &l = b->lines[i];
        const std::string_view chrom(b->text.data() + l.chrom_off, l.chrom_len);
        const auto it = tid_of.find(chrom);
        if (it == tid_of.end()) { g_err = bed_at(b, l.line_no) + "reference '" + std::string(chrom) + "' is not in the alignment file's header (a BED file for another assembly?)"; return COV_ERR_INVALID_ARG; }
        if (l.end > h->target_len[it->second]) {
            g_err = bed_at(b, l.line_no) + "end " + std::to_string(l.end) + " lies behind the length " + std::to_string(h->target_len[it->second]) + " of reference '" + std::string(chrom) + "'";
            return COV_ERR_INVALID_ARG;
        }
        out[i].tid = it->second; out[i].start = l.start; out[i].end = l.end; out[i].reserved = 0;
    }
    return COV_OK;
}

int covh_depth_regions_format(const covh_bed *b, const cov_depth_bin *results, int value, int no_zeros, int threads, int out_fd) {
    if (!b) { g_err = "covh_depth_regions_format: no regions"; return COV_ERR_INVALID_ARG; }
    if (value < COVH_BIN_MEAN || value > COVH_BIN_COVERED) { g_err = "covh_depth_regions_format: an unknown value kind"; return COV_ERR_INVALID_ARG; }
    const uint64_t n = b->lines.size();
    if (n && !results) { g_err = "covh_depth_regions_format: no results"; return COV_ERR_INVALID_ARG; }
    constexpr uint64_t PIECE = 1ull << 17;      // regions per piece: a few MB of text
    const unsigned T = (unsigned)std::max(1, std::min(threads, 64));
    std::vector<std::string> text(T);
    for (uint64_t base = 0; base < n; base += PIECE * T) {      // T pieces side by side, written in their order
        const unsigned np = (unsigned)std::min<uint64_t>(T, (n - base + PIECE - 1) / PIECE);
        auto piece = [&](unsigned i) { format_regions_piece(b, results, value, no_zeros != 0, base + i * PIECE, std::min(n, base + (i + 1) * PIECE), text[i]); };
        std::vector<std::thread> th;
        for (unsigned i = 1; i < np; i++) th.emplace_back(piece, i);
        piece(0);
        for (auto &t : th) t.join();
        for (unsigned i = 0; i < np; i++)
            if (!write_all(out_fd, text[i].data(), text[i].size())) { g_err = "covh_depth_regions_format: write failed"; return COV_ERR_INVALID_ARG; }
    }
    return COV_OK;
}

namespace {

// The chunks of a finished session that hold a region: cov_depth_regions_set, then compute / fetch chunk by chunk through page-locked
// memory, SKIPPING targets without a region, scattered by input_index into results[n] (and, with thresholds set on the session, their
// counts into counts[n x n_thr]).
int collect_regions(cov_session *s, const covh_header *h, const char *who, const cov_depth_region *regions, uint64_t n, cov_depth_bin *results, uint32_t *counts,
                    uint32_t n_thr) {
    int rc = (int)cov_depth_regions_set(s, regions, n);
    if (rc != COV_OK) { g_err = cov_last_error(s); return rc; }
    std::vector<uint8_t> has(h->n_targets, 0);
    for (uint64_t i = 0; i < n; i++) has[regions[i].tid] = 1;
    const size_t per = sizeof(cov_depth_bin) + sizeof(uint64_t) + (counts ? (size_t)n_thr * 4 : 0);
    void *pinned = nullptr; size_t cap = 0;     // page-locked, grown to the largest chunk: the results, their input indices, their counts
    struct Free { void *&p; ~Free() { if (p) cov_host_free(p); } } free_pinned{pinned};
    uint64_t total = 0;
    uint32_t lo = 0;
    while (lo < h->n_targets && !has[lo]) lo++;      // targets without a region are skipped: their depth is never materialised
    while (lo < h->n_targets) {
        uint32_t next = 0; uint64_t m = 0;
        rc = (int)cov_depth_regions_compute(s, lo, h->n_targets, &next, &m);
        if (rc != COV_OK) { g_err = cov_last_error(s); return rc; }
        if (m > cap) {
            if (pinned) { cov_host_free(pinned); pinned = nullptr; }
            cap = (size_t)m;
            pinned = cov_host_alloc(cap * per);
            if (!pinned) { g_err = std::string(who) + ": no page-locked memory for a chunk's results"; return COV_ERR_HIP; }
        }
        cov_depth_bin *res = static_cast<cov_depth_bin *>(pinned);
        uint64_t *idx = reinterpret_cast<uint64_t *>(res + cap);
        uint32_t *cnt = reinterpret_cast<uint32_t *>(idx + cap);
        rc = (int)cov_depth_regions_fetch(s, idx, res);
        if (rc == COV_OK && counts) rc = (int)cov_depth_regions_counts_fetch(s, cnt);
        if (rc != COV_OK) { g_err = cov_last_error(s); return rc; }
        for (uint64_t i = 0; i < m; i++) results[idx[i]] = res[i];
        if (counts)
            for (uint64_t i = 0; i < m; i++) memcpy(counts + idx[i] * n_thr, cnt + i * n_thr, (size_t)n_thr * 4);
        total += m;
        lo = next;
        while (lo < h->n_targets && !has[lo]) lo++;
    }
    if (total != n) { g_err = std::string(who) + ": the chunks returned " + std::to_string(total) + " of " + std::to_string(n) + " regions"; return COV_ERR_STATE; }
    return COV_OK;
}

}  // namespace

int covh_depth_regions_write(cov_session *s, const covh_header *h, const covh_bed *b, int value, int no_zeros, int threads, int out_fd, uint64_t *n_regions_out) {
    if (!s || !h || !b) { g_err = "covh_depth_regions_write: no session, header or regions"; return COV_ERR_INVALID_ARG; }
    if (n_regions_out) *n_regions_out = 0;
    const uint64_t n = b->lines.size();
    std::vector<cov_depth_region> regions(n);
    int rc = covh_bed_resolve(b, h, regions.data());
    if (rc != COV_OK) return rc;
    if (n == 0) return COV_OK;
    std::vector<cov_depth_bin> results(n);      // the sample's results in the file's order, 24 B per region
    rc = collect_regions(s, h, "covh_depth_regions_write", regions.data(), n, results.data(), nullptr, 0);
    if (rc != COV_OK) return rc;
    rc = covh_depth_regions_format(b, results.data(), value, no_zeros, threads, out_fd);
    if (rc != COV_OK) return rc;
    if (n_regions_out) *n_regions_out = n;
    return COV_OK;
}

// ---------------------------------------------------------------------------------------------- depth classes (`coverm-amd depth --quantize`, `--thresholds`)
namespace {

// decimal fields separated by `sep` into v[0 .. n); an empty field is -1
bool class_fields(const char *text, char sep, std::vector<int64_t> &v, std::string &why) {
    v.clear();
    const std::string_view t(text);
    for (size_t at = 0;;) {
        const size_t e = t.find(sep, at);
        const std::string_view f = t.substr(at, e == std::string_view::npos ? std::string_view::npos : e - at);
        uint32_t x = 0;
        if (f.empty()) v.push_back(-1);
        else if (bed_number(f, x)) v.push_back(x);
        else { why = "'" + std::string(f) + "' is not a decimal integer of at most 2147483647"; return false; }
        if (v.size() > 64) { why = "more than 16 values"; return false; }
        if (e == std::string_view::npos) return true;
        at = e + 1;
    }
}

int class_list(const char *who, const char *text, const std::vector<int64_t> &v, int32_t *out, uint32_t *n_out) {
    std::vector<int32_t> c(v.begin(), v.end());
    uint32_t at = 0;
    if (const char *what = dclc::validate(c.data(), (uint32_t)c.size(), &at)) { g_err = std::string(who) + ": '" + text + "': value " + std::to_string(at) + ": " + what; return COV_ERR_INVALID_ARG; }
    for (size_t i = 0; i < c.size(); i++) out[i] = c[i];
    *n_out = (uint32_t)c.size();
    return COV_OK;
}

// The label of class c under (cuts, open_end): empty when the class is not printed.
void class_labels(const int32_t *cuts, uint32_t n, bool open_end, std::vector<std::string> &lab) {
    lab.assign((size_t)n + 1, std::string());
    for (uint32_t c = 1; c < n; c++) lab[c] = std::to_string(cuts[c - 1]) + ":" + std::to_string(cuts[c]);
    if (open_end) lab[n] = std::to_string(cuts[n - 1]) + ":inf";
}

// n items as text on up to `threads` threads in ordered pieces of 2^17, written in their order: the same text for every thread count.
template <class Piece>
int write_in_pieces(const char *who, uint64_t n, int threads, int out_fd, Piece piece_text) {
    constexpr uint64_t PIECE = 1ull << 17;
    const unsigned T = (unsigned)std::max(1, std::min(threads, 64));
    std::vector<std::string> text(T);
    for (uint64_t base = 0; base < n; base += PIECE * T) {
        const unsigned np = (unsigned)std::min<uint64_t>(T, (n - base + PIECE - 1) / PIECE);
        auto piece = [&](unsigned i) { text[i].clear(); piece_text(base + i * PIECE, std::min(n, base + (i + 1) * PIECE), text[i]); };
        std::vector<std::thread> th;
        for (unsigned i = 1; i < np; i++) th.emplace_back(piece, i);
        piece(0);
        for (auto &t : th) t.join();
        for (unsigned i = 0; i < np; i++)
            if (!write_all(out_fd, text[i].data(), text[i].size())) { g_err = std::string(who) + ": write failed"; return COV_ERR_INVALID_ARG; }
    }
    return COV_OK;
}

struct PutNumber {
    std::string &out; char num[24];
    void operator()(uint64_t v) { const auto r = std::to_chars(num, num + sizeof num, v); out.append(num, (size_t)(r.ptr - num)); }
};

// The thresholds of a session while a _write function runs: set, and cleared again behind it.
struct SessionThresholds {
    cov_session *s; int rc;
    SessionThresholds(cov_session *s_, const int32_t *thr, uint32_t n) : s(s_), rc((int)cov_depth_thresholds_set(s_, thr, n)) { if (rc != COV_OK) g_err = cov_last_error(s); }
    ~SessionThresholds() { (void)cov_depth_thresholds_set(s, nullptr, 0); }
};

}  // namespace

int covh_depth_quantize_parse(const char *spec, int32_t *cuts, uint32_t *n_cuts, int *open_end) {
    if (!spec || !cuts || !n_cuts || !open_end) { g_err = "covh_depth_quantize_parse: no spec"; return COV_ERR_INVALID_ARG; }
    std::vector<int64_t> v;
    std::string why;
    const std::string at = std::string("covh_depth_quantize_parse: '") + spec + "': ";
    if (!class_fields(spec, ':', v, why)) { g_err = at + why; return COV_ERR_INVALID_ARG; }
    if (v.size() < 2) { g_err = at + "no class: at least two cuts, or one and an open end (0:1:5: gives [0,1), [1,5) and [5,inf))"; return COV_ERR_INVALID_ARG; }
    const bool open = v.back() < 0;
    if (open) v.pop_back();
    if (!v.empty() && v[0] < 0) v[0] = 0;      // an empty first field means 0
    for (size_t i = 0; i < v.size(); i++)
        if (v[i] < 0) { g_err = at + "value " + std::to_string(i) + ": an empty field (only the first and the last may be empty)"; return COV_ERR_INVALID_ARG; }
    if (v.empty() || (v.size() < 2 && !open)) { g_err = at + "no class: at least two cuts, or one and an open end"; return COV_ERR_INVALID_ARG; }
    const int rc = class_list("covh_depth_quantize_parse", spec, v, cuts, n_cuts);
    if (rc == COV_OK) *open_end = open ? 1 : 0;
    return rc;
}

int covh_depth_thresholds_parse(const char *list, int32_t *thr, uint32_t *n_thr) {
    if (!list || !thr || !n_thr) { g_err = "covh_depth_thresholds_parse: no list"; return COV_ERR_INVALID_ARG; }
    std::vector<int64_t> v;
    std::string why;
    const std::string at = std::string("covh_depth_thresholds_parse: '") + list + "': ";
    if (!class_fields(list, ',', v, why)) { g_err = at + why; return COV_ERR_INVALID_ARG; }
    for (size_t i = 0; i < v.size(); i++)
        if (v[i] < 0) { g_err = at + "value " + std::to_string(i) + ": an empty field"; return COV_ERR_INVALID_ARG; }
    return class_list("covh_depth_thresholds_parse", list, v, thr, n_thr);
}

int covh_depth_class_runs_format(const covh_header *h, uint32_t tid_lo, uint32_t n_targets, const uint64_t *run_off, const cov_depth_run *runs, const int32_t *cuts,
                                 uint32_t n_cuts, int open_end, int threads, int out_fd) {
    if (!h || !run_off || (uint64_t)tid_lo + n_targets > h->n_targets) { g_err = "covh_depth_class_runs_format: targets outside the header"; return COV_ERR_INVALID_ARG; }
    uint32_t bad = 0;
    if (!cuts || dclc::validate(cuts, n_cuts, &bad)) { g_err = "covh_depth_class_runs_format: a bad cut list"; return COV_ERR_INVALID_ARG; }
    const uint64_t n = run_off[n_targets];
    if (n && !runs) { g_err = "covh_depth_class_runs_format: no runs"; return COV_ERR_INVALID_ARG; }
    std::vector<std::string> lab;
    class_labels(cuts, n_cuts, open_end != 0, lab);
    return write_in_pieces("covh_depth_class_runs_format", n, threads, out_fd, [&](uint64_t j0, uint64_t j1, std::string &out) {
        uint32_t k = (uint32_t)(std::upper_bound(run_off, run_off + n_targets + 1, j0) - run_off) - 1u;      // last target whose offset is <= j0
        PutNumber put{out, {}};
        for (uint64_t j = j0; j < j1; j++) {
            while (j >= run_off[k + 1]) k++;
            const cov_depth_run r = runs[j];
            if (r.depth < 0 || (uint32_t)r.depth > n_cuts || lab[(size_t)r.depth].empty()) continue;      // class 0, a closed spec's class n
            const uint32_t t = tid_lo + k;
            const uint64_t end = j + 1 < run_off[k + 1] ? runs[j + 1].start : h->target_len[t];      // the next run's start, printed or not
            out.append(h->names + h->name_off[t], h->name_off[t + 1] - h->name_off[t]);
            out.push_back('\t'); put(r.start); out.push_back('\t'); put(end); out.push_back('\t');
            out.append(lab[(size_t)r.depth]);
            out.push_back('\n');
        }
    });
}

int covh_depth_class_runs_write(cov_session *s, const covh_header *h, const int32_t *cuts, uint32_t n_cuts, int open_end, int threads, int out_fd, uint64_t *n_runs_out) {
    if (!s || !h) { g_err = "covh_depth_class_runs_write: no session"; return COV_ERR_INVALID_ARG; }
    uint64_t total = 0;
    if (n_runs_out) *n_runs_out = 0;
    cov_depth_run *runs = nullptr; size_t cap = 0;      // page-locked, grown to the largest chunk
    struct Free { cov_depth_run *&p; ~Free() { if (p) cov_host_free(p); } } free_runs{runs};
    std::vector<uint64_t> run_off;
    for (uint32_t lo = 0; lo < h->n_targets;) {
        uint32_t next = 0; uint64_t n = 0;
        int rc = (int)cov_depth_class_runs_compute(s, cuts, n_cuts, lo, h->n_targets, &next, &n);
        if (rc != COV_OK) { g_err = cov_last_error(s); return rc; }
        if (n > cap) {
            if (runs) { cov_host_free(runs); runs = nullptr; }
            cap = (size_t)n;
            runs = static_cast<cov_depth_run *>(cov_host_alloc(cap * sizeof(cov_depth_run)));
            if (!runs) { g_err = "covh_depth_class_runs_write: no page-locked memory for a chunk's runs"; return COV_ERR_HIP; }
        }
        run_off.resize((size_t)(next - lo) + 1);
        rc = (int)cov_depth_runs_fetch(s, run_off.data(), runs);
        if (rc != COV_OK) { g_err = cov_last_error(s); return rc; }
        rc = covh_depth_class_runs_format(h, lo, next - lo, run_off.data(), runs, cuts, n_cuts, open_end, threads, out_fd);
        if (rc != COV_OK) return rc;
        total += n; lo = next;
    }
    if (n_runs_out) *n_runs_out = total;
    return COV_OK;
}

int covh_depth_regions_counts_format(const covh_bed *b, const cov_depth_bin *results, const uint32_t *counts, uint32_t n_thr, int no_zeros, int threads, int out_fd) {
    if (!b) { g_err = "covh_depth_regions_counts_format: no regions"; return COV_ERR_INVALID_ARG; }
    if (n_thr == 0 || n_thr > COV_DEPTH_MAX_CUTS) { g_err = "covh_depth_regions_counts_format: 1 .. 16 thresholds"; return COV_ERR_INVALID_ARG; }
    const uint64_t n = b->lines.size();
    if (n && (!counts || (no_zeros && !results))) { g_err = "covh_depth_regions_counts_format: no counts or no results"; return COV_ERR_INVALID_ARG; }
    return write_in_pieces("covh_depth_regions_counts_format", n, threads, out_fd, [&](uint64_t j0, uint64_t j1, std::string &out) {
        PutNumber put{out, {}};
        for (uint64_t j = j0; j < j1; j++) {
            const covh_bed::Line &l = b->lines[j];
            if (no_zeros && results[j].max == 0) continue;
            out.append(b->text, l.chrom_off, l.chrom_len);
            out.push_back('\t'); put(l.start); out.push_back('\t'); put(l.end);
            if (l.has_name) { out.push_back('\t'); out.append(b->text, l.name_off, l.name_len); }
            for (uint32_t t = 0; t < n_thr; t++) { out.push_back('\t'); put(counts[j * n_thr + t]); }
            out.push_back('\n');
        }
    });
}

int covh_depth_regions_counts_write(cov_session *s, const covh_header *h, const covh_bed *b, const int32_t *thr, uint32_t n_thr, int no_zeros, int threads, int out_fd,
                                    uint64_t *n_regions_out) {
    if (!s || !h || !b) { g_err = "covh_depth_regions_counts_write: no session, header or regions"; return COV_ERR_INVALID_ARG; }
    if (n_regions_out) *n_regions_out = 0;
    if (n_thr == 0) { g_err = "covh_depth_regions_counts_write: no thresholds"; return COV_ERR_INVALID_ARG; }
    const uint64_t n = b->lines.size();
    std::vector<cov_depth_region> regions(n);
    int rc = covh_bed_resolve(b, h, regions.data());
    if (rc != COV_OK) return rc;
    SessionThresholds set(s, thr, n_thr);
    if (set.rc != COV_OK) return set.rc;
    if (n == 0) return COV_OK;
    std::vector<cov_depth_bin> results(n);
    std::vector<uint32_t> counts((size_t)n * n_thr);
    rc = collect_regions(s, h, "covh_depth_regions_counts_write", regions.data(), n, results.data(), counts.data(), n_thr);
    if (rc != COV_OK) return rc;
    rc = covh_depth_regions_counts_format(b, results.data(), counts.data(), n_thr, no_zeros, threads, out_fd);
    if (rc != COV_OK) return rc;
    if (n_regions_out) *n_regions_out = n;
    return COV_OK;
}

int covh_depth_bins_counts_format(const covh_header *h, uint32_t tid_lo, uint32_t n_targets, uint32_t bin_size, const uint64_t *bin_off, const cov_depth_bin *bins,
                                  const uint32_t *counts, uint32_t n_thr, int no_zeros, int threads, int out_fd) {
    if (!h || !bin_off || (uint64_t)tid_lo + n_targets > h->n_targets) { g_err = "covh_depth_bins_counts_format: targets outside the header"; return COV_ERR_INVALID_ARG; }
    if (bin_size == 0 || n_thr == 0 || n_thr > COV_DEPTH_MAX_CUTS) { g_err = "covh_depth_bins_counts_format: bin size 0, or not 1 .. 16 thresholds"; return COV_ERR_INVALID_ARG; }
    const uint64_t n = bin_off[n_targets];
    if (n && (!counts || (no_zeros && !bins))) { g_err = "covh_depth_bins_counts_format: no counts or no bins"; return COV_ERR_INVALID_ARG; }
    return write_in_pieces("covh_depth_bins_counts_format", n, threads, out_fd, [&](uint64_t j0, uint64_t j1, std::string &out) {
        uint32_t k = (uint32_t)(std::upper_bound(bin_off, bin_off + n_targets + 1, j0) - bin_off) - 1u;      // last target whose offset is <= j0
        PutNumber put{out, {}};
        for (uint64_t j = j0; j < j1; j++) {
            while (j >= bin_off[k + 1]) k++;
            if (no_zeros && bins[j].max == 0) continue;
            const uint32_t t = tid_lo + k;
            const uint64_t start = (j - bin_off[k]) * bin_size, end = std::min<uint64_t>(start + bin_size, h->target_len[t]);
            out.append(h->names + h->name_off[t], h->name_off[t + 1] - h->name_off[t]);
            out.push_back('\t'); put(start); out.push_back('\t'); put(end);
            for (uint32_t c = 0; c < n_thr; c++) { out.push_back('\t'); put(counts[j * n_thr + c]); }
            out.push_back('\n');
        }
    });
}

int covh_depth_bins_counts_write(cov_session *s, const covh_header *h, uint32_t bin_size, const int32_t *thr, uint32_t n_thr, int no_zeros, int threads, int out_fd,
                                 uint64_t *n_bins_out) {
    if (!s || !h) { g_err = "covh_depth_bins_counts_write: no session"; return COV_ERR_INVALID_ARG; }
    if (n_bins_out) *n_bins_out = 0;
    if (bin_size == 0 || bin_size > 0x7fffffffu || n_thr == 0) { g_err = "covh_depth_bins_counts_write: the bin size is 1 .. 2^31 - 1 bases, with at least one threshold"; return COV_ERR_INVALID_ARG; }
    // the windows of every reference, tiled into regions in target order, then position order: result i is window i
    std::vector<uint64_t> bin_off((size_t)h->n_targets + 1);
    uint64_t n = 0;
    for (uint32_t t = 0; t < h->n_targets; t++) { bin_off[t] = n; n += h->target_len[t] ? (h->target_len[t] - 1) / bin_size + 1 : 0; }
    bin_off[h->n_targets] = n;
    if (n >= (1ull << 32)) {      // refused in cov_depth_regions_set's words (which reads no region before it refuses)
        const cov_depth_region none{};
        const int rc = (int)cov_depth_regions_set(s, &none, n);
        g_err = cov_last_error(s);
        return rc != COV_OK ? rc : COV_ERR_INVALID_ARG;
    }
    SessionThresholds set(s, thr, n_thr);
    if (set.rc != COV_OK) return set.rc;
    if (n == 0) return COV_OK;
    std::vector<cov_depth_region> regions((size_t)n);
    for (uint32_t t = 0; t < h->n_targets; t++)
        for (uint64_t j = bin_off[t]; j < bin_off[t + 1]; j++) {
            const uint64_t start = (j - bin_off[t]) * bin_size;
            regions[j] = cov_depth_region{t, (uint32_t)start, (uint32_t)std::min<uint64_t>(start + bin_size, h->target_len[t]), 0u};
        }
    std::vector<cov_depth_bin> results((size_t)n);
    std::vector<uint32_t> counts((size_t)n * n_thr);
    int rc = collect_regions(s, h, "covh_depth_bins_counts_write", regions.data(), n, results.data(), counts.data(), n_thr);
    if (rc != COV_OK) return rc;
    rc = covh_depth_bins_counts_format(h, 0, h->n_targets, bin_size, bin_off.data(), results.data(), counts.data(), n_thr, no_zeros, threads, out_fd);
    if (rc != COV_OK) return rc;
    if (n_bins_out) *n_bins_out = n;
    return COV_OK;
}

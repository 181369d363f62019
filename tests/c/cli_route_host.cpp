// csrc/cli_route.h beside the route conditions of ingest() as csrc/host_cli.cpp held them before the routes were gathered into that header
// (commit e01187b; the numbers in the comments are that file's lines): tests/test_cli_route.py compares the two over every combination
// of the facts.  The frozen side is a transcription, expression for expression, folded into "first route" and "route after a decline".
#include <cstdint>
#include <cstdio>
#include <string>

#include "../../coverm_amd/csrc/cli_route.h"

namespace {

enum { DEVICE_BGZF = 0, CPU_STREAM = 1, DEVICE_SAM = 2, HOST_WHOLE = 3, REFUSED = -1 };

struct Frozen {
    bool bgzf, piped, no_stream, per_gene, fp, no_gpu_ingest, pair_on_host, sam_on_host, genes_decode_on_host;
    uint32_t span_count;
    bool pair_dev() const { return fp && !no_stream && !per_gene && bgzf && !no_gpu_ingest && !pair_on_host; }                       // 296
    bool stream() const { return !no_stream && (!fp || pair_dev()) && !per_gene && bgzf; }                                           // 297
    bool sam_dev() const { return !bgzf && !no_stream && !sam_on_host && span_count == 1 && !(fp && pair_on_host) && (piped || !no_gpu_ingest); }   // 411
    bool gff_dev() const { return per_gene && bgzf && !no_stream && span_count == 1 && !no_gpu_ingest && !genes_decode_on_host && !pair_on_host; }   // 481

    int first(std::string &msg) const {
        if (span_count > 1 && !stream()) { msg = "--devices with fewer BAM files than devices needs streamable input (BAM, no --gff)"; return REFUSED; }   // 298
        if (stream() && !no_gpu_ingest) return DEVICE_BGZF;                                                                           // 303
        if (stream() && !fp) return CPU_STREAM;                                                                                       // 371
        if (!bgzf && piped && !sam_dev()) {                                                                                           // 412
            msg = "a pipe ('-b -', a FIFO) is decoded on the device only: COVERM_SAM_ON_HOST / COVERM_PAIR_ON_HOST need a file";
            return REFUSED;
        }
        if (sam_dev()) return DEVICE_SAM;                                                                                             // 413
        if (gff_dev()) return DEVICE_BGZF;                                                                                            // 481
        return HOST_WHOLE;                                                                                                            // 522-531
    }
    int after(int declined, const std::string &stoit, const std::string &err, std::string &msg) const {
        if (declined == DEVICE_BGZF && stream() && !no_gpu_ingest) {      // the block at 303 fell through (367-370)
            if (fp && span_count > 1) {                                                                                               // 369
                msg = std::string("--devices with fewer BAM files than devices and a pair-mode filter needs the device ingest, which declined this file: ") + err;
                return REFUSED;
            }
            if (stream() && !fp) return CPU_STREAM;                                                                                   // 371
            if (sam_dev()) return DEVICE_SAM;                                                                                         // 413
            if (gff_dev()) return DEVICE_BGZF;                                                                                        // 481
            return HOST_WHOLE;
        }
        if (declined == DEVICE_SAM) {
            if (piped) { msg = stoit + ": " + err + " — a pipe cannot be read again: write the stream to a file"; return REFUSED; }   // 449
            if (gff_dev()) return DEVICE_BGZF;                                                                                        // 481
            return HOST_WHOLE;
        }
        return HOST_WHOLE;      // the block at 481 declined (517-520): have_records stays false
    }
};

Frozen frozen_of(const int32_t *v) { return Frozen{v[0] != 0, v[1] != 0, v[2] != 0, v[3] != 0, v[4] != 0, v[5] != 0, v[6] != 0, v[7] != 0, v[8] != 0, (uint32_t)v[9]}; }

cli_route::RouteFacts facts_of(const int32_t *v) {
    cli_route::RouteFacts f;
    f.bgzf = v[0]; f.piped = v[1]; f.no_stream = v[2]; f.per_gene = v[3]; f.pair_filter = v[4];
    f.no_gpu_ingest = v[5]; f.pair_on_host = v[6]; f.sam_on_host = v[7]; f.genes_decode_on_host = v[8]; f.span_count = (uint32_t)v[9];
    return f;
}

int code_of(cli_route::Route r) {
    switch (r) {
    case cli_route::Route::DeviceBgzf: return DEVICE_BGZF;
    case cli_route::Route::CpuStream: return CPU_STREAM;
    case cli_route::Route::DeviceSam: return DEVICE_SAM;
    case cli_route::Route::HostWhole: return HOST_WHOLE;
    }
    return -2;
}

int answer(const cli_route::Decision &d, char *msg, size_t cap) {
    snprintf(msg, cap, "%s", d.refusal.c_str());
    return d.refused() ? REFUSED : code_of(d.route);
}

}  // namespace

// facts: bgzf, piped, no_stream, per_gene, pair_filter, no_gpu_ingest, pair_on_host, sam_on_host, genes_decode_on_host, span_count.
// Return a route (0 DeviceBgzf, 1 CpuStream, 2 DeviceSam, 3 HostWhole) or -1 with the refusal's text in msg.
extern "C" int route_first(const int32_t *facts, char *msg, size_t cap) { return answer(cli_route::first_route(facts_of(facts)), msg, cap); }

extern "C" int route_first_frozen(const int32_t *facts, char *msg, size_t cap) {
    std::string m;
    const int r = frozen_of(facts).first(m);
    snprintf(msg, cap, "%s", m.c_str());
    return r;
}

extern "C" int route_after(int declined, const int32_t *facts, const char *sample, const char *reason, char *msg, size_t cap) {
    static const cli_route::Route R[4] = {cli_route::Route::DeviceBgzf, cli_route::Route::CpuStream, cli_route::Route::DeviceSam, cli_route::Route::HostWhole};
    return answer(cli_route::after_decline(R[declined], facts_of(facts), sample, reason), msg, cap);
}

extern "C" int route_after_frozen(int declined, const int32_t *facts, const char *sample, const char *reason, char *msg, size_t cap) {
    std::string m;
    const int r = frozen_of(facts).after(declined, sample, reason, m);
    snprintf(msg, cap, "%s", m.c_str());
    return r;
}

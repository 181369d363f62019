// Which reader takes one sample of `coverm-amd contig|genome`, and which one takes it next when that reader hands the file back — as
// pure functions of the facts csrc/host_cli.cpp ingest() collects, so that the decision can be read in one place and tested without a
// device (tests/test_cli_route.py).  No I/O and no environment look-ups here: the four COVERM_* switches arrive as facts.
//
//   DeviceBgzf  the compressed BAM goes to HBM, the device inflates, finds the records and fills its store (covh_bam_gpu_ingest_span)
//   CpuStream   the host inflates and parses window by window and pushes batches (covh_bam_stream_*)
//   DeviceSam   SAM text, a file or a pipe, decoded on the device as it is read (covh_sam_gpu_ingest)
//   HostWhole   the whole file decoded on the host (covh_bam_open), with the host's grouping and pair filter
//
// --gff is no route of its own: after DeviceBgzf or DeviceSam the records come back from the store for the gene driver (per_gene).
// A device route declines a file by returning 1, or when its pair filter returns COV_ERR_INGEST_FALLBACK; errors are not declines.
#pragma once
#include <cstdint>
#include <string>

namespace cli_route {

struct RouteFacts {
    bool bgzf = false;            // the file starts with the gzip magic (never true for a pipe)
    bool piped = false;           // "-", a FIFO or a character device: can be read once
    bool no_stream = false;       // --no-stream
    bool per_gene = false;        // --gff
    bool pair_filter = false;     // a pair-mode reader filter is on (Run::fp)
    uint32_t span_count = 1;      // > 1: --devices with fewer files than devices, this sample is one tid span of its file
    bool no_gpu_ingest = false;          // COVERM_NO_GPU_INGEST
    bool pair_on_host = false;           // COVERM_PAIR_ON_HOST
    bool sam_on_host = false;            // COVERM_SAM_ON_HOST
    bool genes_decode_on_host = false;   // COVERM_GENES_DECODE_ON_HOST
};

enum class Route { DeviceBgzf, CpuStream, DeviceSam, HostWhole };

struct Decision {
    Route route = Route::HostWhole;
    std::string refusal;      // not empty: no route, the run ends with this message
    bool refused() const { return !refusal.empty(); }
};

inline Decision take(Route r) { Decision d; d.route = r; return d; }
inline Decision refuse(const std::string &why) { Decision d; d.refusal = why; return d; }

inline Decision first_route(const RouteFacts &f) {
    const bool streamable = f.bgzf && !f.no_stream && !f.per_gene && (!f.pair_filter || (!f.no_gpu_ingest && !f.pair_on_host));
    if (f.span_count > 1 && !streamable) return refuse("--devices with fewer BAM files than devices needs streamable input (BAM, no --gff)");
    const bool pair_here = f.pair_filter && f.pair_on_host;      // the pair filter is to run on the host: no device route
    if (f.bgzf && !f.no_stream) {
        const bool device = !f.no_gpu_ingest && (f.per_gene ? !f.genes_decode_on_host && !f.pair_on_host : !pair_here);
        if (device) return take(Route::DeviceBgzf);
        if (streamable) return take(Route::CpuStream);      // (no pair filter here: with one, streamable means the device took the file)
    }
    if (!f.bgzf && !f.no_stream && !f.sam_on_host && !pair_here && (f.piped || !f.no_gpu_ingest)) return take(Route::DeviceSam);
    if (!f.bgzf && f.piped) return refuse("a pipe ('-b -', a FIFO) is decoded on the device only: COVERM_SAM_ON_HOST / COVERM_PAIR_ON_HOST need a file");
    return take(Route::HostWhole);
}

// `declined` handed the file back with `reason`; `sample` names it in a refusal.  CpuStream and HostWhole never decline.
inline Decision after_decline(Route declined, const RouteFacts &f, const std::string &sample, const std::string &reason) {
    if (declined == Route::DeviceSam) {
        if (f.piped) return refuse(sample + ": " + reason + " — a pipe cannot be read again: write the stream to a file");
        return take(Route::HostWhole);
    }
    if (f.per_gene) return take(Route::HostWhole);
    if (!f.pair_filter) return take(Route::CpuStream);      // same span
    if (f.span_count > 1)
        return refuse("--devices with fewer BAM files than devices and a pair-mode filter needs the device ingest, which declined this file: " + reason);
    return take(Route::HostWhole);
}

}  // namespace cli_route

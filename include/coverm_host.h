/*
 * coverm_host.h — host side ABOVE the covermhip C ABI, in C++ with a C surface.
 *
 * The reference keeps these layers in Rust; no Rust toolchain exists in this build environment, so
 * they are written in C++ with the same names, argument meaning and error behaviour:
 *
 *   CoverageEstimator::{new_estimator_*, calculate_coverage, print_coverage, print_zero_coverage}
 *                                   src/mosdepth_genome_coverage_estimators.rs:107-224, 530-839, 936-991
 *   contig_coverage                 src/contig.rs:13-253           (flush + zero-row logic :40-104, 255-277)
 *   mosdepth_genome_coverage_with_contig_names   src/genome.rs:17-322
 *   mosdepth_genome_coverage        src/genome.rs:419-929
 *   CoverageTaker implementations   src/coverage_takers.rs:74-219, 265-377
 *   CoveragePrinter                 src/coverage_printer.rs:20-553
 *   EstimatorsAndTaker / FilterParameters  src/bin/coverm.rs:1315-1504, 1648-1704
 *   BAM/SAM reading (rust-htslib in the reference)  src/bam_generator.rs:103-144, 356-371
 *
 * The scan loops here do not touch reads: they consume the per-contig integer statistics a
 * covermhip session produced (cov_contig_stats + histograms) where the reference would have called
 * add_contig(ups_and_downs, ...).  Every f32 is formed from those integers with the reference's
 * operation order, so results are bit-identical, not merely within tolerance.
 */
#ifndef COVERM_HOST_H
#define COVERM_HOST_H

#include <stddef.h>
#include <stdint.h>

#include "covermhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* enum CoverageEstimator variant order, estimators.rs:4-81 */
typedef enum {
    COVH_MEAN = 0,
    COVH_TRIMMED_MEAN = 1,
    COVH_PILEUP_COUNTS = 2,
    COVH_COVERED_FRACTION = 3,
    COVH_COVERED_BASES = 4,
    COVH_RPKM = 5,
    COVH_TPM = 6,
    COVH_VARIANCE = 7,
    COVH_LENGTH = 8,
    COVH_READ_COUNT = 9,
    COVH_READS_PER_BASE = 10,
    COVH_ANIR = 11
} covh_kind;

/* Constructor parameters (estimators.rs:107-224). */
typedef struct {
    int32_t kind;
    float min_fraction_covered_bases;
    uint64_t contig_end_exclusion; /* must equal the session's cov_config.contig_end_exclusion */
    int32_t exclude_mismatches;
    float trim_min, trim_max;
} covh_estimator;

typedef struct {
    uint64_t num_mapped_reads, num_reads; /* ReadsMapped, lib.rs:54-57 */
} covh_reads_mapped;

/* One sample's device results, as returned by cov_finish / cov_fetch_hist. */
typedef struct {
    const char *stoit_name;
    const cov_contig_stats *stats; /* n_targets entries */
    const uint64_t *hist;          /* may be NULL when no estimator needs histograms */
    uint64_t num_detected_primary_alignments;
} covh_sample;

/* BAM header as the scan loops use it (names + lengths). */
typedef struct {
    uint32_t n_targets;
    const char *names;        /* concatenated, not NUL separated */
    const uint32_t *name_off; /* n_targets + 1 */
    const uint64_t *target_len;
} covh_header;

typedef enum {
    COVH_TAKER_STREAM = 0, /* SingleFloatCoverageStreamingCoveragePrinter */
    COVH_TAKER_PILEUP = 1, /* PileupCoverageCoveragePrinter */
    COVH_TAKER_CACHED = 2  /* CachedSingleFloatCoverageTaker */
} covh_taker_kind;

typedef struct covh_taker covh_taker;     /* owns an output text buffer */
covh_taker *covh_taker_new(int kind, size_t num_coverages);
void covh_taker_free(covh_taker *t);
const char *covh_taker_text(const covh_taker *t, size_t *len); /* streamed output so far */
void covh_taker_clear_text(covh_taker *t);
/* Cached taker: the f32 coverages recorded for sample `stoit`, in recording order (entries x estimators);
 * returns the number available (copies at most cap). */
size_t covh_taker_cached_coverages(const covh_taker *t, size_t stoit, float *out, size_t cap);

/* trait CoverageTaker (coverage_takers.rs:29-38): start_stoit once per BAM; per entry start_entry -> add_* (one per
 * estimator, in estimator order) -> finish_entry.  The scan drivers below make these calls themselves. */
void covh_taker_start_stoit(covh_taker *t, const char *stoit_name);
void covh_taker_start_entry(covh_taker *t, size_t entry_order_id, const char *entry_name);
void covh_taker_add_single_coverage(covh_taker *t, float coverage);
void covh_taker_add_coverage_entry(covh_taker *t, uint64_t num_reads, uint64_t num_bases);
void covh_taker_finish_entry(covh_taker *t);
int covh_taker_names_mismatch(const covh_taker *t); /* an entry id arrived with two different names (:140-148) */
/* Cached taker: CoverageTakerTypeIterator (coverage_takers.rs:265-377), flattened; returns the item count. */
size_t covh_taker_iterate(const covh_taker *t, uint64_t *entry_index, uint64_t *stoit_index, float *coverages, size_t cap);

/* Which need a histogram / identity sums from the device (COV_WANT_* for the session). */
uint32_t covh_wants(const covh_estimator *est, size_t n_est);

/* The three scan entry points.  Return COV_OK or a cov_status; *err (optional) receives a static message. */
int covh_contig_coverage(const covh_header *h, const covh_sample *samples, size_t n_samples, covh_taker *taker,
                         const covh_estimator *est, size_t n_est, int print_zero_coverage_contigs,
                         covh_reads_mapped *reads_mapped_out);
/* The same loop with calculate_coverage already evaluated on the device: estimates[i] = the n_targets x n_est floats cov_fetch_estimates
 * returned for sample i (after cov_set_estimators with these estimators), or NULL for a sample to evaluate here; estimates itself may be
 * NULL.  The floats are the same bit for bit, so rows, zero rows and ReadsMapped (contig.rs:40-104) are those of covh_contig_coverage.
 * COVH_PILEUP_COUNTS and COVH_TPM are never evaluated on the device: COV_ERR_INVALID_ARG when floats are given with one of them. */
int covh_contig_coverage_estimated(const covh_header *h, const covh_sample *samples, size_t n_samples, covh_taker *taker,
                                   const covh_estimator *est, size_t n_est, int print_zero, covh_reads_mapped *rm_out,
                                   const float *const *estimates);
int covh_genome_coverage_with_contig_names(const covh_header *h, const covh_sample *samples, size_t n_samples,
                                           const int32_t *genome_of_tid, const char *const *genome_names,
                                           size_t n_genomes, covh_taker *taker, int print_zero_coverage_genomes,
                                           const covh_estimator *est, size_t n_est,
                                           covh_reads_mapped *reads_mapped_out);
/* The contig-names genome scan of ONE sample with the genomes already aggregated and evaluated on the device (cov_set_genomes):
 * estimates = the n_genomes x n_est floats of cov_fetch_genome_estimates, gstats = cov_fetch_genome_stats' entries, any_contig_seen =
 * some reference of the sample had a considered record (cov_summary.n_considered != 0; genome.rs:230-234 prints nothing otherwise when
 * the sample has no primary alignment either).  What is left here is genome.rs:236-302's control flow: zero rows, --no-zeros,
 * ReadsMapped, the taker calls, in genome order — the entries covh_genome_coverage_with_contig_names emits.  COVH_PILEUP_COUNTS and
 * COVH_TPM are never evaluated on the device: COV_ERR_INVALID_ARG. */
int covh_genome_coverage_estimated(const char *stoit_name, uint64_t num_detected_primary_alignments, int any_contig_seen,
                                   const char *const *genome_names, size_t n_genomes, covh_taker *taker, int print_zero_coverage_genomes,
                                   const covh_estimator *est, size_t n_est, const float *estimates, const cov_genome_stats *gstats,
                                   covh_reads_mapped *reads_mapped_out);
int covh_genome_coverage_separator(const covh_header *h, const covh_sample *samples, size_t n_samples,
                                   uint8_t split_char, covh_taker *taker, int print_zero_coverage_genomes,
                                   const covh_estimator *est, size_t n_est, int single_genome,
                                   covh_reads_mapped *reads_mapped_out);
/* The separator / single-genome scan's genome ids of a header (cov_set_genome_runs' gid_of_tid): dense ids of the names' prefixes before
 * split_char in order of first appearance, all 0 for single_genome.  Returns the number of ids, or 0 when some name does not contain
 * split_char (the scan raises "Contig name does not contain split symbol" only for the names it touches: such a header stays with
 * covh_genome_coverage_separator). */
uint32_t covh_genome_separator_ids(const covh_header *h, uint8_t split_char, int single_genome, int32_t *gid_of_tid);
/* The entries of ONE sample's separator scan aggregated on the host from per-contig statistics: the table entry -> targets by
 * csrc/sep_entry_core.h's CPU emulation, EntryAcc::add_contig over each entry's observed targets in ascending order and
 * calculate_coverage with its unobserved lengths — what covh_genome_coverage_separator computes and what cov_fetch_genome_entries /
 * cov_fetch_genome_estimates return from the device, bit for bit.  entries: room for n_targets, estimates: n_targets x n_est. */
int covh_genome_separator_entries(const covh_header *h, const covh_sample *sample, const int32_t *gid_of_tid, const covh_estimator *est,
                                  size_t n_est, cov_genome_entry *entries, float *estimates, size_t *n_entries);
/* The separator / single-genome scan of ONE sample with its entries aggregated and evaluated already (cov_set_genome_runs, or
 * covh_genome_separator_entries): n_entries > 0 entries (a sample without an observed target runs covh_genome_coverage_separator:
 * nothing to aggregate) and n_entries x n_est floats.  What is left is genome.rs:419-797's control flow: start_entry(first_tid, name),
 * the zero rows of the genomes between two entries, --no-zeros, ReadsMapped.  Every name of the header contains split_char. */
int covh_genome_coverage_separator_estimated(const covh_header *h, const char *stoit_name, uint64_t num_detected_primary_alignments,
                                             uint8_t split_char, int single_genome, covh_taker *taker, int print_zero_coverage_genomes,
                                             const covh_estimator *est, size_t n_est, const cov_genome_entry *entries, size_t n_entries,
                                             const float *estimates, covh_reads_mapped *reads_mapped_out);
const char *covh_last_error(void);

/* CoveragePrinter (coverage_printer.rs).  printer: 0 streamed, 1 sparse cached, 2 dense cached, 3 MetaBAT.
 * Appends to the taker's text buffer. */
void covh_print_headers(covh_taker *t, int printer, const char *entry_type, const char *const *headers, size_t n);
void covh_finalise_printing(covh_taker *t, int printer, const char *entry_type, const char *const *headers,
                            size_t n_headers, const covh_reads_mapped *reads_mapped, size_t n_samples,
                            const int64_t *columns_to_normalise, size_t n_norm, int64_t rpkm_column,
                            int64_t tpm_column);

/* Rust `Display` for f32 / f64 (shortest round-trip, positional notation).  Returns bytes written. */
size_t covh_format_f32(float v, char *buf, size_t cap);
size_t covh_format_f64(double v, char *buf, size_t cap);

/* ---- BGZF / BAM / SAM reader (rust-htslib's role: bam_generator.rs:113-119, 125-129, 356-371).
 * Decodes the whole file with `threads` inflate/parse threads and exposes the records as a cov_batch whose
 * arrays stay owned by the handle.  want_names also keeps read names (pair-mode filtering, filter.rs:164). */
typedef struct covh_bam covh_bam;
covh_bam *covh_bam_open(const char *path, int threads, int want_names, char *err, size_t errcap);
void covh_bam_close(covh_bam *h);
/* Keep the largest inflate buffer mapped between files (off by default; turning it off frees it).  A tool that
 * reads many BAMs in a row saves the unmap + first-touch of gigabytes per file. */
void covh_bam_set_buffer_cache(int on);
/* Decode record arrays into page-locked memory from cov_host_alloc (off by default; falls back to ordinary memory
 * when no device is usable), so that cov_push_batch is a plain DMA. */
void covh_bam_set_pinned(int on);
/* 1: covh_bam_gpu_ingest* gives its page-locked staging slots back to the system as soon as their last uploads are through (a session
 * that reads no further file; page-locked memory still held at process exit costs ~0.13 s per GiB).  Default 0: the slots are parked for
 * the next file. */
void covh_bam_set_release_staging(int on);
/* 1 when COVERM_CLI_TIMING is set: the library's and the host layer's timing stamps go to stderr (read once per process). */
int covh_timing_on(void);
/* How many device ingests (covh_bam_gpu_ingest*) the caller runs at once, one per GPU.  With more than two and no COVERM_INGEST_IO the
 * file is mapped and its span registered with the device once, up front, instead of copied through page-locked staging slots: N feeders
 * share one host memory system, and a staged byte crosses it three times, a mapped one once (unmeasured on more
 * than one device).  Default 1. */
void covh_bam_set_concurrent_feeders(int n);
uint32_t covh_bam_n_targets(const covh_bam *h);
const char *covh_bam_target_name(const covh_bam *h, uint32_t i);
uint64_t covh_bam_target_len(const covh_bam *h, uint32_t i);
uint64_t covh_bam_n_records(const covh_bam *h);
uint64_t covh_bam_n_cigar(const covh_bam *h);
void covh_bam_batch(const covh_bam *h, cov_batch *out);
const int32_t *covh_bam_mtid(const covh_bam *h);
const uint32_t *covh_bam_qname_off(const covh_bam *h); /* n_records + 1, NULL without want_names */
const char *covh_bam_qnames(const covh_bam *h);
/* Writes a batch as a coordinate-sorted BGZF BAM (benchmark/test inputs), NM typed C/S/I by magnitude.  with_seq: 0 = SEQ
 * '*'; 1 = read names r<i>, SEQ all 'A', QUAL 0xff (compresses ~18x: inflate cost far below a real BAM's); 2 = realistic
 * entropy: random bases, Phred-like binned qualities, Illumina-style names (~65 compressed bytes per 150 bp read).
 * Chunked, bounded memory.  Returns 0 on success. */
int covh_bam_write(const char *path, uint32_t n_targets, const char *const *names, const uint64_t *lens,
                   const cov_batch *batch, int with_seq, int level, int threads);

/* ---- streamed reader: the same decode window by window with bounded memory (three ~32 MiB-compressed windows and three
 * page-locked SoA batches circulate), so that inflate, record parsing and the H2D copy of finished batches overlap inside one
 * file.  BAM only (BGZF); no read names (pair-mode filtering and --gff use covh_bam_open).  span_count > 1 selects the
 * span_index-th of span_count tid ranges, cut where the tid changes nearest to k/span_count of the file; the rank's first
 * BGZF block is located by probing the file, so each rank inflates only its own part.  A sorted BAM's records
 * fall into exactly one span each (records with tid -1 go to the last one).
 *   h = covh_bam_stream_open(path, threads, 0, 1, err, cap);   header accessors are valid at once
 *   while (covh_bam_stream_next(h, &batch) == 1) cov_push_batch(session, &batch);   arrays stay valid until the next call
 * covh_bam_stream_next returns 1 (batch), 0 (end of file / span), -1 (covh_bam_stream_error) or -2 (the same, and the error is
 * "the record keys decrease inside this span": see covh_bam_gpu_ingest_span). */
typedef struct covh_bam_stream covh_bam_stream;
covh_bam_stream *covh_bam_stream_open(const char *path, int threads, uint32_t span_index, uint32_t span_count, char *err, size_t errcap);
uint32_t covh_bam_stream_n_targets(const covh_bam_stream *h);
const char *covh_bam_stream_target_name(const covh_bam_stream *h, uint32_t i);
uint64_t covh_bam_stream_target_len(const covh_bam_stream *h, uint32_t i);
int covh_bam_stream_next(covh_bam_stream *h, cov_batch *out);
const char *covh_bam_stream_error(const covh_bam_stream *h);
/* Which inflate the HOST readers of this process use (covh_bam_open, covh_bam_stream_*, coverm-amd filter): "libdeflate" when
 * libdeflate.so.0 could be bound at run time, else "zlib" — so that a CPU baseline timed with them can say what it was timed on. */
const char *covh_inflate_backend(void);
uint64_t covh_bam_stream_n_records(const covh_bam_stream *h);  /* records handed out so far */
uint64_t covh_bam_stream_peak_bytes(const covh_bam_stream *h); /* largest total of window + batch buffers held */
void covh_bam_stream_timing(const covh_bam_stream *h, double *out5); /* s: read, inflate, parse, inflate-side wait, parse-side wait */
void covh_bam_stream_close(covh_bam_stream *h);

/* ---- device ingest driver (cov_ingest_* of covermhip.h): header on the host, everything else on the GPU.
 *   hd = covh_bam_read_header(path, ...)  -> reference names / lengths (cov_set_targets) and where the records start
 *   covh_bam_gpu_ingest(path, threads, session, hd, check_crc, &n, timing, err, cap)
 *       0 = the records are in the session's store; 1 = this file needs the CPU reader (reason in err, nothing appended:
 *       use covh_bam_stream_* / covh_bam_open); -1 = error.  threads read the file into page-locked staging buffers. */
typedef struct covh_bam_header covh_bam_header;
covh_bam_header *covh_bam_read_header(const char *path, char *err, size_t errcap);
void covh_bam_header_free(covh_bam_header *h);
uint32_t covh_bam_header_n_targets(const covh_bam_header *h);
const char *covh_bam_header_target_name(const covh_bam_header *h, uint32_t i);
uint64_t covh_bam_header_target_len(const covh_bam_header *h, uint32_t i);
uint64_t covh_bam_header_first_record(const covh_bam_header *h); /* offset in the inflated stream */
/* covh_bam_gpu_ingest_span: one tid span of the file (span definition of covh_bam_stream_open): only the span's part of the file
 * is read and fed; 0 with *n_records = 0 for an empty span.  -2 (instead of -1) when the record keys decrease inside the span: a span
 * trusts the file's order, so the caller decides (coverm-amd then sends the file through one device whole, where the reference's
 * own rule, contig.rs:118-132, judges it). */
int covh_bam_gpu_ingest_span(const char *path, int threads, cov_session *s, const covh_bam_header *hd, int check_crc, uint32_t span_index,
                             uint32_t span_count, uint64_t *n_records, double *timing8, char *err, size_t errcap);
int covh_bam_gpu_ingest(const char *path, int threads, cov_session *s, const covh_bam_header *hd, int check_crc, uint64_t *n_records,
                        double *timing8, char *err, size_t errcap);   /* s: file read, staging waits, cov_ingest_end, total, buffers, block-header walk, cov_ingest_feed; [7] = where the DMA read the bytes (0 staging slots, 1 the mapped file, 2 mapped and registered up front) */
/* SAM text to the device (cov_sam_*), from a regular file, a FIFO, a character device or standard input (path "-"): the stream is read
 * with read() alone.  covh_sam_open reads up to the end of the header (the `@` lines in front of the first alignment line) and tells the
 * format from the first bytes read: covh_sam_kind 0 = SAM text, 1 = BGZF magic (a BAM), 2 = not text (NUL bytes).  covh_sam_gpu_ingest
 * (after cov_set_targets with the header's lengths) replays those bytes and reads on into COV_INGEST_SLOTS page-locked slots of one decode
 * window each — a reader thread fills a slot while the previous one uploads — keeping lines whole: each piece is cut at its last '\n'
 * and the rest is carried into the next.  Returns 0 = the records are in the session's store; 1 = irregular input (a header line behind
 * the first alignment line): nothing appended, decode the file on the host if it can be read again; -1 = error (err names the line).
 * tm (4 doubles, may be NULL): seconds in read(), waiting for slots, in cov_sam_feed, in total. */
typedef struct covh_sam covh_sam;
covh_sam *covh_sam_open(const char *path, char *err, size_t errcap);
int covh_sam_kind(const covh_sam *h);
int covh_sam_is_pipe(const covh_sam *h);
uint32_t covh_sam_n_targets(const covh_sam *h);
const char *covh_sam_target_name(const covh_sam *h, uint32_t i);
uint64_t covh_sam_target_len(const covh_sam *h, uint32_t i);
const char *covh_sam_header_text(const covh_sam *h);
int covh_sam_gpu_ingest(covh_sam *h, int threads, cov_session *s, uint64_t *n_records, double *tm, char *err, size_t errcap);
void covh_sam_close(covh_sam *h);

/* ---- reader-stage PAIR filter (ReferenceSortedBamFilter::read pair branch, filter.rs:117-228, filter_out = true).
 * The single-read branch runs on the device (cov_config.filter_single); the pair branch needs read names, which never
 * cross the covermhip ABI, so it runs here, threaded over references.  Thresholds as FilterParameters holds them
 * (coverm.rs:1648-1704); filter_single = ReferenceSortedBamFilter::filter_single (filter.rs:48-55). */
typedef struct {
    int32_t filter_single;
    uint8_t min_mapq; /* 255 = off */
    uint32_t min_aligned_length_single;
    float min_percent_identity_single, min_aligned_percent_single;
    uint32_t min_aligned_length_pair;
    float min_percent_identity_pair, min_aligned_percent_pair;
} covh_pair_filter;
/* Indices of the records the reference's filter would return, in its order (first mate then second mate, pairs
 * ordered by where the second mate sits in the file).  *order_out is released with covh_free.  Returns COV_OK, or
 * COV_ERR_NM_MISSING / COV_ERR_NM_BADTYPE where the reference's nm() would have panicked. */
int covh_pair_mode_order(const cov_batch *b, const int32_t *mtid, const uint32_t *qname_off, const char *qnames,
                         const covh_pair_filter *f, int threads, uint64_t **order_out, uint64_t *n_out);
/* ReferenceSortedBamFilter::read as a whole (filter.rs:84-228), serial: the single-read branch when f->filter_single && !filter_pairs,
 * the pair branch otherwise; filter_out = 0 is `coverm filter --inverse` (unmapped records and — in the pair branch — improper pairs are
 * returned, and a record / pair is returned iff it FAILS its judgement).  The selection of the `filter` subcommand. */
int covh_reader_filter_order(const cov_batch *b, const int32_t *mtid, const uint32_t *qname_off, const char *qnames, const covh_pair_filter *f,
                             int filter_pairs, int include_supplementary, int include_secondary, int filter_out, uint64_t **order_out, uint64_t *n_out);
/* `coverm filter` (bin/coverm.rs:408-472): the records of the BAM file `in_path` that the reader filter returns, byte for byte (names,
 * bases, qualities, tags) and in its order, under the input's header, as a new BGZF-compressed BAM.  Host code, like the reference's.
 * Returns 0, or -1 with a message. */
int covh_bam_filter_file(const char *in_path, const char *out_path, const covh_pair_filter *f, int filter_pairs, int include_supplementary,
                         int include_secondary, int filter_out, int level, int threads, uint64_t *n_in, uint64_t *n_out, char *err, size_t errcap);
void covh_free(void *p);
/* --unsorted on the host (whole-file arrays: SAM text, --no-stream, files the device ingest declines, ahead of covh_pair_mode_order and the
 * gene driver): the stable order cov_group_records gives on the device — order[new] = old, references in ascending tid order, records
 * without a reference (tid < 0 or >= n_targets) last, the input's order kept inside a reference.  *order_out (n entries) is released with
 * covh_free; *n_moved = entries with order[j] != j.  Gather with covh_batch_select. */
int covh_group_by_reference(const int32_t *tid, uint64_t n, uint32_t n_targets, uint64_t **order_out, uint64_t *n_moved);
/* Gathers records order[0..n) of src into a new batch (page-locked memory when a device is usable). */
int covh_batch_select(const cov_batch *src, const uint64_t *order, uint64_t n, int threads, cov_batch *out);
void covh_batch_free(cov_batch *b);

/* ---- per-gene coverage (--gff; src/genes.rs:182-567).  The contig's depth comes through a callback (cov_copy_depth of a
 * finished session in the product); GFF parsing, gene resolution, per-gene window statistics and per-gene read aggregates
 * (reads are assigned to the gene their leftmost position falls in) are this host code.  One call per BAM. */
typedef struct covh_genes covh_genes;
covh_genes *covh_genes_read_gff(const char *path, const char *feature_type /* NULL = every feature */, char *err, size_t errcap);
covh_genes *covh_genes_from_arrays(const char *const *ids, const char *const *contigs, const uint64_t *start,
                                   const uint64_t *end, size_t n); /* 0-based half-open */
size_t covh_genes_count(const covh_genes *g);
void covh_genes_get(const covh_genes *g, size_t i, const char **id, const char **contig, uint64_t *start, uint64_t *end);
void covh_genes_free(covh_genes *g);
typedef int (*covh_depth_fn)(void *ctx, uint32_t tid, int32_t *depth_out); /* target_len[tid] entries; COV_OK or a status */
typedef struct {
    int32_t mode; /* 0 no genome column (contig mode), 1 single genome "genome1", 2 prefix before `separator`, 3 table */
    uint8_t separator;
    const int32_t *genome_of_tid;    /* mode 3: -1 = contig in no genome (its genes are not reported) */
    const char *const *genome_names; /* mode 3 */
} covh_genome_namer;
/* records = what the scan sees (after a pair-mode reader stage, if any); cfg carries the flag filter, the single-read
 * thresholds (filter_single) and nothing else that matters here; num_detected_primary_alignments as the reader counted it.
 * device_session (a finished session holding these records) selects the device reductions (cov_interval_stats_compute: one
 * wave per gene over the depth kept in HBM); with NULL the depth callback is used and the reductions run on the host. */
int covh_gene_coverage(const covh_header *h, const covh_genes *genes, const covh_genome_namer *namer, const char *stoit_name,
                       const cov_batch *records, const cov_config *cfg, cov_session *device_session, covh_depth_fn depth,
                       void *depth_ctx, uint64_t num_detected_primary_alignments, covh_taker *taker, const covh_estimator *est,
                       size_t n_est, int print_zero_coverage_genes, covh_reads_mapped *reads_mapped_out);
/* The same scan with the per-read numbers of every gene from whoever holds the records, in place of the records: `reads` is called once,
 * before anything is written, with every resolved gene as an interval (tid ascending, inside a tid by start: the order of the entries) and
 * fills one cov_interval_reads per interval, *mapped_total and *sorted_by_start as cov_interval_reads_compute does — which is what the
 * product passes (covh_session_interval_reads, ctx = the session).  Its status is returned as it is (COV_ERR_NM_* / COV_ERR_UNSORTED /
 * COV_ERR_BAD_TID with covh_gene_coverage's texts).  *sorted_by_start = 0 on return: starts decrease inside a contig, NOTHING was written to
 * the taker and COV_OK is returned: run covh_gene_coverage over the records.  Contigs are emitted in tid order, those with
 * contig_taken > 0 as the scan emits a contig it saw, the others as zero rows.  Everything else as covh_gene_coverage. */
typedef int (*covh_interval_reads_fn)(void *ctx, const cov_interval *intervals, uint64_t n, int want_identity, cov_interval_reads *out,
                                      uint64_t *mapped_total, int *sorted_by_start);
int covh_gene_coverage_reads(const covh_header *h, const covh_genes *genes, const covh_genome_namer *namer, const char *stoit_name,
                             covh_interval_reads_fn reads, void *reads_ctx, cov_session *device_session, covh_depth_fn depth,
                             void *depth_ctx, uint64_t num_detected_primary_alignments, covh_taker *taker, const covh_estimator *est,
                             size_t n_est, int print_zero_coverage_genes, covh_reads_mapped *reads_mapped_out, int *sorted_by_start);
int covh_session_interval_reads(void *ctx, const cov_interval *intervals, uint64_t n, int want_identity, cov_interval_reads *out,
                                uint64_t *mapped_total, int *sorted_by_start);

/* ---- depth runs as a bedGraph (`coverm-amd depth`): the runs cov_depth_runs_compute leaves on the device, as text lines
 *   name \t start \t end \t depth \n        0-based, half open; end = the start of the target's next run, or the target's length
 * in target order, then position order.  no_zeros drops the lines of depth 0 (the device always emits every run).
 * covh_depth_runs_format needs no device: the runs of targets [tid_lo, tid_lo + n_targets) of `h` (run_off: n_targets + 1 entries, as
 * cov_depth_runs_fetch returns them), formatted on up to `threads` threads in ordered pieces and written to the descriptor out_fd in order;
 * the text is the same for every thread count.  covh_depth_runs_write does that for every target of a finished session, chunk by chunk
 * (cov_depth_runs_compute / cov_depth_runs_fetch into page-locked memory): host memory is bounded by the chunk's runs.  *n_runs_out (may be
 * NULL) = the runs the device emitted.  COV_OK, or the ABI's status with its text in covh_last_error (COV_ERR_STATE after a spill of the
 * bounded record store); COV_ERR_INVALID_ARG "write failed" when the descriptor refuses the bytes. */
int covh_depth_runs_format(const covh_header *h, uint32_t tid_lo, uint32_t n_targets, const uint64_t *run_off, const cov_depth_run *runs,
                           int no_zeros, int threads, int out_fd);
int covh_depth_runs_write(cov_session *s, const covh_header *h, int no_zeros, int threads, int out_fd, uint64_t *n_runs_out);

/* ---- depth bins as a bedGraph (`coverm-amd depth --bin-size N`): the bins cov_depth_bins_compute leaves on the device, as text lines
 *   name \t start \t end \t value \n        0-based, half open; start = b * bin_size, end = min(start + bin_size, the target's length)
 * in target order, then position order.  `value` picks what is printed: sum, min, max and covered as integers, mean as
 * (double)sum / (double)(end - start) with "%.3f" (sum < 2^53: the text is an exact function of the two integers).  no_zeros drops the bins
 * whose max is 0, for every value.
 * covh_depth_bins_format needs no device: the bins of targets [tid_lo, tid_lo + n_targets) of `h` (bin_off: n_targets + 1 entries, as
 * cov_depth_bins_fetch returns them), formatted on up to `threads` threads in ordered pieces and written to out_fd in order; the text is the
 * same for every thread count.  covh_depth_bins_write does that for every target of a finished session, chunk by chunk, through page-locked
 * memory.  *n_bins_out (may be NULL) = the bins the device computed.  Status and errors as for the runs. */
typedef enum { COVH_BIN_MEAN = 0, COVH_BIN_SUM = 1, COVH_BIN_MIN = 2, COVH_BIN_MAX = 3, COVH_BIN_COVERED = 4 } covh_bin_value;
int covh_depth_bins_format(const covh_header *h, uint32_t tid_lo, uint32_t n_targets, uint32_t bin_size, const uint64_t *bin_off,
                           const cov_depth_bin *bins, int value, int no_zeros, int threads, int out_fd);
int covh_depth_bins_write(cov_session *s, const covh_header *h, uint32_t bin_size, int value, int no_zeros, int threads, int out_fd,
                          uint64_t *n_bins_out);

/* ---- depth regions of a BED file (`coverm-amd depth --regions r.bed`): per region the value cov_depth_regions_compute leaves on the device.
 * covh_bed_read needs no device.  It reads lines  chrom \t start \t end [\t name [\t ...]]  (0-based, half open); a trailing \r is stripped;
 * empty lines and lines beginning with '#', "track" or "browser" are skipped; start and end are decimal integers <= 2^31 - 1; field 4, if
 * present, is the region's name, verbatim.  A syntax error or start >= end returns NULL with "<path>:<line>: <what>" in covh_last_error.
 * covh_bed_line returns region i as the file gave it (chrom and name are NOT NUL terminated; name == NULL for a line without one).
 * covh_bed_resolve fills out[covh_bed_count] against a header: chrom must equal a reference name exactly; an unknown name and an end beyond
 * the reference's length are errors with the same "<path>:<line>: " prefix (a BED file for another assembly is a mistake worth hearing about).
 * covh_depth_regions_format needs no device: one line per region IN THE FILE'S ORDER from results[covh_bed_count] in that order,
 *   chrom \t start \t end \t value \n     or     chrom \t start \t end \t name \t value \n     when the line had a name;
 * `value` is a covh_bin_value, printed exactly as the bins print it (mean = (double)sum / (double)(end - start) with "%.3f"); no_zeros drops
 * the regions whose max is 0; formatted on up to `threads` threads in ordered pieces, the same text for every thread count.
 * covh_depth_regions_write resolves, calls cov_depth_regions_set and walks the chunks of a finished session, SKIPPING targets without a
 * region (the next chunk begins at the first target at or behind tid_next that has one), fetches through page-locked memory, scatters by
 * input_index into one array of 24 B per region and formats once, at the end.  *n_regions_out (may be NULL) = the regions computed. */
typedef struct covh_bed covh_bed;
covh_bed *covh_bed_read(const char *path);
void covh_bed_free(covh_bed *b);
uint64_t covh_bed_count(const covh_bed *b);
int covh_bed_line(const covh_bed *b, uint64_t i, const char **chrom, uint32_t *chrom_len, uint32_t *start, uint32_t *end, const char **name,
                  uint32_t *name_len, uint64_t *line_no);
int covh_bed_resolve(const covh_bed *b, const covh_header *h, cov_depth_region *out);
int covh_depth_regions_format(const covh_bed *b, const cov_depth_bin *results, int value, int no_zeros, int threads, int out_fd);
int covh_depth_regions_write(cov_session *s, const covh_header *h, const covh_bed *b, int value, int no_zeros, int threads, int out_fd,
                             uint64_t *n_regions_out);

/* ---- depth classes (`coverm-amd depth --quantize SPEC`, `--thresholds LIST`): the text of cov_depth_class_runs_compute's runs and of the
 * threshold counts cov_depth_regions_compute leaves beside its results.
 * covh_depth_quantize_parse reads a --quantize spec: decimal non-negative integers separated by ':'; an empty first field means 0, an empty
 * last field means that the last class is open-ended; at least one class must result ("0:1:" gives [0,1) and [1,inf), "5" alone is an
 * error).  cuts: COV_DEPTH_MAX_CUTS entries.  covh_depth_thresholds_parse reads a --thresholds list: decimal non-negative integers
 * separated by ','.  Both apply the cut list's rules (1 .. 16 values in 0 .. 2^31 - 1, strictly ascending); COV_ERR_INVALID_ARG with the
 * reason in covh_last_error.  Neither needs a device.
 * The classes a quantised track prints: [cuts[i-1], cuts[i]) for i = 1 .. n-1 with the label "lo:hi", and [cuts[n-1], inf) with the label
 * "lo:inf" when the spec is open-ended.  Class 0 (below the first cut) is never printed, and neither is class n of a closed spec.  A line is
 *   name \t start \t end \t label \n      end = the start of the target's next run, printed or not, or the target's length.
 * covh_depth_class_runs_format needs no device, works in ordered pieces like covh_depth_runs_format and gives the same text for every
 * thread count; covh_depth_class_runs_write walks a finished session chunk by chunk through page-locked memory.
 * The threshold counts print one line per region,
 *   chrom \t start \t end [\t name] \t c_1 .. \t c_K \n      c_j = the region's bases with depth >= threshold j,
 * in the file's order (covh_depth_regions_counts_format: results[] as for covh_depth_regions_format, used by no_zeros, which drops the
 * regions whose max is 0; counts: n x n_thr, row-major), or one line per window of bin_size bases, name \t start \t end \t c_1 .. c_K, in
 * target order, then position order (covh_depth_bins_counts_format: bin_off as for covh_depth_bins_format).  The two _write functions set
 * the thresholds on the session (cov_depth_thresholds_set), go the regions' way (the windows are tiled into regions on the host; 2^32
 * windows or more are refused with cov_depth_regions_set's message) and clear the thresholds again. */
int covh_depth_quantize_parse(const char *spec, int32_t *cuts, uint32_t *n_cuts, int *open_end);
int covh_depth_thresholds_parse(const char *list, int32_t *thr, uint32_t *n_thr);
int covh_depth_class_runs_format(const covh_header *h, uint32_t tid_lo, uint32_t n_targets, const uint64_t *run_off, const cov_depth_run *runs,
                                 const int32_t *cuts, uint32_t n_cuts, int open_end, int threads, int out_fd);
int covh_depth_class_runs_write(cov_session *s, const covh_header *h, const int32_t *cuts, uint32_t n_cuts, int open_end, int threads, int out_fd,
                                uint64_t *n_runs_out);
int covh_depth_regions_counts_format(const covh_bed *b, const cov_depth_bin *results, const uint32_t *counts, uint32_t n_thr, int no_zeros,
                                     int threads, int out_fd);
int covh_depth_regions_counts_write(cov_session *s, const covh_header *h, const covh_bed *b, const int32_t *thr, uint32_t n_thr, int no_zeros,
                                    int threads, int out_fd, uint64_t *n_regions_out);
int covh_depth_bins_counts_format(const covh_header *h, uint32_t tid_lo, uint32_t n_targets, uint32_t bin_size, const uint64_t *bin_off,
                                  const cov_depth_bin *bins, const uint32_t *counts, uint32_t n_thr, int no_zeros, int threads, int out_fd);
int covh_depth_bins_counts_write(cov_session *s, const covh_header *h, uint32_t bin_size, const int32_t *thr, uint32_t n_thr, int no_zeros,
                                 int threads, int out_fd, uint64_t *n_bins_out);

/* ---- genomes defined by FASTA files (`coverm genome -f / -d -x / --genome-fasta-list`; src/genome_parsing.rs:10-70,
 * src/genomes_and_contigs.rs:25-40).  Host code only: nothing here touches the GPU.
 * covh_genome_fasta_paths resolves a directory (directory != NULL: regular files, symlinks followed, whose name ends in
 * "." + extension; NULL or "fna" by default, one leading '.' accepted; sorted bytewise) or a list file (list_file != NULL: one
 * path per line, a trailing '\r' stripped, blank lines skipped).  NULL with a message when nothing is found. */
typedef struct covh_path_list covh_path_list;
covh_path_list *covh_genome_fasta_paths(const char *directory, const char *extension, const char *list_file, char *err, size_t errcap);
size_t covh_path_list_count(const covh_path_list *l);
const char *covh_path_list_get(const covh_path_list *l, size_t i);
void covh_path_list_free(covh_path_list *l);
/* One genome per file, in the order given, named by the file stem of the path once its last ".gz" (else ".bz", else ".xz")
 * and what follows are cut off; its contigs are the files' record ids, cut at the first space unless use_full_contig_names.
 * Plain text or gzip (by magic bytes); files are read on up to `threads` threads, with the same result for any count.
 * NULL with the first error a one-file-at-a-time read meets: unreadable, empty or unsupported file, not FASTA, a genome
 * name from two files, a contig in two records. */
typedef struct covh_genome_set covh_genome_set;
covh_genome_set *covh_genome_set_from_fasta(const char *const *paths, size_t n, int use_full_contig_names, int threads, char *err,
                                            size_t errcap);
size_t covh_genome_set_n_genomes(const covh_genome_set *s);
const char *covh_genome_set_genome_name(const covh_genome_set *s, size_t genome);
size_t covh_genome_set_n_contigs(const covh_genome_set *s);
/* contig i in file order: its name and the index of its genome */
void covh_genome_set_contig(const covh_genome_set *s, size_t i, const char **name, int32_t *genome);
/* genome index of a contig name of `len` bytes; -1 = in no genome */
int32_t covh_genome_set_genome_of(const covh_genome_set *s, const char *contig, size_t len);
/* out[tid] = genome index of each target of h (-1 = in no genome); returns how many targets are in a genome */
size_t covh_genome_set_genome_of_tid(const covh_genome_set *s, const covh_header *h, int32_t *out);
void covh_genome_set_free(covh_genome_set *s);

/* ---- the orchestrator of `coverm contig|genome --bam-files ...` (src/bin/coverm.rs:1315-1704, 2088-2131, 1539-1628): argv as the
 * coverm-amd binary takes it (argv[1] = "contig" | "genome", the reference's flag names, plus --device N / --devices a,b,...
 * and --no-stream).  Writes the table to --output-file or stdout; returns the process exit code (1 after printing an error). */
int covh_cli_main(int argc, char **argv);
/* For a process that exits right after covh_cli_main (the coverm-amd binary): leave the sessions to the OS instead of
 * destroying them one allocation at a time. */
void covh_cli_set_fast_exit(int on);

/* ---- trait MosdepthGenomeCoverageEstimator (estimators.rs:245-265), one export per method, for hosts that keep the reference's
 * scan-loop shape (a Rust `impl MosdepthGenomeCoverageEstimator` forwards 1:1).  add_contig takes the contig's
 * integer statistics from cov_finish where the reference passes the delta array.  `hist` is copied by the call (the bins of this
 * contig only): a binding may hand in a temporary buffer, as the reference's add_contig borrows its slice for the call alone. */
typedef struct covh_estimator_state covh_estimator_state;
covh_estimator_state *covh_estimator_new(const covh_estimator *params);                 /* CoverageEstimator::new_estimator_* */
void covh_estimator_free(covh_estimator_state *s);
void covh_estimator_setup(covh_estimator_state *s);                                     /* fn setup(&mut self) */
void covh_estimator_add_contig_stats(covh_estimator_state *s, const cov_contig_stats *stats, uint64_t target_len,
                                     const uint64_t *hist /* cov_fetch_hist array or NULL */, uint64_t num_mapped_reads,
                                     double sum_identity);                              /* fn add_contig(&mut self, ...) */
float covh_estimator_calculate_coverage(covh_estimator_state *s, const uint64_t *unobserved_contig_lengths, size_t n);
void covh_estimator_print_coverage(const covh_estimator_state *s, float coverage, covh_taker *t);
void covh_estimator_print_zero_coverage(const covh_estimator_state *s, covh_taker *t, uint64_t entry_length);
covh_estimator_state *covh_estimator_copy(const covh_estimator_state *s);               /* fn copy(&self) */
uint64_t covh_estimator_num_mapped_reads(const covh_estimator_state *s);

/* calculate_coverage for one entry built from explicit sums (used by unit tests). */
typedef struct {
    uint64_t win_len, win_sum_d, win_sum_d2, win_covered, full_len, full_covered, n_reads, mismatches;
    uint32_t win_min_d;
    uint32_t hist_len;
    const uint64_t *hist;
    double sum_identity;
} covh_entry;
float covh_calculate_coverage(const covh_estimator *e, const covh_entry *entry, const uint64_t *unobserved,
                              size_t n_unobserved);

#ifdef __cplusplus
}
#endif
#endif

/*
 * covermhip.h — C ABI of the MI355X-native coverage engine (libcovermhip.so).
 *
 * This is the drop-in boundary for CoverM's BAM -> pileup -> per-contig hot path.  The reference
 * (wwood/CoverM v0.8.0) has no FFI of its own; the seam is the body of its three scan loops
 *   contig_coverage                               src/contig.rs:13-253
 *   mosdepth_genome_coverage_with_contig_names    src/genome.rs:17-322
 *   mosdepth_genome_coverage                      src/genome.rs:419-797
 * and of `CoverageEstimator::add_contig` (src/mosdepth_genome_coverage_estimators.rs:366-528).
 * A host (Rust via `extern "C"`, C++, Python/ctypes) keeps decoding BAM on the CPU and keeps
 * `calculate_coverage` / `CoverageTaker` untouched; it streams packed record batches through this
 * ABI and receives, per contig, the exact integer sufficient statistics from which every
 * estimator's f32 is finalised (INTEGRATION.md shows the Rust binding).
 *
 * Plain C, POD only, caller-owned buffers.  Every function returns a cov_status; on failure
 * cov_last_error() describes it.  A session is bound to one HIP device and one sample (BAM); it is
 * not thread-safe (single producer), and owns its own HIP stream.
 */
#ifndef COVERMHIP_H
#define COVERMHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define COVERMHIP_ABI_VERSION 1

typedef struct cov_session cov_session;

/* Status codes.  The UNSORTED / NM_* / POS_OOB codes map 1:1 onto the reference's panics. */
typedef enum {
    COV_OK = 0,
    COV_ERR_UNSORTED = 1,   /* contig.rs:129-132, genome.rs:133-136, 549-552 */
    COV_ERR_NM_MISSING = 2, /* lib.rs:149-156 */
    COV_ERR_NM_BADTYPE = 3, /* lib.rs:144-147 */
    COV_ERR_POS_OOB = 4,    /* index panic at contig.rs:178 (M/=/X run starting at or past contig end) */
    COV_ERR_BAD_CIGAR = 6,  /* CIGAR op code > 8 */
    COV_ERR_BAD_TID = 7,    /* considered record whose tid is outside the header ("Corrupt BAM file?", contig.rs:145) */
    COV_ERR_INVALID_ARG = 16,
    COV_ERR_HIP = 17,       /* HIP runtime failure or no usable device: the engine never falls back to the CPU */
    COV_ERR_STATE = 18,
    COV_ERR_INGEST_FALLBACK = 19 /* cov_ingest_end: the file needs the CPU reader (see cov_last_error); nothing was appended */
} cov_status;

/* nm_kind values: how the record's NM aux tag was encoded (lib.rs:138-158). */
#define COV_NM_ABSENT 0
#define COV_NM_UNSIGNED 1 /* BAM type C, S or I */
#define COV_NM_BADTYPE 2  /* any other type: the reference panics */

/* cov_config.want bits */
#define COV_WANT_HIST 1u     /* per-contig depth histogram (trimmed_mean, coverage_histogram) */
#define COV_WANT_IDENTITY 2u /* ordered f64 identity sums (anir) */
/* with COV_WANT_IDENTITY: compute only one of the two sums (the other comes back 0).  contig_coverage and the
 * separator / single-genome scan use the primary-read sum (contig.rs:208, genome.rs:724), the contig-names genome scan
 * the not-supplementary one (genome.rs:220). */
#define COV_WANT_IDENTITY_PRIMARY_ONLY 4u
#define COV_WANT_IDENTITY_NONSUPP_ONLY 8u
/* A device ingest will follow (cov_ingest_begin): its streams, events and fixed tables — ~50 ms of runtime calls — are created by a helper thread
 * from cov_create on, beside the caller's next steps, instead of inside cov_ingest_begin.  Nothing else changes. */
#define COV_WANT_INGEST 16u

typedef struct {
    int32_t device; /* HIP device ordinal */
    /* FlagFilter, lib.rs:60-79 (CLI defaults: improper in, supplementary in, secondary out; coverm.rs:1661-1665) */
    uint8_t include_improper_pairs;
    uint8_t include_supplementary;
    uint8_t include_secondary;
    /* Single-read alignment thresholds = the stateless branch of ReferenceSortedBamFilter::read
     * (filter.rs:88-116, 243-279).  filter_single = 1 iff that branch is the active reader
     * (filtering_single && !filtering_pairs, filter.rs:48-61). */
    uint8_t filter_single;
    uint8_t min_mapq; /* 255 = no MAPQ test (filter.rs:13) */
    uint8_t reserved0[3];
    uint32_t min_aligned_length;
    float min_percent_identity; /* fraction in [0,1] */
    float min_aligned_percent;  /* fraction in [0,1] */
    /* --contig-end-exclusion: window [excl, L-excl) for the mean / trimmed_mean / variance /
     * histogram family (estimators.rs:386-398, 436-449). */
    uint64_t contig_end_exclusion;
    uint32_t want; /* COV_WANT_* */
    uint32_t reserved1;
} cov_config;

/*
 * One batch of BAM records in file order, struct-of-arrays.  Field provenance (rust-htslib accessors
 * used by the reference): tid/pos contig.rs:124,166; flag lib.rs:67-78; mapq filter.rs:251; NM
 * lib.rs:138-158; l_seq = record.seq().len() filter.rs:277; cigar contig.rs:168.
 * cigar words are raw BAM: len << 4 | op, op order MIDNSHP=X.  cigar_off has n_records + 1 entries
 * indexing `cigar` (cigar_off[0] may be non-zero; n_cigar = cigar_off[n] - cigar_off[0]).
 */
typedef struct {
    const int32_t *tid;
    const int32_t *pos;
    const uint16_t *flag;
    const uint8_t *mapq;
    const uint32_t *nm;
    const uint8_t *nm_kind;
    const uint32_t *l_seq;
    const uint32_t *cigar_off;
    const uint32_t *cigar;
    uint64_t n_records;
} cov_batch;

/*
 * Per-contig result.  "considered" = record survives the reader stage (filter_single), passes
 * FlagFilter and is mapped — i.e. reaches the CIGAR walk of the scan loops.  Depth statistics are
 * over per-base depth d[p] = prefix sum of the +1/-1 events of every M/=/X run (contig.rs:171-186):
 *   window  = [excl, L-excl) if 2*excl < L, else empty           (estimators.rs:386-398)
 *   full    = [0, L)                                              (estimators.rs:492-501)
 */
typedef struct {
    uint64_t n_primary;  /* considered && !secondary && !supplementary        contig.rs:157-159 */
    uint64_t n_pass;     /* considered                                         genome.rs:173-174 */
    uint64_t n_nonsupp;  /* considered && !supplementary                       genome.rs:677-682 */
    uint64_t sum_nm;     /* sum of NM over considered records                  contig.rs:207 */
    uint64_t sum_indel;  /* sum of I and D lengths                             contig.rs:189,197 */
    double sum_identity_primary; /* in file order; contig.rs:208-211, genome.rs:724-727 (COV_WANT_IDENTITY) */
    double sum_identity_nonsupp; /* in file order; genome.rs:220-223                      (COV_WANT_IDENTITY) */
    uint64_t win_sum_d;   /* sum of d over window (wrapping u64) */
    uint64_t win_sum_d2;  /* sum of d*d over window (wrapping u64) */
    uint64_t win_covered; /* #{p in window : d > 0} */
    uint64_t full_covered; /* #{p in [0,L) : d > 0} */
    uint64_t first_record; /* file-order index of the first / last considered record of this contig */
    uint64_t last_record;  /*   (sortedness is judged from these, see cov_finish) */
    uint32_t win_min_d;    /* min / max depth over the window (0 / 0 when the window is empty) */
    uint32_t win_max_d;
    uint32_t hist_len;     /* COV_WANT_HIST: win_max_d + 1 bins at hist[hist_off ..], else 0 */
    uint32_t reserved;
    uint64_t hist_off;
} cov_contig_stats;

typedef struct {
    uint64_t num_detected_primary_alignments; /* every record pushed with !secondary && !supplementary
                                                 (bam_generator.rs:114-118, filter.rs:94-96) */
    uint64_t n_records;
    uint64_t n_considered;
    uint64_t hist_total; /* number of u64 bins cov_fetch_hist() will write */
} cov_summary;

/* Named kernels of the device pipeline, for cov_kernel_ms(). */
typedef enum {
    COV_K_PREP = 0,     /* filter + CIGAR summary + per-contig record counters */
    COV_K_RANGES = 1,   /* tile -> candidate record range */
    COV_K_PILEUP = 2,   /* LDS-tiled events + scan + statistics (the dominant kernel) */
    COV_K_IDENTITY = 3, /* ordered f64 identity sums */
    COV_K_HIST = 4,     /* histogram arena layout + zero fill (before the pileup) */
    COV_K_HIST_COMPACT = 5, /* compact histogram (behind the pileup) */
    COV_K_ESTIMATE = 6, /* CoverageEstimator::calculate_coverage of every contig (cov_set_estimators) */
    COV_K_GENOME = 7,   /* cov_set_genomes: contigs reduced into genomes, histograms merged, calculate_coverage of every genome */
    COV_K_GROUP = 8,    /* cov_group_records: order check, sort passes and gather of the last call, summed (not part of a finish) */
    COV_K_SAM = 9,      /* cov_sam_*: the decode kernels of the last SAM text ingest, summed over its windows (not part of a finish) */
    COV_K_SEP = 10,     /* cov_set_genome_runs: the table entry -> targets of the finish (scans, compaction, segments), in front of COV_K_GENOME */
    COV_K_GENE_READS = 11, /* cov_interval_reads_compute: the kernels of the last call, summed (not part of a finish) */
    COV_K_DEPTH_RUNS = 12, /* cov_depth_runs_compute: the run kernels of the last chunk (marks, the two scans, emit), summed (not part of a finish) */
    COV_K_DEPTH_BINS = 13, /* cov_depth_bins_compute: the bin kernels of the last chunk (marks, the rank scan, init, reduce), summed (not part of a finish) */
    COV_K_DEPTH_REGIONS = 14, /* cov_depth_regions_compute: the region kernels of the last chunk (marks, the rank scan, init, reduce), summed (not part of a finish) */
    COV_K_COUNT = 15
} cov_kernel_id;

/* --- lifecycle ------------------------------------------------------------------------------- */
int cov_abi_version(void);
/* Creates a session on cfg->device.  Fails with COV_ERR_HIP (never falls back) if no GPU. */
cov_status cov_create(const cov_config *cfg, cov_session **out);
void cov_destroy(cov_session *s);
const char *cov_last_error(const cov_session *s); /* s may be NULL for cov_create failures */

/* BAM header: n reference sequences and their lengths (HeaderView::target_len, contig.rs:145). */
cov_status cov_set_targets(cov_session *s, uint32_t n_targets, const uint64_t *target_len);

/* Optional: mask[t] == 0 removes target t from the CIGAR walk, the NM requirement and the depth
 * statistics while its records still take part in the sortedness check — exactly what
 * mosdepth_genome_coverage_with_contig_names does for contigs outside every genome
 * (genome.rs:170-171).  NULL (default) = every target participates. */
cov_status cov_set_target_mask(cov_session *s, const uint8_t *mask);

/* Appends a batch of records held in HOST memory (copied to the device on the session stream).  The arrays may
 * be changed or freed as soon as the call returns.  Arrays in page-locked memory (cov_host_alloc, hipHostMalloc)
 * move by DMA at link rate without the runtime's per-call pinning of pageable pages. */
cov_status cov_push_batch(cov_session *s, const cov_batch *host_batch);
/* Appends a batch whose arrays already live in DEVICE memory (no copy; the caller keeps them
 * alive and unmodified until cov_finish returns).  Used when ingest writes straight to HBM. */
cov_status cov_push_batch_device(cov_session *s, const cov_batch *device_batch);

/*
 * Runs the device pipeline over everything pushed and writes one cov_contig_stats per target into
 * `stats` (n_targets entries, caller-owned).  Returns COV_ERR_UNSORTED / COV_ERR_NM_* /
 * COV_ERR_POS_OOB exactly when the reference's scan would have panicked.  The session keeps its
 * records, so cov_finish may be called again (e.g. for benchmarking) and cov_copy_depth works
 * afterwards; cov_reset drops the records.
 */
cov_status cov_finish(cov_session *s, cov_contig_stats *stats, cov_summary *summary);
/* After cov_finish with COV_WANT_HIST: concatenated histograms, hist[stats[t].hist_off + d] =
 * #{p in window of contig t : depth == d}, summary.hist_total entries. */
cov_status cov_fetch_hist(cov_session *s, uint64_t *hist);
/* Bit-exact per-base depth of one contig (target_len[tid] entries), for parity checks. */
cov_status cov_copy_depth(cov_session *s, uint32_t tid, int32_t *depth_out);
cov_status cov_reset(cov_session *s);
/* Optional: size the record store for n_records / n_cigar up front (a streamed ingest that knows roughly what is coming
 * avoids regrowing the HBM arrays while it pushes). */
cov_status cov_reserve(cov_session *s, uint64_t n_records, uint64_t n_cigar);

/*
 * Device ingest (optional accelerator for hosts with few cores): the BGZF-compressed BAM goes to HBM as it is; the GPU inflates
 * every block (one lane per block, RFC 1951 decoder with LDS tables), checks its CRC-32, finds the record boundaries
 * (speculative per segment, verified to equal the serial hop) and writes the records straight into the session's record store —
 * the same store cov_push_batch appends to, so cov_finish does not care where the records came from.  The inflated stream
 * exists only one window at a time (the blocks one inflate launch holds, ~3 GB; a record cut by a window's end is carried
 * into the next), so device memory stays bounded whatever the file size.  The host only reads the
 * file into page-locked buffers, hops the 18-byte BGZF block headers and parses the BAM header (reference names / lengths,
 * offset of the first record in the inflated stream).
 *   cov_set_targets(s, ...)                         reference lengths: the record-boundary test uses them
 *   cov_ingest_begin(s, file_bytes, first_record_offset, check_crc)       first_record_offset: in the inflated stream, behind the BAM header
 *   loop: cov_ingest_slot_wait(s, slot) -> fill the slot's buffer -> cov_ingest_feed(s, slot, buf, file_offset, n, blocks, n_blocks)
 *         (COV_INGEST_SLOTS staging buffers rotate; slot_wait may be called from a reader thread while another thread feeds;
 *          `blocks` = the BGZF blocks COMPLETED by this piece: offsets are absolute in the file / the inflated stream; the
 *          copy is asynchronous, the inflate kernels of these blocks run behind it)
 *   cov_ingest_end(s, &n_records)
 * Anything irregular (inflate or CRC failure, boundaries that do not verify, a CG:B,I long-CIGAR placeholder) makes
 * cov_ingest_end return COV_ERR_INGEST_FALLBACK with nothing appended: decode that file on the host and cov_push_batch it.
 */
#define COV_INGEST_SLOTS 4
typedef struct {
    uint64_t in_off;  /* first byte of the block's raw DEFLATE data, offset in the file */
    uint64_t out_off; /* offset of its inflated bytes in the inflated stream (running sum of ISIZE) */
    uint32_t in_len, isize, crc, pad;
} cov_bgzf_block;
cov_status cov_ingest_begin(cov_session *s, uint64_t compressed_bytes, uint64_t first_record_offset, int check_crc);
/* Optional, between cov_ingest_begin and the first feed — one rank of a span-sharded file: only records with key_lo <= key < key_hi
 * are taken (key = tid; 0x7fffffff for records without a reference, which sort last); search_first_record: the bytes fed start
 * at a BGZF block somewhere inside the file (first_record_offset is then 0 and the first record boundary is searched);
 * open_end: the bytes fed end before the file does, so a record cut by their end is expected — it must lie beyond key_hi,
 * else COV_ERR_INGEST_FALLBACK; [file_lo, file_hi) = the file bytes that will be fed (sizes the record store once). */
cov_status cov_ingest_span(cov_session *s, int64_t key_lo, int64_t key_hi, int search_first_record, int open_end, uint64_t file_lo, uint64_t file_hi);
cov_status cov_ingest_slot_wait(cov_session *s, int slot);
cov_status cov_ingest_feed(cov_session *s, int slot, const void *host_bytes, uint64_t file_offset, uint64_t n_bytes,
                           const cov_bgzf_block *blocks, uint32_t n_blocks);
cov_status cov_ingest_end(cov_session *s, uint64_t *n_records);
/* What the last cov_ingest_end's ingest did (also when it handed the file back): how well the record search cut the stream in pieces. */
typedef struct {
    uint64_t windows, segments, segments_with_start, records,
             max_hop_records,   /* most records any one lane hopped over in k_bam_hop, over all windows */
             long_records,      /* records that went through k_bam_extract_long */
             repaired_starts;   /* starts dropped by the repair */
} cov_ingest_stats;
cov_status cov_ingest_last_stats(const cov_session *s, cov_ingest_stats *out);  /* of the last cov_ingest_end */
/* Gives up an ingest that was begun but cannot be ended (a malformed block header met by the driver, a read error): waits for
 * everything queued on the device, appends nothing, leaves the session ready for cov_push_batch.  cov_reset and cov_push_batch
 * call it themselves when an ingest is still open. */
cov_status cov_ingest_abort(cov_session *s);
cov_status cov_ingest_release(cov_session *s); /* frees the compressed / inflated buffers (kept between files otherwise) */
cov_status cov_ingest_copy_inflated(cov_session *s, uint64_t offset, uint64_t n, void *out); /* test hook; single-window files only */
/*
 * SAM text ingest: what a mapper writes to its standard output (`bwa mem`, `minimap2 -a`), decoded on the device window by window into the
 * same record store, from a file or from a pipe.  The host only reads bytes into page-locked slots and keeps lines whole; the device finds
 * the lines and the tabs (one coalesced pass: a 64-bit mask of each per 64 bytes), numbers the lines by a scan, and decodes a line per lane
 * (csrc/sam_parse_core.h is the arithmetic, field for field what the host's SAM reader produces).
 *   cov_set_targets(s, ...)                         reference lengths, from the @SQ lines
 *   cov_sam_begin(s, names_blob, name_off, n_names, expected_bytes)
 *         reference name i = names_blob[name_off[i] .. name_off[i + 1])  (n_names + 1 offsets): RNAME / RNEXT -> tid through a hash table built
 *         here, a hit confirmed by comparing the bytes; a duplicate name resolves to its first occurrence, an unknown one to -1.
 *         expected_bytes: the text's size when known (sizes the record store once), 0 for a pipe (the store grows as records arrive).
 *   loop: cov_sam_slot_wait(s, slot) -> fill the slot's buffer -> cov_sam_feed(s, slot, buf, n)
 *         every piece holds WHOLE lines (cut it at its last '\n' and carry the rest into the next piece), at most cov_sam_window_bytes(s)
 *         bytes (32 MiB; COVERM_KNOBS sam_window_bytes); only the last piece may end without '\n' — that last line is a record.  Header
 *         lines (@) in front of the first alignment line and empty lines are skipped, so the text may be fed from its first byte and line
 *         numbers in errors are the file's.  The upload is asynchronous (slot_wait tells when the buffer may be written again); the call
 *         waits for this window's line and record counts and leaves its decode running beside the next upload.
 *   cov_sam_end(s, &n_records)
 * Device memory is two windows of text, their masks and per-line words, whatever the input's length.  cov_ingest_want_mates and
 * cov_ingest_want_grouping apply as to the BGZF ingest (the name hash is the same function), the bounded record store spills as for
 * cov_push_batch, and cov_ingest_abort gives an open SAM ingest up.  Errors are decided on the device for the first offending line in
 * file order, 1-based line number in cov_last_error: COV_ERR_INVALID_ARG "malformed SAM line" (fewer than 11 fields), a CIGAR of more than
 * 65535 operations, a line longer than the window; COV_ERR_INGEST_FALLBACK for a header line behind the first alignment line (decode that
 * file on the host).  After an error nothing was appended and the session is ready for cov_push_batch.  COV_ERR_STATE: cov_sam_feed /
 * cov_sam_end without cov_sam_begin, cov_sam_begin (or cov_ingest_begin) while an ingest is open.
 */
cov_status cov_sam_begin(cov_session *s, const char *names_blob, const uint64_t *name_off, uint32_t n_names, uint64_t expected_bytes);
uint64_t cov_sam_window_bytes(const cov_session *s);
cov_status cov_sam_slot_wait(cov_session *s, int slot);
cov_status cov_sam_feed(cov_session *s, int slot, const void *host_bytes, uint64_t n_bytes);
cov_status cov_sam_end(cov_session *s, uint64_t *n_records);
/* ---- reader-stage PAIR filter on the device: ReferenceSortedBamFilter::read, pair branch (src/filter.rs:117-228, filter_out = true) +
 * read_pair_passes_filter (:281-336) over the records the device ingest put into the session's store.
 *   cov_ingest_want_mates(s, 1)      before cov_ingest_begin: the extraction also keeps next_refID and a 96-bit hash of each read name
 *   ... ingest one or more files ...
 *   cov_pair_filter_apply(s, &f, &n_selected, &n_primary)
 * replaces the store by the records the reference's filter would return, in its order (pairs by their second record; first record,
 * then second); *n_primary = num_detected_primary_alignments (filter.rs:129-131: every primary record of the input).  cov_finish then
 * runs with cov_config.filter_single = 0.  COV_ERR_NM_MISSING / COV_ERR_NM_BADTYPE where the reference's nm() would have panicked;
 * COV_ERR_INGEST_FALLBACK (store untouched) when more than 2^20 records carry a read name that occurs more than twice among the
 * primary proper-pair records of one reference (fewer are replayed exactly): run the host filter (covh_pair_mode_order) on the CPU
 * reader's records then.  (Tests lower the 2^20 with the knob pair_multi_cap, csrc/knobs.h.)  Same layout as covh_pair_filter. */
typedef struct {
    int32_t filter_single;     /* single-read thresholds apply to both mates as well (filter.rs:48-55) */
    uint8_t min_mapq;          /* 255 = off */
    uint8_t pad[3];
    uint32_t min_aligned_length_single;
    float min_percent_identity_single, min_aligned_percent_single;
    uint32_t min_aligned_length_pair;
    float min_percent_identity_pair, min_aligned_percent_pair;
} cov_pair_filter;
cov_status cov_ingest_want_mates(cov_session *s, int on);
cov_status cov_pair_filter_apply(cov_session *s, const cov_pair_filter *f, uint64_t *n_selected, uint64_t *n_primary);
/* ---- records grouped by reference on the device, for a BAM / SAM that is not sorted by reference (a mapper's output in read order).
 * The pipeline needs the records of one reference to be contiguous, not sorted by position; one stable sort of the record indices by tid
 * and one gather of the store do that in milliseconds where `samtools sort` takes minutes.
 * Between the last push / cov_ingest_end and cov_pair_filter_apply / cov_finish / cov_finish_genomes / cov_copy_records:
 * makes the records of every reference contiguous, references in ascending tid order, records without a reference last,
 * the file's order kept inside a reference (stable).  *n_moved = records whose index changed (0: the store was grouped
 * already and was not touched).  Every result afterwards is the result for the file whose records are the input's records in that
 * order; per-record errors are reported for the first offending record of that order.
 * COV_ERR_STATE: an adopted device batch (cov_push_batch_device), a tid span (cov_ingest_span with anything but the whole key range),
 * after a spill of the bounded record store (a sample that is not sorted by reference must fit the store: the spill has already judged
 * the order).  Needs room for a second copy of the store while it runs.
 * cov_ingest_want_grouping(s, 1) before cov_ingest_begin announces it: a file whose keys decrease is then not handed back to the CPU
 * reader for the pair filter's sake (cov_ingest_want_mates); span ingests keep refusing such a file. */
cov_status cov_ingest_want_grouping(cov_session *s, int on);
cov_status cov_group_records(cov_session *s, uint64_t *n_moved);
/* Test hook: the session's own record store copied back into caller-sized host arrays (host == NULL: only the counts). */
cov_status cov_copy_records(cov_session *s, const cov_batch *host, uint64_t *n_records, uint64_t *n_cigar);
/* Test hook: what an ingest with cov_ingest_want_mates kept beside the records — the mate's reference and the 96-bit read-name hash
 * (csrc/name_hash_core.h), n_records entries each.  COV_ERR_STATE without want_mates. */
cov_status cov_copy_mates(cov_session *s, int32_t *mtid, uint64_t *qh1, uint32_t *qh2);
/* Test hook, the counterpart of cov_copy_mates: overwrites the three mate columns of a store that already has them (n_records entries
 * each, host arrays), before cov_pair_filter_apply.  The filter then joins records by the keys given here: two records with equal
 * (qh1 with 0 read as 1, qh2) on one reference are one read name to it, whatever their names were, which is how tests reach key
 * collisions that no pair of names produces.  COV_ERR_STATE as cov_copy_mates, and when the columns do not cover the whole store. */
cov_status cov_set_mates(cov_session *s, const int32_t *mtid, const uint64_t *qh1, const uint32_t *qh2);

/* Multi-GPU, one process: after cov_finish on every session (one per device, same targets), ONE RCCL gather moves each
 * rank's per-contig result block (fixed size: 160 B per contig + counters) to the device of sessions[root] over xGMI and
 * from there to the host in one DMA; cov_gathered then decodes rank r's block exactly as cov_finish decodes its own
 * (same error reporting).  librccl is bound at run time; COV_ERR_HIP if it is missing.  A device listed more than once
 * (functional checks on a single-GPU box) is served by plain device copies, since RCCL refuses two ranks on one device. */
cov_status cov_gather(cov_session *const *sessions, uint32_t n, uint32_t root);
cov_status cov_gathered(cov_session *root_session, uint32_t rank, cov_contig_stats *stats, cov_summary *summary);

/* Average duration (ms) of one launch of kernel `k` during the last cov_finish, measured with HIP
 * events recorded on the session's stream around that kernel; *launches receives the count. */
cov_status cov_kernel_ms(const cov_session *s, cov_kernel_id k, double *ms_total, uint32_t *launches);
/* Which paths the last cov_finish took — diagnostics, so that a parity case built for one branch of the device pipeline can assert that the
 * branch ran (tests/test_gpu_step_shapes.py).  listed_steps: steps of 64 records k_prep_lean left to k_prep_generic (generic_only = 1: a
 * sample of fewer than 128 records per contig, k_prep_generic walked all of them and nothing was listed); slow_tiles: tiles k_pileup_fast
 * left to k_pileup_stream; bucket_records: records whose CIGAR went through the bucket list (more than CX_MIN_OPS operations);
 * bucket_entries: the (operation, tile) pairs those records expanded to (saturated at 2^32 - 1); passes: how often the finish ran the
 * pipeline over the store (2: the bucket buffer was too small for bucket_entries, it was grown and the pass repeated). */
typedef struct { uint32_t listed_steps, generic_only, slow_tiles, bucket_records, bucket_entries, passes; } cov_path_counts;
cov_status cov_last_paths(const cov_session *s, cov_path_counts *out);
/* How the last cov_finish handed k_pileup_fast's tiles to its waves (csrc/pileup_schedule_core.h): out[0] = tiles on the deep-tile list
 * (0: no list was used), out[1] = waves launched, out[2] = tiles per chunk, out[3] = the list's threshold in candidate runs
 * (COVERM_KNOBS pileup_deep_min; 0 = off). */
cov_status cov_pileup_schedule(const cov_session *s, uint32_t out[4]);
/* Test hook: the 8-byte run words k_prep left in the last cov_finish, one per record of the store in store order, as x | (uint64_t)y << 32
 * (x = start of the first merged M/=/X run, y = 0 or type << 30 | fields: SINGLE 0, DOUBLE 1 with len1 | gap << 10 | len2 << 18, COMPLEX 2,
 * BUCKET 3).  COV_ERR_STATE when the last finish did not leave run words for the whole store: no finish, no records, an adopted device
 * batch (cov_push_batch_device), or part of the sample already left the bounded record store. */
cov_status cov_copy_run_words(const cov_session *s, uint64_t *out);
/* Algorithmic HBM bytes of the last cov_finish (DESIGN.md "Algorithmic bytes"): record SoA + CIGAR
 * words read once, plus result structs written. */
cov_status cov_algorithmic_bytes(const cov_session *s, uint64_t *bytes);

/* ---- CoverageEstimator::calculate_coverage on the device (estimators.rs:530-839), for `coverm contig`: one entry per contig, unobserved
 * lengths [0] (contig.rs:62-66).  cov_set_estimators before cov_finish; cov_finish then also evaluates every estimator for every contig
 * (one wave per contig, the reference's float expressions in the reference's order, one rounding per operation) and
 * cov_fetch_estimates copies the n_targets x n_est floats out (row = contig, 0 for a contig without a considered record; RPKM before the
 * printer's normalisation, as calculate_coverage returns it).  The floats equal the host path's (coverm_host.h covh_contig_coverage over
 * cov_contig_stats) bit for bit; a host that takes them skips the per-contig finalisation and, unless it prints histograms, the
 * histogram fetch.  Kinds = enum CoverageEstimator's variant order (coverm_host.h covh_kind).  Not offered: COV_EST_TPM (f64 exp / ln of the
 * host's libm) and COV_EST_PILEUP_COUNTS (prints the histogram itself) — COV_ERR_INVALID_ARG, evaluate those on the host.  Needs
 * COV_WANT_HIST for a trimmed mean and COV_WANT_IDENTITY for ANIr.  With a target mask the entries are genomes, not contigs: cov_fetch_estimates
 * then returns COV_ERR_STATE, and the estimators are evaluated per genome when cov_set_genomes (below) gave the genomes' table. */
typedef struct {
    int32_t kind;                      /* COV_EST_* */
    float min_fraction_covered_bases;
    uint64_t contig_end_exclusion;     /* as the session's cov_config.contig_end_exclusion */
    int32_t exclude_mismatches;
    float trim_min, trim_max;
} cov_estimator;                       /* same layout as coverm_host.h's covh_estimator */
#define COV_EST_MEAN 0
#define COV_EST_TRIMMED_MEAN 1
#define COV_EST_PILEUP_COUNTS 2
#define COV_EST_COVERED_FRACTION 3
#define COV_EST_COVERED_BASES 4
#define COV_EST_RPKM 5
#define COV_EST_TPM 6
#define COV_EST_VARIANCE 7
#define COV_EST_LENGTH 8
#define COV_EST_READ_COUNT 9
#define COV_EST_READS_PER_BASE 10
#define COV_EST_ANIR 11
#define COV_EST_MAX 16
cov_status cov_set_estimators(cov_session *s, const cov_estimator *est, uint32_t n_est); /* n_est = 0: off (the default) */
cov_status cov_fetch_estimates(cov_session *s, float *out);                              /* after cov_finish: n_targets * n_est floats */

/* ---- the contig-names genome scan on the device (mosdepth_genome_coverage_with_contig_names, genome.rs:17-322): one entry per GENOME.
 * cov_set_genomes after cov_set_targets: genome_of_tid[t] = the genome of target t, -1 = outside every genome.  It implies the target mask
 * cov_set_target_mask(genome_of_tid[t] >= 0) would set (genome.rs:170-171) and keeps a table genome -> targets in ascending target order
 * on the device.  NULL or n_genomes = 0 turns it off (and drops the mask); cov_set_targets and cov_set_target_mask turn it off as well
 * (estimators holding a genome's ANIr are dropped with it: the per-contig evaluation has no identity sum for them — set them again).
 * With genomes set, cov_set_estimators is accepted together with the mask, and cov_finish also
 *   - reduces the per-contig results over each genome's targets: integer sums, min / max depth, the unobserved lengths of the targets
 *     without a considered record (estimators.rs:226-242), and the not-supplementary identity sum added target by target in ascending
 *     order (one ordered chain per genome: f64 addition is not associative, genome.rs:220-223);
 *   - merges the depth histograms of each genome's targets (COV_WANT_HIST);
 *   - evaluates every estimator for every genome with the expressions cov_fetch_estimates' floats come from, the reads counted as
 *     genome.rs:173-174 counts them (every considered record) — ANIr therefore needs the not-supplementary identity sum here.
 * cov_fetch_genome_estimates: n_genomes x n_est floats, bit for bit what coverm_host.h's covh_genome_coverage_with_contig_names computes
 * from cov_contig_stats and the histogram; cov_fetch_genome_stats: what the scan's control flow needs beside them (ReadsMapped, zero rows,
 * --no-zeros).  A host that takes both needs neither the per-contig statistics nor the histogram.  After a spill of the bounded record
 * store (below) the contigs that left are on the host: both fetches return COV_ERR_STATE, aggregate on the host then. */
typedef struct {
    uint64_t reads_in_genome;  /* sum of n_pass over the genome's targets (genome.rs:173-174) */
    uint64_t genome_len;       /* sum of the lengths of its targets */
    uint32_t n_contigs_seen;   /* targets with a considered record */
    uint32_t any_nonzero;      /* some estimator's value is > 0 */
} cov_genome_stats;
cov_status cov_set_genomes(cov_session *s, const int32_t *genome_of_tid, uint32_t n_genomes);
/* cov_finish for a host that takes the genome results only (genomes and estimators set): the same pipeline and the same verdicts —
 * COV_ERR_UNSORTED / COV_ERR_NM_* / COV_ERR_POS_OOB / ... exactly when cov_finish returns them, the order rule judged on the device — but no
 * cov_contig_stats array: the per-contig block (160 B per target) stays on the device and no pass over the targets runs on the host.
 * summary->hist_total is 0.  cov_fetch_genome_estimates / cov_fetch_genome_stats / cov_kernel_ms afterwards as after cov_finish; cov_fetch_hist
 * and cov_gather need a cov_finish.  COV_ERR_STATE without genomes or estimators, and after a spill of the bounded record store (cov_finish
 * then, and aggregate on the host). */
cov_status cov_finish_genomes(cov_session *s, cov_summary *summary);
cov_status cov_fetch_genome_estimates(cov_session *s, float *out);          /* after cov_finish: n_genomes * n_est floats */
cov_status cov_fetch_genome_stats(cov_session *s, cov_genome_stats *out);   /* after cov_finish: n_genomes entries */

/* ---- the separator / single-genome scan on the device (mosdepth_genome_coverage, genome.rs:419-929): one entry per run of observed
 * targets of one genome.  cov_set_genome_runs after cov_set_targets: gid_of_tid[t] >= 0 is the dense id of target t's genome (the part
 * of its name before the separator; all 0 for --single-genome), n_gids the number of ids.  It sets no mask.  NULL or n_gids = 0 turns it
 * off; so do cov_set_targets, cov_set_target_mask and cov_set_genomes — and cov_set_genome_runs turns cov_set_genomes (and its mask) off.
 * Which targets form an entry, and which targets without a considered record count as its unobserved lengths, depends on where the
 * sample's reads fall: with runs and estimators set, cov_finish / cov_finish_genomes build the table entry -> targets on the device
 * behind the per-contig pass (the rule: csrc/sep_entry_core.h), then reduce, merge and evaluate over it as for cov_set_genomes, with the
 * reads counted as genome.rs:677-682 counts them (considered and not supplementary) and ANIr over the primary-read identity sum
 * (genome.rs:724-727).  cov_fetch_estimates returns COV_ERR_STATE (the entries are genomes).
 * cov_genome_entry_count: entries of the last finish (0 when no target had a considered record).  cov_fetch_genome_entries: one
 * cov_genome_entry each, in the order the scan prints them; cov_fetch_genome_estimates: n_entries x n_est floats, bit for bit what
 * coverm_host.h's covh_genome_coverage_separator computes.  After a spill of the bounded record store all of them return COV_ERR_STATE. */
typedef struct {
    uint64_t reads;            /* sum of n_nonsupp over the entry's observed targets (genome.rs:677-682) */
    uint32_t first_tid;        /* first target of the run of the genome's names the entry starts in (start_entry's index) */
    int32_t gid;               /* gid_of_tid of its targets */
    uint32_t n_contigs_seen;   /* targets with a considered record */
    uint32_t any_nonzero;      /* some estimator's value is > 0 */
} cov_genome_entry;
cov_status cov_set_genome_runs(cov_session *s, const int32_t *gid_of_tid, uint32_t n_gids);
cov_status cov_genome_entry_count(cov_session *s, uint32_t *n_entries);
cov_status cov_fetch_genome_entries(cov_session *s, cov_genome_entry *out);

/* ---- bounded record store.  The reference holds one contig at a time and flushes it when the tid changes (contig.rs:128-155), so a
 * sample may be arbitrarily large.  The session's record store keeps as many contigs as fit under a cap (2^31 records / 2^31 CIGAR
 * words by default; COVERM_KNOBS="store_cap_records=N,store_cap_cigar=M", read by cov_create).  When cov_push_batch, cov_push_batch_device
 * or the device ingest would take it past the cap, the pipeline runs over what the store holds, the contigs that are complete stay on
 * the host, the records from the first considered record of the contig in flight onwards move to the front of the store and the call
 * goes on ("a spill"); cov_finish / cov_fetch_hist / cov_gather then return the whole sample (record indices count from the sample's first
 * record).  What remains: ONE reference's records must fit (2^32 - 16 records and CIGAR words); after a spill cov_copy_depth,
 * cov_interval_stats_compute, cov_interval_reads_compute, cov_depth_runs_compute, cov_depth_class_runs_compute, cov_depth_bins_compute, cov_depth_regions_compute, cov_copy_records and cov_pair_filter_apply return COV_ERR_STATE (they need every record) and a device ingest
 * that has to hand its file to the CPU reader fails with COV_ERR_STATE instead of COV_ERR_INGEST_FALLBACK; a store that carries mate
 * columns (cov_ingest_want_mates) or an adopted device batch is never spilled.  cov_store_spills: spills since the last cov_reset. */
uint32_t cov_store_spills(const cov_session *s);


/* ---- per-interval statistics (per-gene coverage, the reference's src/genes.rs:508-535).  After cov_finish: the depth of
 * every target is materialised once in HBM (4 B per base, kept until the next push / reset / finish) and each interval
 * [start, end) of target `tid` is reduced by one wave.  contig_end_exclusion applies to the INTERVAL's own ends: the
 * window is [start+excl, end-excl) when 2*excl < end-start, else empty; full_covered has no exclusion. */
typedef struct { uint32_t tid, pad; uint64_t start, end; } cov_interval;
typedef struct {
    uint64_t win_sum_d, win_sum_d2, win_covered, full_covered;
    uint32_t win_min_d, win_max_d; /* over the window; 0 when it is empty */
    uint32_t hist_len, pad;        /* window non-empty: win_max_d + 1 bins at hist[hist_off ..] (when want_hist), else 0 */
    uint64_t hist_off;
} cov_interval_stats;
cov_status cov_interval_stats_compute(cov_session *s, const cov_interval *intervals, uint64_t n, uint64_t contig_end_exclusion,
                                      int want_hist, cov_interval_stats *out, uint64_t *hist_total);
cov_status cov_fetch_interval_hist(cov_session *s, uint64_t *hist);

/* ---- per-interval read aggregates (per-gene coverage, the reference's src/genes.rs:206-304, 493-524): what the gene scan keeps per read
 * — num_mapped_reads, mismatches = NM.saturating_sub(I + D) and the identity of the reads whose leftmost position lies inside the interval
 * — computed from the session's own record store; 32 bytes per interval come back and no record.  Callable while the store holds the
 * sample, before or after cov_finish.  The records pass cov_config's filter as covh_gene_coverage applies it (the single-read reader stage
 * when filter_single, the flag filter, mapped, NM present); the target mask does not apply (the reference's gene scan has none).
 *   n_reads       primary records among them               mismatches    sum of NM.saturating_sub(I + D)
 *   sum_identity  P[hi] - P[lo], P the serial f64 running sum of the primary reads' (aligned - NM) / aligned from the first record of the
 *                 interval's target on (genes.rs:500-526; replayed in file order, bit for bit); 0 unless want_identity
 *   contig_taken  records of the interval's target that passed: 0 = the scan never saw that target
 * *mapped_total = the primary records that passed, over the whole store (ReadsMapped.num_mapped_reads).
 * *sorted_by_start = 0: some start decreases inside a target (a file grouped by reference but not sorted); `out` was NOT written — the
 * reference's partition_point over such starts depends on its probe sequence, run covh_gene_coverage over cov_copy_records then.
 * COV_ERR_NM_MISSING / COV_ERR_NM_BADTYPE / COV_ERR_UNSORTED / COV_ERR_BAD_TID for the first offending record in file order, as the host
 * scan reports them; COV_ERR_STATE after a spill of the bounded record store; COV_ERR_INVALID_ARG for an interval outside its target. */
typedef struct { uint64_t n_reads, mismatches; double sum_identity; uint64_t contig_taken; } cov_interval_reads; /* 32 B */
cov_status cov_interval_reads_compute(cov_session *s, const cov_interval *intervals, uint64_t n, int want_identity,
                                      cov_interval_reads *out, uint64_t *mapped_total, int *sorted_by_start);

/* ---- depth runs: the per-base depth the pileup computes (under cov_config's filters, the depth cov_copy_depth returns), run-length
 * encoded on the device, for a coverage track that integrates to the table.  A depth run of target t is a maximal stretch [start, end) of
 * equal depth inside t, stretches of depth 0 included: the runs of a target tile [0, L) exactly, never cross a target boundary (two
 * adjacent targets whose last and first depths are equal still give two runs), and a target with L == 0 has none.  A run's end is the next
 * run's start, or L for the target's last run.
 * The work goes a CHUNK of whole targets at a time, so that device and host memory are bounded by the chunk and not by the sample:
 *   cov_depth_runs_compute(s, tid_lo, tid_hi, &tid_next, &n_runs)
 *         materialises the depth of targets [tid_lo, tid_next) — as many whole targets from tid_lo on as fit a budget of 2^28 bases (4 B per
 *         base in HBM; COVERM_KNOBS depth_chunk_bases; every target takes a multiple of four bases and at least four; a single target above
 *         the budget is a chunk of its own), tid_lo < tid_next <= tid_hi <= n_targets — and encodes it: marks, two scans, emit
 *         (csrc/depth_kernels.hip.h).  The accumulated statistics stay as they are (the pileup runs against a scratch copy, as for
 *         cov_copy_depth).  The chunk's n_runs runs stay on the device until the next compute / push / reset / finish.
 *   cov_depth_runs_fetch(s, run_off, runs)
 *         run_off: tid_next - tid_lo + 1 entries, the runs of target tid_lo + k are runs[run_off[k] .. run_off[k + 1]) (an empty target
 *         repeats its neighbour's offset); runs: n_runs entries in target order, then position order (page-locked memory moves by DMA).
 *   loop with tid_lo = tid_next until tid_next == tid_hi.
 * Both are valid after cov_finish; COV_ERR_STATE before it, while an ingest is open, and after a spill of the bounded record store (the
 * depth needs every record); cov_depth_runs_fetch also without a computed chunk.  cov_kernel_ms(COV_K_DEPTH_RUNS) and
 * cov_depth_runs_last describe the last chunk. */
typedef struct { uint32_t start; int32_t depth; } cov_depth_run; /* 8 B */
typedef struct {
    uint64_t arena_bases; /* entries of the chunk's arena (padding included) */
    uint64_t n_runs;
    double arena_ms;      /* the pileup into the arena (with its zero fill), HIP-event time */
    double runs_ms;       /* the run kernels = cov_kernel_ms(COV_K_DEPTH_RUNS) */
    uint32_t tid_lo, tid_next;
} cov_depth_runs_info;
cov_status cov_depth_runs_compute(cov_session *s, uint32_t tid_lo, uint32_t tid_hi, uint32_t *tid_next, uint64_t *n_runs);
cov_status cov_depth_runs_fetch(cov_session *s, uint64_t *run_off, cov_depth_run *runs);
cov_status cov_depth_runs_last(const cov_session *s, cov_depth_runs_info *out);

/* ---- depth bins: the same per-base depth reduced over fixed windows on the device, for coverage plots, copy-number windows and binning
 * input (one value per window, not one line per depth change).  For a bin size B, 1 <= B <= 2^31 - 1, target t of length L has
 * ceil(L / B) bins; bin b covers bases [b * B, min((b + 1) * B, L)): bins never cross a target boundary, the last bin of a target is short
 * when B does not divide L, and a target with L == 0 has none.  Per bin: the sum, the smallest and the largest depth of its bases and the
 * number of bases with depth > 0; all integers, no float is computed on the device.
 * The chunking is that of the depth runs (the same planner and budget, the same arena):
 *   cov_depth_bins_compute(s, bin_size, tid_lo, tid_hi, &tid_next, &n_bins)
 *         materialises the depth of targets [tid_lo, tid_next) as cov_depth_runs_compute does and reduces it: every arena word is read
 *         once (csrc/depth_bins_kernels.hip.h).  The chunk's n_bins bins stay on the device until the next compute / push / reset / finish.
 *         bin_size 0 or above 2^31 - 1 is COV_ERR_INVALID_ARG; a chunk of 2^32 bins is refused.
 *   cov_depth_bins_fetch(s, bin_off, bins)
 *         bin_off: tid_next - tid_lo + 1 entries relative to the chunk, the bins of target tid_lo + k are bins[bin_off[k] .. bin_off[k + 1])
 *         (an empty target repeats its neighbour's offset); bins: n_bins entries in target order, then position order.
 * The states are those of the depth runs.  The runs and the bins of a session share the chunk's arena (with the regions below): a cov_depth_runs_compute makes
 * cov_depth_bins_fetch return COV_ERR_STATE until the next cov_depth_bins_compute, and the reverse.  cov_kernel_ms(COV_K_DEPTH_BINS) and
 * cov_depth_bins_last describe the last chunk. */
typedef struct { uint64_t sum; int32_t min; int32_t max; uint32_t covered; uint32_t reserved; } cov_depth_bin; /* 24 B */
typedef struct {
    uint64_t arena_bases; /* entries of the chunk's arena (padding included) */
    uint64_t n_bins;
    double arena_ms;      /* the pileup into the arena (with its zero fill), HIP-event time */
    double bins_ms;       /* the bin kernels = cov_kernel_ms(COV_K_DEPTH_BINS) */
    uint32_t tid_lo, tid_next;
    uint32_t bin_size, reserved;
} cov_depth_bins_info;
cov_status cov_depth_bins_compute(cov_session *s, uint32_t bin_size, uint32_t tid_lo, uint32_t tid_hi, uint32_t *tid_next, uint64_t *n_bins);
cov_status cov_depth_bins_fetch(cov_session *s, uint64_t *bin_off, cov_depth_bin *bins);
cov_status cov_depth_bins_last(const cov_session *s, cov_depth_bins_info *out);

/* ---- depth regions: the same per-base depth reduced over arbitrary intervals on the device (the regions of a BED file: exome or amplicon
 * targets, genes, prophage or plasmid intervals, windows around a breakpoint).  A region is [start, end) of target tid, 0-based and half
 * open, with start < end <= the target's length; regions may overlap, repeat and come in any order, and range from one base to a whole
 * target.  Per region the fields of cov_depth_bin: the sum, the smallest and the largest depth of its bases and the number of bases with
 * depth > 0 (no end exclusion: every base of the region counts).
 *   cov_depth_regions_set(s, regions, n)
 *         validates the regions against the session's targets and keeps a copy in a stable order by tid (the input order inside a target
 *         is kept).  n == 0 clears them.  COV_ERR_STATE before cov_set_targets; COV_ERR_INVALID_ARG, with the first offending index in
 *         cov_last_error, for tid >= n_targets, start >= end, end > length, reserved != 0 or n >= 2^32 (the regions set before stay).
 *         cov_set_targets drops the regions; cov_reset and cov_finish keep them.
 *   cov_depth_regions_compute(s, tid_lo, tid_hi, &tid_next, &n_regions)
 *         chunks as cov_depth_runs_compute does (the same planner, budget and arena), and reduces the regions whose target lies in
 *         [tid_lo, tid_next): a wave per piece of 4096 bases of a region (csrc/depth_regions_kernels.hip.h).  A chunk without a region is
 *         legal (n_regions = 0); a chunk of 2^32 pieces or more is refused (COV_ERR_STATE); without regions set: COV_ERR_STATE.
 *   cov_depth_regions_fetch(s, input_index, out)
 *         the chunk's n_regions results; input_index[i] is the position of result i in the array given to cov_depth_regions_set.
 * The states are those of the depth runs and bins.  Runs, bins and regions share the chunk's arena: a compute of one makes the fetch of the
 * other two return COV_ERR_STATE until their own next compute.  cov_kernel_ms(COV_K_DEPTH_REGIONS) and cov_depth_regions_last describe the
 * last chunk. */
typedef struct { uint32_t tid, start, end, reserved; } cov_depth_region; /* 16 B, [start, end) */
typedef struct {
    uint64_t arena_bases; /* entries of the chunk's arena (padding included) */
    uint64_t n_regions;   /* regions of the chunk */
    uint64_t n_pieces;    /* waves of the reduction */
    double arena_ms;      /* the pileup into the arena (with its zero fill), HIP-event time */
    double regions_ms;    /* the region kernels = cov_kernel_ms(COV_K_DEPTH_REGIONS) */
    uint32_t tid_lo, tid_next;
} cov_depth_regions_info;
cov_status cov_depth_regions_set(cov_session *s, const cov_depth_region *regions, uint64_t n);
cov_status cov_depth_regions_compute(cov_session *s, uint32_t tid_lo, uint32_t tid_hi, uint32_t *tid_next, uint64_t *n_regions);
cov_status cov_depth_regions_fetch(cov_session *s, uint64_t *input_index, cov_depth_bin *out);
cov_status cov_depth_regions_last(const cov_session *s, cov_depth_regions_info *out);

/* ---- depth classes: a depth classified against a short ascending list of cut points (csrc/depth_class_core.h).  A cut list holds n values,
 * 1 <= n <= COV_DEPTH_MAX_CUTS, each in [0, 2^31 - 1], strictly ascending; the class of a depth d is the number of cuts c with c <= d:
 * class 0 lies below the first cut, class n at or above the last.  A bad list is COV_ERR_INVALID_ARG with the first offending index in
 * cov_last_error ("value <index>: ...").
 *   cov_depth_class_runs_compute(s, cuts, n_cuts, tid_lo, tid_hi, &tid_next, &n_runs)
 *         cov_depth_runs_compute over the depth CLASSES: the maximal stretches of equal class inside each target, every class included
 *         (0 and n too), in target order, then position order.  States, chunking, knob and refusals are those of cov_depth_runs_compute.
 *         The chunk belongs to the runs: cov_depth_runs_fetch fetches it (the `depth` field of a run holds its class),
 *         cov_depth_runs_last and cov_kernel_ms(COV_K_DEPTH_RUNS) describe it (seven launches, as for the plain runs).
 *   cov_depth_thresholds_set(s, thr, n)
 *         the thresholds (a cut list) cov_depth_regions_compute counts from now on; n == 0 clears them.  Valid any time after cov_create;
 *         kept over cov_set_targets, cov_reset and cov_finish.  Setting them drops a regions chunk that awaits its fetch.
 *         With thresholds set, cov_depth_regions_compute also leaves, per region and threshold t, the number of the region's bases with
 *         depth >= t (the threshold variant of the region kernel: the same six launches, or four for a chunk without a region; the
 *         results of cov_depth_regions_fetch are the bytes they are without thresholds).
 *   cov_depth_regions_counts_fetch(s, counts)
 *         n_regions * n thresholds values, row-major: row i belongs to result i of cov_depth_regions_fetch.  The states are those of
 *         cov_depth_regions_fetch, its arena-was-taken sentence included; COV_ERR_STATE when no thresholds are set. */
#define COV_DEPTH_MAX_CUTS 16
cov_status cov_depth_class_runs_compute(cov_session *s, const int32_t *cuts, uint32_t n_cuts,
                                        uint32_t tid_lo, uint32_t tid_hi, uint32_t *tid_next, uint64_t *n_runs);
cov_status cov_depth_thresholds_set(cov_session *s, const int32_t *thr, uint32_t n);   /* n == 0 clears */
cov_status cov_depth_regions_counts_fetch(cov_session *s, uint32_t *counts);

/* Page-locked host memory for record batches, pooled: a freed block is kept for the next request of similar size
 * (a decoder filling one batch per BAM file gets its arrays back without re-pinning).  cov_host_alloc returns NULL
 * when no HIP device is usable; cov_host_free returns 0 if `p` did not come from cov_host_alloc; cov_host_trim
 * gives the parked blocks back to the system. */
/* Binds the CALLING THREAD (and the threads it creates afterwards) to the CPUs of the NUMA node device `device` is attached to;
 * returns that node, or -1 when nothing was changed.  Call it in the thread that is going to read and feed a file for that device. */
int cov_bind_thread_to_device_node(int device);
void *cov_host_alloc(size_t bytes);
/* Host memory the caller owns (e.g. an mmap of the BAM file, page aligned) made readable by the session's device, so that
 * cov_ingest_feed can take its bytes from there without a staging copy; unregister once the session has synchronised
 * (after cov_ingest_end / cov_ingest_abort).  COV_ERR_HIP when the runtime refuses the range: use staging buffers then. */
cov_status cov_host_register(cov_session *s, void *p, size_t bytes);
cov_status cov_host_unregister(cov_session *s, void *p);
int cov_host_free(void *p);
void cov_host_trim(void);

#ifdef __cplusplus
}
#endif
#endif /* COVERMHIP_H */

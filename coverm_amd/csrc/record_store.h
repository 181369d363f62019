// The session's device record store: nine SoA columns and three optional mate columns, with the rules of their growth in ONE place.  Host
// code only: the kernels see the columns through their own pointer structs, which view() fills.
//   cigar_off  has one entry more than there are records: [n_records] is the closing offset, == n_cigar; seal() writes it, before any pass.
//   cigar      is reserved with one spare word behind the last CIGAR word (the callers count it in).
//   mtid, qh1, qh2   exist only where an ingest asked for them (cov_ingest_want_mates) and describe records [0, mates_valid).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <utility>
#include "../../include/covermhip.h"

#define RS_TRY(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) return e_; } while (0)

template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;  // elements
    hipError_t reserve(size_t n, hipStream_t st, size_t keep = 0) {
        if (n <= cap) return hipSuccess;
        const size_t nc = std::max(n, cap + cap / 2);
        T *q = nullptr;
        RS_TRY(hipMalloc(&q, nc * sizeof(T)));
        if (keep && p) { RS_TRY(hipMemcpyAsync(q, p, keep * sizeof(T), hipMemcpyDeviceToDevice, st)); RS_TRY(hipStreamSynchronize(st)); }
        if (p) (void)hipFree(p);
        p = q; cap = nc; return hipSuccess;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

struct RecordStore {
    DevBuf<int32_t> tid, pos; DevBuf<uint16_t> flag; DevBuf<uint8_t> mapq, nm_kind; DevBuf<uint32_t> nm, l_seq, cigar_off, cigar;
    DevBuf<int32_t> mtid; DevBuf<unsigned long long> qh1; DevBuf<uint32_t> qh2;      // the mate's next_refID, the 96-bit hash of the read name
    uint64_t n_records = 0, n_cigar = 0, mates_valid = 0;      // (n_records also counts an adopted device batch, which the columns do not hold)
    DevBuf<uint8_t> bounce;                   // move_front: a tail that overlaps its destination goes through here

    RecordStore() = default; RecordStore(const RecordStore &) = delete; RecordStore &operator=(const RecordStore &) = delete; ~RecordStore() { release(); }

    // Room for n_rec records and cig_words CIGAR words; a column that grows keeps its first keep_rec / keep_cig elements (copied on `st`,
    // which is drained), cigar_off the closing offset too.  (On an empty store that is one stale word: the first record written replaces it.)
    hipError_t reserve(size_t n_rec, size_t cig_words, hipStream_t st, size_t keep_rec, size_t keep_cig, bool with_mates) {
        RS_TRY(tid.reserve(n_rec, st, keep_rec)); RS_TRY(pos.reserve(n_rec, st, keep_rec)); RS_TRY(flag.reserve(n_rec, st, keep_rec));
        RS_TRY(mapq.reserve(n_rec, st, keep_rec)); RS_TRY(nm_kind.reserve(n_rec, st, keep_rec)); RS_TRY(nm.reserve(n_rec, st, keep_rec));
        RS_TRY(l_seq.reserve(n_rec, st, keep_rec)); RS_TRY(cigar_off.reserve(n_rec + 1, st, keep_rec + 1)); RS_TRY(cigar.reserve(cig_words, st, keep_cig));
        if (with_mates) { RS_TRY(mtid.reserve(n_rec, st, keep_rec)); RS_TRY(qh1.reserve(n_rec, st, keep_rec)); RS_TRY(qh2.reserve(n_rec, st, keep_rec)); }
        return hipSuccess;
    }
    void release() {
        tid.release(); pos.release(); flag.release(); mapq.release(); nm_kind.release(); nm.release(); l_seq.release(); cigar_off.release(); cigar.release();
        mtid.release(); qh1.release(); qh2.release(); bounce.release();
    }
    // The columns and the counts change hands (the mate columns only with_mates; mates_valid stays where it is).
    void swap(RecordStore &o, bool with_mates) {
        std::swap(tid, o.tid); std::swap(pos, o.pos); std::swap(flag, o.flag); std::swap(mapq, o.mapq); std::swap(nm_kind, o.nm_kind);
        std::swap(nm, o.nm); std::swap(l_seq, o.l_seq); std::swap(cigar_off, o.cigar_off); std::swap(cigar, o.cigar);
        if (with_mates) { std::swap(mtid, o.mtid); std::swap(qh1, o.qh1); std::swap(qh2, o.qh2); }
        std::swap(n_records, o.n_records); std::swap(n_cigar, o.n_cigar);
    }
    // The store holds n_rec records and n_cig CIGAR words: the closing offset is written (on `st`, which is drained), the counts are committed.
    hipError_t seal(uint64_t n_rec, uint64_t n_cig, hipStream_t st) {
        const uint32_t end_off = (uint32_t)n_cig;
        RS_TRY(hipMemcpyAsync(cigar_off.p + n_rec, &end_off, sizeof end_off, hipMemcpyHostToDevice, st)); RS_TRY(hipStreamSynchronize(st));
        n_records = n_rec; n_cigar = n_cig; return hipSuccess;
    }
    // Records [rec_from, n_records) and CIGAR words [cig_from, n_cigar) move to the front of their columns, queued on `st`; the offsets still
    // count from the old front and the counts are the caller's to commit.  Not the mate columns: a store that carries them does not spill.
    hipError_t move_front(uint64_t rec_from, uint64_t cig_from, hipStream_t st) {
        const size_t n = (size_t)(n_records - rec_from);
        RS_TRY(front_(tid.p, rec_from, n, st)); RS_TRY(front_(pos.p, rec_from, n, st)); RS_TRY(front_(flag.p, rec_from, n, st)); RS_TRY(front_(mapq.p, rec_from, n, st));
        RS_TRY(front_(nm_kind.p, rec_from, n, st)); RS_TRY(front_(nm.p, rec_from, n, st)); RS_TRY(front_(l_seq.p, rec_from, n, st)); RS_TRY(front_(cigar_off.p, rec_from, n + 1, st));
        return front_(cigar.p, cig_from, (size_t)(n_cigar - cig_from), st);
    }
    // The nine columns by field name into the pointer struct of the kernels that read or write them (covk::Records, covi::RecStore, covs::Out,
    // covp::Store); view_unplaced: all but pos (covp::PairCols).  view_mates: for the structs that carry the mate pointers.
    template <typename V> void view(V &v) const { v.pos = pos.p; view_unplaced(v); }
    template <typename V> void view_unplaced(V &v) const { v.tid = tid.p; v.flag = flag.p; v.mapq = mapq.p; v.nm_kind = nm_kind.p; v.nm = nm.p; v.l_seq = l_seq.p; v.cigar_off = cigar_off.p; v.cigar = cigar.p; }
    template <typename V> void view_mates(V &v) const { v.mtid = mtid.p; v.qh1 = qh1.p; v.qh2 = qh2.p; }
    // n records of batch `b` (host or device arrays: `kind`) behind the store's own, and its ncig CIGAR words from b.cigar[off0] on; the copied
    // offsets still count as b's do.  Queued on `st`; room has been reserved, the counts are the caller's to commit.
    hipError_t copy_in(const cov_batch &b, uint64_t n, uint32_t off0, uint64_t ncig, hipMemcpyKind kind, hipStream_t st) {
        const uint64_t R = n_records;
        RS_TRY(hipMemcpyAsync(tid.p + R, b.tid, n * 4, kind, st)); RS_TRY(hipMemcpyAsync(pos.p + R, b.pos, n * 4, kind, st)); RS_TRY(hipMemcpyAsync(flag.p + R, b.flag, n * 2, kind, st));
        RS_TRY(hipMemcpyAsync(mapq.p + R, b.mapq, n, kind, st)); RS_TRY(hipMemcpyAsync(nm_kind.p + R, b.nm_kind, n, kind, st)); RS_TRY(hipMemcpyAsync(nm.p + R, b.nm, n * 4, kind, st));
        RS_TRY(hipMemcpyAsync(l_seq.p + R, b.l_seq, n * 4, kind, st)); RS_TRY(hipMemcpyAsync(cigar_off.p + R, b.cigar_off, (n + 1) * 4, kind, st));
        return ncig ? hipMemcpyAsync(cigar.p + n_cigar, b.cigar + off0, ncig * 4, kind, st) : hipSuccess;
    }
    // The whole store to host arrays (a cov_batch of writable pointers), the mate columns likewise; queued on `st`.
    hipError_t copy_out(const cov_batch &h, hipStream_t st) const {
        const uint64_t n = n_records; const hipMemcpyKind kind = hipMemcpyDeviceToHost;
        if (!n) return hipSuccess;
        RS_TRY(hipMemcpyAsync((void *)h.tid, tid.p, n * 4, kind, st)); RS_TRY(hipMemcpyAsync((void *)h.pos, pos.p, n * 4, kind, st)); RS_TRY(hipMemcpyAsync((void *)h.flag, flag.p, n * 2, kind, st));
        RS_TRY(hipMemcpyAsync((void *)h.mapq, mapq.p, n, kind, st)); RS_TRY(hipMemcpyAsync((void *)h.nm, nm.p, n * 4, kind, st)); RS_TRY(hipMemcpyAsync((void *)h.nm_kind, nm_kind.p, n, kind, st));
        RS_TRY(hipMemcpyAsync((void *)h.l_seq, l_seq.p, n * 4, kind, st)); RS_TRY(hipMemcpyAsync((void *)h.cigar_off, cigar_off.p, (n + 1) * 4, kind, st));
        return n_cigar ? hipMemcpyAsync((void *)h.cigar, cigar.p, n_cigar * 4, kind, st) : hipSuccess;
    }
    hipError_t copy_mates_out(int32_t *h_mtid, uint64_t *h_qh1, uint32_t *h_qh2, hipStream_t st) const {
        const uint64_t n = n_records;
        if (!n) return hipSuccess;
        RS_TRY(hipMemcpyAsync(h_mtid, mtid.p, n * 4, hipMemcpyDeviceToHost, st)); RS_TRY(hipMemcpyAsync(h_qh1, qh1.p, n * 8, hipMemcpyDeviceToHost, st));
        return hipMemcpyAsync(h_qh2, qh2.p, n * 4, hipMemcpyDeviceToHost, st);
    }
    hipError_t copy_mates_in(const int32_t *h_mtid, const uint64_t *h_qh1, const uint32_t *h_qh2, hipStream_t st) {
        const uint64_t n = n_records;
        if (!n) return hipSuccess;
        RS_TRY(hipMemcpyAsync(mtid.p, h_mtid, n * 4, hipMemcpyHostToDevice, st)); RS_TRY(hipMemcpyAsync(qh1.p, h_qh1, n * 8, hipMemcpyHostToDevice, st));
        return hipMemcpyAsync(qh2.p, h_qh2, n * 4, hipMemcpyHostToDevice, st);
    }
    template <typename T>
    hipError_t front_(T *p, size_t from, size_t n, hipStream_t st) {
        if (!n || !from) return hipSuccess;
        if (n <= from) return hipMemcpyAsync(p, p + from, n * sizeof(T), hipMemcpyDeviceToDevice, st);      // disjoint
        RS_TRY(bounce.reserve(n * sizeof(T), st));
        RS_TRY(hipMemcpyAsync(bounce.p, p + from, n * sizeof(T), hipMemcpyDeviceToDevice, st));
        return hipMemcpyAsync(p, bounce.p, n * sizeof(T), hipMemcpyDeviceToDevice, st);
    }
#undef RS_TRY
};

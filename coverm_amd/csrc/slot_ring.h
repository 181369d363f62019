// One producer fills NS staging slots in turn, one consumer feeds them in order (the two device ingest feeders of csrc/host_bam.cpp: BGZF
// pieces and SAM text windows).  Piece k lives in slot k % NS; the producer may refill that slot once piece k - NS has been fed.  (That the
// piece's UPLOAD has left the slot as well is the producer's own wait behind acquire(): cov_ingest_slot_wait / cov_sam_slot_wait.)
// Every wait returns on stop(), fail() and finish(): neither side can be left waiting for the other.  Host only, nothing of the project;
// tests/c/slot_ring_host.cpp runs it under the thread and address sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <condition_variable>
#include <mutex>
#include <string>

template <int NS>
class SlotRing {
    std::mutex mu_;
    std::condition_variable cv_;
    uint64_t published_ = 0, fed_ = 0;      // pieces announced so far / pieces fed so far
    size_t bytes_[NS] = {};
    bool finished_ = false, failed_ = false, soft_ = false, stopped_ = false;
    std::string err_;
    template <class F> void set(F f) { { std::lock_guard<std::mutex> lk(mu_); f(); } cv_.notify_all(); }
public:
    // ---- producer
    // Blocks until slot k % NS may be refilled (piece k - NS has been fed); false: the run has ended, fill nothing more.
    bool acquire(uint64_t k) {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return stopped_ || failed_ || finished_ || k < (uint64_t)NS || fed_ + NS > k; });
        return !(stopped_ || failed_ || finished_);
    }
    void publish(uint64_t k, size_t n_bytes) { set([&] { bytes_[k % NS] = n_bytes; published_ = k + 1; }); }
    void finish() { set([&] { finished_ = true; }); }      // no more pieces (a reader of a pipe does not know their count in advance)
    void fail(const std::string &msg, bool soft) { set([&] { if (!failed_) { failed_ = true; soft_ = soft; err_ = msg; } }); }
    // ---- consumer
    // Blocks until piece k is there (PIECE, its size in *n_bytes), the producer has failed (FAILED: at once, pieces already announced are
    // not fed any more) or no piece k will come (END: the producer finished, or the run was stopped).
    enum Take { PIECE, END, FAILED };
    Take take(uint64_t k, size_t *n_bytes) {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return failed_ || stopped_ || finished_ || published_ > k; });
        if (failed_) return FAILED;
        if (stopped_ || published_ <= k) return END;
        *n_bytes = bytes_[k % NS];
        return PIECE;
    }
    void fed(uint64_t k) { set([&] { fed_ = k + 1; }); }
    void stop() { set([&] { stopped_ = true; }); }
    // the producer's failure, to be read once take() has said FAILED or the producer's thread has been joined
    bool failed() { std::lock_guard<std::mutex> lk(mu_); return failed_; }
    bool soft() { std::lock_guard<std::mutex> lk(mu_); return soft_; }      // soft: the input can still go another way (the CPU reader)
    std::string error() { std::lock_guard<std::mutex> lk(mu_); return err_; }
};

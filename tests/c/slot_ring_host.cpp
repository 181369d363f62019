// csrc/slot_ring.h between two threads: a producer that fills NS = 4 slots in turn and a consumer that takes them in order, with
// pseudo-random yields seeded from the case number.  Every case must END — both threads return whatever the other does —, the consumer must
// see pieces 0, 1, 2, .. in order with the sizes and the slot contents the producer gave them, and the producer must never hold slot
// k % NS for piece k before piece k - NS has been fed.  Test infrastructure (tests/test_slot_ring.py builds it with
// -fsanitize=thread and with -fsanitize=address,undefined and runs it under a time limit: a hang is a failure); not part of the product.
#include <stdint.h>
#include <stdio.h>

#include <atomic>
#include <string>
#include <thread>

#include "../../coverm_amd/csrc/slot_ring.h"

constexpr int NS = 4;
typedef SlotRing<NS> Ring;

struct Rng {
    uint32_t s;
    void pause() {      // yield now and then, sometimes several times in a row
        s = s * 1664525u + 1013904223u;
        for (uint32_t n = (s >> 24) % 5 == 0 ? (s >> 16) % 4 + 1 : 0; n; n--) std::this_thread::yield();
    }
};
static size_t size_of_piece(uint64_t k) { return (size_t)(k * 7 + 3); }

struct Case {
    uint64_t pieces; bool known;      // known: the consumer asks for exactly `pieces`; else it takes until the producer has finished
    int64_t fail_at, stop_at;         // the producer fails instead of giving piece fail_at / the consumer stops when it has fed stop_at pieces; -1 = never
    bool soft;
};

// -> what went wrong, empty if nothing
static std::string run(const Case &c, uint32_t seed) {
    Ring ring;
    uint64_t slot[NS] = {};                    // the slots' contents: written by the producer while it holds them, read by the consumer
    std::atomic<uint64_t> fed_count{0};        // set by the consumer BEFORE it tells the ring
    std::string p_bad, c_bad;
    uint64_t produced = 0, consumed = 0;
    bool producer_stopped = false;
    std::thread producer([&] {
        Rng r{seed * 2654435761u + 1};
        for (uint64_t k = 0; k < c.pieces; k++) {
            r.pause();
            if (!ring.acquire(k)) { producer_stopped = true; return; }
            if (k >= NS && fed_count.load() + NS <= k) { p_bad = "slot held before piece k - NS was fed, k = " + std::to_string(k); ring.fail(p_bad, false); return; }
            r.pause();
            if ((int64_t)k == c.fail_at) { ring.fail("failed at " + std::to_string(k), c.soft); return; }
            slot[k % NS] = k * 1000003u + 17;
            r.pause();
            ring.publish(k, size_of_piece(k));
            produced = k + 1;
        }
        r.pause();
        ring.finish();
    });
    Ring::Take got = Ring::END;
    {
        Rng r{seed * 40503u + 7};
        for (uint64_t k = 0; !c.known || k < c.pieces; k++) {
            if ((int64_t)k == c.stop_at) { ring.stop(); break; }
            r.pause();
            size_t n = ~(size_t)0;
            if ((got = ring.take(k, &n)) != Ring::PIECE) break;
            if (n != size_of_piece(k)) { c_bad = "wrong size of piece " + std::to_string(k); ring.stop(); break; }
            r.pause();
            if (slot[k % NS] != k * 1000003u + 17) { c_bad = "slot overwritten under piece " + std::to_string(k); ring.stop(); break; }
            consumed = k + 1;
            fed_count.store(k + 1);
            r.pause();
            ring.fed(k);
        }
    }
    producer.join();
    if (!p_bad.empty()) return p_bad;
    if (!c_bad.empty()) return c_bad;
    const bool fails = c.fail_at >= 0 && (uint64_t)c.fail_at < c.pieces && (c.stop_at < 0 || c.fail_at < c.stop_at + NS);
    const bool stops = c.stop_at >= 0 && (uint64_t)c.stop_at < c.pieces + (c.known ? 0 : 1);
    if (fails && !stops) {
        // pieces in front of the failure may or may not have been taken (a failure is reported at once), none behind it
        if (got != Ring::FAILED || consumed > (uint64_t)c.fail_at) return "failure not seen, or pieces behind it";
        if (!ring.failed() || ring.soft() != c.soft || ring.error() != "failed at " + std::to_string(c.fail_at)) return "failure reported wrongly";
    } else if (stops && !fails) {
        if (consumed != (uint64_t)c.stop_at) return "stopped after the wrong piece";
        if (produced > (uint64_t)c.stop_at + NS) return "producer ran on past the stop";
        if (!producer_stopped && produced != c.pieces) return "producer ended without a reason";
    } else if (!fails && !stops) {
        if (consumed != c.pieces || produced != c.pieces) return "pieces missing: " + std::to_string(consumed) + " of " + std::to_string(c.pieces);
        if (!c.known && got != Ring::END) return "end not seen";
        if (ring.failed()) return "failure out of nowhere";
    } else if (consumed > (uint64_t)c.stop_at || consumed > (uint64_t)c.fail_at) return "pieces behind a stop or a failure";      // both: either may win
    return "";
}

int main() {
    unsigned long long n = 0, bad = 0;
    auto check = [&](const Case &c) {
        for (uint32_t rep = 0; rep < 8; rep++, n++) {
            const std::string e = run(c, (uint32_t)n);
            if (!e.empty()) { bad++; printf("case %llu (pieces %llu known %d fail_at %lld stop_at %lld soft %d): %s\n", n, (unsigned long long)c.pieces, (int)c.known, (long long)c.fail_at, (long long)c.stop_at, (int)c.soft, e.c_str()); }
        }
    };
    for (uint64_t pieces : {0u, 1u, 4u, 5u, 1000u})
        for (bool known : {true, false}) check(Case{pieces, known, -1, -1, false});
    for (int64_t j : {0, 3, 4, 7})
        for (bool known : {true, false}) {
            check(Case{1000, known, j, -1, false});      // the producer fails hard
            check(Case{1000, known, j, -1, true});       // ... or softly
            check(Case{1000, known, -1, j, false});      // the consumer stops
            check(Case{1000, known, j, j, true});        // both at the same piece
            check(Case{8, known, j, -1, false});         // a failure at or near the last piece
        }
    printf("%llu cases, %llu bad\n", n, bad);
    return bad ? 1 : 0;
}

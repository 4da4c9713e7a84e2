// slp_dga_draws.h -- the window of tie draws the host keeps for the dual gradient ascent handles (slp_dga.hip, slp_dga_batch.hip,
// slp_dga_many.hip).  Pure host code, all unsigned arithmetic on positions in the stream of draws; no HIP, no device buffer: the
// handle uploads data() after a push and hands (device copy, base, size()) to its kernels.
//
// The readers (one solve, the instances of a batch, the LPs of a list) take their draws on the device, nothing is read back
// inside an iterate call, and an iteration takes at most two draws per reader.  So the host keeps `bound`, a position no reader
// can have passed, and lets an iteration start only while two more draws lie behind it (reserve); reading the controls back
// tightens it to the furthest reader (observe).
//
// A reader that meets a tie beyond the window takes 0.5, raises the device's dry flag and moves on, so `passed` -- the position
// every moving reader has passed -- can lie beyond end() when draws are pushed.  The three handles answer that overrun
// differently, and push() keeps each answer as it was: kJump (the single solve) empties the window and sets base = passed, the
// new draws continue the stream where its one reader stands and no pushed draw is skipped; kDropFirst (the batch) empties the
// window, leaves base at the old end() and appends there, positions stay absolute for the other readers and the draws the
// reader ran past stay in the host copy until the next push; kAppendFirst (the list) appends at the old end() and then drops up
// to passed, the same positions as kDropFirst with the fresh draws the reader ran past dropped at once.  Without an overrun the
// three are the same window.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace slp {

enum DgaOverrun { kJump, kDropFirst, kAppendFirst };

struct DgaDrawWindow {
    std::vector<double> host;   // the draws from position `base` on
    uint64_t base = 0;          // position (in the stream of draws) of host[0]
    uint64_t bound = 0;         // no reader stands behind this position (2 per iteration since the last observe)
    bool dry = false;           // sticky: an iterate call stopped early because the window could have run dry

    const double *data() const { return host.data(); }
    uint64_t size() const { return (uint64_t)host.size(); }
    uint64_t end() const { return base + size(); }

    void observe(uint64_t furthest) { bound = furthest; }

    // Iterations <= want that cannot run dry; moves `bound` two draws per iteration granted.
    int64_t reserve(int64_t want) {
        const uint64_t safe = end() > bound ? (end() - bound) / 2 : 0;
        const int64_t got = want > 0 ? (int64_t)std::min<uint64_t>((uint64_t)want, safe) : 0;
        if (got == 0 && want > 0) dry = true;
        bound += 2 * (uint64_t)got;
        return got;
    }

    int64_t left() const { return (int64_t)end() - (int64_t)bound; }

    // Appends `count` draws; what every moving reader has passed is dropped from the front (passed == ~0: no reader moves,
    // nothing is dropped).  `mode`: see the head of this file.
    void push(const double *draws, int64_t count, uint64_t passed, DgaOverrun mode) {
        if (mode == kAppendFirst) host.insert(host.end(), draws, draws + count);
        if (passed != ~(uint64_t)0 && passed > base) {
            const uint64_t drop = std::min<uint64_t>(passed - base, size());
            host.erase(host.begin(), host.begin() + (int64_t)drop);
            base = mode == kJump ? passed : base + drop;
        }
        if (mode != kAppendFirst) host.insert(host.end(), draws, draws + count);
        dry = false;
    }
};

// The two positions the window takes from its readers.  `moves(k)`: reader k still takes draws; `position(k)`: where it stands in
// the stream.  A reader that stands still for ever (a frozen start; in the list handle also an LP its stopping test has stopped)
// must not count: as the furthest it would only ask for draws nobody reads, as the hindmost it would hold the front of the window
// where it stands and the window would grow with every push.
// observe(): the furthest moving reader, 0 when none moves.
template <class Moves, class Position>
inline uint64_t dga_furthest_reader(size_t count, Moves moves, Position position) {
    uint64_t mx = 0;
    for (size_t k = 0; k < count; ++k)
        if (moves(k)) mx = std::max<uint64_t>(mx, position(k));
    return mx;
}

// push(): what every moving reader has passed, ~0 when none moves.
template <class Moves, class Position>
inline uint64_t dga_passed_by_all(size_t count, Moves moves, Position position) {
    uint64_t passed = ~(uint64_t)0;
    for (size_t k = 0; k < count; ++k)
        if (moves(k)) passed = std::min<uint64_t>(passed, position(k));
    return passed;
}

}  // namespace slp

// Stand-alone check of DgaDrawWindow with the moving-reader predicate of the list handle (pysparselp_amd/csrc/slp_dga_draws.h:
// dga_furthest_reader, dga_passed_by_all), built with -fsanitize=address,undefined and run as a child process by
// tests/test_dga_many_stop_host.py.  The readers are what slp_many_dga keeps per LP: where the LP's positions begin in the stream
// (its draw offset), the tie draws it has taken, and whether it is frozen or stopped.  A stopped LP stands still for ever: with it
// counted as a reader the front of the window would stay at its position and every push would make the window longer.
#include "slp_dga_draws.h"

#include <cstdio>
#include <vector>

using slp::DgaDrawWindow;

static int failures = 0, checks = 0;

static void expect_eq(const char *what, long long got, long long want) {
    ++checks;
    if (got == want) return;
    ++failures;
    std::printf("FAIL %s: %lld, expected %lld\n", what, got, want);
}

static void expect_true(const char *what, bool ok) { expect_eq(what, ok ? 1 : 0, 1); }

struct Reader {
    uint64_t offset, consumed;
    bool frozen, stopped;
};

// what dgm_read_ctl and slp_many_dga_push_random do with the controls they have read back
static void observe(DgaDrawWindow &w, const std::vector<Reader> &r, bool stopped_moves) {
    w.observe(slp::dga_furthest_reader(
        r.size(), [&](size_t k) { return !r[k].frozen && (stopped_moves || !r[k].stopped); }, [&](size_t k) { return r[k].offset + r[k].consumed; }));
}

static void push(DgaDrawWindow &w, const std::vector<Reader> &r, const std::vector<double> &fresh, bool stopped_moves) {
    const uint64_t passed = slp::dga_passed_by_all(
        r.size(), [&](size_t k) { return !r[k].frozen && (stopped_moves || !r[k].stopped); }, [&](size_t k) { return r[k].offset + r[k].consumed; });
    w.push(fresh.data(), (int64_t)fresh.size(), passed, slp::kAppendFirst);
}

static void predicate_cases() {
    const std::vector<Reader> r = {{4, 3, false, true}, {0, 12, false, false}, {6, 10, false, false}, {30, 0, true, false}};
    auto pos = [&](size_t k) { return r[k].offset + r[k].consumed; };
    auto all = [](size_t) { return true; };
    auto none = [](size_t) { return false; };
    auto moving = [&](size_t k) { return !r[k].frozen && !r[k].stopped; };
    auto not_frozen = [&](size_t k) { return !r[k].frozen; };
    expect_eq("furthest of all", (long long)slp::dga_furthest_reader(r.size(), all, pos), 30);
    expect_eq("furthest of those not frozen", (long long)slp::dga_furthest_reader(r.size(), not_frozen, pos), 16);
    expect_eq("furthest of the moving", (long long)slp::dga_furthest_reader(r.size(), moving, pos), 16);
    expect_eq("furthest of none", (long long)slp::dga_furthest_reader(r.size(), none, pos), 0);
    expect_eq("passed by those not frozen: the stopped reader holds it", (long long)slp::dga_passed_by_all(r.size(), not_frozen, pos), 7);
    expect_eq("passed by the moving", (long long)slp::dga_passed_by_all(r.size(), moving, pos), 12);
    expect_true("passed by none: nothing is dropped", slp::dga_passed_by_all(r.size(), none, pos) == ~(uint64_t)0);
    expect_true("no reader at all", slp::dga_passed_by_all(0, all, pos) == ~(uint64_t)0 && slp::dga_furthest_reader(0, all, pos) == 0);
}

// three LPs read the stream; LP 0 stops early and stays behind.  Every round: refill to two draws per iteration behind the
// furthest reader (DeviceDGA.iterate), reserve, and every moving LP takes its two draws per iteration.
static void run(bool stopped_moves, size_t *largest, long long *granted, uint64_t *front) {
    DgaDrawWindow w;
    std::vector<Reader> r = {{5, 0, false, false}, {0, 0, false, false}, {9, 0, false, false}};
    *largest = 0;
    *granted = 0;
    const int rounds = 200, per_round = 7;
    for (int round = 0; round < rounds; ++round) {
        if (round == 3) r[0].stopped = true;
        observe(w, r, stopped_moves);
        const long long left = w.left();
        if (left < 2 * per_round) push(w, r, std::vector<double>((size_t)(2 * per_round - left), 0.5), stopped_moves);
        const long long it = w.reserve(per_round);
        *granted += it;
        for (size_t k = 0; k < r.size(); ++k) {
            if (r[k].frozen || r[k].stopped) continue;
            r[k].consumed += 2 * (uint64_t)it;   // a tie in both searches of every iteration
            expect_true("a moving reader stays inside the window", r[k].offset + r[k].consumed <= w.end());
        }
        *largest = w.size() > *largest ? (size_t)w.size() : *largest;
    }
    *front = w.base;
    expect_eq("every round ran in full", *granted, (long long)rounds * per_round);
    expect_eq("never dry", w.dry, 0);
}

static void window_cases() {
    size_t largest = 0;
    long long granted = 0;
    uint64_t front = 0;
    run(false, &largest, &granted, &front);
    // the moving readers stand 9 draws apart (their offsets); a push drops what lies before the hindmost and leaves 2 * 7 draws
    // behind the furthest: the window never holds more than that
    expect_true("a stopped reader behind: the front advances", front >= 199 * 2 * 7);
    expect_true("a stopped reader behind: the window stays bounded", largest <= 9 + 2 * 7);
    size_t largest_old = 0;
    uint64_t front_old = 0;
    run(true, &largest_old, &granted, &front_old);
    expect_eq("counted as a reader it holds the front where it stands", (long long)front_old, 5 + 3 * 2 * 7);
    expect_true("... and the window holds every draw since", largest_old >= 2 * 190 * 7);
    expect_true("the predicate is what keeps it short", largest < largest_old);
}

// every LP stopped or frozen: nothing moves, nothing is dropped, and an observe sees no reader
static void nothing_moves() {
    DgaDrawWindow w;
    const std::vector<Reader> r = {{0, 4, false, true}, {2, 0, true, false}};
    push(w, r, {0.1, 0.2, 0.3, 0.4, 0.5, 0.6}, false);
    expect_eq("nothing dropped", (long long)w.base, 0);
    expect_eq("all kept", (long long)w.size(), 6);
    observe(w, r, false);
    expect_eq("no reader: bound 0", (long long)w.bound, 0);
    expect_eq("reserve grants what the window holds", w.reserve(5), 3);
}

int main() {
    predicate_cases();
    window_cases();
    nothing_moves();
    std::printf("%s: %d checks, %d failures\n", failures ? "FAILED" : "ok", checks, failures);
    return failures ? 1 : 0;
}

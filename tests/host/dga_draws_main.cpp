// Stand-alone check of DgaDrawWindow (pysparselp_amd/csrc/slp_dga_draws.h), built with -fsanitize=address,undefined and run as
// a child process by tests/test_dga_draws_host.py.  The expected windows are written out by hand from what the three handles'
// push_random / iterate / status did before they shared the struct: kJump = slp_dga, kDropFirst = slp_batch_dga,
// kAppendFirst = slp_many_dga.
#include "slp_dga_draws.h"

#include <cstdio>
#include <initializer_list>

using slp::DgaDrawWindow;
using slp::DgaOverrun;

static int failures = 0, checks = 0;
static const uint64_t kNone = ~(uint64_t)0;
static const char *kNames[] = {"kJump", "kDropFirst", "kAppendFirst"};

static void expect(const char *what, const char *mode, const DgaDrawWindow &w, uint64_t base, std::initializer_list<double> host,
                   bool dry) {
    ++checks;
    const std::vector<double> want(host);
    if (w.base == base && w.host == want && w.dry == dry && w.end() == base + want.size() && w.size() == want.size()) return;
    ++failures;
    std::printf("FAIL %s [%s]: base %llu (expected %llu), dry %d (expected %d), host {", what, mode, (unsigned long long)w.base,
                (unsigned long long)base, (int)w.dry, (int)dry);
    for (double v : w.host) std::printf(" %g", v);
    std::printf(" } expected {");
    for (double v : want) std::printf(" %g", v);
    std::printf(" }\n");
}

static void expect_eq(const char *what, long long got, long long want) {
    ++checks;
    if (got == want) return;
    ++failures;
    std::printf("FAIL %s: %lld, expected %lld\n", what, got, want);
}

// positions 10 .. 13 hold 1 2 3 4, the dry flag is up; {7, 8} (or nothing) is pushed with the readers at `passed`
static DgaDrawWindow pushed(DgaOverrun mode, uint64_t passed, bool empty = false) {
    static const double fresh[2] = {7.0, 8.0};
    DgaDrawWindow w;
    w.base = 10;
    w.host = {1.0, 2.0, 3.0, 4.0};
    w.bound = 12;
    w.dry = true;
    if (empty) w.push(nullptr, 0, passed, mode);
    else w.push(fresh, 2, passed, mode);
    expect_eq("push leaves bound alone", (long long)w.bound, 12);
    return w;
}

static void push_cases() {
    for (int m = 0; m < 3; ++m) {
        const DgaOverrun mode = (DgaOverrun)m;
        const char *name = kNames[m];
        // without an overrun the three handles kept the same window
        expect("empty push, reader in the middle", name, pushed(mode, 12, true), 12, {3, 4}, false);
        expect("empty push, nothing passed", name, pushed(mode, 10, true), 10, {1, 2, 3, 4}, false);
        expect("nothing passed", name, pushed(mode, 10), 10, {1, 2, 3, 4, 7, 8}, false);
        expect("reader before the window", name, pushed(mode, 4), 10, {1, 2, 3, 4, 7, 8}, false);
        expect("reader in the middle", name, pushed(mode, 12), 12, {3, 4, 7, 8}, false);
        expect("reader exactly at the end", name, pushed(mode, 14), 14, {7, 8}, false);
        expect("all readers frozen", name, pushed(mode, kNone), 10, {1, 2, 3, 4, 7, 8}, false);
        expect("empty push, all readers frozen", name, pushed(mode, kNone, true), 10, {1, 2, 3, 4}, false);
    }
    // the overrun: the reader stands past position 14, the end of the window
    expect("reader 1 past the end", "kJump", pushed(slp::kJump, 15), 15, {7, 8}, false);              // base = passed
    expect("reader 5 past the end", "kJump", pushed(slp::kJump, 19), 19, {7, 8}, false);
    expect("empty push, 1 past", "kJump", pushed(slp::kJump, 15, true), 15, {}, false);
    expect("reader 1 past the end", "kDropFirst", pushed(slp::kDropFirst, 15), 14, {7, 8}, false);    // base += what was dropped: 4
    expect("reader 5 past the end", "kDropFirst", pushed(slp::kDropFirst, 19), 14, {7, 8}, false);
    expect("empty push, 1 past", "kDropFirst", pushed(slp::kDropFirst, 15, true), 14, {}, false);
    expect("reader 1 past the end", "kAppendFirst", pushed(slp::kAppendFirst, 15), 15, {8}, false);   // 7 sits at 14: dropped
    expect("reader 5 past the end", "kAppendFirst", pushed(slp::kAppendFirst, 19), 16, {}, false);    // both fresh draws dropped
    expect("empty push, 1 past", "kAppendFirst", pushed(slp::kAppendFirst, 15, true), 14, {}, false);
}

// eight draws at positions 3 .. 10, the furthest reader `left` draws before the end
static DgaDrawWindow with_left(int left) {
    DgaDrawWindow w;
    w.base = 3;
    w.host.assign(8, 0.25);
    w.observe(11 - (uint64_t)left);
    expect_eq("left() after observe", w.left(), left);
    return w;
}

static void reserve_cases() {
    for (int left = 0; left <= 3; ++left) {
        DgaDrawWindow w = with_left(left);
        expect_eq("reserve(0)", w.reserve(0), 0);
        expect_eq("reserve(0) leaves the dry flag down", w.dry, 0);
        expect_eq("reserve(0) leaves bound alone", w.left(), left);
        const long long got = left / 2;   // one iteration needs two draws: 0, 0, 1, 1
        expect_eq("reserve(4)", w.reserve(4), got);
        expect_eq("reserve(4): dry exactly when no iteration can run", w.dry, got == 0);
        expect_eq("reserve(4) moves bound by two per iteration", w.left(), left - 2 * got);
    }
    {   // plenty: the request is the limit
        DgaDrawWindow w = with_left(8);
        expect_eq("reserve(3) of 8 draws", w.reserve(3), 3);
        expect_eq("left after it", w.left(), 2);
        expect_eq("reserve(4) of 2 draws", w.reserve(4), 1);
        expect_eq("not dry yet", w.dry, 0);
        expect_eq("reserve(1) of none", w.reserve(1), 0);
        expect_eq("dry", w.dry, 1);
    }
    {   // a reader that ran past the window: left() is negative, nothing can run
        DgaDrawWindow w = with_left(-5);
        expect_eq("reserve(4) behind an overrun", w.reserve(4), 0);
        expect_eq("dry behind an overrun", w.dry, 1);
        expect_eq("bound stays", w.left(), -5);
    }
    for (int m = 0; m < 3; ++m) {   // the flag reserve raised is cleared by push, and the pushed draws can be reserved
        DgaDrawWindow w = with_left(1);
        expect_eq("reserve(4) of 1 draw", w.reserve(4), 0);
        expect_eq("dry raised", w.dry, 1);
        expect_eq("sticky", (w.reserve(0), w.dry), 1);
        static const double fresh[3] = {0.5, 0.5, 0.5};
        w.push(fresh, 3, 10, (DgaOverrun)m);
        expect("push clears the dry flag", kNames[m], w, 10, {0.25, 0.5, 0.5, 0.5}, false);
        expect_eq("reserve(4) of 4 draws", w.reserve(4), 2);
        expect_eq("still not dry", w.dry, 0);
    }
    {   // a fresh window
        DgaDrawWindow w;
        expect_eq("fresh: end", (long long)w.end(), 0);
        expect_eq("fresh: left", w.left(), 0);
        expect_eq("fresh: reserve(1)", w.reserve(1), 0);
        expect_eq("fresh: dry", w.dry, 1);
    }
}

int main() {
    push_cases();
    reserve_cases();
    std::printf("%s: %d checks, %d failures\n", failures ? "FAILED" : "ok", checks, failures);
    return failures ? 1 : 0;
}

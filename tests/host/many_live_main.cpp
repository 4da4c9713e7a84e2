// Stand-alone check of the chunk plan of the live list and of the cap of a call (pysparselp_amd/csrc/slp_many_plan.h: what
// k_many_live of slp_many.h and slp_many_dga_iterate take from it), built with -fsanitize=address,undefined and run as a child
// process by tests/test_many_live_host.py.  The scatter is restated serially over the plan's own functions -- a lane's count, the
// exclusive prefix of the counts in lane order, a lane's stores -- into a buffer of exactly `count` entries, so a store past the
// end is the sanitizer's; the expected list is the increasing numbers of the set flags, formed without the plan.
#include "slp_many_plan.h"

#include <cstdio>

using namespace slp;

static int failures = 0, checks = 0;

static void expect(const char *what, long long a, long long b, bool ok) {
    ++checks;
    if (ok) return;
    ++failures;
    std::printf("FAIL %s (%lld, %lld)\n", what, a, b);
}

static void expect_eq(const char *what, long long got, long long want) {
    ++checks;
    if (got == want) return;
    ++failures;
    std::printf("FAIL %s: %lld, expected %lld\n", what, got, want);
}

// the ranges of the 1024 lanes tile [0, count) in lane order; a lane past the end is empty
static void tiling(int32_t count) {
    const int32_t per = many_live_per(count);
    expect_eq("per = ceil(count / 1024)", per, ((long long)count + 1023) / 1024);
    int32_t at = 0;
    bool ended = false;
    for (int32_t t = 0; t < kManyLiveLanes; ++t) {
        const ManyLiveRange r = many_live_range(count, t);
        expect("a range starts where the one before ends", count, t, r.lo == at);
        expect("a range does not run backwards or past the end", count, t, r.lo <= r.hi && r.hi <= count);
        expect("a range holds at most `per` LPs", count, t, r.hi - r.lo <= per);
        if (r.hi < count) expect("a lane in front of the end is full", count, t, r.hi - r.lo == per);
        if (ended) expect("a lane past the end is empty at the end", count, t, r.lo == count && r.hi == count);
        if (r.hi == count) ended = true;
        at = r.hi;
    }
    expect_eq("the ranges end at count", at, count);
}

static void scatter(int32_t count, const char *name, const std::vector<char> &flag) {
    const auto live = [&](int32_t k) { return flag[(size_t)k] != 0; };
    std::vector<int32_t> want;
    for (int32_t k = 0; k < count; ++k)
        if (flag[(size_t)k]) want.push_back(k);
    std::vector<int32_t> mine((size_t)kManyLiveLanes), before((size_t)kManyLiveLanes);
    int32_t total = 0;
    for (int32_t t = 0; t < kManyLiveLanes; ++t) {
        mine[(size_t)t] = many_live_count(many_live_range(count, t), live);
        before[(size_t)t] = total;
        total += mine[(size_t)t];
    }
    std::vector<int32_t> out((size_t)count, -1);   // exactly `count` entries
    for (int32_t t = kManyLiveLanes - 1; t >= 0; --t)   // the lanes in any order: their stores do not meet
        many_live_write(many_live_range(count, t), before[(size_t)t], out.data(), live);
    ++checks;
    bool ok = total == (int32_t)want.size();
    for (size_t i = 0; ok && i < want.size(); ++i) ok = out[i] == want[i];
    for (size_t i = want.size(); ok && i < out.size(); ++i) ok = out[i] == -1;
    if (!ok) {
        ++failures;
        std::printf("FAIL scatter, count %d, pattern %s: %d live, expected %zu\n", count, name, total, want.size());
    }
}

static void patterns(int32_t count) {
    const size_t n = (size_t)count;
    std::vector<char> f(n, 0);
    scatter(count, "none", f);
    f.assign(n, 1);
    scatter(count, "all", f);
    f.assign(n, 0);
    for (size_t k = 0; k < n / 2; ++k) f[k] = 1;
    scatter(count, "the first half", f);
    f.assign(n, 0);
    for (size_t k = 0; k < n; k += 2) f[k] = 1;
    scatter(count, "every second", f);
    f.assign(n, 0);
    f[0] = 1;
    scatter(count, "only the first", f);
    f.assign(n, 0);
    f[n - 1] = 1;
    scatter(count, "only the last", f);
    {   // 64 set flags (as many as the list has, below 64) across the boundary of two chunks in the middle of the list
        const int32_t per = many_live_per(count), lanes = (count + per - 1) / per;
        const int64_t edge = (int64_t)per * std::max(1, lanes / 2);   // the first LP of a chunk
        const int64_t lo = std::max<int64_t>(0, edge - 32), hi = std::min<int64_t>(count, lo + 64);
        f.assign(n, 0);
        for (int64_t k = lo; k < hi; ++k) f[(size_t)k] = 1;
        if (lanes > 1) expect("the run straddles a chunk boundary", count, edge, lo < edge && edge < hi);
        scatter(count, "a run of 64 across a chunk boundary", f);
    }
    {   // fixed pseudo-random: a 64-bit linear congruential generator, its top bit
        uint64_t x = 0x9E3779B97F4A7C15ull + (uint64_t)count;
        for (size_t k = 0; k < n; ++k) {
            x = x * 6364136223846793005ull + 1442695040888963407ull;
            f[k] = (char)(x >> 63);
        }
        scatter(count, "pseudo-random", f);
    }
}

// the cap of a call with L live LPs on 256 compute units: many_launch_cap for L workgroups, never more for more of them
static void cap_cases() {
    const int64_t passes = 69, cus = 256, top = kManyMaxItersPerLaunch;   // 69: a pass count that keeps 8192 / (69 r) apart for r = 1 .. 4
    const int64_t ls[] = {1, 256, 257, 512, 1024};
    const int64_t want[] = {118, 118, 59, 59, 29};   // 8192 / 69, 8192 / 138, 8192 / 276
    int64_t last = top + 1;
    for (int i = 0; i < 5; ++i) {
        const int64_t got = many_live_cap(passes, ls[i], cus, top);
        expect_eq("the cap of a call is many_launch_cap of its live LPs", got, many_launch_cap(kManyUnitsPerLaunch, passes, ls[i], cus, top));
        expect_eq("... by hand", got, want[i]);
        expect("the cap does not grow with the live LPs", ls[i], got, got <= last);
        last = got;
        expect_eq("the switch lowers it", many_live_cap(passes, ls[i], cus, 7), 7);
        expect_eq("one iteration per launch", many_live_cap(passes, ls[i], cus, 1), 1);
    }
    for (int64_t l = 1; l < 1100; ++l)
        expect("non-increasing, every L", l, 0, many_live_cap(passes, l + 1, cus, top) <= many_live_cap(passes, l, cus, top));
    expect_eq("no live LP is asked about as one", many_live_cap(passes, 0, cus, top), many_live_cap(passes, 1, cus, top));
}

int main() {
    for (int32_t count : {1, 63, 64, 65, 1023, 1024, 1025, 2047, 2049, 65535}) {
        tiling(count);
        patterns(count);
    }
    cap_cases();
    std::printf("%s: %d checks, %d failures\n", failures ? "FAILED" : "ok", checks, failures);
    return failures ? 1 : 0;
}

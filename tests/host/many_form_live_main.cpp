// Stand-alone check of what a compacted call of the Chambolle-Pock and the ADMM list solver is made of (pysparselp_amd/csrc/
// slp_many_plan.h: the predicate ManyFormLive -- "LP k has form g and is not stopped" -- and many_form_call, the live count and
// the launch cap per form), built with -fsanitize=address,undefined and run as a child process by
// tests/test_many_form_live_host.py.  The expected numbers come from a plain loop over the flags and the forms, and from
// many_launch_cap; the records are fake ones of the two sizes the solvers' records have (the head of ManyCtl plus two or three
// doubles), in arrays of exactly `count` entries, so a read past the end is the sanitizer's.
#include "slp_many_plan.h"

#include <cstdio>

using namespace slp;

static int failures = 0, checks = 0;

static void expect_eq(const char *what, long long got, long long want) {
    ++checks;
    if (got == want) return;
    ++failures;
    std::printf("FAIL %s: %lld, expected %lld\n", what, got, want);
}

// the head of slp_many.h's ManyCtl, restated: slp_many.h itself needs HIP
struct Head {
    int64_t done, stop_iter;
    int32_t stopped, pad;
};
struct Rec40 : Head {   // the size of CpmCtl
    double step, dx;
};
struct Rec48 : Head {   // the size of AdmmmCtl
    double residual, step, dx;
};
static_assert(sizeof(Rec40) == 40 && sizeof(Rec48) == 48, "the two record sizes");

struct Lp {   // a table entry: something in front of the form, as in CpmLp and AdmmmLp
    int64_t col0;
    int32_t n, form;
};

constexpr int64_t kCus = 256, kTop = kManyMaxItersPerLaunch;

// one list: forms and flags -> the helper's counts and caps against a plain loop, and the predicate through the chunk plan
template <class Rec>
static void one_list(const char *name, const std::vector<int32_t> &form, const std::vector<char> &stopped, int64_t passes0, int64_t passes1) {
    const int32_t count = (int32_t)form.size();
    std::vector<Lp> lps((size_t)count);
    std::vector<Rec> rec((size_t)count);
    ManyGroup group[2];
    for (int32_t k = 0; k < count; ++k) {
        lps[(size_t)k] = Lp{7 * (int64_t)k, 60, form[(size_t)k]};
        rec[(size_t)k] = Rec{};
        rec[(size_t)k].done = 100 + k;
        rec[(size_t)k].stop_iter = stopped[(size_t)k] ? 50 : 0;
        rec[(size_t)k].stopped = stopped[(size_t)k];
        rec[(size_t)k].step = 1e-3;   // a word behind the head that is not a flag
        group[form[(size_t)k]].ids.push_back(k);
    }
    group[0].passes = passes0;
    group[1].passes = passes1;
    int64_t want[2] = {0, 0};
    std::vector<int32_t> order[2];
    for (int32_t k = 0; k < count; ++k)
        if (!stopped[(size_t)k]) {
            ++want[form[(size_t)k]];
            order[form[(size_t)k]].push_back(k);
        }
    for (int64_t cap : {kTop, (int64_t)7, (int64_t)1}) {
        const ManyFormCall c = many_form_call(lps, rec.data(), group, kCus, cap);
        for (int g = 0; g < 2; ++g) {
            expect_eq(name, c.live[g], want[g]);
            expect_eq("the cap is many_live_cap of the group's passes and the live count", c.cap[g],
                      many_live_cap(group[g].passes, want[g], kCus, cap));
            expect_eq("... that is many_launch_cap of max(1, live) workgroups", c.cap[g],
                      many_launch_cap(kManyUnitsPerLaunch, group[g].passes, want[g] > 0 ? want[g] : 1, kCus, cap));
        }
    }
    // the predicate as k_many_live uses it: every lane's count, the exclusive prefix in lane order, every lane's stores
    for (int g = 0; g < 2; ++g) {
        const ManyFormLive<Lp, Rec> pred{lps.data(), rec.data(), g};
        std::vector<int32_t> before((size_t)kManyLiveLanes);
        int32_t total = 0;
        for (int32_t t = 0; t < kManyLiveLanes; ++t) {
            before[(size_t)t] = total;
            total += many_live_count(many_live_range(count, t), pred);
        }
        expect_eq("the lanes' counts add up to the live LPs of the form", total, want[g]);
        std::vector<int32_t> out(group[g].ids.size(), -1);   // exactly as many entries as the form has LPs
        for (int32_t t = kManyLiveLanes - 1; t >= 0; --t) many_live_write(many_live_range(count, t), before[(size_t)t], out.data(), pred);
        ++checks;
        bool ok = (size_t)total == order[g].size();
        for (size_t i = 0; ok && i < order[g].size(); ++i) ok = out[i] == order[g][i];
        for (size_t i = order[g].size(); ok && i < out.size(); ++i) ok = out[i] == -1;
        if (!ok) {
            ++failures;
            std::printf("FAIL the list of form %d, %s, count %d\n", g, name, count);
        }
    }
}

static void lists(int32_t count) {
    const size_t n = (size_t)count;
    std::vector<int32_t> form(n, 0);
    std::vector<char> stopped(n, 0);
    const auto both = [&](const char *name) {
        one_list<Rec40>(name, form, stopped, 3, 11);
        one_list<Rec48>(name, form, stopped, 69, 5);
    };
    const auto flags = [&](const char *name) {   // nothing stopped, everything, every second, a pseudo-random half
        stopped.assign(n, 0);
        both(name);
        stopped.assign(n, 1);
        both(name);
        for (size_t k = 0; k < n; ++k) stopped[k] = (char)(k & 1);
        both(name);
        uint64_t x = 0x9E3779B97F4A7C15ull + (uint64_t)count;
        for (size_t k = 0; k < n; ++k) {
            x = x * 6364136223846793005ull + 1442695040888963407ull;
            stopped[k] = (char)(x >> 63);
        }
        both(name);
    };
    form.assign(n, 0);
    flags("all LPs of the lds form");
    form.assign(n, 1);
    flags("all LPs of the global form");
    for (size_t k = 0; k < n; ++k) form[k] = (int32_t)(k & 1);
    flags("the two forms interleaved");
    for (size_t k = 0; k < n; ++k) form[k] = (int32_t)(k % 3 == 1);
    flags("every third LP of the global form");
    // a form with no live LP: every LP of the global form is stopped, the lds form runs on (and the other way round)
    for (size_t k = 0; k < n; ++k) stopped[k] = (char)(form[k] == 1);
    both("the global form has no live LP");
    for (size_t k = 0; k < n; ++k) stopped[k] = (char)(form[k] == 0);
    both("the lds form has no live LP");
}

// the cap at the live counts where the rounds over the compute units change, and at none
static void cap_edges() {
    const int64_t passes = 69;   // keeps 8192 / (69 r) apart for r = 1, 2
    std::vector<Lp> lps(600, Lp{0, 1, 0});
    std::vector<Rec40> rec(600, Rec40{});
    ManyGroup group[2];
    for (int32_t k = 0; k < 600; ++k) group[0].ids.push_back(k);
    group[0].passes = passes;
    const int64_t lives[] = {1, kCus, kCus + 1, 0}, want[] = {118, 118, 59, 118};   // 8192 / 69, 8192 / 138; none: one workgroup's
    for (int i = 0; i < 4; ++i) {
        for (int32_t k = 0; k < 600; ++k) rec[(size_t)k].stopped = k >= lives[i];
        const ManyFormCall c = many_form_call(lps, rec.data(), group, kCus, kTop);
        expect_eq("live", c.live[0], lives[i]);
        expect_eq("the cap by hand", c.cap[0], want[i]);
        expect_eq("the cap of one workgroup's", many_live_cap(passes, 0, kCus, kTop), many_live_cap(passes, 1, kCus, kTop));
        expect_eq("the form without an LP", c.live[1], 0);
        expect_eq("... is clamped to one workgroup's cap", c.cap[1], many_live_cap(group[1].passes, 1, kCus, kTop));
        expect_eq("the switch lowers it", many_form_call(lps, rec.data(), group, kCus, 7).cap[0], 7);
    }
}

int main() {
    for (int32_t count : {1, 2, 65, 1023, 1024, 1025}) lists(count);
    cap_edges();
    std::printf("%s: %d checks, %d failures\n", failures ? "FAILED" : "ok", checks, failures);
    return failures ? 1 : 0;
}

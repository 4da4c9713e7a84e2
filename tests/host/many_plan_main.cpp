// Stand-alone check of the launch planner of the list solvers (pysparselp_amd/csrc/slp_many_plan.h), built with
// -fsanitize=address,undefined and run as a child process by tests/test_many_plan_host.py.  The expected values are literals,
// worked out by hand from the rules: lds when the doubles are at most the limit; the smallest power of two >= want in 64 .. 1024;
// min(cap, max(1, units / (passes * ceil(workgroups / compute units)))).
#include "slp_many_plan.h"

#include <cstdio>
#include <functional>

using namespace slp;

static int failures = 0, checks = 0;

static void expect_eq(const char *what, long long got, long long want) {
    ++checks;
    if (got == want) return;
    ++failures;
    std::printf("FAIL %s: %lld, expected %lld\n", what, got, want);
}

static void expect_ids(const char *what, const std::vector<int32_t> &got, std::vector<int32_t> want) {
    ++checks;
    if (got == want) return;
    ++failures;
    std::printf("FAIL %s: the list of LPs differs\n", what);
}

// f() throws a message that holds every one of `parts` (NULL-terminated)
static void expect_refusal(const char *what, const std::function<void()> &f, std::initializer_list<const char *> parts) {
    ++checks;
    try {
        f();
    } catch (const std::exception &e) {
        const std::string msg = e.what();
        for (const char *p : parts)
            if (msg.find(p) == std::string::npos) {
                ++failures;
                std::printf("FAIL %s: the refusal \"%s\" lacks \"%s\"\n", what, msg.c_str(), p);
                return;
            }
        return;
    }
    ++failures;
    std::printf("FAIL %s: not refused\n", what);
}

static void form_cases() {
    const char *who = "slp_x_many_create", *sw = "SLP_X_MANY_FORM";
    {   // the boundary, nothing forced
        ManyGroup g[2];
        const std::vector<int32_t> f = many_assign_forms({20000, 20001, 5}, 20000, -1, who, sw, "2 n + m", g);
        expect_eq("20000 doubles: lds", f[0], 0);
        expect_eq("20001 doubles: global", f[1], 1);
        expect_eq("5 doubles: lds", f[2], 0);
        expect_ids("the lds list", g[0].ids, {0, 2});
        expect_ids("the global list", g[1].ids, {1});
    }
    {   // global forced on a small LP
        ManyGroup g[2];
        const std::vector<int32_t> f = many_assign_forms({5, 20001}, 20000, 1, who, sw, "2 n + m", g);
        expect_eq("forced global, small", f[0], 1);
        expect_eq("forced global, large", f[1], 1);
        expect_ids("forced global: no lds LP", g[0].ids, {});
        expect_ids("forced global: all LPs", g[1].ids, {0, 1});
    }
    {   // lds forced
        ManyGroup g[2];
        const std::vector<int32_t> f = many_assign_forms({20000}, 20000, 0, who, sw, "2 n + m", g);
        expect_eq("forced lds at the limit", f[0], 0);
        ManyGroup h[2];
        expect_refusal("forced lds beyond the limit", [&] { many_assign_forms({7, 20001}, 20000, 0, who, sw, "2 N + m", h); },
                       {"slp_x_many_create: SLP_X_MANY_FORM=lds, but LP 1 needs 20001 doubles of LDS (2 N + m) and the form holds 20000"});
    }
}

static void width_cases() {
    expect_eq("width(1)", many_width(1, 1024), 64);
    expect_eq("width(64)", many_width(64, 1024), 64);
    expect_eq("width(65)", many_width(65, 1024), 128);
    expect_eq("width(1000)", many_width(1000, 1024), 1024);
    expect_eq("width(1024)", many_width(1024, 1024), 1024);
    expect_eq("width(5000)", many_width(5000, 1024), 1024);
}

static void cap_cases() {
    expect_eq("one workgroup, 2 passes: the cap", many_launch_cap(8192, 2, 1, 256, 1024), 1024);
    expect_eq("257 workgroups on 256 units, 2 passes: 2048, clamped", many_launch_cap(8192, 2, 257, 256, 1024), 1024);
    expect_eq("257 workgroups, 40 passes: 8192 / 80", many_launch_cap(8192, 40, 257, 256, 1024), 102);
    expect_eq("10000 passes: at least 1", many_launch_cap(8192, 10000, 1, 256, 1024), 1);
    expect_eq("KMAX 7", many_launch_cap(8192, 2, 1, 256, 7), 7);
    // no compute units known counts as one: 100 workgroups are 100 rounds, 8192 / (4 * 100) = 20
    expect_eq("0 compute units", many_launch_cap(8192, 4, 100, 0, 1024), 20);
    expect_eq("1 compute unit", many_launch_cap(8192, 4, 100, 1, 1024), 20);
    expect_eq("256 workgroups on 256 units are one round", many_launch_cap(8192, 40, 256, 256, 1024), 204);
}

static void switch_cases() {
    const char *k = "SLP_X_MANY_KMAX", *f = "SLP_X_MANY_FORM";
    unsetenv(k);
    expect_eq("KMAX unset", many_kmax_switch(k, 1024), 1024);
    setenv(k, "", 1);
    expect_eq("KMAX empty", many_kmax_switch(k, 1024), 1024);
    setenv(k, "1", 1);
    expect_eq("KMAX 1", many_kmax_switch(k, 1024), 1);
    setenv(k, "7", 1);
    expect_eq("KMAX 7", many_kmax_switch(k, 1024), 7);
    setenv(k, "5000", 1);
    expect_eq("KMAX 5000 against 1024", many_kmax_switch(k, 1024), 1024);
    for (const char *bad : {"0", "-3", "abc", "7x"}) {
        setenv(k, bad, 1);
        const std::string tail = std::string("must be a positive number of iterations, not ") + bad;
        expect_refusal(bad, [&] { many_kmax_switch(k, 1024); }, {"SLP_X_MANY_KMAX", tail.c_str()});
    }
    unsetenv(k);
    unsetenv(f);
    expect_eq("FORM unset", many_form_switch(f), -1);
    setenv(f, "", 1);
    expect_eq("FORM empty", many_form_switch(f), -1);
    setenv(f, "lds", 1);
    expect_eq("FORM lds", many_form_switch(f), 0);
    setenv(f, "global", 1);
    expect_eq("FORM global", many_form_switch(f), 1);
    setenv(f, "nonsense", 1);
    expect_refusal("FORM nonsense", [&] { many_form_switch(f); }, {"SLP_X_MANY_FORM must be lds or global, not nonsense"});
    unsetenv(f);
}

static void block_cases() {
    // two LPs in one block: LP 0 has rows 0, 1 and columns [0, 3), LP 1 has rows 2, 3, 4 and columns [3, 5)
    const std::vector<ManyRows> lps = {{0, 0, 2, 0, 3}, {1, 2, 5, 3, 5}};
    const ManyBlockText range = {"create", "indptr", "must be non-decreasing", "", false};
    const ManyBlockText local = {"create", "the row pointer of the equality block", "decreases", "the equality block of ", true};
    const std::vector<int64_t> ptr = {0, 2, 3, 3, 5, 6};
    const std::vector<int32_t> idx = {0, 2, 1, 3, 4, 4};
    many_check_block(range, ptr.data(), idx.data(), true, 5, lps);
    ++checks;  // a good block passes (it throws otherwise)
    {
        std::vector<int64_t> p = ptr;
        p[0] = 1;
        expect_refusal("indptr[0] = 1", [&] { many_check_block(range, p.data(), idx.data(), true, 5, lps); },
                       {"create: indptr must start at 0"});
        expect_refusal("indptr[0] = 1, the other wording", [&] { many_check_block(local, p.data(), idx.data(), true, 5, lps); },
                       {"create: the row pointer of the equality block must start at 0"});
    }
    {
        std::vector<int64_t> p = {0, 2, 3, 2, 5, 6};
        expect_refusal("a decreasing pointer", [&] { many_check_block(range, p.data(), idx.data(), true, 5, lps); },
                       {"create: indptr must be non-decreasing"});
        expect_refusal("a decreasing pointer, the other wording", [&] { many_check_block(local, p.data(), idx.data(), true, 5, lps); },
                       {"create: the row pointer of the equality block decreases"});
    }
    expect_refusal("entries without arrays", [&] { many_check_block(range, ptr.data(), nullptr, false, 5, lps); }, {"create: NULL argument"});
    {
        std::vector<int32_t> j = idx;
        j[1] = 3;  // one past LP 0's columns
        expect_refusal("LP 0 reaches into LP 1", [&] { many_check_block(range, ptr.data(), j.data(), true, 5, lps); },
                       {"create: a row of LP 0 has the column index 3 outside the LP's columns [0, 3)"});
    }
    {
        std::vector<int32_t> j = idx;
        j[5] = 2;  // a column of LP 0 in the last row of LP 1
        expect_refusal("LP 1 reaches into LP 0", [&] { many_check_block(range, ptr.data(), j.data(), true, 5, lps); },
                       {"create: a row of LP 1 has the column index 2 outside the LP's columns [3, 5)"});
        expect_refusal("LP 1 reaches into LP 0, the other wording", [&] { many_check_block(local, ptr.data(), j.data(), true, 5, lps); },
                       {"create: a row of the equality block of LP 1 has the column index 2, not local to the LP's 2 columns"});
    }
    {   // LP 1 of three has no rows in the block; a block without any entry needs no entry arrays
        const std::vector<ManyRows> three = {{0, 0, 2, 0, 3}, {1, 2, 2, 3, 4}, {2, 2, 5, 4, 6}};
        const std::vector<int32_t> j = {0, 2, 1, 4, 5, 5};
        many_check_block(range, ptr.data(), j.data(), true, 5, three);
        const std::vector<int64_t> none = {0, 0, 0, 0, 0, 0};
        many_check_block(range, none.data(), nullptr, false, 5, three);
        ++checks;
    }
}

int main() {
    form_cases();
    width_cases();
    cap_cases();
    switch_cases();
    block_cases();
    std::printf("%s: %d checks, %d failures\n", failures ? "FAILED" : "ok", checks, failures);
    return failures ? 1 : 0;
}

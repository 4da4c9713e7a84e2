// The planner's choice of the packets' form (pysparselp_amd/csrc/slp_tall_plan.h: tall_plan_records) on the CPU, built with
// -fsanitize=address,undefined and run as a child process by tests/test_tall_records_plan_host.py.  The growth the rule is held
// against is worked out here from the format's description, packet by packet, never through the header's own size functions:
// a list of len items has, in packet g, a = min(4, len - 8 g) items in slots 0-3 and b = min(4, len - 8 g - 4) in slots 4-7;
// slot-major they take a + b words, as records 4 (if a > 0) + b; items with a value id add a word of fifth bytes for either group
// that is not empty.  Prints "ok: <plans> plans, 0 failures".
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "slp_tall_plan.h"

using namespace slp;

static long g_fail = 0, g_plans = 0;
#define CHECK(c, ...)                                   \
    do {                                                \
        if (!(c)) {                                     \
            ++g_fail;                                   \
            if (g_fail < 30) { printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); } \
        }                                               \
    } while (0)

static long long list_words(long long len, bool dict, bool records) {
    long long words = 0;
    for (long long g = 0; 8 * g < len; ++g) {
        const long long a = std::min<long long>(4, len - 8 * g), b = std::max<long long>(0, std::min<long long>(4, len - 8 * g - 4));
        words += (records ? 4 : a) + b + (dict ? 1 + (b > 0 ? 1 : 0) : 0);
    }
    return words;
}
// n items over 1024 lanes: n % 1024 lists of ceil(n / 1024) items, the rest one shorter
static double growth_of(long long n, bool dict) {
    const long long tau = (n + 1023) / 1024, more = n % 1024 ? n % 1024 : 1024;
    const double rec = (double)(more * list_words(tau, dict, true) + (1024 - more) * list_words(tau - 1, dict, true));
    const double slot = (double)(more * list_words(tau, dict, false) + (1024 - more) * list_words(tau - 1, dict, false));
    return rec / slot - 1.0;
}
static long long items_of(const TallPlanIn &in, const TallPlan &p) {
    const double per_cell = (double)in.nnz / (double)std::max<int64_t>(in.nrow, 1) / (double)p.T;
    return std::max<long long>(1, std::llround((double)std::min<int64_t>(p.R, in.nrow) * per_cell));
}

static TallPlanIn shape(int64_t nrow, int64_t ncol, double density, int D, int64_t cus) {
    TallPlanIn in;
    in.nrow = nrow; in.ncol = ncol; in.D = D; in.cus = cus;
    in.nnz = std::max<int64_t>(1, (int64_t)((double)nrow * (double)ncol * density));
    return in;
}

// the rule on a plan without switch or carry
static void check_rule(const TallPlanIn &in, const TallPlan &p, long *records, long *slot_major) {
    ++g_plans;
    const double gr = growth_of(items_of(in, p), in.D > 0);
    if (in.D <= 0) {   // items with an fp64 value stay slot-major whatever the growth (their kernel is bound by the bytes: measured)
        CHECK(!p.records, "records for fp64 items (%lld items, R %d C %d S %d)", items_of(in, p), p.R, p.C, p.S);
        ++*slot_major;
    } else if (p.records) { CHECK(gr <= 1.0 / 16, "records at a growth of %g (%lld items, R %d C %d S %d)", gr, items_of(in, p), p.R, p.C, p.S); ++*records; }
    else { CHECK(gr > 1.0 / 16, "slot-major at a growth of %g (%lld items, R %d C %d S %d)", gr, items_of(in, p), p.R, p.C, p.S); ++*slot_major; }
}

// the chunks of a chunked matrix in order, the way slp_matrix_chunked_append hands on what the first chunk decided; the copy of A
// (rows chunked) or of A^T (columns chunked: the same row blocks in every chunk).  Returns how many chunks planned records.
static int plan_chunks(int K, int64_t rows, int64_t cols, double density, int D, bool transposed, int env_records, TallPlan *first, std::vector<TallPlan> *all = nullptr) {
    TallPlan p0;
    int nrec = 0;
    int64_t blocks = 0;
    for (int k = 0; k < K; ++k) {
        TallPlanIn in = transposed ? shape(cols, rows / K, density, D, 256) : shape(rows / K, cols, density, D, 256);
        in.env_records = env_records;
        if (!transposed) { in.rows_before = (int64_t)k * (rows / K); in.rows_total = rows; }
        if (k > 0) {
            in.carry_C = p0.C; in.carry_dcap = D > 0 ? p0.dcap : -1; in.carry_records = p0.records ? 1 : 0;
            if (transposed) in.carry_R = p0.R;
            else { in.carry_total = p0.total; in.carry_blocks = blocks; }
        }
        const TallPlan p = tall_plan(in);
        ++g_plans;
        if (k == 0) p0 = p;
        blocks += (in.nrow + p.R - 1) / p.R;
        nrec += p.records ? 1 : 0;
        if (all) all->push_back(p);
    }
    *first = p0;
    return nrec;
}

int main() {
    // ---- the table of DESIGN.md section 3 (ix), from the description --------------------------------------------------------
    CHECK(std::fabs(growth_of(4000, true) - (5120.0 / 5024.0 - 1.0)) < 1e-12 && growth_of(4000, true) < 0.02, "4000 items: %g", growth_of(4000, true));
    CHECK(growth_of(3795, true) <= 1.0 / 16 && growth_of(3794, true) > 1.0 / 16, "lists of four: the threshold is 3795 items (%g, %g)", growth_of(3795, true), growth_of(3794, true));
    CHECK(growth_of(3072, true) == 0.25 && growth_of(2048, true) > 0.25, "mean list <= 3: %g", growth_of(3072, true));
    for (long long n = 5 * 1024; n <= 8 * 1024; n += 1024) CHECK(growth_of(n, true) == 0.0 && growth_of(n, false) == 0.0, "lists of %lld: %g", n / 1024, growth_of(n, true));
    CHECK(growth_of(9 * 1024, true) == 0.25, "lists of exactly 9: %g", growth_of(9 * 1024, true));
    CHECK(growth_of(140, true) == 1.5, "140 items in lists of one: %g", growth_of(140, true));
    // the header's own sizes agree with the description, list by list
    for (unsigned len = 0; len <= 40; ++len)
        for (int dict = 0; dict < 2; ++dict)
            for (int rec = 0; rec < 2; ++rec)
                CHECK((long long)tall_packet_lane_words(len, dict != 0, rec != 0) == list_words(len, dict != 0, rec != 0), "lane words of a list of %u (dict %d, records %d): %u", len,
                      dict, rec, tall_packet_lane_words(len, dict != 0, rec != 0));
    CHECK(kTallRecordGrowth == 1.0 / 16, "the cap: %g", kTallRecordGrowth);

    // ---- the benchmark's LP (BASELINE config 4): 1e7 x 2e7 at 1e-4 in 16 chunks, both orientations, every chunk ----------------
    {
        const double d = 19920432269.0 / 2e14;
        for (int transposed = 0; transposed < 2; ++transposed) {
            TallPlan first;
            std::vector<TallPlan> all;
            const int nrec = plan_chunks(16, 20000000, 10000000, d, 1152, transposed != 0, -1, &first, &all);
            CHECK(nrec == 16, "config 4 (%s): %d of 16 chunks plan records", transposed ? "A^T" : "A", nrec);
            for (const TallPlan &p : all) CHECK(p.R == 13021 && p.C == 3072 && p.S == 1, "config 4 (%s): R %d C %d", transposed ? "A^T" : "A", p.R, p.C);
            // the first chunk by the rule alone: about 4000 items per cell (3983 at the generator's exact density) in lists of four:
            // 5 x 1024 words against n + 1024, + 1.9 % at 4000 items and below + 3 % from 3950
            TallPlanIn in = transposed ? shape(10000000, 1250000, d, 1152, 256) : shape(1250000, 10000000, d, 1152, 256);
            if (!transposed) in.rows_total = 20000000;
            const TallPlan p = tall_plan(in);
            const long long n = items_of(in, p);
            CHECK(p.records && n > 3950 && n < 4050 && std::fabs(growth_of(n, true) - (5120.0 / (double)(n + 1024) - 1.0)) < 1e-12 && growth_of(n, true) < 0.03, "config 4 (%s): %lld items per cell, growth %g", transposed ? "A^T" : "A", n, growth_of(n, true));
            printf("config 4 %s: R %d C %d, %lld items per cell, records grow the cell by %.2f %%\n", transposed ? "A^T" : "A", p.R, p.C, n, 100.0 * growth_of(n, true));
        }
    }
    // ---- 60 000 x 300 000 at 2e-4 in 8 chunks: small cells in lists of one -- slot-major in every chunk, both orientations ------
    for (int D : {3, 1152, 0})
        for (int transposed = 0; transposed < 2; ++transposed) {
            TallPlan first;
            const int nrec = plan_chunks(8, 60000, 300000, 2e-4, D, transposed != 0, -1, &first);
            TallPlanIn in = transposed ? shape(300000, 7500, 2e-4, D, 256) : shape(7500, 300000, 2e-4, D, 256);
            const long long n = items_of(in, first);
            CHECK(nrec == 0, "small cells (%s, D %d): %d of 8 chunks plan records (%lld items per cell)", transposed ? "A^T" : "A", D, nrec, n);
            CHECK(growth_of(n, D > 0) > 1.0, "small cells (%s, D %d): %lld items per cell, growth %g", transposed ? "A^T" : "A", D, n, growth_of(n, D > 0));
        }
    // ---- the sweep: records exactly where the predicted growth is at most 1 / 16 ------------------------------------------------
    {
        const int64_t rows[] = {1000, 7500, 30000, 300000, 1000000, 2500000, 20000000}, cols[] = {1000, 7500, 100000, 300000, 10000000, 50000000};
        const double dens[] = {1e-5, 3e-5, 1e-4, 2e-4, 4.5e-4, 1e-3};
        const int dicts[] = {0, 1, 64, 1152, 2048};
        long records = 0, slot_major = 0, split = 0;
        for (int64_t m : rows)
            for (int64_t n : cols)
                for (double d : dens)
                    for (int D : dicts) {
                        for (int env_C : {0, 4096, 2048, 1024})
                            for (int env_R : {0, 1024, 13021}) {
                                TallPlanIn in = shape(m, n, d, D, 256);
                                in.env_C = env_C; in.env_R = env_R;
                                check_rule(in, tall_plan(in), &records, &slot_major);
                                // the switch forces either form
                                for (int force = 0; force < 2; ++force) {
                                    in.env_records = force;
                                    CHECK(tall_plan(in).records == (force != 0), "SLP_TALL_RECORDS=%d", force);
                                    ++g_plans;
                                }
                            }
                        for (int env_split : {-1, 5}) {   // copies with a strip-range split go through the same rule
                            TallPlanIn in = shape(m, n, d, D, 256);
                            in.env_split = env_split;
                            const TallPlan p = tall_plan(in);
                            if (p.S > 1) ++split;
                            check_rule(in, p, &records, &slot_major);
                        }
                        // a carried form overrides the chunk's own rule; the switch overrides both
                        for (int carried = 0; carried < 2; ++carried) {
                            TallPlanIn in = shape(m, n, d, D, 256);
                            in.carry_C = 3072; in.carry_dcap = D > 0 ? 2048 : -1; in.carry_records = carried;
                            CHECK(tall_plan(in).records == (carried != 0), "carried form %d", carried);
                            in.env_records = 1 - carried;
                            CHECK(tall_plan(in).records == (carried == 0), "the switch against the carried form %d", carried);
                            g_plans += 2;
                        }
                        // ... unless the chunk's item kind differs from the first chunk's (a chunk that fell back to fp64 items behind
                        // a first chunk with a value table, or the other way round): no common launch, so its own rule
                        for (int carried = 0; carried < 2; ++carried) {
                            TallPlanIn in = shape(m, n, d, D, 256), own = in;
                            in.carry_C = 3072; in.carry_dcap = D > 0 ? -1 : 2048; in.carry_records = carried;
                            own.env_C = 3072;   // (the carried width is followed either way)
                            CHECK(tall_plan(in).records == tall_plan(own).records, "carried form %d over another item kind (D %d)", carried, D);
                            if (D == 0) CHECK(!tall_plan(in).records, "fp64 items behind a first chunk with records");
                            ++g_plans;
                        }
                    }
        printf("sweep: %ld plans with records, %ld slot-major, %ld with a strip-range split\n", records, slot_major, split);
        CHECK(records > 200 && slot_major > 200 && split > 50, "the sweep met %ld / %ld / %ld", records, slot_major, split);
    }
    printf("%s: %ld plans, %ld failures\n", g_fail ? "FAILED" : "ok", g_plans, g_fail);
    return g_fail ? 1 : 0;
}

// The geometry planner of the tall-cell format (pysparselp_amd/csrc/slp_tall_plan.h) on the CPU: a sweep over shapes, densities,
// dictionaries and chunkings with the rules every plan has to keep, the geometry with a strip-range split against a copy of the
// code it replaced, and the shapes of the benchmark's LP (BASELINE config 4).  Prints "ok: <plans> plans, 0 failures".
#include <cstdio>
#include <vector>

#include "slp_tall_plan.h"

using namespace slp;

static long g_fail = 0, g_plans = 0;
static bool g_last_has_no_height = false;   // plan_chunks: no R gives the last chunk the row blocks left for it (rows not far above blocks squared)
#define CHECK(c, ...)                                   \
    do {                                                \
        if (!(c)) {                                     \
            ++g_fail;                                   \
            if (g_fail < 30) { printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); } \
        }                                               \
    } while (0)

// ---- the geometry before the planner (tall_geometry and the width loop of tall_build), switches as arguments --------------
static void ref_geometry(int64_t cus_all, int64_t nrow, int64_t T, double per_cell, int64_t block_multiple, int want, int env_r, int *R_out,
                         int *S_out, int64_t rows_before, int64_t rows_total) {
    const int kRmax = 9984;
    const int64_t cus = block_multiple > 0 ? std::min<int64_t>(block_multiple, cus_all) : cus_all;
    const double p2 = 1.0 - exp(-per_cell) * (1.0 + per_cell);
    const int64_t rcap = std::max<int64_t>(1024, std::min<int64_t>(kRmax, p2 > 0.0 ? (int64_t)(900.0 / p2) : kRmax));
    if (rows_total > 0 && rows_before >= 0 && rows_before + nrow <= rows_total && want == 0 && !(env_r > 0)) {
        const int64_t all = cus_all;
        const int64_t total = std::max<int64_t>(1, (int64_t)ceil((double)rows_total / ((double)all * (double)rcap * 0.985))) * all;
        auto upto = [&](int64_t r) { return (int64_t)llround((double)total * (double)r / (double)rows_total); };
        const int64_t blocks = upto(rows_before + nrow) - upto(rows_before);
        if (blocks > 0) {
            const int64_t R = (nrow + blocks - 1) / blocks;
            if (R >= 1024 && R <= rcap && (nrow + R - 1) / R == blocks) { *S_out = 1; *R_out = (int)R; return; }
        }
    }
    if (want != 0 && !(env_r > 0)) {
        const int64_t R = std::min<int64_t>(rcap, std::max<int64_t>(nrow, 1)), B = (nrow + R - 1) / R;
        int64_t S = want > 0 ? want : std::max<int64_t>(1, cus / B);
        S = std::max<int64_t>(1, std::min<int64_t>(S, std::max<int64_t>(1, T / 64)));
        if (S > 1) { *R_out = (int)R; *S_out = (int)S; return; }
    }
    *S_out = 1;
    if (env_r > 0) { *R_out = std::min(env_r, kRmax); return; }
    int64_t k = (nrow + cus * rcap - 1) / (cus * rcap);
    if (k < 1) k = 1;
    int64_t R = (nrow + k * cus - 1) / (k * cus);
    if (R < 1024) R = std::min<int64_t>(1024, std::max<int64_t>(nrow, 1));
    *R_out = (int)std::min<int64_t>(R, rcap);
}

static void ref_plan(const TallPlanIn &in, int *R, int *C, int *S) {
    int cshift = 12;
    double best = 0.0;
    for (int cs = 12; cs >= 10; --cs) {
        const int64_t Tc = (in.ncol + ((int64_t)1 << cs) - 1) >> cs;
        const double pc = (double)in.nnz / (double)in.nrow / (double)Tc;
        int Rc = 0, Sc = 1;
        ref_geometry(in.cus, in.nrow, Tc, pc, in.block_multiple, in.env_split, in.env_R, &Rc, &Sc, in.rows_before, in.rows_total);
        const double n = std::max(1.0, (double)std::min<int64_t>(Rc, in.nrow) * pc), tau = std::ceil(n / 1024);
        const double bytes = in.D > 0 ? 4.0 + 4.0 * std::min(n, 1024.0) * std::ceil(tau / 4.0) / n : 12.0;
        const double cost = 0.393 * bytes + (0.95 + 0.34 * (double)((int64_t)1 << cs) / 4096) * 4000.0 / n;
        if (cs == 12 || cost < best) { best = cost; cshift = cs; }
    }
    if (in.env_C == 4096 || in.env_C == 2048 || in.env_C == 1024) cshift = in.env_C == 4096 ? 12 : (in.env_C == 2048 ? 11 : 10);
    const int64_t Cw = (int64_t)1 << cshift, T = (in.ncol + Cw - 1) / Cw;
    ref_geometry(in.cus, in.nrow, T, (double)in.nnz / (double)in.nrow / (double)T, in.block_multiple, in.env_split, in.env_R, R, S, in.rows_before,
                 in.rows_total);
    *C = (int)Cw;
}

// ---- what every plan keeps ---------------------------------------------------------------------------------------------
static void check_plan(const TallPlanIn &in, const TallPlan &p) {
    ++g_plans;
    CHECK(p.lds_bytes <= 163840, "product kernel LDS %d (R %d C %d dcap %d)", p.lds_bytes, p.R, p.C, p.dcap);
    CHECK(p.build_lds_bytes <= 163840, "builder LDS %d (R %d)", p.build_lds_bytes, p.R);
    CHECK(p.lds_bytes == ((8 * (p.R + 1) + 15) & ~15) + 8 * p.dcap + 16 * p.C, "layout");
    CHECK(p.off_dv % 16 == 0 && p.off_xt % 16 == 0 && p.off_dv >= 8 * (p.R + 1) && p.off_xt == p.off_dv + 8 * p.dcap, "offsets %d %d", p.off_dv, p.off_xt);
    CHECK(p.C % 256 == 0 && p.C >= 1024 && p.C <= 4096, "C %d", p.C);
    CHECK(p.R >= 1 && p.R + 1 < (1 << 14), "R %d", p.R);
    CHECK(p.T == (in.ncol + p.C - 1) / p.C, "T");
    CHECK(in.D > 0 ? (p.dcap >= in.D && p.dcap % 64 == 0 && p.dcap <= 2048) : p.dcap == 0, "dcap %d for D %d", p.dcap, in.D);
    CHECK(p.S >= 1, "S");
    if (p.S > 1) CHECK(p.R <= 9984 && p.dcap == (in.D > 0 ? 2048 : 0) && (p.C == 4096 || p.C == 2048 || p.C == 1024), "split geometry");
}

static TallPlanIn shape(int64_t nrow, int64_t ncol, double density, int D, int64_t cus) {
    TallPlanIn in;
    in.nrow = nrow; in.ncol = ncol; in.D = D; in.cus = cus;
    in.nnz = std::max<int64_t>(1, (int64_t)((double)nrow * (double)ncol * density));
    return in;
}

// the chunks of a chunked matrix, in order, the way slp_matrix_chunked_append hands on the first chunk's decision and the row blocks
// so far; returns whether every chunk took its share and the blocks of all chunks add up to the multiple of the compute units
// the first chunk chose; *blocks: row blocks of all chunks
static bool plan_chunks(const std::vector<int64_t> &sizes, int64_t ncol, double density, int D, int64_t cus, int64_t *blocks, TallPlan *first,
                        int env_C = 0, std::vector<int> *heights = nullptr) {
    int64_t total_rows = 0, before = 0;
    for (int64_t s : sizes) total_rows += s;
    TallPlan p0;
    bool shared = true;
    *blocks = 0;
    g_last_has_no_height = false;
    for (size_t k = 0; k < sizes.size(); ++k) {
        TallPlanIn in = shape(sizes[k], ncol, density, D, cus);
        in.rows_before = before; in.rows_total = total_rows; in.env_C = env_C;
        if (k > 0) { in.carry_C = p0.C; in.carry_dcap = D > 0 ? p0.dcap : -1; in.carry_total = p0.total; in.carry_blocks = *blocks; }
        const TallPlan p = tall_plan(in);
        check_plan(in, p);
        if (k == 0) p0 = p;
        CHECK(p.C == p0.C && p.dcap == p0.dcap, "chunk %zu: C %d dcap %d against the first chunk's %d %d", k, p.C, p.dcap, p0.C, p0.dcap);
        if (p.total <= 0 || p.total != p0.total) shared = false;
        if (heights) heights->push_back(p.R);
        if (k + 1 == sizes.size() && p0.total > *blocks) {   // does any height cut the last chunk into the blocks that are left?
            const int64_t want = p0.total - *blocks, R = (sizes[k] + want - 1) / want;
            g_last_has_no_height = (sizes[k] + R - 1) / R != want;
        }
        *blocks += (sizes[k] + p.R - 1) / p.R;
        before += sizes[k];
    }
    *first = p0;
    return shared && *blocks == p0.total && p0.total % cus == 0;
}

// the same chunks by the rule of before the planner (a 1.5 % margin, every chunk's share rounded on its own): whether every chunk
// took its share (the blocks then add up to a multiple of the compute units)
static bool ref_chunks(const std::vector<int64_t> &sizes, int64_t ncol, double density, int D, int64_t cus) {
    int64_t total_rows = 0, before = 0, blocks = 0;
    for (int64_t s : sizes) total_rows += s;
    for (int64_t s : sizes) {
        TallPlanIn in = shape(s, ncol, density, D, cus);
        in.rows_before = before; in.rows_total = total_rows;
        int R = 0, C = 0, S = 0;
        ref_plan(in, &R, &C, &S);
        blocks += (s + R - 1) / R;
        before += s;
    }
    return blocks % cus == 0;
}

int main() {
    const int64_t rows[] = {1000, 30000, 1000000, 2500000, 20000000}, cols[] = {1000, 100000, 10000000, 50000000};
    const double dens[] = {1e-5, 1e-4, 1e-3};
    const int dicts[] = {0, 1, 64, 1129, 1280, 1281, 2048};
    const int64_t cus = 256;
    long split_cases = 0, legacy_same = 0, chunkings = 0, chunkings_whole = 0;
    for (int64_t m : rows)
        for (int64_t n : cols)
            for (double d : dens)
                for (int D : dicts) {
                    // plain copy, every switch
                    for (int env_C : {0, 4096, 2048, 1024, 1280, 3072, 3584, 5000}) {
                        TallPlanIn in = shape(m, n, d, D, cus);
                        in.env_C = env_C;
                        const TallPlan p = tall_plan(in);
                        check_plan(in, p);
                        if (env_C == 4096 || env_C == 2048 || env_C == 1024 || env_C == 1280 || env_C == 3072 || env_C == 3584)
                            CHECK(p.C == env_C, "SLP_TALL_C=%d gave %d", env_C, p.C);   // (the three widths of before: as before)
                        // where the LDS is not what binds (the table of before fits beside 9984 rows at every width), a forced
                        // width of before gives the row blocks of before
                        int R = 0, C = 0, S = 0;
                        ref_plan(in, &R, &C, &S);
                        if ((env_C == 4096 || env_C == 2048 || env_C == 1024) && R < 9766) { CHECK(p.R == R && p.C == C, "R %d C %d against %d %d", p.R, p.C, R, C); ++legacy_same; }
                    }
                    for (int env_R : {1024, 2048, 9984, 13021, 20000}) {
                        TallPlanIn in = shape(m, n, d, D, cus);
                        in.env_R = env_R;
                        const TallPlan p = tall_plan(in);
                        check_plan(in, p);
                        CHECK(p.R <= env_R && (p.R == env_R || p.R == std::min(tall_lds_rows(p.C, p.dcap), kTallRmax)), "SLP_TALL_R=%d gave %d", env_R, p.R);
                    }
                    // strip-range split: exactly the numbers of before
                    for (int split : {-1, 2, 5})
                        for (int env_C : {0, 2048}) {
                            TallPlanIn in = shape(m, n, d, D, cus);
                            in.env_split = split; in.env_C = env_C;
                            const TallPlan p = tall_plan(in);
                            check_plan(in, p);
                            int R = 0, C = 0, S = 0;
                            ref_plan(in, &R, &C, &S);
                            CHECK((p.S > 1) == (S > 1), "split %d: S %d against %d", split, p.S, S);
                            if (S > 1) { CHECK(p.R == R && p.C == C && p.S == S && p.dcap == (D > 0 ? 2048 : 0), "split: R %d C %d S %d against %d %d %d", p.R, p.C, p.S, R, C, S); ++split_cases; }
                        }
                    // chunks of equal and of unequal size
                    if (m >= 1000000)
                        for (int K : {1, 2, 3, 7, 16}) {
                            std::vector<int64_t> eq((size_t)K, m / K / 2 * 2), un;
                            eq.back() = m - (m / K / 2 * 2) * (K - 1);
                            int64_t left = m;
                            for (int k = 0; k < K; ++k) {   // sizes 1 : 1.5 : 1 : 1.5 ... (even, the rest to the last)
                                int64_t s = k + 1 == K ? left : std::min<int64_t>(left - 2 * (K - 1 - k), (int64_t)((double)m / K * (k % 2 ? 1.2 : 0.8)) / 2 * 2);
                                un.push_back(s);
                                left -= s;
                            }
                            // The blocks of all chunks add up to a multiple of the compute units.  Two exceptions, as before the
                            // planner: cells so dense on the chosen width that the one-row-per-lane rule leaves the 1024-row floor
                            // and nothing above it -- every chunk then takes whole multiples of blocks of 1024 rows -- and a last
                            // chunk that no height cuts into the blocks left (2e7 rows in 6144 blocks: 3256 rows make 6143), which
                            // comes out one block short.
                            for (const std::vector<int64_t> &sizes : {eq, un}) {
                                int64_t blocks = 0;
                                TallPlan first;
                                const bool whole = plan_chunks(sizes, n, d, D, cus, &blocks, &first);
                                ++chunkings;
                                const double per_cell = (double)shape(sizes[0], n, d, D, cus).nnz / (double)sizes[0] / (double)first.T;
                                if (tall_rows_for_lanes(per_cell, kTallRmax) > 1024) {
                                    CHECK(whole || (g_last_has_no_height && blocks + 1 == first.total), "%d chunks of %lld rows x %lld, density %g, D %d: %lld blocks of %lld", K, (long long)m, (long long)n, d, D,
                                          (long long)blocks, (long long)first.total);
                                    ++chunkings_whole;
                                } else {
                                    CHECK(first.R == 1024 && first.total == 0, "dense cells: R %d, %lld blocks planned", first.R, (long long)first.total);
                                }
                            }
                        }
                }
    CHECK(split_cases > 100 && legacy_same > 100, "the sweep met %ld split cases, %ld forced widths of before", split_cases, legacy_same);
    CHECK(chunkings_whole * 3 >= chunkings * 2, "the sweep asserted the multiple on %ld of %ld chunkings", chunkings_whole, chunkings);
    printf("chunkings: %ld, the multiple of the compute units asserted on %ld (the rest: cells at the 1024-row floor)\n", chunkings, chunkings_whole);

    // ---- the benchmark's LP: 1e7 variables x 2e7 rows at 1e-4 in 16 chunks, a dictionary that rounds up to 1152, 256 CUs --------
    {
        const double d = 19920432269.0 / 2e14;
        TallPlanIn at = shape(10000000, 1250000, d, 1152, 256);   // the copy of A^T of one chunk
        const TallPlan pt = tall_plan(at);
        check_plan(at, pt);
        CHECK(pt.C == 3072 && pt.R == 13021 && pt.S == 1, "A^T: C %d R %d", pt.C, pt.R);
        CHECK((10000000 + pt.R - 1) / pt.R == 768, "A^T: 3 x 256 row blocks");
        CHECK(pt.dcap >= 1152 && pt.lds_bytes <= 163840, "A^T: table %d", pt.dcap);
        // A: the chunk rule reaches 96 blocks of 13021 rows per chunk (not 112 of 11161 on 3584 columns)
        int64_t blocks = 0;
        TallPlan first;
        const bool shared = plan_chunks(std::vector<int64_t>(16, 1250000), 10000000, d, 1152, 256, &blocks, &first);
        CHECK(shared && first.dcap == 1152 && first.C == 3072 && first.R == 13021 && first.total == 1536 && blocks == 1536, "A: C %d R %d, %lld blocks of %lld", first.C, first.R,
              (long long)blocks, (long long)first.total);
        printf("config 4: A^T R %d C %d table %d LDS %d; A R %d C %d table %d, %lld row blocks (%lld per chunk)\n", pt.R, pt.C, pt.dcap, pt.lds_bytes,
               first.R, first.C, first.dcap, (long long)blocks, (long long)blocks / 16);
        const int cap = first.dcap;
        // chunks of unequal size still add up to the multiple
        std::vector<int64_t> un;
        for (int k = 0; k < 16; ++k) un.push_back(k % 2 ? 1300000 : 1200000);
        CHECK(plan_chunks(un, 10000000, d, 1152, 256, &blocks, &first) && blocks == 1536, "unequal chunks: %lld blocks", (long long)blocks);
        // a chunk with a share of 38.4 blocks between large ones (38 blocks would be 13158 rows tall, 25 below what the LDS holds; a
        // chunk half its size would not fit that way): 768 + 153 + 39 + 576 blocks
        {
            std::vector<int> hs;
            const bool whole = plan_chunks({10000000, 2000000, 500000, 7500000}, 10000000, d, 1152, 256, &blocks, &first, 0, &hs);
            CHECK(whole && blocks == 1536 && hs.size() == 4 && hs[0] == 13021 && hs[1] == 13072 && hs[2] == 12821 && hs[3] == 13021,
                  "1e7 + 2e6 + 5e5 + 7.5e6 rows: %lld blocks, heights %d %d %d %d", (long long)blocks, hs.size() > 0 ? hs[0] : 0, hs.size() > 1 ? hs[1] : 0,
                  hs.size() > 2 ? hs[2] : 0, hs.size() > 3 ? hs[3] : 0);
        }
        // 2000 random chunkings of the same matrix, 2 to 16 chunks of 0.5 to 1.5 times the mean size: every chunk takes its share,
        // the blocks add up to the multiple of 256 the first chunk chose (1536 where the first chunk has the rows for it, else 1792 or
        // 2048 on wider strips), and no block is more than 5 % below the mean height or above what the LDS holds.  The rule of before
        // (2048 blocks of 9766 rows under a cap of 9984) kept the multiple on all of these as well: no less is asked here.
        {
            unsigned long long state = 0x9E3779B97F4A7C15ull;
            auto uniform = [&]() { state = state * 6364136223846793005ull + 1442695040888963407ull; return (double)(state >> 11) / 9007199254740992.0; };
            long whole = 0, whole_before = 0, at_1536 = 0, short_blocks = 0, tall_blocks = 0;
            for (int trial = 0; trial < 2000; ++trial) {
                const int K = 2 + (int)(uniform() * 15.0);
                std::vector<double> w;
                double sum = 0.0;
                for (int k = 0; k < K; ++k) { w.push_back(0.5 + uniform()); sum += w.back(); }
                std::vector<int64_t> sizes;
                int64_t left = 20000000;
                for (int k = 0; k < K; ++k) {
                    const int64_t sz = k + 1 == K ? left : (int64_t)(2e7 * w[(size_t)k] / sum);
                    sizes.push_back(sz);
                    left -= sz;
                }
                std::vector<int> hs;
                if (plan_chunks(sizes, 10000000, d, 1152, 256, &blocks, &first, 0, &hs)) ++whole;
                if (first.total == 1536 && first.C == 3072) ++at_1536;
                for (int h : hs) {
                    if (first.total > 0 && (double)h < 0.95 * 2e7 / (double)first.total) ++short_blocks;
                    if (h > std::min(tall_lds_rows(first.C, first.dcap), kTallRmax)) ++tall_blocks;
                }
                if (ref_chunks(sizes, 10000000, d, 1152, 256)) ++whole_before;
            }
            printf("random chunkings of config 4: %ld of 2000 add up to the multiple (%ld: 1536 blocks on 3072 columns); the rule of before: %ld\n", whole,
                   at_1536, whole_before);
            CHECK(whole == 2000 && whole >= whole_before, "random chunkings: %ld whole, %ld before", whole, whole_before);
            CHECK(short_blocks == 0 && tall_blocks == 0, "random chunkings: %ld short chunks, %ld too tall", short_blocks, tall_blocks);
        }
        // a later chunk whose dictionary outgrows the carried capacity: the whole table
        TallPlanIn late = shape(1250000, 10000000, d, cap + 1, 256);
        late.carry_C = 3072; late.carry_dcap = cap; late.carry_total = 1536; late.carry_blocks = 96; late.rows_before = 1250000; late.rows_total = 20000000;
        const TallPlan pl = tall_plan(late);
        check_plan(late, pl);
        CHECK(pl.dcap == 2048 && pl.C == 3072 && pl.R == 12255 && pl.total == 1536, "late chunk: table %d C %d R %d", pl.dcap, pl.C, pl.R);
        // forced back to 4096 columns: the geometry of before (9766 rows, 128 blocks per chunk)
        CHECK(plan_chunks(std::vector<int64_t>(16, 1250000), 10000000, d, 1152, 256, &blocks, &first, 4096) && first.R == 9766 && blocks == 2048,
              "A on 4096 columns: R %d, %lld blocks", first.R, (long long)blocks);
    }
    // the whole table leaves fewer rows; fp64 items gain its 16 KB
    {
        TallPlanIn in = shape(13021, 6145, 1e-4, 2048, 256);
        in.env_R = 13021; in.env_C = 3072;
        TallPlan p = tall_plan(in);
        CHECK(p.dcap == 2048 && p.R == 12287, "2048 values: R %d", p.R);
        in.D = 1152;
        p = tall_plan(in);
        CHECK(p.R == 13021 && p.dcap >= 1152, "1152 values: R %d table %d", p.R, p.dcap);
        in.D = 0;
        p = tall_plan(in);
        CHECK(p.R == 13021 && p.dcap == 0 && p.off_xt == p.off_dv, "fp64 items: R %d", p.R);
    }
    printf("%s: %ld plans, %ld failures\n", g_fail ? "FAILED" : "ok", g_plans, g_fail);
    return g_fail ? 1 : 0;
}

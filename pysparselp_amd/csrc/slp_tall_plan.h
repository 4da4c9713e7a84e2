// slp_tall_plan.h -- the geometry of a tall-cell copy (slp_tall.hip): rows per block R, columns per strip C, strip ranges S, the
// capacity of the value table and where the three LDS areas of the product kernel (slp_tall_spmv.hip) lie.  Pure host code: no
// HIP, no device buffer, no context, no environment -- the compute units and the SLP_TALL_* switches are arguments.
//
// The product kernel's workgroup keeps in LDS
//   the running sums of its R rows and the scratch cell      8 (R + 1) bytes, rounded up to 16
//   the value table                                          8 dcap bytes  (dcap: D rounded up to 64 entries, then whatever the sums
//                                                                           of the tallest planned block leave; 0 with fp64 items)
//   two x-tiles                                              16 C bytes
// and all of it has to fit 160 KB.  The tiles start at off_xt; inside the off_xt bytes in front of them the kernel puts the scratch
// cell first, the table behind it and the sums behind the table (slp_tall_item.h: an item's sum field counts from LDS address 0) --
// off_dv is the size of the sums' share, not where the table lies.  The per-cell frame of the kernel moves 8 C bytes of x for the R C density items of a cell,
// 8 / (R density) bytes per item whatever C is: at a given cell size the tile's share falls with taller blocks on narrower
// strips, so the table takes what its dictionary needs, not a fixed 16 KB, and C is any multiple of 256 (the item's 12-bit
// column field needs C <= 4096).  The builder's workgroup needs 10 bytes per row beside kTallBuildFixed bytes of its own: that
// bounds R as well (kTallRmax).
//
// Strip-range split (S > 1, SLP_TALL_SPLIT): the geometry of before this header -- strips of 4096, 2048 or 1024 columns, at
// most kTallRmaxSplit rows, a 2048-entry table.  The ranges' boundaries are strip boundaries, and the partial sums of a row
// are added range by range: another strip width would re-associate them.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "slp_tall_item.h"

namespace slp {

constexpr int kTallLdsBytes = 160 * 1024;   // LDS of one workgroup
constexpr int kTallPlanLanes = 1024;        // lanes a cell's rows are dealt to (kTallT)
constexpr int kTallDictMax = 2048;          // most entries of a value table (11-bit value id)
constexpr int kTallCmax = 4096, kTallCmin = 1024, kTallCstep = 256;
constexpr int kTallBuildFixed = 29440;      // LDS of k_tall_build beside its three per-row arrays (asserted there)
constexpr int kTallBuildRowBytes = 10;
// most rows of a row block: the builder's LDS (the product kernel's allows more on narrow strips); row field: R + 1 < 2^14
constexpr int kTallRmax = 13312;
constexpr int kTallRmaxSplit = 9984;        // ... of a copy with a strip-range split
static_assert(kTallBuildFixed + kTallBuildRowBytes * kTallRmax <= kTallLdsBytes && kTallRmax + 1 < (1 << 14), "tall cells: row blocks");
constexpr double kTallListMax = 3.91;       // mean list length of the operating point the cost model was fitted at

struct TallPlanIn {
    int64_t nrow = 0, ncol = 0, nnz = 0;   // of the copy (the transposed copy: columns of A, rows of A)
    int D = 0;                             // entries of the value dictionary (0: fp64 items)
    int64_t cus = 1;                       // compute units
    int64_t block_multiple = 0;            // row blocks come in multiples of this (0: the compute units)
    int64_t rows_before = 0, rows_total = 0;   // a chunk of a chunked matrix whose chunks run in one grid
    int env_R = 0, env_C = 0, env_split = 0;   // SLP_TALL_R, SLP_TALL_C, SLP_TALL_SPLIT (0: unset)
    // what the first chunk of the chunked matrix decided (0 / -1: nothing carried)
    int carry_C = 0, carry_dcap = -1, carry_R = 0;
    int64_t carry_total = 0;
    int64_t carry_blocks = 0;              // row blocks the chunks in front came out with (beside carry_total)
    int env_records = -1;                  // SLP_TALL_RECORDS: 0 / 1 forces the packets' form (-1: unset)
    int carry_records = -1;                // the form of the first chunk's copy (-1: nothing carried)
};

struct TallPlan {
    int R = 0, C = 0, S = 1, dcap = 0;
    bool records = false;      // the packets' form: the first four list positions as one 16-byte record per lane (slp_tall_item.h)
    int64_t T = 0;             // strips
    int64_t total = 0;         // row blocks of all chunks together, when the chunk took its share of them (else 0)
    int off_dv = 0, off_xt = 0, lds_bytes = 0;   // product kernel: bytes of the sums' share, byte offset of the x-tiles, all of its LDS
    int build_lds_bytes = 0;   // the builder's need at this R
};

inline int tall_table_capacity(int D) { return D <= 0 ? 0 : std::min(kTallDictMax, (D + 63) / 64 * 64); }
inline int tall_sums_bytes(int R) { return ((R + 1) * 8 + 15) & ~15; }
// most rows the product kernel's LDS holds beside a table of dcap entries and tiles of C columns
inline int tall_lds_rows(int C, int dcap) { return (((kTallLdsBytes - 8 * dcap - 16 * C) / 8) & ~1) - 1; }
inline void tall_plan_layout(TallPlan &p) {
    p.off_dv = tall_sums_bytes(p.R);
    p.off_xt = p.off_dv + 8 * p.dcap;
    p.lds_bytes = p.off_xt + 16 * p.C;
    p.build_lds_bytes = kTallBuildFixed + kTallBuildRowBytes * p.R;
}
// rows with two or more entries in a cell fit one per lane: R P(Poisson(per_cell) >= 2) <= 900
inline int64_t tall_rows_for_lanes(double per_cell, int64_t cap) {
    const double p2 = 1.0 - std::exp(-per_cell) * (1.0 + per_cell);
    return p2 > 0.0 ? std::min<int64_t>(cap, (int64_t)(900.0 / p2)) : cap;
}

// ---- the geometry with a strip-range split in reach (SLP_TALL_SPLIT != 0): unchanged ------------------------------------
inline void tall_plan_split_geometry(const TallPlanIn &in, int64_t T, double per_cell, int *R_out, int *S_out) {
    const int64_t cus = in.block_multiple > 0 ? std::min<int64_t>(in.block_multiple, in.cus) : in.cus;
    const int64_t rcap = std::max<int64_t>(1024, tall_rows_for_lanes(per_cell, kTallRmaxSplit));
    if (in.env_R <= 0) {
        const int64_t R = std::min<int64_t>(rcap, std::max<int64_t>(in.nrow, 1)), B = (in.nrow + R - 1) / R;
        int64_t S = in.env_split > 0 ? in.env_split : std::max<int64_t>(1, cus / B);
        S = std::max<int64_t>(1, std::min<int64_t>(S, std::max<int64_t>(1, T / 64)));  // at least 64 strips per range
        if (S > 1) { *R_out = (int)R; *S_out = (int)S; return; }
    }
    *S_out = 1;
    if (in.env_R > 0) { *R_out = std::min(in.env_R, kTallRmaxSplit); return; }
    int64_t k = (in.nrow + cus * rcap - 1) / (cus * rcap);
    if (k < 1) k = 1;
    int64_t R = (in.nrow + k * cus - 1) / (k * cus);
    if (R < 1024) R = std::min<int64_t>(1024, std::max<int64_t>(in.nrow, 1));
    *R_out = (int)std::min<int64_t>(R, rcap);
}

// what the product kernel is predicted to pay per stored entry (fitted on the 2.5e6-row slices, ms per 2.49e9 entries: 0.393
// per byte of the items, 0.95 + 0.34 C / 4096 per cell of 4000 entries; 10 % low where a cell's lists are five items long)
inline double tall_plan_cost(int64_t nrow, int R, int C, double per_cell, bool dict) {
    const double n = std::max(1.0, (double)std::min<int64_t>(R, nrow) * per_cell), tau = std::ceil(n / kTallPlanLanes);
    const double bytes = dict ? 4.0 + 4.0 * std::min(n, (double)kTallPlanLanes) * std::ceil(tau / 4.0) / n : 12.0;
    return 0.393 * bytes + (0.95 + 0.34 * (double)C / kTallCmax) * 4000.0 / n;
}
// ... so a width the model was not fitted on (none of 4096, 2048, 1024) is a candidate only while the mean list of its cells stays
// at or below that of the operating point, 3.91 items; the three fitted widths compete as they always did
inline bool tall_plan_admits(int64_t nrow, int R, int C, double per_cell) {
    if (C == 4096 || C == 2048 || C == 1024) return true;
    return (double)std::min<int64_t>(R, nrow) * per_cell / kTallPlanLanes <= kTallListMax;
}

// ---- the packets' form (slp_tall_item.h) ------------------------------------------------------------------------------------
// Records save the product kernel three of a packet's four loads of slots 0-3 (and their scalar offsets and ends of range) and
// cost a zero word for every list position below four that a lane of slot 0 lacks.  The rule is a condition on the copy's SIZE,
// not a tuned speed: records iff the planned cell -- n = min(R, nrow) x per_cell items dealt in balance over the 1024 lanes --
// grows by at most kTallRecordGrowth.  The two measurements there are put break-even at 11-14 % growth (+2.2 % bytes came with
// -2.3 % time on the benchmark's LP; bytes alone cost about 0.2 % of time per % of bytes: DESIGN.md section 3 (ix)); 1/16 is
// half of that.  It may be lowered; it may not be raised without an A/B at the new edge.
// Lists of four from >= 3795 items and mean lists of 5-8 take records; mean lists <= 3, lists of exactly 9 (the second packet's
// record holds one item: + 25 %) and the small cells of a finely chunked matrix (~140 items in lists of one: + 150 %, more bytes
// than the CSR) stay slot-major.
constexpr double kTallRecordGrowth = 1.0 / 16;
inline int64_t tall_plan_cell_items(int64_t nrow, int R, double per_cell) {
    return std::max<int64_t>(1, std::llround((double)std::min<int64_t>(R, nrow) * per_cell));
}
// predicted words of the planned cell in the one form over the other, minus one
inline double tall_plan_record_growth(int64_t nrow, int R, double per_cell, bool dict) {
    const uint64_t n = (uint64_t)tall_plan_cell_items(nrow, R, per_cell);
    return (double)tall_packet_balanced_words(n, kTallPlanLanes, dict, true) / (double)tall_packet_balanced_words(n, kTallPlanLanes, dict, false) - 1.0;
}
// Items with an fp64 value never take records by the rule: their kernel runs at 0.77-0.78 of the HBM peak, where the records'
// bytes cost what they weigh -- measured on the benchmark's LP with the dictionary ruled out, 4.88 / 4.78 ms per product
// slot-major against 5.39 / 5.34 ms with records (+ 2.9 % bytes, + 10-12 % time).  The switch reaches
// them.
// The switch, then what the first chunk of a chunked matrix decided (one launch over all chunks runs one kernel), then the rule
inline bool tall_plan_records(const TallPlanIn &in, int R, double per_cell, bool dict) {
    if (in.env_records >= 0) return in.env_records != 0;
    // (a chunk whose item kind differs from the first chunk's -- carry_dcap >= 0: that one had a value table -- cannot share its
    // launch anyway, tall_fuse: it goes by its own rule)
    if (in.carry_records >= 0 && dict == (in.carry_dcap >= 0)) return in.carry_records != 0;
    return dict && tall_plan_record_growth(in.nrow, R, per_cell, dict) <= kTallRecordGrowth;
}

inline bool tall_width_ok(int c) { return c >= kTallCmin && c <= kTallCmax && c % kTallCstep == 0; }

// R of a copy without a split on strips of C columns; *total: the row blocks of the whole chunked matrix when the chunk takes
// its share of them; *rcap_out: the most rows the choice was made against
inline int tall_plan_rows(const TallPlanIn &in, int C, int dcap, double per_cell, int64_t *total_out, int64_t *rcap_out) {
    *total_out = 0;
    const int64_t hard = std::min<int64_t>(tall_lds_rows(C, dcap), kTallRmax);   // what the two kernels' LDS holds
    const int64_t rcap = std::max<int64_t>(1024, tall_rows_for_lanes(per_cell, hard));
    *rcap_out = rcap;
    if (in.env_R > 0) return (int)std::min<int64_t>(in.env_R, hard);
    if (in.carry_R > 0 && in.carry_R <= hard) return in.carry_R;
    if (in.rows_total > 0 && in.rows_before >= 0 && in.rows_before + in.nrow <= in.rows_total && in.env_split == 0) {
        // The chunk brings its SHARE of a multiple of the compute units of row blocks.  The first chunk settles the multiple: the
        // smallest whose mean height h leaves room for the rounding of a share of this chunk's size (a share is off by less than
        // one block: a chunk of n rows comes out at most h / (1 - h / n) + 1 rows tall).  Every chunk then takes the blocks that
        // bring the chunks so far up to their cumulative share, rounded down -- counted from what the chunks in front really took
        // (carry_blocks), and never fewer than its rows need at rcap rows a block: a chunk too small for the rounding of its
        // share (or one with a larger table) takes a block more, and the chunks behind it, with more blocks to spread the
        // difference over, take one less.  Rounding down keeps the count behind the exact share, so the last chunk, which
        // takes what is left, has blocks to spare: the blocks of all chunks add up to the multiple unless the last chunk is
        // the one that cannot give way.
        int64_t total = in.carry_total;
        if (total <= 0) {
            int64_t k = std::max<int64_t>(1, (in.rows_total + in.cus * rcap - 1) / (in.cus * rcap));
            for (int tries = 0; tries < 2; ++tries, ++k) {
                const double h = (double)in.rows_total / (double)(k * in.cus);
                if (tries == 1 || ((double)in.nrow > h && h / (1.0 - h / (double)in.nrow) + 1.0 <= (double)rcap)) break;
            }
            total = k * in.cus;
        }
        auto upto = [&](int64_t r) { return (int64_t)((__int128)total * r / in.rows_total); };
        const int64_t before = in.carry_total > 0 ? in.carry_blocks : upto(in.rows_before);
        const int64_t blocks = std::max<int64_t>({upto(in.rows_before + in.nrow) - before, (in.nrow + rcap - 1) / rcap, 1});
        const int64_t R = (in.nrow + blocks - 1) / blocks;
        if (R >= 1024) { *total_out = total; return (int)R; }
    }
    const int64_t cus = in.block_multiple > 0 ? std::min<int64_t>(in.block_multiple, in.cus) : in.cus;
    int64_t k = (in.nrow + cus * rcap - 1) / (cus * rcap);
    if (k < 1) k = 1;
    int64_t R = (in.nrow + k * cus - 1) / (k * cus);
    if (R < 1024) R = std::min<int64_t>(1024, std::max<int64_t>(in.nrow, 1));  // small matrices: fewer, still tall blocks
    return (int)std::min<int64_t>(R, rcap);
}

inline TallPlan tall_plan(const TallPlanIn &in) {
    TallPlan best;
    const bool dict = in.D > 0;
    const double per_row = (double)in.nnz / (double)std::max<int64_t>(in.nrow, 1);
    if (in.env_split != 0) {
        // the three widths, 9984 rows, the whole table
        int C = kTallCmax;
        double bc = 0.0;
        for (int c = kTallCmax; c >= kTallCmin; c /= 2) {
            const int64_t T = (in.ncol + c - 1) / c;
            int R = 0, S = 1;
            tall_plan_split_geometry(in, T, per_row / (double)T, &R, &S);
            const double cost = tall_plan_cost(in.nrow, R, c, per_row / (double)T, dict);
            if (c == kTallCmax || cost < bc) { bc = cost; C = c; }
        }
        if (in.env_C == 4096 || in.env_C == 2048 || in.env_C == 1024) C = in.env_C;
        const int64_t T = (in.ncol + C - 1) / C;
        int R = 0, S = 1;
        tall_plan_split_geometry(in, T, per_row / (double)T, &R, &S);
        if (S > 1) {
            best.R = R; best.C = C; best.S = S; best.T = T; best.dcap = dict ? kTallDictMax : 0;
            best.records = tall_plan_records(in, R, per_row / (double)T, dict);
            tall_plan_layout(best);
            return best;
        }
    }
    // A table the carried capacity cannot hold: the whole table (the composite then runs its chunks launch by launch)
    int dcap = tall_table_capacity(in.D);
    if (dict && in.carry_dcap >= 0) dcap = in.D <= in.carry_dcap ? in.carry_dcap : kTallDictMax;
    const int forced = in.carry_C > 0 && tall_width_ok(in.carry_C) ? in.carry_C : (tall_width_ok(in.env_C) ? in.env_C : 0);
    double bc = 0.0;
    int keep = 0;   // rows the sums keep room for
    for (int c = kTallCmax; c >= kTallCmin; c -= kTallCstep) {
        if (forced && c != forced) continue;
        const int64_t T = (in.ncol + c - 1) / c;
        const double pc = per_row / (double)T;
        int64_t total = 0, rcap = 0;
        const int R = tall_plan_rows(in, c, dcap, pc, &total, &rcap);
        if (!forced && !tall_plan_admits(in.nrow, R, c, pc)) continue;
        const double cost = tall_plan_cost(in.nrow, R, c, pc, dict);
        if (best.C == 0 || cost < bc) {
            bc = cost;
            best.R = R; best.C = c; best.S = 1; best.T = T; best.total = total; best.dcap = dcap;
            keep = in.env_R > 0 || (in.rows_total == 0 && in.block_multiple == 0) ? R : (int)rcap;
        }
    }
    // What the sums leave of the LDS goes to the table (a later chunk's dictionary may be a little larger than the first one's).
    // The sums of a copy whose row blocks are settled chunk by chunk keep all the rows those were planned against: the table
    // never lowers the height the later chunks may reach.
    if (dict && in.carry_dcap < 0) {
        const int room = (kTallLdsBytes - tall_sums_bytes(std::max(keep, best.R)) - 16 * best.C) / 8;
        best.dcap = std::min(kTallDictMax, std::max(best.dcap, room / 64 * 64));
    }
    best.records = tall_plan_records(in, best.R, per_row / (double)best.T, dict);
    tall_plan_layout(best);
    return best;
}

}  // namespace slp

// slp_tall.h -- the tall-cell format shared by its builder (slp_tall.hip) and its product kernel (slp_tall_spmv.hip);
// the format itself is described at the top of slp_tall.hip.
#pragma once
#include "slp_common.h"
#include "slp_tall_item.h"

namespace slp {

constexpr int kTallC = 4096;       // most columns per strip (12-bit column inside the strip); 32 KB of x
constexpr int kTallT = 1024;       // threads per workgroup = lanes a cell's rows are dealt to
constexpr int kTallSlots = 8;      // list positions per packet
// The product kernel's prefetch depths, in packets (slp_tall_spmv.hip).  Items -- payload words, fp64 values -- are loaded
// kTallDepth packets before they are taken, headers 2 x kTallDepth; the x-tile pieces a packet carries for the next cell
// kTallTileDepth <= kTallDepth packets before they are stored (their source column waits in the header ring either way).
// kTallAhead: the first four items of the NEXT packet are decoded and their values read from the table in front of its barrier.
// Kernel-lab builds (`make variant`, -DSLP_LAB_VARIANT) may override the three; the shipped text has no switch.
#if defined(SLP_LAB_VARIANT) && defined(SLP_TALL_DI)
constexpr int kTallDepth = SLP_TALL_DI;
#else
constexpr int kTallDepth = 4;      // packets of payload in flight per lane; headers run 2 x this ahead
#endif
#if defined(SLP_LAB_VARIANT) && defined(SLP_TALL_DT)
constexpr int kTallTileDepth = SLP_TALL_DT;
#else
constexpr int kTallTileDepth = 2;   // (a tile comes from L2 / MALL -- x is re-read by every row block -- not from the HBM stream the items' depth is sized for)
#endif
#if defined(SLP_LAB_VARIANT) && defined(SLP_TALL_AHEAD)
constexpr bool kTallAhead = SLP_TALL_AHEAD != 0;
#else
constexpr bool kTallAhead = true;
#endif
static_assert(kTallTileDepth >= 1 && kTallTileDepth <= kTallDepth, "a tile's source column is taken from the header ring: its packet's header must be unpacked");
constexpr int tall_lcm(int a, int b) { int m = a; while (m % b) m += a; return m; }
// packets per turn of the kernel's unrolled loop (every ring index a constant): a workgroup's packets are padded to whole turns
constexpr int kTallTurn = tall_lcm(2 * kTallDepth, kTallTileDepth);
constexpr int kTallBuckets = 6;    // rows are ordered by min(entries in the cell, 6), descending
// (kTallIdBits = 11, kTallColBits = 12, kTallRowBits = 14 and the stored item: slp_tall_item.h)
constexpr int kTallCellShift = kTallIdBits + kTallColBits + kTallRowBits;  // sort key: cell | row | column | id
static_assert(kTallBuckets * 32 == 3 * kWave, "k_tall_build scans the (count, bank class) buckets three per lane of one wave");
static_assert(1 + kTallDictMax + kTallRmax <= (1 << kTallRowBits), "an item's sum field: scratch cell, value table, the block's rows (slp_tall_item.h)");
static_assert(kTallRmax + 1 < (1 << kTallRowBits) && kTallC == (1 << kTallColBits) && kTallDictMax == (1 << kTallIdBits), "tall geometry");
static_assert(kTallT == kTallPlanLanes && kTallC == kTallCmax, "the planner's constants (slp_tall_plan.h)");
// LDS of the product kernel -- sums (+ the scratch cell) + value table + two x-tiles -- with a strip-range split; every other
// copy's layout is the planner's (slp_tall_plan.h: tall_plan_layout)
static_assert((kTallRmaxSplit + 1) * 8 + kTallDictMax * 8 + 2 * kTallC * 8 <= kTallLdsBytes, "tall cells: LDS budget");

constexpr unsigned int kPktNewCell = 0x80000000u;  // first packet of a cell: barrier, then the other x-tile
constexpr unsigned int kNoTile = 0x7fffffffu;
constexpr unsigned int kOob = 0xffffff00u;         // byte offset past every buffer descriptor: the load returns 0, no request

// 32-byte packet header (8 dwords; lane l & 7 of a wave loads dword l & 7)
struct TallPkt {
    unsigned int off;     // payload offset of the packet inside its row block (words)
    unsigned int xsrc;    // kPktNewCell | first column of the strip whose x-tile this packet carries for the NEXT cell (or kNoTile)
    unsigned int c[4];    // c[i] = w[2i] | w[2i+1] << 16,  w[k] = lanes whose list is longer than slot k of this packet
    unsigned int strip;   // strip index (diagnostics)
    unsigned int pad;
};
static_assert(sizeof(TallPkt) == 32, "packet header");

__host__ __device__ inline unsigned long long tall_value_key(unsigned long long bits) {  // as value_key() of slp_strip.hip
    return (bits >> 63) ? ~bits : (bits | 0x8000000000000000ull);
}

}  // namespace slp

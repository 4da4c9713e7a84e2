// slp_tall_spmv.hip -- the product kernel over tall cells (format, builder and the reasons for both: slp_tall.hip).
// Reference products: `a * x` / `y * a` of ChambollePockPPD.py:206,216,235,240 and ADMM.py:148,220,262.
// A translation unit of its own because it is compiled with another instruction-scheduling strategy than the rest of the
// library (Makefile: -mllvm -amdgpu-sched-strategy=max-ilp; measured on the 2.5e6 x 1e7 slice: A x 3.89 -> 3.73 ms, A^T y
// 3.91 -> 3.77 ms; the same flag makes the sort and the strip kernels slower).
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include "slp_common.h"
#include "slp_kernels.h"
#include "slp_tall.h"

namespace slp {


// ---- the product -------------------------------------------------------------------------------------------------------
template <bool DICT>
struct TallRegs {
    unsigned int lo[kTallSlots];
    unsigned int hi[DICT ? 2 : 1];
    double val[DICT ? 1 : kTallSlots];
};
// this lane's 16-byte pieces of an x-tile: a ring of its own (kTallTileDepth), shorter than the items'
struct TallTile {
    double x[4];
};
// the first four items of a packet, decoded: LDS address of the running sum, column, the value (DICT: read from the table)
struct TallAheadItems {
    unsigned int sa[4], col[4];
    double v[4];
};

// DICT: depth 4 (20 KB of payload per packet); fp64 entries: depth 2 (48 KB per packet, 16 more registers per packet)
// THE PIPELINE of a wave, packet j of its stream (constants: slp_tall.h; measurements: DESIGN.md section 3 (x)):
//   header of packet j + 2 depth     loaded (one dword per lane)                       behind packet j's items
//   header of packet j + depth       unpacked to scalars; its tile word and fifth-item  behind packet j's first four items
//                                    width wait in rings of `depth` scalars (xwq, c4q)
//   items of packet j + depth        loaded into the item ring (regs[depth])            first four: with the unpack; rest: behind all items
//   x-tile pieces of packet          loaded into a ring of their OWN (tiles[tile depth], behind packet j's items; the tile word comes
//     j + tile depth                 tile depth = 2 <= depth) -- the tile comes from    from the header ring: no header is read twice
//                                    L2 / MALL, its lead need not be the HBM stream's
//   first four items of packet j + 1 DICT: decoded (sum address, column, value offset)  behind packet j's first four sum stores, IN FRONT
//                                    and their four values read from the table, held    of packet j + 1's barrier (`ahead`)
//                                    in 16 registers
//   packet j                         [barrier if it opens a cell] tile stores, sum reads and x gathers of the items taken ahead,
//                                    chain, sum stores; then the second group of four, whole, where a wave has fifth items
// Loads complete in issue order (vmcnt), so the wait for a tile issued `tile depth` steps ago also covers every item load issued
// before it: with tile depth 2 the loop waits at vmcnt(5 .. 9) where depth 4 for both waited at vmcnt(15 .. 17) -- an item has had
// tile depth + 1 steps to land instead of depth; measured no slower (config 4), and the 16 registers pay for the items held ahead.
// fp64 entries keep one depth (2) for both and take nothing ahead: those bodies are the instructions they were.
// POW (fp64 entries only): every stored value v enters as |v|^pw * 1.0 -- the sums behind the Chambolle-Pock preconditioners
// (slp_cp.hip, strip_spmv_abs_pow) over a copy without a value table; the same chain of additions as the CSR walk.
// A workgroup runs `nseg` packet streams one after the other over ONE set of running sums (descriptor of segment s of workgroup v:
// wgs[s * gridDim.x + v]): nseg = 1 for a row block of an ordinary copy -- and for the row blocks of ALL chunks of a chunked
// matrix in one grid (A x in one launch); nseg = the chunks for the copy of A^T of a chunked matrix, where the workgroup of a
// column block walks chunk 0, 1, ... in order and the column sums simply stay in LDS between them (A^T y in one launch: the chain
// of additions of the unchunked product, as the chunk-by-chunk launches formed it through `out`).
// C: columns per strip = doubles of an x-tile: a run-time multiple of 256 up to 4096 (slp_tall_plan.h: the width whose cells
// the kernel is predicted to walk fastest; items keep their 12-bit column field).
// LDS: one dynamic block of the size the planner laid out for the copy's R, dictionary and C (slp_tall_plan.h), the same for every
// workgroup of a launch; inside it, from LDS address 0 (the kernel has no other LDS, checked once below):
//   [scratch cell: 8 bytes] [value table: `dcap` doubles from byte 8] [running sums of the block's rows] ... [two x-tiles from double `oxt`]
// An item's SUM FIELD is the index of its running sum among these doubles (1 + dcap + local row: the builder knows the table's
// capacity), its fields are stored as byte offsets (slp_tall_item.h), so the address of a running sum is the field under a mask
// with NO base and that of a value the field under a mask with the constant 8 in the instruction's offset; only the tile's base
// (which alternates per cell) is a register.  With the sums first and the table behind them -- the order up to here -- the
// table's base was one v_add_u32 per item: the sums are up to 104 KB, beyond the 16 bits of a DS offset, and as long as the
// planner sizes both areas per copy only one of them can start at a fixed place.  Same bytes as the planner's budget: R is unchanged.
// The tile's C / 2 16-byte pieces are dealt to the 1024 lanes in order: lane p carries piece p and, where the tile has it,
// piece p + 1024 -- 4096 columns: two pieces on every lane; 3072: a second piece on the first 8 of the 16 waves; 2048 and
// below: one piece on the first C / 2 lanes.  C / 2 is a multiple of 64, so either test is the same for a whole wave.
// CT: the width as a constant (0: the argument `cw`) -- instantiated for the widths the benchmark's LP runs on, where the folded
// tile tests and tile offsets are worth 1.2 % of a product (21.79 -> 22.05 ms with 4096 columns as an argument).
// REC: the copy's packets hold the first four list positions as one 16-byte record per lane (slp_tall_item.h; the planner's
// choice per copy, StripJds::tall_records) -- one load where the slot-major form takes four.  REC = false keeps the slot-major
// loads of before the form existed; the pipeline above is the same for both.
template <bool DICT, bool ACC, bool POW = false, int CT = 0, bool REC = false>
__global__ __launch_bounds__(kTallT) void k_tall_spmv(int nseg, const TallWg *__restrict__ wgs, const double *__restrict__ dict_arg,
                                                      const double *__restrict__ x, double *__restrict__ out, double pw, const int cw,
                                                      const int dcap, const int oxt) {
    const int C = CT ? CT : cw;
    constexpr int kDepth = DICT ? kTallDepth : 2;
    constexpr int kTileDepth = kTallTileDepth < kDepth ? kTallTileDepth : kDepth;
    constexpr int kTurn = tall_lcm(2 * kDepth, kTileDepth);   // packets per turn of the unrolled loop
    constexpr bool AHEAD = DICT && kTallAhead;
    static_assert(kTallTurn % kTurn == 0, "a workgroup's packets are whole turns of the loop (slp_tall.hip pads to kTallTurn)");
    // LDS address 0 is a scratch cell: whatever is not a lane's item -- a slot beyond its list (the load past the buffer
    // descriptor returns 0), a skip item, a padding word of a record -- decodes to sum field 0, value id 0, column 0 and adds into the
    // scratch cell: no predicate on the stores, none on the sums
    extern __shared__ __attribute__((aligned(16))) double tall_lds[];
    double *const dv = tall_lds + kTallItemTableByte / 8;
    double *const acc = tall_lds + tall_item_sum_base(dcap);   // acc[r]: local row r
    double *const xt = tall_lds + oxt;                   // tile buffers at xt and xt + C
    // the item path (consume()) works on LDS byte addresses (32-bit, address space 3)
    typedef __attribute__((address_space(3))) double lds_double;
    auto lds_at = [](unsigned int a) -> lds_double & { return *(lds_double *)(unsigned long long)a; };
    const unsigned int lds0 = (unsigned int)(unsigned long long)(lds_double *)tall_lds;
    if (lds0 != 0u) __builtin_trap();   // (the block's address is a link-time constant: this kernel declares no other LDS)
    const unsigned int xtb = 8u * (unsigned int)oxt;
    const int p = threadIdx.x;
    // (wave-uniform by construction; told to the compiler, so that tests on it are scalar branches, not EXEC masks)
    const unsigned int wbase = (unsigned int)__builtin_amdgcn_readfirstlane(p & ~(kWave - 1));
    const bool piece0 = (int)wbase < (C >> 1), piece1 = (int)wbase + kTallT < (C >> 1);
    const int v = blockIdx.x;
    int cur = 0;   // the tile buffer of the current cell: 0 or C (doubles from xt)
    TallWg wg = wgs[v];
    // ACC: the sums continue from what `out` holds -- a row chunk of a chunked matrix carrying on the column sums of the chunks
    // before it, launch by launch (the strip-range split takes it in k_tall_combine instead: its descriptors point into the
    // partial-sum array).  A template parameter: loads under a run-time condition in front of the pipeline made the compiler
    // wait for vmcnt(0) in the loop.
    if (p == 0) tall_lds[0] = 0.0;
    for (int r = p; r < wg.nrows; r += kTallT) acc[r] = ACC ? out[wg.row0 + r] : 0.0;
  for (int seg = 0; seg < nseg; ++seg) {
    if (seg > 0) wg = wgs[(i64)seg * gridDim.x + v];
    if (DICT) {
        const double *__restrict__ dsrc = dict_arg ? dict_arg : wg.dict;
        for (int q = p; q < wg.D; q += kTallT) dv[q] = dsrc[q];
    }
    // this lane's dword of every header -- through a GLOBAL-address-space pointer: a pointer read from a structure in memory is
    // a generic one to the compiler, its loads become flat_load (complete out of order: every wait a vmcnt(0), the pipeline gone)
    typedef const unsigned int __attribute__((address_space(1))) *gptr_t;
    const gptr_t hd = (gptr_t)(unsigned long long)wg.dir + (p & 7);
    const int npk = (int)wg.npk - 2 * kTallDepth;                             // the last 2 x depth packets are prefetch targets only
    // buffer descriptors: lanes without work address past num_records (the load returns 0 without a memory request)
    const __amdgpu_buffer_rsrc_t rs_x =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(x + wg.x0), 0, (int)(wg.ncol * 8), 0x00020000);

    // A slot is `width` words from word `so` of the payload (so are a packet's records, four words per lane, and its words of
    // fifth bytes; slp_tall_item.h: the order).  ONE descriptor per segment (the payload's; the fp64 values'): a
    // slot's load differs from its neighbour's in the scalar offset (the slot's first byte) and in num_records (the slot's LAST
    // byte + 1) only, so the four descriptor words stay in one register quad whose third word is rewritten in front of each
    // load -- with the sum the next slot's offset needs anyway.  The range check of a raw buffer on this hardware covers the
    // scalar offset: a lane is out of range when scalar offset + vector offset >= num_records (measured -- with num_records =
    // the slot's width alone every lane of a slot behind the first reads 0; tests/test_gpu_tall_frame.py pins it: under the other
    // rule the lanes past a slot would read the next slot's items).  So the lanes past the slot's width lie behind the
    // descriptor's end (the load returns 0, no memory request) with no per-lane predicate.  Round 6 gave every load a descriptor
    // of its own, base included: a 64-bit shift and add, the mask of the high word, the size, on the CU's one scalar unit in all
    // 16 waves (7 scalar instructions per load, 46 of a packet's 63).  The descriptor is kept as four plain words because
    // __builtin_amdgcn_make_buffer_rsrc per load makes the compiler copy base and flags into a fresh quad each time (3 s_mov per
    // load).
    // (A row block's payload is addressed in 32-bit bytes here: below 4 GB, i.e. 2^29 fp64 entries per row block.)
    typedef unsigned int rsrc_words_t __attribute__((ext_vector_type(4)));
    auto words_of = [](const void *base) {
        const unsigned long long a = (unsigned long long)base;
        rsrc_words_t d;
        d[0] = (unsigned int)a; d[1] = (unsigned int)(a >> 32) & 0xffffu; d[2] = 0u; d[3] = 0x00020000u;
        return d;
    };
    auto as_rsrc = [](const rsrc_words_t &d) {
        __amdgpu_buffer_rsrc_t r;
        __builtin_memcpy(&r, &d, sizeof(r));
        return r;
    };
    rsrc_words_t dpay = words_of(wg.pay), dval = words_of(DICT ? (const void *)x : (const void *)wg.val);
    auto slot_pay = [&](unsigned int end) { dpay[2] = end; return as_rsrc(dpay); };            // (end: byte behind the slot's words)
    auto slot_val = [&](unsigned int end) { dval[2] = 2u * end; return as_rsrc(dval); };

    TallRegs<DICT> regs[kDepth];
    TallTile tiles[kTileDepth];
    unsigned int hw[kDepth];        // this lane's dword of the headers of the packets depth .. 2 depth - 1 ahead

    // A packet's header is read ONCE, when its payload is about to be issued (`depth` packets before its items are taken):
    // six v_readlane and the unpacking to scalars that both halves of the issue share; the two fields consume() needs `depth`
    // steps later (tile word, lanes with a fifth item) wait in scalar registers (2 x depth of them).  Offsets and widths are
    // unpacked as BYTES of payload words, the unit of the scalar offset and of num_records.  (Round 6 read lanes 0 and 2-5 in
    // either half of the issue and lanes 1 and 4 again in consume(): 13 v_readlane per packet for 6 dwords.)
    struct TallHdr {
        unsigned int off;              // payload offset of the packet inside its row block
        unsigned int xw;               // TallPkt::xsrc
        unsigned int w[kTallSlots];    // lanes whose list is longer than slot k
    };
    static_assert(kTallT <= (1 << 14), "a width's two bits below its upper half-word are zero: (c >> 14) is 4 x the upper width");
    auto unpack = [&](unsigned int h) {
        TallHdr t;
        t.off = (unsigned int)__builtin_amdgcn_readlane((int)h, 0) * 4u;
        t.xw = (unsigned int)__builtin_amdgcn_readlane((int)h, 1);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const unsigned int v = (unsigned int)__builtin_amdgcn_readlane((int)h, 2 + i);
            t.w[2 * i] = (v & 0xffffu) * 4u;
            t.w[2 * i + 1] = v >> 14;
        }
        return t;
    };
    const unsigned int wbytes = wbase * 4u;   // (a wave takes slot k's items iff wbytes < w[k])
    unsigned int xwq[kDepth], c4q[kDepth];

    // this lane's 16-byte pieces of an x-tile (pieces p and p + 1024: doubles 2p, 2p + 1 and 2048 + 2p, 2049 + 2p).  A piece that straddles the end of x
    // (odd width) may fetch the 8 bytes behind it: every device block carries 16 bytes of slack, and no item names that column
    auto load_tile = [&](TallTile &g, const unsigned int xo) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {   // (a piece the lane does not carry: past the descriptor, no memory request)
            const unsigned int o = (i == 0 ? piece0 : piece1) && xo != kOob ? xo + (unsigned int)i * (unsigned int)(kTallT * 16) : kOob;
            const auto v = __builtin_amdgcn_raw_buffer_load_b128(rs_x, o, 0, 0);
            g.x[2 * i] = __hiloint2double((int)v[1], (int)v[0]);
            g.x[2 * i + 1] = __hiloint2double((int)v[3], (int)v[2]);
        }
    };

    // The payload of a packet goes out in two halves: the registers of slots 0-3 are free once the first four items are done, so
    // their loads for the packet `depth` ahead go out BETWEEN the two groups of items (in the shadow of the LDS latency) instead
    // of behind all of them
    auto issue_part = [&](TallRegs<DICT> &g, const TallHdr &t, const int part) {
        const unsigned int mine = (unsigned int)p * 4u;
        // A packet without a fifth item (lists of <= 4 items: the metric's density, where a cell is one such packet) issues no
        // loads for slots 4-7 and their fifth bytes -- a uniform branch; consume() takes the second group under the same test.  The
        // compiler then counts the loads in flight by the path without them (vmcnt(24-26) instead of 36-41): exact for those
        // packets, a shorter prefetch distance behind a packet that has the second group.  3.30 / 3.30 -> 3.25 / 3.22 ms on the
        // slice, unchanged where lists are five long (profiles/r05_tall_half_packets.log).
        if (REC && part == 0) {
            // slots 0-3 of a copy with records: the lane's four items (16 bytes at 16 p of the packet's first 4 w[0] words) in ONE
            // load, and its word of fifth bytes behind the records -- lanes past w[0] lie behind the descriptor's end, a list
            // shorter than four has zero words (the scratch cell) in its record
            const unsigned int so = t.off, end = so + 4u * t.w[0];   // (bytes)
            const auto v = __builtin_amdgcn_raw_buffer_load_b128(slot_pay(end), 4u * mine, (int)so, 2);   // streamed once
#pragma unroll
            for (int k = 0; k < 4; ++k) g.lo[k] = v[k];
            if (!DICT) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {   // the four values: double i of the parallel array belongs to word i
                    const auto u = __builtin_amdgcn_raw_buffer_load_b128(slot_val(end), 8u * mine + 16u * (unsigned int)h, (int)(2u * so), 2);
                    g.val[DICT ? 0 : 2 * h] = __hiloint2double((int)u[1], (int)u[0]);
                    g.val[DICT ? 0 : 2 * h + 1] = __hiloint2double((int)u[3], (int)u[2]);
                }
            }
            if (DICT) g.hi[0] = __builtin_amdgcn_raw_buffer_load_b32(slot_pay(end + t.w[0]), mine, (int)end, 2);
        } else if (part == 0 || wbytes < t.w[4]) {   // (per wave: the waves past the fifth items' lanes skip them too)
            unsigned int so = t.off;   // (bytes)
            if (part == 1) so += tall_packet_group1_word(t.w, DICT, REC);   // (slot-major: w[0] + w[1] + w[2] + w[3])
#pragma unroll
            for (int k = 4 * part; k < 4 * part + 4; ++k) {
                const unsigned int end = so + t.w[k];   // (= the next slot's first byte)
                g.lo[k] = __builtin_amdgcn_raw_buffer_load_b32(slot_pay(end), mine, (int)so, 2);   // streamed once
                if (!DICT) {
                    const auto v = __builtin_amdgcn_raw_buffer_load_b64(slot_val(end), 2u * mine, (int)(2u * so), 2);
                    g.val[DICT ? 0 : k] = __hiloint2double((int)v[1], (int)v[0]);
                }
                so = end;
            }
            if (DICT) {
                if (part == 0) so += t.w[4] + t.w[5] + t.w[6] + t.w[7];   // the fifth bytes follow the eight slots: slots 0-3, then slots 4-7
                else if (!REC) so += t.w[0];                              // (records: those of slots 4-7 follow slot 7 directly)
                g.hi[DICT ? part : 0] = __builtin_amdgcn_raw_buffer_load_b32(slot_pay(so + t.w[4 * part]), mine, (int)so, 2);
            }
        }
    };
    // The tile that the packet with tile word `txw` carries (the packet `kTileDepth` ahead): issued behind all of the current
    // packet's items (issue_part(..., 1)).  Its word is the header's own where the tile runs as far ahead as the items, and waits
    // in the header ring (xwq) where it runs shorter.
    auto issue_tile = [&](TallTile &g, const unsigned int txw) {
        // columns past ncol read 0: the displacement of each double is part of the voffset, which the descriptor's range check
        // covers
        // lane p carries doubles 2p, 2p + 1 of the tile and, where the tile has them, 2048 + 2p, 2049 + 2p: consecutive lanes then write
        // consecutive 16-byte pieces of the LDS tile (no bank conflicts; with 4p .. 4p + 3 per lane the two 16-byte writes of a
        // lane pair collided -- the tile write was the largest single item of the kernel's ablation, 0.9 of 4.1 ms)
        const unsigned int xs = txw & 0x7fffffffu;
        const unsigned int xo = xs == kNoTile ? kOob : (xs + 2u * (unsigned int)p) * 8u;
        load_tile(g, xo);
    };

    // AHEAD (items with a value id): what a packet's first four items need that does NOT depend on the cell's barrier -- the
    // decode of the sum address, column and value offset (the words landed `depth` packets ago) and the four reads of the value
    // table (constant within a segment) -- is done one packet early, behind the first group's sum stores of the packet before,
    // and held across the barrier (16 registers); behind the barrier remain the sum reads (other waves' stores) and the x
    // gathers (the tile).  Same products, same chains: the sums are the same bits.
    //   * the first packet of a segment is taken ahead behind the prologue's __syncthreads (the segment's table is in LDS);
    //   * the last real packet takes a prefetch-target packet ahead: zero words, entry 0 of the table, never used;
    //   * that read stands in front of the segment-end __syncthreads in program order, the next segment's table is written
    //     behind it: no read reaches another segment's table;
    //   * a continuation packet (no barrier) takes the same path; the second group of four stays where it was.
    // fp64 items (DICT = false) stay as they were: they have no table read to move, and their decode is two instructions per
    // item that the scheduler already places freely inside the block behind the barrier.
    auto ahead = [&](const TallRegs<DICT> &g, TallAheadItems &d) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned int w = g.lo[k];
            d.sa[k] = tall_item_sum_bytes(w, g.hi[0] >> (8 * k));
            unsigned int col = tall_item_column(w);
            asm("" : "+v"(col));   // (as in group(): the column stays an index)
            d.col[k] = col;
            d.v[k] = lds_at(tall_item_value_bytes(w) + kTallItemTableByte);
        }
    };

    // (xw, c4: the packet's tile word and the bytes of its lanes with a fifth item, as its header's unpack() left them;
    // AHEAD: nx holds the packet's first four items on entry and those of the next packet, whose registers are gn, on return)
    auto consume = [&](TallRegs<DICT> &g, const TallRegs<DICT> &gn, TallAheadItems &nx, const TallTile &tile, const unsigned int xw,
                       const unsigned int c4, auto &&between) {
        if (xw & kPktNewCell) {
            // sums of the previous cell (other lanes owned these rows there) and the x-tile: LDS only, loads stay in flight
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            cur = C - cur;
        }
        auto stage_tile = [&]() {
            if ((xw & 0x7fffffffu) != kNoTile) {
                // (Bringing the tile in by LDS-DMA -- __builtin_amdgcn_global_load_lds, no registers, no ds_write -- was built and
                // measured: 4.71 ms against 3.99.  With two tile buffers the DMA can only start at the cell's barrier and must
                // have landed by the next one, 1.6 us later; the register path issued the loads four cells ahead (now: kTallTileDepth).  A third buffer
                // does not fit beside 78 KB of running sums.)
                double *dst = static_cast<double *>(__builtin_assume_aligned(xt + (C - cur) + 2 * p, 16));
                if (piece0) *reinterpret_cast<double2 *>(dst) = make_double2(tile.x[0], tile.x[1]);
                if (piece1) *reinterpret_cast<double2 *>(dst + 2 * kTallT) = make_double2(tile.x[2], tile.x[3]);
            }
        };
        // WHERE the wave stores its share of the NEXT cell's x-tile (it only has to be there by the next cell's barrier; lab
        // patch: tools/lab/patches).  Round 5, with the predicate-free item code: right behind the barrier (0) 3.28-3.29 ms on the
        // 2.5e6 x 1e7 slice; behind the first four items (1) 3.74-3.77; between the two item groups' loads (2) 3.44-3.46; behind all
        // of the packet's items (3) 3.44 (profiles/r05_tall_stage_position.log).  Round 4's kernel -- a select and a compare
        // per store -- had it the other way round (behind the items 3.92 against 3.99 behind the barrier: there every wave's
        // gathers queued behind 32 KB of stores): with the shorter item code the stores are out of the way before the first
        // gathers are ready to issue, and they no longer sit between a packet's items and the next packet's.
        stage_tile();
        // the tile's first byte: the scalar that an item's column `* 8` is added onto in one v_lshl_add_u32
        const unsigned int tileb = xtb + 8u * (unsigned int)cur;
        // Four slots at a time: all twelve LDS reads (running sums, values, x) are issued together, the products do not
        // depend on the sums, and a sum that the lane has just updated is carried in a register (a lane's items of one
        // row are consecutive) -- the LDS latency is paid once per group, not once per item.  The additions of a row
        // stay one chain in list order.
        auto group = [&](const int k0) {
            unsigned int w[4], sa[4];   // sa: LDS address of the item's running sum (0: the scratch cell)
            double ar[4], pr[4], t[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                w[k] = g.lo[k0 + k];
                sa[k] = (DICT ? tall_item_sum_bytes(w[k], g.hi[DICT ? (k0 >> 2) : 0] >> (8 * k)) : tall_item64_sum_bytes(w[k]));
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) ar[k] = lds_at(sa[k]);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                // (the column stays an index in a register of its own -- the empty asm keeps the compiler from folding its `* 8` into
                // the extraction as shift, mask and add: three instructions for v_bfe_u32 and v_lshl_add_u32)
                unsigned int col = DICT ? tall_item_column(w[k]) : tall_item64_column(w[k]);
                asm("" : "+v"(col));
                const double xv = lds_at((col << 3) + tileb);
                pr[k] = DICT ? lds_at(tall_item_value_bytes(w[k]) + kTallItemTableByte) * xv
                             : (POW ? abs_pow(g.val[DICT ? 0 : k0 + k], pw) * 1.0 : g.val[DICT ? 0 : k0 + k]) * xv;
            }
            t[0] = ar[0] + pr[0];
#pragma unroll
            for (int k = 1; k < 4; ++k) t[k] = ((sa[k] == sa[k - 1]) ? t[k - 1] : ar[k]) + pr[k];
            // Unconditional stores, no predicate at all: what is not this lane's item lands in the scratch cell by its own
            // decoding -- a packet's items stay ONE basic block, which the instruction scheduler may interleave with the loads of
            // the packets ahead (rounds 3-4: a branch, then a select, per store: 3 vector instructions per item more)
#pragma unroll
            for (int k = 0; k < 4; ++k) lds_at(sa[k]) = t[k];
        };
        // the first group of a packet taken ahead: sum reads, x gathers, the chain and the stores of group()
        auto group_taken = [&]() {
            double ar[4], pr[4], t[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) ar[k] = lds_at(nx.sa[k]);
#pragma unroll
            for (int k = 0; k < 4; ++k) pr[k] = nx.v[k] * lds_at((nx.col[k] << 3) + tileb);
            t[0] = ar[0] + pr[0];
#pragma unroll
            for (int k = 1; k < 4; ++k) t[k] = ((nx.sa[k] == nx.sa[k - 1]) ? t[k - 1] : ar[k]) + pr[k];
#pragma unroll
            for (int k = 0; k < 4; ++k) lds_at(nx.sa[k]) = t[k];
        };
        if (AHEAD) {
            group_taken();
            ahead(gn, nx);   // the next packet's, behind this group's sum stores and in front of the next barrier
        } else {
            group(0);   // (a wave without items -- nearly never -- reads cell 0 of the arrays and stores into the scratch cell)
        }
        between();
        if (wbytes < c4) group(4);
    };

    // prologue: headers of the first 2 x depth packets, payload of the first depth
#pragma unroll
    for (int u = 0; u < kDepth; ++u) {
        const TallHdr t = unpack(hd[(i64)u * 8]);
        xwq[u] = t.xw;
        c4q[u] = t.w[4];
        issue_part(regs[u], t, 0);
        issue_part(regs[u], t, 1);
        if (u < kTileDepth) issue_tile(tiles[u], t.xw);   // (the tiles of the first `tile depth` packets only)
        hw[u] = hd[(i64)(u + kDepth) * 8];
    }
    __syncthreads();
    TallAheadItems nx;   // AHEAD: the first four items of the packet about to be taken
    if (AHEAD) ahead(regs[0], nx);   // (behind the barrier: this segment's value table is in LDS)
    for (int jj = 0; jj < npk; jj += kTurn) {
#pragma unroll
        for (int u = 0; u < kTurn; ++u) {
            const int i = u % kDepth, it = u % kTileDepth;
            const unsigned int xw = xwq[i], c4 = c4q[i];                     // packet jj + u
            // header of packet jj + u + depth: unpacked BEHIND this packet's first items, in the shadow of their LDS reads.  In
            // front of the cell's barrier the same instructions made A x 0.2 and 0.35 ms slower (mean of three alternating runs) on the
            // two boxes where both places were timed side by side
            TallHdr t;
            consume(regs[i], regs[(u + 1) % kDepth], nx, tiles[it], xw, c4, [&]() {
                t = unpack(hw[i]);
                xwq[i] = t.xw;
                c4q[i] = t.w[4];
                issue_part(regs[i], t, 0);
            });
            issue_part(regs[i], t, 1);
            // the tile of packet jj + u + tile depth into the registers this packet's tile has just left: its word was unpacked
            // depth - tile depth steps ago (tile depth = depth: just now)
            issue_tile(tiles[it], kTileDepth == kDepth ? t.xw : xwq[(u + kTileDepth) % kDepth]);
            hw[i] = hd[(i64)(jj + u + 2 * kDepth) * 8];                      // header of packet jj + u + 2 depth
        }
    }
    __syncthreads();   // (every wave is done with this segment's tiles and value table)
  }
    // (S > 1: row0 points into the partial-sum array -- the sums of this strip range, added up in range order by k_tall_combine)
    for (int r = p; r < wg.nrows; r += kTallT) out[wg.row0 + r] = acc[r];
}


__global__ void k_tall_combine(i64 nrow, int S, const double *__restrict__ part, double *__restrict__ out, int accum) {
    for (i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x; r < nrow; r += (i64)gridDim.x * blockDim.x) {
        double a = accum ? out[r] + part[r] : part[r];
        for (int s = 1; s < S; ++s) a += part[(i64)s * nrow + r];  // strip ranges in order: deterministic
        out[r] = a;
    }
}

// One launch with the LDS layout of the copy (slp_tall_plan.h): R rows of sums, a table of dcap entries, tiles of C columns
template <bool DICT, bool ACC, bool POW>
static void tall_launch(const StripJds &f, unsigned grid, int nseg, const TallWg *wgs, const double *dict, const double *x, double *out, double pw) {
    TallPlan lay;
    lay.R = f.tall_R; lay.C = (int)f.C; lay.dcap = DICT ? f.tall_dcap : 0;
    tall_plan_layout(lay);
    SLP_REQUIRE(tall_width_ok(lay.C) && lay.R > 0 && lay.lds_bytes <= kTallLdsBytes && f.D <= lay.dcap, "tall cells: LDS layout");
    auto go = [&](auto kernel, bool &raised) {
        if (!raised) {
            SLP_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kTallLdsBytes));
            raised = true;
        }
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(kTallT), (size_t)lay.lds_bytes, ctx().stream, nseg, wgs, dict, x, out, pw, lay.C, lay.dcap,
                           lay.off_xt / 8);
    };
    static bool raised[2][3] = {{false, false, false}, {false, false, false}};   // (per instantiation: the packets' form, the width)
    auto by_width = [&](auto rec) {   // rec: the packets' form as a constant
        constexpr bool REC = decltype(rec)::value;
        if (DICT && !POW && lay.C == 3072) go(k_tall_spmv<DICT, ACC, POW, (DICT && !POW) ? 3072 : 0, REC>, raised[REC][1]);
        else if (DICT && !POW && lay.C == 4096) go(k_tall_spmv<DICT, ACC, POW, (DICT && !POW) ? 4096 : 0, REC>, raised[REC][2]);
        else go(k_tall_spmv<DICT, ACC, POW, 0, REC>, raised[REC][0]);
    };
    if (f.tall_records) by_width(std::true_type());
    else by_width(std::false_type());
}

void tall_spmv(const StripJds &f, const double *x, double *out, int accum) {
    double *dst = f.S > 1 ? f.part.p : out;
    const unsigned grid = (unsigned)(f.B * f.S);
    const bool acc = accum && f.S == 1;
    const double *none = nullptr;
    if (f.D > 0) { if (acc) tall_launch<true, true, false>(f, grid, 1, f.tall_wg.p, f.dict, x, dst, 0.0); else tall_launch<true, false, false>(f, grid, 1, f.tall_wg.p, f.dict, x, dst, 0.0); }
    else { if (acc) tall_launch<false, true, false>(f, grid, 1, f.tall_wg.p, none, x, dst, 0.0); else tall_launch<false, false, false>(f, grid, 1, f.tall_wg.p, none, x, dst, 0.0); }
    if (f.S > 1)
        hipLaunchKernelGGL(k_tall_combine, dim3(grid_for(f.nrow, kBlock)), dim3(kBlock), 0, ctx().stream, f.nrow, f.S, f.part.p, out, accum);
    SLP_HIP(hipGetLastError());
}

// A composite of tall-cell copies (the chunks of a chunked matrix) in ONE launch: the descriptor table tall_fuse() laid out.
// Rows orientation: a grid over the row blocks of all chunks (2048 workgroups drained by 256 compute units: no launch ends at
// its slowest workgroup eight times per product).  Columns orientation: one workgroup per column block walks the chunks in
// order, the column sums stay in LDS (no hand-over of the sums through `out` between launches).
void tall_spmv_fused(const StripJds &f, const double *x, double *out) {
    const int nseg = f.parts_cols ? (int)f.parts.size() : 1;
    const unsigned grid = (unsigned)(f.tall_wg.n / (size_t)nseg);
    if (f.D > 0) tall_launch<true, false, false>(f, grid, nseg, f.tall_wg.p, nullptr, x, out, 0.0);
    else tall_launch<false, false, false>(f, grid, nseg, f.tall_wg.p, nullptr, x, out, 0.0);
    SLP_HIP(hipGetLastError());
}

// The fused descriptor table of a composite whose parts are all tall-cell copies of one kind (all with a dictionary or all
// without, no strip-range split; columns orientation: the same row blocks in every chunk).  False: the composite keeps its
// chunk-by-chunk launches.
bool tall_fuse(StripJds &f) {
    f.tall_wg.release();
    const char *e = getenv("SLP_TALL_FUSE");
    if (e && e[0] == '0') return false;
    if (f.parts.empty()) return false;
    const StripJds &f0 = *f.parts[0];
    for (const StripJds *g : f.parts)
        if (!g->ok || !g->tall || g->S != 1 || g->C != f0.C || (g->D > 0) != (f0.D > 0) || g->tall_dcap != f0.tall_dcap ||
            g->tall_records != f0.tall_records ||   // (one launch runs one instantiation of the kernel)
            (f.parts_cols && (g->B != f0.B || g->tall_R != f0.tall_R || g->nrow != f0.nrow)))
            return false;
    std::vector<TallWg> all;
    for (size_t k = 0; k < f.parts.size(); ++k) {
        const StripJds &g = *f.parts[k];
        std::vector<TallWg> wg((size_t)g.B);
        SLP_HIP(hipMemcpy(wg.data(), g.tall_wg.p, wg.size() * sizeof(TallWg), hipMemcpyDeviceToHost));
        for (TallWg &w : wg) {
            w.dict = g.dict;                                   // every chunk has a value table of its own
            if (f.parts_cols) w.x0 = f.part_off[k];            // the chunk multiplies its slice of x ...
            else w.row0 += f.part_off[k];                      // ... or writes its own rows
            all.push_back(w);
        }
    }
    f.tall_wg.upload(all.data(), all.size());
    // one LDS layout for the launch: the tallest row block's sums, the chunks' common table capacity and strip width
    f.C = f0.C;
    f.tall_dcap = f0.tall_dcap;
    f.tall_records = f0.tall_records;
    f.tall_R = 0;
    for (const StripJds *g : f.parts) f.tall_R = std::max(f.tall_R, g->tall_R);
    return true;
}

// out = |A|^pw x over a tall-cell copy with fp64 entries (strip_spmv_abs_pow)
void tall_spmv_pow(const StripJds &f, double pw, const double *x, double *out, int accum) {
    SLP_REQUIRE(f.ok && f.tall && f.D == 0, "tall_spmv_pow: not a tall-cell copy with fp64 entries");
    double *dst = f.S > 1 ? f.part.p : out;
    const unsigned grid = (unsigned)(f.B * f.S);
    if (accum && f.S == 1) tall_launch<false, true, true>(f, grid, 1, f.tall_wg.p, nullptr, x, dst, pw);
    else tall_launch<false, false, true>(f, grid, 1, f.tall_wg.p, nullptr, x, dst, pw);
    if (f.S > 1)
        hipLaunchKernelGGL(k_tall_combine, dim3(grid_for(f.nrow, kBlock)), dim3(kBlock), 0, ctx().stream, f.nrow, f.S, f.part.p, out, accum);
    SLP_HIP(hipGetLastError());
}
}  // namespace slp

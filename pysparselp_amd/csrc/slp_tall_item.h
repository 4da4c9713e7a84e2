// slp_tall_item.h -- the stored item of the tall-cell format (slp_tall.hip): how the builder packs (value id, column inside the
// strip, sum field) and how the product kernel (slp_tall_spmv.hip) turns the stored bits into LDS BYTE addresses.  One text
// for both, so that they cannot disagree; plain constexpr functions without any HIP header, so that the host compiler can test
// them (tests/host/tall_item_main.cpp).
//
// The kernel's LDS, in doubles from LDS address 0:  [0: scratch cell] [1 .. dcap: value table] [1 + dcap + r: running sum of
// local row r] ... [x-tiles].  The SUM FIELD of an item is the index of its running sum among these doubles: tall_item_sum_base(dcap)
// + local row, 14 bits (1 + 2048 + 13312 < 2^14: asserted in slp_tall.h).  Sum field 0 is the scratch cell.
//
// Every field is stored where the LDS address wants it: a running sum, a table entry and an x of the tile are 8 bytes, so a
// field at bit 3 (or moved there by the one shift that extracts it) IS its byte offset -- the kernel has no `<< 3` per field
// (before: fields stored as indices from bit 0, three instructions per column and three to four per row), and neither the sums
// nor the table need a base register: the sums' is in the field, the table's is the constant 8 (the offset of a DS instruction).
//
//   item with a value id (5 bytes):  word = 0 (3 bits) | id (11) << 3 | column (12) << 14 | low 6 bits of the sum field << 26
//                                    fifth byte = bits 6-13 of the sum field
//       running sum   LDS address = ((fifth : word) >> 23) & 0x1fff8          one v_alignbit_b32 and one v_and_b32
//       value         LDS address = (word & 0x3ff8) + 8                       one v_and_b32
//       x             byte offset = ((word >> 14) & 0xfff) * 8                one v_bfe_u32; the * 8 and the tile's base are ONE
//                                                                            v_lshl_add_u32 (the base alternates per cell: a scalar)
//   item with an fp64 value (4 bytes, the value in a parallel array; no table: dcap = 0):
//                                    word = 0 (3 bits) | sum field (14) << 3 | column (12) << 17
//       running sum   LDS address = word & 0x1fff8
//       x             byte offset = (word >> 17) * 8                          (bits 29-31 are zero)
//
// The all-zero item decodes to (sum field 0, id 0, column 0): the scratch cell, entry 0 of the table and column 0 of the tile --
// a skip item, a padding word of a record (below) and the zero a load past its buffer descriptor returns need no predicate.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SLP_ITEM_FN __host__ __device__ constexpr inline
#else
#define SLP_ITEM_FN constexpr inline
#endif

namespace slp {

constexpr int kTallIdBits = 11, kTallColBits = 12, kTallRowBits = 14;   // (kTallRowBits: the local row in the sort key, the sum field in the item)
constexpr int kTallItemIdShift = 3, kTallItemColShift = kTallItemIdShift + kTallIdBits;      // 3, 14
constexpr int kTallItemSumLoShift = kTallItemColShift + kTallColBits;                        // 26: the sum field's low bits
constexpr int kTallItemSumLoBits = 32 - kTallItemSumLoShift;                                 // 6 of them in the word
constexpr int kTallItemSumShift = kTallItemSumLoShift - 3;                                   // (fifth : word) >> 23 = 8 x sum field
constexpr unsigned int kTallItemSumMask = ((1u << kTallRowBits) - 1u) << 3;                  // 0x1fff8
constexpr unsigned int kTallItemValMask = ((1u << kTallIdBits) - 1u) << kTallItemIdShift;    // 0x3ff8
constexpr unsigned int kTallItemTableByte = 8;                                               // the table's first byte in LDS
constexpr int kTallItem64SumShift = 3, kTallItem64ColShift = kTallItem64SumShift + kTallRowBits;   // 3, 17
static_assert(kTallItemSumLoBits + 8 == kTallRowBits, "the sum field: 6 bits in the word, 8 in the fifth byte");
static_assert(kTallItem64ColShift + kTallColBits <= 32, "fp64 item: sum field and column in one word");

struct TallItem {
    unsigned int word;    // the item's low four bytes
    unsigned int fifth;   // its fifth byte (0 .. 255)
};

// sum field of local row 0: behind the scratch cell and a value table of `dcap` entries (0 with fp64 values)
SLP_ITEM_FN unsigned int tall_item_sum_base(int dcap) { return 1u + (unsigned int)dcap; }

// ---- items with a value id -----------------------------------------------------------------------------------------------
SLP_ITEM_FN TallItem tall_item_encode(unsigned int id, unsigned int col, unsigned int sum) {
    return TallItem{(id << kTallItemIdShift) | (col << kTallItemColShift) | ((sum & ((1u << kTallItemSumLoBits) - 1u)) << kTallItemSumLoShift),
                    sum >> kTallItemSumLoBits};
}
// LDS byte address of the running sum.  `fifth`: the item's fifth byte in bits 0-7; whatever stands above them is masked away
// with the column bits, so the kernel passes its word of four fifth bytes shifted down, not the byte alone.
SLP_ITEM_FN unsigned int tall_item_sum_bytes(unsigned int word, unsigned int fifth) {
    return ((word >> kTallItemSumShift) | (fifth << (32 - kTallItemSumShift))) & kTallItemSumMask;   // (a funnel shift: v_alignbit_b32)
}
// byte offset of the value from the table's first byte (kTallItemTableByte)
SLP_ITEM_FN unsigned int tall_item_value_bytes(unsigned int word) { return word & kTallItemValMask; }
// column inside the strip (an index: the kernel scales it onto the tile's base in the same instruction that adds the base)
SLP_ITEM_FN unsigned int tall_item_column(unsigned int word) { return (word >> kTallItemColShift) & ((1u << kTallColBits) - 1u); }

SLP_ITEM_FN unsigned int tall_item_sum(unsigned int word, unsigned int fifth) { return tall_item_sum_bytes(word, fifth) >> 3; }
SLP_ITEM_FN unsigned int tall_item_id(unsigned int word) { return tall_item_value_bytes(word) >> 3; }

// ---- items with an fp64 value --------------------------------------------------------------------------------------------
SLP_ITEM_FN unsigned int tall_item64_encode(unsigned int col, unsigned int sum) {
    return (sum << kTallItem64SumShift) | (col << kTallItem64ColShift);
}
SLP_ITEM_FN unsigned int tall_item64_sum_bytes(unsigned int word) { return word & kTallItemSumMask; }
SLP_ITEM_FN unsigned int tall_item64_column(unsigned int word) { return word >> kTallItem64ColShift; }
SLP_ITEM_FN unsigned int tall_item64_sum(unsigned int word) { return tall_item64_sum_bytes(word) >> 3; }

// ---- the payload of a packet ---------------------------------------------------------------------------------------------
// A packet is 8 consecutive list positions ("slots") of all lanes; w[k] = lanes whose list is longer than slot k (non-increasing).
// A copy stores ALL its packets in one of two forms (the planner's choice per copy, slp_tall_plan.h: tall_plan_records).  In
// words from the packet's offset, `dict`: items with a value id (with fp64 values there are no fifth bytes, and the value of
// the item at word i is double i of the parallel array):
//   slot-major (records = false)
//     [slot 0: w[0] words, lane p's at p] [slot 1] ... [slot 7]
//     [dict: w[0] words: the fifth bytes of lane p's slots 0-3, slot k in byte k] [dict: w[4] words: those of slots 4-7]
//   records (records = true)
//     [w[0] RECORDS of 4 words: lane p's items of slots 0-3 at 4 p .. 4 p + 3 -- zero words where its list is shorter]
//     [dict: w[0] words: the fifth bytes of slots 0-3]
//     [slot 4: w[4] words, lane p's at p] [slot 5] [slot 6] [slot 7]          (slot-major: these slots are mostly empty)
//     [dict: w[4] words: the fifth bytes of slots 4-7]
// Records: the first four list positions lane-major, ONE 16-byte load per lane (fp64: and two for the values) where the
// slot-major order takes four loads of 4 bytes, each with its own scalar offset and end of range -- paid for with a zero word
// for every list position below four that a lane of slot 0 does not have.
struct TallPacketLayout {
    unsigned int slot[8];    // first word of slot k (records: slots 0-3 have none -- tall_packet_record_word)
    unsigned int fifth0;     // the fifth bytes of slots 0-3
    unsigned int fifth1;     // the fifth bytes of slots 4-7
    unsigned int words;      // all of the packet
};
// records: where lane `lane`'s item of slot 0 .. 3 lies
SLP_ITEM_FN unsigned int tall_packet_record_word(unsigned int lane, int slot) { return 4u * lane + (unsigned int)slot; }
// where the second group (slots 4-7) starts: behind the four slots, or behind the records and their fifth bytes.  (Linear in the
// widths: the kernel calls it with widths in bytes.)
SLP_ITEM_FN unsigned int tall_packet_group1_word(const unsigned int *w, bool dict, bool records) {
    return records ? (dict ? 5u : 4u) * w[0] : w[0] + w[1] + w[2] + w[3];
}
SLP_ITEM_FN TallPacketLayout tall_packet_layout(const unsigned int *w, bool dict, bool records) {
    TallPacketLayout l{};
    unsigned int so = 0;
    for (int k = 0; k < 4; ++k) { l.slot[k] = so; so += records ? 0u : w[k]; }
    so = tall_packet_group1_word(w, dict, records);
    for (int k = 4; k < 8; ++k) { l.slot[k] = so; so += w[k]; }
    if (records) {
        l.fifth0 = 4u * w[0];
        l.fifth1 = so;
        l.words = so + (dict ? w[4] : 0u);
    } else {
        l.fifth0 = so;
        l.fifth1 = so + w[0];
        l.words = so + (dict ? w[0] + w[4] : 0u);
    }
    return l;
}
// where lane `lane`'s item of slot k lies
SLP_ITEM_FN unsigned int tall_packet_item_word(const TallPacketLayout &l, bool records, unsigned int lane, int k) {
    return records && k < 4 ? tall_packet_record_word(lane, k) : l.slot[k] + lane;
}
// words that a lane whose list (envelope) is `len` items long takes in the packets of its cell: the builder's sizes (per cell: the
// sum over the lanes, rounded up to 4 words), its estimate and the planner's prediction
SLP_ITEM_FN unsigned int tall_packet_lane_words(unsigned int len, bool dict, bool records) {
    const unsigned int n0 = (len + 7u) / 8u;                 // packets in which the lane has a word of fifth bytes for slots 0-3 (a record)
    const unsigned int n1 = len > 4u ? (len + 3u) / 8u : 0u;   // ... and one for slots 4-7
    if (!records) return len + (dict ? n0 + n1 : 0u);
    const unsigned int second = 4u * (len / 8u) + (len % 8u > 4u ? len % 8u - 4u : 0u);   // its items in slots 4-7
    return 4u * n0 + second + (dict ? n0 + n1 : 0u);
}
// words of a cell whose n items are dealt in balance over `lanes` lanes (what the dealing aims at): n % lanes lists of
// ceil(n / lanes) items, the rest one shorter
SLP_ITEM_FN unsigned long long tall_packet_balanced_words(unsigned long long n, unsigned int lanes, bool dict, bool records) {
    if (!n) return 0ull;
    const unsigned long long tau = (n + lanes - 1u) / lanes, more = n % lanes ? n % lanes : lanes;
    return more * tall_packet_lane_words((unsigned int)tau, dict, records) + (lanes - more) * tall_packet_lane_words((unsigned int)tau - 1u, dict, records);
}

}  // namespace slp

// Stand-alone check of the stored item of the tall-cell format (pysparselp_amd/csrc/slp_tall_item.h: the one text the builder
// packs with and the product kernel decodes with), built with -fsanitize=address,undefined and run as a child process by
// tests/test_tall_item_host.py.  Expected values are worked out here from the format's definition, never from the header's own
// constants: an item is (value id: 11 bits, column inside the strip: 12 bits, sum field: 14 bits), every field stored as the
// BYTE offset of an 8-byte LDS entry.
#include "slp_tall_item.h"

#include <cstdint>
#include <cstdio>
#include <random>

using namespace slp;

static int failures = 0, checks = 0;

static void expect_eq(const char *what, unsigned long long got, unsigned long long want, unsigned a = 0, unsigned b = 0, unsigned c = 0) {
    ++checks;
    if (got == want) return;
    if (++failures <= 20) std::printf("FAIL %s (id %u, column %u, sum field %u): %llu, expected %llu\n", what, a, b, c, got, want);
}

// one item with a value id: the identity, the three byte addresses, the layout bit by bit
static void dict_item(unsigned id, unsigned col, unsigned sum, unsigned tile_base) {
    const TallItem it = tall_item_encode(id, col, sum);
    expect_eq("fifth byte fits a byte", it.fifth <= 0xffu, 1, id, col, sum);
    expect_eq("low three bits are zero", it.word & 7u, 0, id, col, sum);
    // the layout as the format's description states it
    expect_eq("word", it.word, ((unsigned long long)id << 3) | ((unsigned long long)col << 14) | ((unsigned long long)(sum & 63u) << 26), id, col, sum);
    expect_eq("fifth", it.fifth, sum >> 6, id, col, sum);
    // decode(encode(.)) is the identity
    expect_eq("id", tall_item_id(it.word), id, id, col, sum);
    expect_eq("column", tall_item_column(it.word), col, id, col, sum);
    expect_eq("sum field", tall_item_sum(it.word, it.fifth), sum, id, col, sum);
    // the byte addresses: 8 x index + base (the sums' base is 0, the table's the constant 8, the tile's a run-time scalar)
    expect_eq("sum address", tall_item_sum_bytes(it.word, it.fifth), 8ull * sum, id, col, sum);
    expect_eq("value address", tall_item_value_bytes(it.word) + kTallItemTableByte, 8ull * id + 8ull, id, col, sum);
    expect_eq("x address", (tall_item_column(it.word) << 3) + tile_base, 8ull * col + tile_base, id, col, sum);
    // the kernel hands over its word of four fifth bytes shifted down by 8 k: the bytes above the item's own must not matter
    for (unsigned junk : {0xffffff00u, 0x5a5a5a00u, 0x00000100u})
        expect_eq("sum address under the other items' fifth bytes", tall_item_sum_bytes(it.word, it.fifth | junk), 8ull * sum, id, col, sum);
}

static void fp64_item(unsigned col, unsigned sum, unsigned tile_base) {
    const unsigned w = tall_item64_encode(col, sum);
    expect_eq("fp64 word", w, ((unsigned long long)sum << 3) | ((unsigned long long)col << 17), 0, col, sum);
    expect_eq("fp64 column", tall_item64_column(w), col, 0, col, sum);
    expect_eq("fp64 sum field", tall_item64_sum(w), sum, 0, col, sum);
    expect_eq("fp64 sum address", tall_item64_sum_bytes(w), 8ull * sum, 0, col, sum);
    expect_eq("fp64 x address", (tall_item64_column(w) << 3) + tile_base, 8ull * col + tile_base, 0, col, sum);
}

int main() {
    // field boundaries: 0, 1, every power of two and its neighbours, the largest value
    const unsigned ids[] = {0, 1, 2, 1023, 1024, 1025, 2046, 2047};
    const unsigned cols[] = {0, 1, 2047, 2048, 3071, 3072, 4094, 4095};
    const unsigned sums[] = {0, 1, 62, 63, 64, 65, 127, 128, 255, 256, 8191, 8192, 8193, 13021, 13022, 15361, 16382, 16383};
    for (unsigned id : ids)
        for (unsigned col : cols)
            for (unsigned sum : sums) {
                dict_item(id, col, sum, 106496u);
                fp64_item(col, sum, 106496u);
            }
    std::mt19937 rng(20251);
    for (int i = 0; i < 100000; ++i) {
        const unsigned id = rng() & 2047u, col = rng() & 4095u, sum = rng() & 16383u, tile = (rng() % 20000u) * 8u;
        dict_item(id, col, sum, tile);
        fp64_item(col, sum, tile);
    }
    // the all-zero item is the scratch cell (LDS address 0), entry 0 of the table, column 0
    expect_eq("zero item: sum address", tall_item_sum_bytes(0u, 0u), 0);
    expect_eq("zero item: value offset", tall_item_value_bytes(0u), 0);
    expect_eq("zero item: column", tall_item_column(0u), 0);
    expect_eq("zero fp64 item: sum address", tall_item64_sum_bytes(0u), 0);
    expect_eq("zero fp64 item: column", tall_item64_column(0u), 0);
    // and nothing else is: local row 0 lies behind the scratch cell and the table
    expect_eq("sum field of local row 0, no table", tall_item_sum_base(0), 1);
    expect_eq("sum field of local row 0, table of 1280", tall_item_sum_base(1280), 1281);
    expect_eq("the largest sum field fits 14 bits", tall_item_sum_base(2048) + 13312u - 1u < 16384u, 1);
    std::printf("%s: %d checks, %d failures\n", failures ? "FAILED" : "ok", checks, failures);
    return failures ? 1 : 0;
}

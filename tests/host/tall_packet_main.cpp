// The payload of a packet of the tall-cell format in its two forms (pysparselp_amd/csrc/slp_tall_item.h: tall_packet_layout and
// its companions -- the one text the builder writes with, the product kernel reads with and the planner sizes with), built with
// -fsanitize=address,undefined and run as a child process by tests/test_tall_packet_host.py.  The reading side is written out
// here from the format's description, never from the header's constants.  w[k]: lanes whose list is longer than slot k.
//   slot-major: slot k's word of lane p at off + w[0] + .. + w[k-1] + p; the fifth bytes of slots 0-3 at off + w[0] + .. + w[7] + p,
//               those of slots 4-7 w[0] words further on
//   records:    the record of lane p is the four words at off + 4 p, its fifth bytes the word at off + 4 w[0] + p; the second
//               group starts at off + 5 w[0] (fp64 values: 4 w[0]) with slot k's word of lane p at the sum of the widths of the
//               slots 4 .. k - 1 + p, and the fifth bytes of slots 4-7 follow slot 7
// Prints "ok: <checks> checks, 0 failures".
#include "slp_tall_item.h"

#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

using namespace slp;

static int failures = 0, checks = 0;
static void expect_eq(const char *what, unsigned long long got, unsigned long long want, unsigned a = 0, unsigned b = 0, unsigned c = 0) {
    ++checks;
    if (got == want) return;
    if (++failures <= 20) std::printf("FAIL %s (lane %u, slot %u, packet %u): %llu, expected %llu\n", what, a, b, c, got, want);
}

// A host model of one cell's packets.  `len[p]`: the list length of lane p (non-increasing).  The builder's side writes every
// lane's items through tall_packet_layout / tall_packet_item_word into a payload filled with a sentinel, exactly as k_tall_build
// does; the kernel's side reads them back by the formulas above.  Item of lane p at list position q: a unique (id, column, sum
// field) triple.
static void packet_model(const std::vector<unsigned> &len, bool dict, bool records) {
    const unsigned lanes = (unsigned)len.size(), kSentinel = 0xdeadbeefu;
    unsigned longest = 0, lane_words = 0;
    for (unsigned l : len) { longest = l > longest ? l : longest; lane_words += tall_packet_lane_words(l, dict, records); }
    auto triple = [&](unsigned p, unsigned q, unsigned *id, unsigned *col, unsigned *sum) {
        *id = (p * 7u + q * 131u) & 2047u; *col = (p * 3u + q * 517u) & 4095u; *sum = 1u + ((p * 11u + q * 1031u) % 16383u);
    };
    std::vector<unsigned> pay;
    std::vector<unsigned> offs;   // every packet's offset
    std::vector<std::vector<unsigned>> widths;
    for (unsigned g = 0; g * 8u < longest || g == 0; ++g) {
        unsigned w[8];
        for (unsigned k = 0; k < 8; ++k) { w[k] = 0; for (unsigned l : len) w[k] += l > 8u * g + k; }
        const TallPacketLayout lay = tall_packet_layout(w, dict, records);
        const unsigned off = (unsigned)pay.size();
        pay.resize(off + lay.words, kSentinel);
        offs.push_back(off);
        widths.emplace_back(w, w + 8);
        for (unsigned p = 0; p < lanes; ++p) {       // the builder's lane p
            unsigned fifth[2] = {0, 0};
            for (unsigned k = 0; k < 8; ++k) {
                if (p >= w[records && k < 4 ? 0 : k]) continue;   // (records: a lane of slot 0 writes its whole record)
                unsigned word = 0, hib = 0, id, col, sum;
                if (len[p] > 8u * g + k) {
                    triple(p, 8u * g + k, &id, &col, &sum);
                    if (dict) { const TallItem it = tall_item_encode(id, col, sum); word = it.word; hib = it.fifth; }
                    else word = tall_item64_encode(col, sum);
                }
                const unsigned at = off + tall_packet_item_word(lay, records, p, (int)k);
                expect_eq("a payload word is written once", pay.at(at), kSentinel, p, k, g);
                pay.at(at) = word;
                fifth[k / 4] |= hib << (8 * (k % 4));
            }
            if (dict && p < w[0]) { expect_eq("fifth-byte word written once", pay.at(off + lay.fifth0 + p), kSentinel, p, 0, g); pay.at(off + lay.fifth0 + p) = fifth[0]; }
            if (dict && p < w[4]) { expect_eq("fifth-byte word written once", pay.at(off + lay.fifth1 + p), kSentinel, p, 4, g); pay.at(off + lay.fifth1 + p) = fifth[1]; }
        }
        // where the kernel's second half starts
        expect_eq("the second group's first word", tall_packet_group1_word(w, dict, records), records ? (dict ? 5u : 4u) * w[0] : w[0] + w[1] + w[2] + w[3]);
    }
    expect_eq("the cell's words are the sum of the lanes' words", pay.size(), lane_words);
    for (unsigned w : pay) expect_eq("no word is left unwritten", w != kSentinel, 1);
    // the kernel's side
    std::vector<unsigned> seen(pay.size(), 0);
    for (size_t g = 0; g < offs.size(); ++g) {
        const unsigned off = offs[g];
        const std::vector<unsigned> &w = widths[g];
        for (unsigned p = 0; p < lanes; ++p) {
            unsigned lo[8] = {0, 0, 0, 0, 0, 0, 0, 0}, hi[2] = {0, 0};
            unsigned so = off;
            if (records) {
                if (p < w[0]) {      // one 16-byte load; past w0 the descriptor ends: zeros
                    for (unsigned k = 0; k < 4; ++k) { lo[k] = pay.at(off + 4u * p + k); ++seen.at(off + 4u * p + k); }
                    if (dict) { hi[0] = pay.at(off + 4u * w[0] + p); ++seen.at(off + 4u * w[0] + p); }
                }
                so = off + (dict ? 5u : 4u) * w[0];
            } else {
                for (unsigned k = 0; k < 4; ++k) {   // four loads, each with its slot's end: past w[k] zeros
                    if (p < w[k]) { lo[k] = pay.at(so + p); ++seen.at(so + p); }
                    so += w[k];
                }
            }
            for (unsigned k = 4; k < 8; ++k) {
                if (p < w[k]) { lo[k] = pay.at(so + p); ++seen.at(so + p); }
                so += w[k];
            }
            if (dict && !records && p < w[0]) { hi[0] = pay.at(so + p); ++seen.at(so + p); }
            if (!records) so += dict ? w[0] : 0u;
            if (dict && p < w[4]) { hi[1] = pay.at(so + p); ++seen.at(so + p); }
            for (unsigned k = 0; k < 8; ++k) {
                const unsigned q = 8u * (unsigned)g + k;
                const unsigned sum_addr = dict ? tall_item_sum_bytes(lo[k], hi[k / 4] >> (8 * (k % 4))) : tall_item64_sum_bytes(lo[k]);
                if (len[p] > q) {
                    unsigned id, col, sum;
                    triple(p, q, &id, &col, &sum);
                    expect_eq("item found: sum address", sum_addr, 8ull * sum, p, k, (unsigned)g);
                    expect_eq("item found: column", dict ? tall_item_column(lo[k]) : tall_item64_column(lo[k]), col, p, k, (unsigned)g);
                    if (dict) expect_eq("item found: value offset", tall_item_value_bytes(lo[k]), 8ull * id, p, k, (unsigned)g);
                } else {
                    expect_eq("padding and words past a slot are zero", lo[k], 0, p, k, (unsigned)g);
                    expect_eq("... and land in the scratch cell", sum_addr, 0, p, k, (unsigned)g);
                }
            }
        }
    }
    for (unsigned n : seen) expect_eq("every word is read by exactly one lane", n, 1);
}

static void packet_cases() {
    for (bool records : {false, true})
        for (bool dict : {true, false}) {
            std::mt19937 rng(7);
            // lists of 0 .. 9 items over 1024 lanes, non-increasing, every width an odd number of lanes (no multiple of 64)
            {
                std::vector<unsigned> len(1024);
                const unsigned steps[10] = {1023, 1001, 901, 777, 503, 333, 131, 67, 3, 1};   // lanes whose list is longer than k
                for (unsigned p = 0; p < 1024; ++p) { len[p] = 0; for (unsigned k = 0; k < 10; ++k) len[p] += p < steps[k]; }
                packet_model(len, dict, records);
            }
            // lists of 3, 4 and 5: slot 3 narrower than slot 0, a fifth-item slot one and two lanes wide
            for (unsigned five : {1u, 2u}) {
                std::vector<unsigned> len(1024);
                for (unsigned p = 0; p < 1024; ++p) len[p] = p < five ? 5 : p < 504 ? 4 : 3;
                packet_model(len, dict, records);
            }
            // all lanes alike (widths of 1024): lists of 4, of 8 and of 9 (a second packet whose record holds one item), an empty
            // cell's single packet
            for (unsigned l : {0u, 4u, 8u, 9u}) packet_model(std::vector<unsigned>(1024, l), dict, records);
            // random non-increasing lists
            for (int t = 0; t < 20; ++t) {
                std::vector<unsigned> len(1024);
                unsigned cur = rng() % 10u;
                for (unsigned p = 0; p < 1024; ++p) { if (cur && rng() % 97u == 0) --cur; len[p] = cur; }
                packet_model(len, dict, records);
            }
        }
}

int main() {
    packet_cases();
    std::printf("%s: %d checks, %d failures\n", failures ? "FAILED" : "ok", checks, failures);
    return failures ? 1 : 0;
}

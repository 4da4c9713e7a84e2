// The scalar arithmetic of the duality-gap certificate (csrc/slp_cp_gap.h) under the host compiler: reads cases from the file
// named on the command line, one per line -- an operation and its arguments as the 64-bit patterns of doubles in hexadecimal --
// and prints the bits of each result.  tests/test_cp_gap_decide_host.py writes the cases and compares.
//   max a b | min a b | col d lb ub | row y b | viol so_far v equality | decide primal cols sy violation tol_gap tol_feas
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "slp_cp_gap.h"

static double from_bits(uint64_t u) {
    double d;
    std::memcpy(&d, &u, sizeof d);
    return d;
}

static uint64_t bits(double d) {
    uint64_t u;
    std::memcpy(&u, &d, sizeof u);
    return u;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::FILE *f = std::fopen(argv[1], "r");
    if (!f) return 2;
    char op[16];
    int cases = 0;
    while (std::fscanf(f, "%15s", op) == 1) {
        const int want = !std::strcmp(op, "decide") ? 6 : (!std::strcmp(op, "col") || !std::strcmp(op, "viol")) ? 3 : 2;
        double a[6] = {0, 0, 0, 0, 0, 0};
        for (int k = 0; k < want; ++k) {
            uint64_t u;
            if (std::fscanf(f, "%" SCNx64, &u) != 1) return 3;
            a[k] = from_bits(u);
        }
        if (!std::strcmp(op, "max")) std::printf("%016" PRIx64 "\n", bits(slp::nan_max(a[0], a[1])));
        else if (!std::strcmp(op, "min")) std::printf("%016" PRIx64 "\n", bits(slp::nan_min(a[0], a[1])));
        else if (!std::strcmp(op, "col")) std::printf("%016" PRIx64 "\n", bits(slp::cp_gap_col_term(a[0], a[1], a[2])));
        else if (!std::strcmp(op, "row")) std::printf("%016" PRIx64 "\n", bits(slp::cp_gap_row_term(a[0], a[1])));
        else if (!std::strcmp(op, "viol")) std::printf("%016" PRIx64 "\n", bits(slp::cp_gap_violation(a[0], a[1], a[2] != 0.0)));
        else if (!std::strcmp(op, "decide")) {
            double bound;
            const bool stop = slp::cp_gap_decide(a[0], a[1], a[2], a[3], a[4], a[5], &bound);
            std::printf("%016" PRIx64 " %d\n", bits(bound), stop ? 1 : 0);
        } else return 4;
        ++cases;
    }
    std::fclose(f);
    std::fprintf(stdout, "ok: %d cases\n", cases);
    return 0;
}

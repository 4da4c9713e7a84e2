// The scalar rule that repairs an ADMM multiplier for the duality-gap certificate (csrc/slp_admm_gap.h) under the host compiler:
// reads cases from the file named on the command line, one per line -- a, lam, lb, ub as the 64-bit patterns of doubles in
// hexadecimal -- and prints, per case, whether the slack column answers "unbounded" and the bits of the multiplier the
// certificate uses.  tests/test_admm_gap_dual_host.py writes the cases and compares with tests/admm_gap_cpu.py.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "slp_admm_gap.h"

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
    int cases = 0;
    uint64_t u[4];
    while (std::fscanf(f, "%" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64, &u[0], &u[1], &u[2], &u[3]) == 4) {
        const double a = from_bits(u[0]), lam = from_bits(u[1]), lb = from_bits(u[2]), ub = from_bits(u[3]);
        const bool repaired = slp::admm_gap_slack_unbounded(a, lam, lb, ub);
        std::printf("%d %016" PRIx64 "\n", repaired ? 1 : 0, bits(slp::admm_gap_dual(lam, repaired)));
        ++cases;
    }
    std::fclose(f);
    std::fprintf(stdout, "ok: %d cases\n", cases);
    return 0;
}

// slp_many.h -- what the list solvers (slp_cp_many.hip, slp_admm_many.hip, slp_dga_many.hip) share on the HIP side; the decisions
// that need no device are in slp_many_plan.h.
#pragma once
#include "slp_common.h"
#include "slp_kernels.h"
#include "slp_many_plan.h"

namespace slp {

// row `r` of an LP (equality rows first) in a matrix that holds the equality rows of all LPs before their inequality rows
__device__ __forceinline__ i64 many_row(i64 eq0, i64 in0, i32 m_eq, i32 r) { return r < m_eq ? eq0 + r : in0 + (r - m_eq); }

// max as np.max: a NaN on either side stays (the per-LP stopping tests of slp_cp_many.hip and slp_admm_many.hip)
__device__ __forceinline__ double many_nanmax(double m, double d) { return (d > m || d != d) ? d : m; }

// the same over the 64 lanes of a wave, by shuffles: lane 0 holds the result
__device__ __forceinline__ double many_wave_nanmax(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = many_nanmax(v, __shfl_down(v, off, kWave));
    return v;
}

// the sum over the 64 lanes of a wave, by shuffles in a fixed order (32, 16, ..., 1): lane 0 holds the result, a function of the
// lanes' values only (the certificate of slp_cp_many.hip)
__device__ __forceinline__ double many_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
    return v;
}

// the lists of the LPs of each form, on the device
inline void many_upload_lists(const ManyGroup group[2], DevBuf<i32> list[2]) {
    for (int g = 0; g < 2; ++g)
        if (!group[g].ids.empty()) list[g].upload(group[g].ids.data(), group[g].ids.size());
}

// dynamic LDS beyond 48 KiB is asked for by name, once per kernel: up to the whole limit of the form
inline void many_lds_opt_in(const void *kernel, size_t lds_bytes, size_t limit_bytes) {
    if (lds_bytes > 48 * 1024) SLP_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)limit_bytes));
}

// `k` iterations in launches of at most `kmax`: launch(want) enqueues up to `want` iterations and returns how many it took
// (0 ends the run early)
template <class F>
void many_split(i64 k, i64 kmax, F launch) {
    for (i64 done = 0; done < k;) {
        const int it = launch((int)std::min<i64>(kmax, k - done));
        if (it < 1) break;
        SLP_HIP(hipGetLastError());
        done += it;
    }
}

// refuses a list whose set-up would not fit: `need` bytes against what the driver and the library's own cache have free
inline void many_require_memory(const char *who, i64 count, double need) {
    i64 free_b = 0, total_b = 0;
    SLP_REQUIRE(slp_device_memory(&free_b, &total_b) == 0, slp_last_error());
    const double have = (double)free_b + (double)slp_cached_bytes();
    if (need > have)
        throw Error(std::string(who) + ": " + std::to_string(count) + " LPs need " + std::to_string(need / 1e9) + " GB of device memory, " +
                    std::to_string(have / 1e9) + " GB are free");
}

}  // namespace slp

// slp_many.h -- what the list solvers (slp_cp_many.hip, slp_admm_many.hip, slp_dga_many.hip) share on the HIP side; the decisions
// that need no device are in slp_many_plan.h.  The NaN-propagating nan_max / nan_min of every per-LP stopping test are in
// slp_cp_gap.h, included here: that header compiles without HIP, so the host test of the certificate pins the same text.
#pragma once
#include "slp_common.h"
#include "slp_cp_gap.h"
#include "slp_kernels.h"
#include "slp_many_plan.h"

namespace slp {

// row `r` of an LP (equality rows first) in a matrix that holds the equality rows of all LPs before their inequality rows
__device__ __forceinline__ i64 many_row(i64 eq0, i64 in0, i32 m_eq, i32 r) { return r < m_eq ? eq0 + r : in0 + (r - m_eq); }

// Q values over the 64 lanes of a wave, by shuffles in a fixed order (32, 16, ..., 1) -- bit q of MAXES: v[q] by nan_max
// (slp_cp_gap.h), else a sum, a function of the lanes' values only -- the Q chains side by side: lane 0 holds the results
template <int Q, unsigned MAXES>
__device__ __forceinline__ void many_wave_reduce(double *v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const double o = __shfl_down(v[q], off, kWave);
            v[q] = ((MAXES >> q) & 1) ? nan_max(v[q], o) : v[q] + o;
        }
    }
}
// one nan-max (slp_dga_many.hip)
__device__ __forceinline__ double many_wave_nanmax(double v) {
    many_wave_reduce<1, 1>(&v);
    return v;
}

// ---- the per-LP stopping protocol of a list kernel that can be resumed (k_cpm_iterate with either test, k_admmm_iterate) ----
// The head of an LP's control record in device memory; a solver's record derives from it and adds what its test evaluates.
// Written by lane 0 of the LP's workgroup and by the host between launches; the unarmed kernels touch no word of it.
struct ManyCtl {
    i64 done;       // whole iterations completed
    i64 stop_iter;  // `done` when it stopped
    i32 stopped, pad;
};

// Entering a launch: false for an LP that stopped in an earlier launch (the same for every lane: the workgroup returns before
// its first barrier).  *done: iterations completed; *until: iterations up to and including the next check.  Lane 0 writes the
// record only behind a barrier that follows these loads.
__device__ __forceinline__ bool many_enter(const ManyCtl *ctl, i64 check_every, i64 *done, i64 *until) {
    if (ctl->stopped) return false;
    *done = ctl->done;
    *until = check_every - *done % check_every;
    return true;
}

// a wave's many_wave_reduce of v[0..Q) into its slots, slots[q * stride + wave]; read behind a later barrier.  The Q reductions
// run side by side before the one guarded block of stores (one after the other, each with its store, they cost 4 % of an iteration
// of k_cpm_iterate_gap at check_every = 1: profiles/cp_fold_ab.json)
template <int Q, unsigned MAXES>
__device__ __forceinline__ void many_post(double *slots, int stride, i32 tid, double *v) {
    many_wave_reduce<Q, MAXES>(v);
    if ((tid & (kWave - 1)) == 0) {
#pragma unroll
        for (int q = 0; q < Q; ++q) slots[q * stride + tid / kWave] = v[q];
    }
}

// lane 0: Q quantities of a workgroup of W lanes, quantity q in slots[q * stride + wave], each folded over the waves in
// increasing order -- bit q of MAXES: by nan_max, else a sum -- in ONE loop, so that the Q chains of LDS loads overlap (a loop per
// quantity cost 4 % of an iteration of k_cpm_iterate<., true> and 7 % of one of k_cpm_iterate_gap at check_every = 1:
// profiles/cp_fold_ab.json)
template <int Q, unsigned MAXES>
__device__ __forceinline__ void many_fold(const double *slots, int stride, i32 W, double *out) {
#pragma unroll
    for (int q = 0; q < Q; ++q) out[q] = slots[q * stride];
    for (i32 w = 1; w < W / kWave; ++w) {
#pragma unroll
        for (int q = 0; q < Q; ++q) out[q] = ((MAXES >> q) & 1) ? nan_max(out[q], slots[q * stride + w]) : out[q] + slots[q * stride + w];
    }
}

// lane 0, at the end of check iteration `done`: the record's head and the ONE decision slot
__device__ __forceinline__ void many_decide(ManyCtl *ctl, i64 done, bool stop, double *slot) {
    if (stop) {
        ctl->stopped = 1;
        ctl->stop_iter = done;
    }
    *slot = stop ? 1.0 : 0.0;
}

// every lane: the barrier the test adds to a check iteration, then the slot -- read by every lane, so the break is uniform
__device__ __forceinline__ bool many_decided(const double *slot) {
    __syncthreads();
    return *slot != 0.0;
}

// ---- the list of the live LPs, built on the device in front of a launch that runs over it (slp_dga_many.hip) ----
// ONE workgroup of kManyLiveLanes lanes; `pred(k)` says whether LP k is live.  live[0 .. *live_n) receives the live LPs in
// increasing order, the rest of live[] (`count` entries) stays as it was.  The chunk of a lane, its count and its stores are
// slp_many_plan.h's; here is the exclusive prefix of the 1024 counts: inclusive over the wave by shuffles, the 16 wave totals
// through LDS, one fold that gives a lane the waves in front of it and the total.  Integers only, so the order of additions is
// free.  No atomic, no wait; both loops of a lane are bounded by `count`; the one barrier is reached by every lane.  The flags
// `pred` reads are written by earlier launches on the same stream only, so a lane's two passes see the same values.
template <class Pred>
__global__ __launch_bounds__(kManyLiveLanes) void k_many_live(Pred pred, i32 count, i32 *__restrict__ live, i32 *__restrict__ live_n) {
    __shared__ i32 totals[kManyLiveLanes / kWave];
    const i32 tid = (i32)threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const ManyLiveRange r = many_live_range(count, tid);
    const i32 mine = many_live_count(r, pred);
    i32 upto = mine;   // inclusive over the wave
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const i32 o = __shfl_up(upto, off, kWave);
        if (lane >= off) upto += o;
    }
    if (lane == kWave - 1) totals[wave] = upto;
    __syncthreads();
    i32 before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kManyLiveLanes / kWave; ++w) {
        const i32 t = totals[w];
        before += w < wave ? t : 0;
        all += t;
    }
    many_live_write(r, before + upto - mine, live, pred);
    if (tid == 0) *live_n = all;
}

// the live list of each form of a solver with two forms (slp_cp_many.hip, slp_admm_many.hip), and what its last launches were
struct ManyFormLists {
    DevBuf<i32> ids[2], n[2];   // allocated at the first use: as many entries as the form has LPs, and one
    bool on = false;            // compaction (slp_many_*_set_compaction; off after create)
    i64 launched[2] = {0, 0};   // the workgroups of the form's last iteration launch
    i64 cap[2] = {0, 0};        // the cap of the last call that launched the form
};

inline void many_form_alloc(ManyFormLists &l, const ManyGroup group[2]) {
    for (int g = 0; g < 2; ++g) {
        if (l.n[g].p) continue;
        l.ids[g].alloc(std::max<size_t>(1, group[g].ids.size()));
        l.n[g].alloc(1);
    }
}

// the list of form g from the flags as they are on the device, behind everything enqueued so far: at most the form's LPs
template <class Lp, class Ctl>
void many_form_list(ManyFormLists &l, const ManyGroup group[2], int g, const Lp *lps, const Ctl *ctl, i64 count) {
    many_form_alloc(l, group);
    hipLaunchKernelGGL((k_many_live<ManyFormLive<Lp, Ctl>>), dim3(1), dim3(kManyLiveLanes), 0, ctx().stream, ManyFormLive<Lp, Ctl>{lps, ctl, g},
                       (i32)count, l.ids[g].p, l.n[g].p);
}

// what both *_live_state calls do behind their handle check (include/slp_hip_ext_many_live.h); synchronises
template <class Lp, class Ctl>
void many_form_state(const char *who, ManyFormLists &l, const ManyGroup group[2], const Lp *lps, const Ctl *ctl, i64 count, int64_t *live,
                     int32_t *order, int64_t *launched, int64_t *cap) {
    i64 at = 0;
    for (int g = 0; g < 2; ++g) {
        many_form_list(l, group, g, lps, ctl, count);
        SLP_HIP(hipGetLastError());
        i32 n = 0;
        l.n[g].download(&n, 1);   // synchronises
        if (n < 0 || n > (i64)group[g].ids.size()) throw Error(std::string(who) + ": the device's count of live LPs is out of range");
        if (live) live[g] = n;
        if (order && n) l.ids[g].download(order + at, (size_t)n);
        at += n;
        if (launched) launched[g] = l.launched[g];
        if (cap) cap[g] = l.cap[g];
    }
    if (order) std::fill(order + at, order + count, -1);
}

// host: the records with the iterations of the unarmed launches added (no LP is stopped while the test is off); synchronises
template <class Ctl>
std::vector<Ctl> many_read_ctl(const DevBuf<Ctl> &ctl, i64 count, i64 uncounted) {
    std::vector<Ctl> h((size_t)count);
    ctl.download(h.data(), h.size());
    for (Ctl &c : h) c.done += uncounted;
    return h;
}

// host: every flag cleared and the uncounted iterations moved into the records, for a set_stop call
template <class Ctl>
void many_rearm(DevBuf<Ctl> &ctl, i64 count, i64 *uncounted) {
    std::vector<Ctl> h = many_read_ctl(ctl, count, *uncounted);
    for (Ctl &c : h) c.stopped = 0;
    ctl.upload(h.data(), h.size());
    *uncounted = 0;
}

// host: what every *_state call reports from the head of record k
inline void many_state_head(const ManyCtl &c, size_t k, int64_t *iterations, int32_t *stopped) {
    if (iterations) iterations[k] = c.stopped ? c.stop_iter : c.done;
    if (stopped) stopped[k] = c.stopped;
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

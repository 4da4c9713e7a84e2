// slp_many_plan.h -- what the three list solvers (slp_cp_many.hip, slp_admm_many.hip, slp_dga_many.hip: one workgroup per LP, whole
// iterations inside one launch) decide from the shapes of the LPs and the environment switches alone.  Pure host code: no HIP, no
// device buffer, no context -- the number of compute units is an argument.  A refusal is a std::runtime_error, which the
// SLP_API_* macros of slp_common.h turn into slp_last_error like every other.
//
// Two forms (Chambolle-Pock and ADMM), the same arithmetic, chosen per LP from its shape only:
//   lds     the iterates of the LP (`doubles` of them, the solver's own count) are at most the solver's limit: they live in LDS for
//           the whole launch, loaded at its start and written back at its end;
//   global  they stay in global memory and are re-read across the barriers with workgroup-scope relaxed loads, nothing kept in a
//           register across a barrier.
// SLP_<solver>_MANY_FORM=lds|global forces one form on every LP; a forced lds that does not fit is refused.  The LPs of each form
// are one launch (ManyGroup): the list of its LPs, its workgroup width, its dynamic LDS and its launch cap.
//
// Workgroup width: the smallest power of two >= what the solver wants for the LPs of the launch, clamped to 64 .. max_block lanes
// (lanes loop beyond).
//
// Launch cap.  A pass is the workgroup once over its columns, its rows, a level or a stage -- each solver counts the passes of one
// iteration of its largest LP.  A launch holds at most kManyUnitsPerLaunch passes per compute unit:
//   iterations per launch = kManyUnitsPerLaunch / (passes * ceil(workgroups / compute units)),
// between 1 and kManyMaxItersPerLaunch; longer runs are split (many_split, slp_many.h).  SLP_<solver>_MANY_KMAX=<k> lowers the upper
// end (1: one iteration per launch).  The iterates do not depend on the split.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

namespace slp {

constexpr int64_t kManyUnitsPerLaunch = 8192;
constexpr int64_t kManyMaxItersPerLaunch = 1024;

// the LPs of one launch
struct ManyGroup {
    std::vector<int32_t> ids;
    int block = 64;
    size_t lds_bytes = 0;
    int64_t kmax = 1;  // iterations one launch may hold
    int64_t passes = 1;  // what kmax was made of: the passes of one iteration of the group's largest LP
};

// the switch `name`: -1 when unset or empty, 0 for lds, 1 for global
inline int many_form_switch(const char *name) {
    const char *e = getenv(name);
    if (!e || !e[0]) return -1;
    if (!strcmp(e, "lds")) return 0;
    if (!strcmp(e, "global")) return 1;
    throw std::runtime_error(std::string(name) + " must be lds or global, not " + e);
}

// the switch `name` as the upper end of the launch cap: `cap` when unset or empty, else min(cap, its value)
inline int64_t many_kmax_switch(const char *name, int64_t cap) {
    const char *e = getenv(name);
    if (!e || !e[0]) return cap;
    char *end = nullptr;
    const long long v = strtoll(e, &end, 10);
    if (v < 1 || *end) throw std::runtime_error(std::string(name) + " must be a positive number of iterations, not " + e);
    return std::min<int64_t>(cap, v);
}

// The form of every LP (0 lds, 1 global) from the doubles it would hold in LDS; group[f].ids receives the LPs of form f in
// increasing order.  `force`: many_form_switch(form_switch); `what`: the solver's count of doubles in words, e.g. "2 n + m".
inline std::vector<int32_t> many_assign_forms(const std::vector<int64_t> &doubles, int64_t limit, int force, const char *who,
                                              const char *form_switch, const char *what, ManyGroup group[2]) {
    std::vector<int32_t> form(doubles.size());
    for (size_t k = 0; k < doubles.size(); ++k) {
        const bool fits = doubles[k] <= limit;
        if (force == 0 && !fits)
            throw std::runtime_error(std::string(who) + ": " + form_switch + "=lds, but LP " + std::to_string(k) + " needs " +
                                     std::to_string(doubles[k]) + " doubles of LDS (" + what + ") and the form holds " + std::to_string(limit));
        form[k] = force >= 0 ? force : (fits ? 0 : 1);
        group[form[k]].ids.push_back((int32_t)k);
    }
    return form;
}

inline int many_width(int64_t want, int max_block) {
    int w = 64;
    while (w < want && w < max_block) w *= 2;
    return w;
}

// iterations one launch of `workgroups` workgroups may hold; `cap`: many_kmax_switch
inline int64_t many_launch_cap(int64_t units, int64_t passes, int64_t workgroups, int64_t cus, int64_t cap) {
    cus = std::max<int64_t>(1, cus);
    const int64_t rounds = (workgroups + cus - 1) / cus;
    return std::min(cap, std::max<int64_t>(1, units / (passes * rounds)));
}

// ---- the list of the live LPs (k_many_live, slp_many.h): one workgroup of kManyLiveLanes lanes, lane t owns the LPs
// [t per, min((t + 1) per, count)) with per = ceil(count / kManyLiveLanes), counts its live ones and writes their numbers, in
// increasing order, from the exclusive prefix of the counts on.  The arithmetic below is the kernel's and the host test's one text
// (constexpr: host and device alike under hipcc).
constexpr int32_t kManyLiveLanes = 1024;

struct ManyLiveRange {
    int32_t lo, hi;   // lo == hi: a lane past the end owns nothing
};

constexpr int32_t many_live_per(int32_t count) { return (count + kManyLiveLanes - 1) / kManyLiveLanes; }

constexpr ManyLiveRange many_live_range(int32_t count, int32_t lane) {
    const int64_t per = many_live_per(count), lo = per * lane, hi = lo + per;   // 64 bits: 1023 per may pass count by far
    return ManyLiveRange{(int32_t)(lo < count ? lo : count), (int32_t)(hi < count ? hi : count)};
}

// a lane's live LPs; `live(k)` is the solver's predicate
template <class Pred>
constexpr int32_t many_live_count(ManyLiveRange r, const Pred &live) {
    int32_t n = 0;
    for (int32_t k = r.lo; k < r.hi; ++k) n += live(k) ? 1 : 0;
    return n;
}

// the lane's live LPs into out[at], out[at + 1], ...: `at` is the number of live LPs of the lanes before it
template <class Pred>
constexpr void many_live_write(ManyLiveRange r, int32_t at, int32_t *out, const Pred &live) {
    for (int32_t k = r.lo; k < r.hi; ++k)
        if (live(k)) out[at++] = k;
}

// iterations a launch of a call may hold when `live` LPs are live at its start: the cap of that many workgroups
inline int64_t many_live_cap(int64_t passes, int64_t live, int64_t cus, int64_t cap) {
    return many_launch_cap(kManyUnitsPerLaunch, passes, std::max<int64_t>(1, live), cus, cap);
}

// ---- the live list per form (slp_cp_many.hip, slp_admm_many.hip: the LPs of each form are a launch of their own) ----
// "LP k has form `form` and is not stopped", over ALL LPs of the list: the predicate k_many_live takes for the list of one form.
// Lp: the solver's table entry (its `form`: 0 lds, 1 global); Ctl: its control record, whose head is ManyCtl (its `stopped`) -- a
// template, because the records of the solvers differ in size.  constexpr: host and device alike under hipcc.
template <class Lp, class Ctl>
struct ManyFormLive {
    const Lp *lps;
    const Ctl *ctl;
    int32_t form;
    constexpr bool operator()(int32_t k) const { return lps[k].form == form && ctl[k].stopped == 0; }
};

// per form: the LPs live now and the iterations a launch over that many workgroups may hold
struct ManyFormCall {
    int64_t live[2], cap[2];
};

// What a compacted call is made of, from the records read back (`ctl`, one per LP of `lps`): per form the number of live LPs --
// ManyFormLive counted by the chunk plan's own loop -- and many_live_cap of the group's passes for that many workgroups (a form
// without a live LP launches nothing; its cap is that of one workgroup).  `cap`: many_kmax_switch.
template <class Lp, class Ctl>
inline ManyFormCall many_form_call(const std::vector<Lp> &lps, const Ctl *ctl, const ManyGroup group[2], int64_t cus, int64_t cap) {
    ManyFormCall r;
    for (int g = 0; g < 2; ++g) {
        r.live[g] = many_live_count(ManyLiveRange{0, (int32_t)lps.size()}, ManyFormLive<Lp, Ctl>{lps.data(), ctl, g});
        r.cap[g] = many_live_cap(group[g].passes, r.live[g], cus, cap);
    }
    return r;
}

// rows r0 <= r < r1 of a CSR block belong to LP `lp`, whose column indices there lie in lo <= j < hi
struct ManyRows {
    int64_t lp, r0, r1, lo, hi;
};

// the wording of many_check_block's refusals: "<who>: <ptr> must start at 0", "<who>: <ptr> <order>",
// "<who>: a row of <rows>LP k has the column index j" + (local ? ", not local to the LP's n columns"
//                                                              : " outside the LP's columns [lo, hi)")
struct ManyBlockText {
    std::string who, ptr, order, rows;
    bool local;
};

// One CSR block of a list, host arrays only: the row pointer starts at 0 and does not decrease over its `rows` rows, the entry
// arrays are there when it has entries, and every LP's rows hold column indices of that LP only.
inline void many_check_block(const ManyBlockText &t, const int64_t *indptr, const int32_t *indices, bool have_entries, int64_t rows,
                             const std::vector<ManyRows> &lps) {
    if (indptr[0] != 0) throw std::runtime_error(t.who + ": " + t.ptr + " must start at 0");
    for (int64_t r = 0; r < rows; ++r)
        if (indptr[r + 1] < indptr[r]) throw std::runtime_error(t.who + ": " + t.ptr + " " + t.order);
    if (indptr[rows] != 0 && !have_entries) throw std::runtime_error(t.who + ": NULL argument");
    for (const ManyRows &s : lps)
        for (int64_t q = indptr[s.r0]; q < indptr[s.r1]; ++q)
            if (indices[q] < s.lo || indices[q] >= s.hi)
                throw std::runtime_error(t.who + ": a row of " + t.rows + "LP " + std::to_string(s.lp) + " has the column index " +
                                         std::to_string(indices[q]) +
                                         (t.local ? ", not local to the LP's " + std::to_string(s.hi - s.lo) + " columns"
                                                  : " outside the LP's columns [" + std::to_string(s.lo) + ", " + std::to_string(s.hi) + ")"));
}

}  // namespace slp

/*
 * slp_hip_ext_dga_many_live.h -- the entry points of libslp_hip.so for running the dual-ascent list solver over the list of its
 * live LPs (compaction).  Included by include/slp_hip_ext.h, so whoever includes that header has these too; a file of its own,
 * so that the text of slp_hip.h, of slp_hip_ext.h's own entry points and of slp_hip_ext_dga_many.h stays as it is.
 * Same conventions as include/slp_hip.h: plain pointers and sizes, 0 on success, slp_last_error() describes a failure,
 * one host thread per handle.
 */
#ifndef SLP_HIP_EXT_DGA_MANY_LIVE_H
#define SLP_HIP_EXT_DGA_MANY_LIVE_H

#include <stdint.h>

#include "slp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- dual gradient ascent on a list of LPs: hand the live LPs consecutive workgroups ---------- *
 * No counterpart in the reference.  An LP is live when it is neither frozen (its start is dual infeasible) nor stopped (by the
 * step test or a cut-off for its bound, slp_hip_ext_dga_many.h).  Without compaction LP k is workgroup k of every iteration
 * launch for the life of the state: a retired LP's workgroup returns at once, but it keeps its place among the workgroups the
 * hardware deals to its XCDs in turn, the grid stays `count` and so does the launch cap.  With compaction on, every iteration
 * launch of a call that is armed, or whose state has a stopped or a frozen LP, runs over a list of the live LPs that a kernel
 * builds on the device in front of it, in increasing LP order: the grid is the number of LPs live when the call began, the
 * iterations one launch holds are those of that many workgroups (slp_many_dga_kmax keeps returning the value of the whole
 * list), and an LP that stops during the call leaves the list at the next launch.  Every LP's x, y, tie draws, flags, stop record
 * and report are bit for bit those of the state without compaction; a call on a state where no LP can stand still is the same
 * launches.  on: 1 or 0 (off, the state after create); anything else is an error.  The list is allocated at the first `on`;
 * nothing else is launched and no record changes.  To be called between iterate calls. */
int slp_many_dual_set_compaction(slp_many_dga *s, int on);
/* Builds the list from the flags as they are and reads it back, whether compaction is on or not: *live its length, order[0 ..
 * *live) the live LPs in the device's order (increasing), order[*live .. count) = -1; *launched the number of workgroups of the
 * last iteration launch and *cap the iterations per launch the last iterate call that launched anything was held to (both 0
 * before the first).  Any pointer may be NULL.  Synchronises. */
int slp_many_dual_live_state(slp_many_dga *s, int64_t *live, int32_t *order, int64_t *launched, int64_t *cap);

#ifdef __cplusplus
}
#endif
#endif /* SLP_HIP_EXT_DGA_MANY_LIVE_H */

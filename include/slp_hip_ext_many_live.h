/*
 * slp_hip_ext_many_live.h -- the entry points of libslp_hip.so for running the Chambolle-Pock and the ADMM list solver over the
 * lists of their live LPs (compaction).  Included by include/slp_hip_ext.h, so whoever includes that header has these too; a file
 * of its own, so that the text of slp_hip.h, of slp_hip_ext.h's own entry points and of the other extension headers stays as it is.
 * Same conventions as include/slp_hip.h: plain pointers and sizes, 0 on success, slp_last_error() describes a failure,
 * one host thread per handle.
 */
#ifndef SLP_HIP_EXT_MANY_LIVE_H
#define SLP_HIP_EXT_MANY_LIVE_H

#include <stdint.h>

#include "slp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Chambolle-Pock and ADMM on a list of LPs: hand the live LPs consecutive workgroups ---------- *
 * No counterpart in the reference.  An LP is live while its stopped flag is clear (the step test or the certificate of
 * Chambolle-Pock, the residual and step test of ADMM; a set_stop call clears every flag).  The LPs of each form (0 lds, 1 global:
 * slp_cp_many_form, slp_admm_many_form) are a launch of their own.  Without compaction an LP keeps its workgroup index in its
 * form's launch for the life of the state: a stopped LP's workgroup returns at once, but the grid stays the number of LPs of the
 * form and so does the launch cap.  With compaction on, a call on an ARMED state (iterate, primal_step / dual_step, sweep_step /
 * multiplier_step) first reads the records back -- one download, which synchronises -- and then runs every launch of a form over
 * a list of that form's live LPs, which a kernel builds on the device in front of the launch, in increasing LP order: the grid is
 * the number of LPs of the form live when the call began, the iterations one launch holds are those of that many workgroups, a
 * form without a live LP launches nothing, and an LP that stops during the call leaves the list at the next launch.  Every LP's
 * iterates, record and report are bit for bit those of the state without compaction.  A call on a state that is not armed (no LP
 * can be stopped) and the timing calls' plain halves are the launches of a state without compaction.  on: 1 or 0 (off, the state
 * after create); anything else is an error.  The lists are allocated at the first `on`; nothing is launched and no record
 * changes.  To be called between iterate calls. */
int slp_many_cp_set_compaction(slp_cp_many *s, int on);
int slp_many_admm_set_compaction(slp_admm_many *s, int on);
/* Builds both forms' lists from the flags as they are and reads them back, whether compaction is on or not: live[g] the number of
 * live LPs of form g; order (`count` entries) the live LPs of the lds form in increasing order, then those of the global form in
 * increasing order, then -1; launched[g] the number of workgroups of that form's last iteration launch and cap[g] the iterations
 * per launch that form was held to in the last call that launched it (both 0 before the first).  Any pointer may be NULL.
 * Synchronises. */
int slp_many_cp_live_state(slp_cp_many *s, int64_t live[2], int32_t *order, int64_t launched[2], int64_t cap[2]);
int slp_many_admm_live_state(slp_admm_many *s, int64_t live[2], int32_t *order, int64_t launched[2], int64_t cap[2]);

#ifdef __cplusplus
}
#endif
#endif /* SLP_HIP_EXT_MANY_LIVE_H */

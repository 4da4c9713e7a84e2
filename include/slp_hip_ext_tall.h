/*
 * slp_hip_ext_tall.h -- a diagnostic of libslp_hip.so for the tall-cell product copies, beside slp_matrix_strip_width and
 * slp_matrix_tall_rows of include/slp_hip.h.  Included by include/slp_hip_ext.h, so whoever includes that header has it too; a
 * file of its own, so that slp_hip.h keeps its 215 entry points and the text of slp_hip_ext.h its two.
 * Same conventions as include/slp_hip.h.
 */
#ifndef SLP_HIP_EXT_TALL_H
#define SLP_HIP_EXT_TALL_H

#include <stdint.h>

#include "slp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 if the orientation's tall-cell copy (builds it if need be) stores the first four list positions of a packet as one 16-byte
 * record per lane, 0 if it stores them slot by slot or is no tall-cell copy; -1 for NULL.  The build's planner chooses per copy
 * by the bytes the records would add (slp_tall_plan.h: at most 1/16 of the planned cell); SLP_TALL_RECORDS=0|1 forces the form.
 * A chunked matrix reports its first chunk's, which every later chunk follows.  Diagnostics: what a test asserts. */
int64_t slp_matrix_tall_records(slp_matrix *a, int transposed);

#ifdef __cplusplus
}
#endif
#endif /* SLP_HIP_EXT_TALL_H */

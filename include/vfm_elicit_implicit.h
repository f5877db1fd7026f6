/*
 * vfm_elicit_implicit.h -- C ABI of the implicit elicitation session of libvfm_hip.so (gfx950): ask, solve the
 * respondent's optimum over EVERY (respondent, partner) pair, ask again -- every round of every respondent of a
 * two-field 'reg' model in one launch.
 *
 * vfm_elicit_solve_f32 (vfm_elicit.h) with the fold of a round exchanged: where that session sets the respondent's
 * posterior to the exact fold-in's optimum over the rows asked alone, this one sets it to the optimum of the respondent's
 * share of the implicit-feedback objective J_imp of vfm_implicit.h, under which the users of a click model were fitted:
 * the rows of the history and the rows asked so far are the observed pairs (their targets, the weight w1), every other
 * partner of the base's range a pair of target 0 and weight w0.
 *
 * Per respondent e of column `field` independently, for round q = 0 .. n_rounds - 1:
 *  1. Score and choose: steps 1-2 of vfm_elicit_field_f32, unchanged in meaning and in bits (vfm_elicit_solve_f32's).  A
 *     pool row whose partner lies outside [lo, lo + n) is never a candidate.
 *  2. Fold in.  e's observed rows are its history in the given order, then the asked rows in the order asked; e's
 *     posterior becomes bitwise what vfm_foldin_solve_implicit_f32 (with the prior: vfm_foldin_solve_implicit_prior_f32)
 *     writes for E = 1 in the row-list form on exactly those rows with this base, w0, w1, kl_weight and lds_dim, and
 *     out_loss is that call's out_loss.  With dw = w1 - w0:
 *       H = kl I + prec [ w0 (T_B + diag(0, SA_B)) + dw sum_{history + asked} (u u^T + diag(0, A)) ]
 *       b = prec [ w0 tu_B + sum (w1 y - dw c_mean) u ],   theta = H^-1 b
 *     and the scales and L_e as vfm_implicit.h gives them.  Always the primal (d + 1) x (d + 1) system; the triangle lives
 *     in LDS when d + 1 <= min(VFM_FOLDIN_SOLVE_LDS_DIM, lds_dim) and in the workgroup's slab otherwise.  The optimum does
 *     not depend on the current row, so `reset` affects round 0's scoring only; the no-answer posterior under J_imp is not
 *     the prior but the base-only optimum, which vfm_foldin_solve_implicit_f32 writes for an entity without rows.
 * The partner field is frozen over the session: `base` is its block, assembled once by vfm_implicit_base_f32 before the
 * call.  A partner's operands are read from the fp32 tables where they are used: the fold has no operand block, and only
 * the score's operand pass over op_x runs before the session kernel.  A respondent's result does not depend on the other
 * respondents, the grid, the stream or where its triangle is stored.  No atomics, no host synchronisation.
 *
 * Conventions: those of vfm_elicit.h (device pointers, launch-only, caller-owned workspace, 0 / VFM_E_* / hipError_t, every
 * argument checked before any HIP call).
 */
#ifndef VFM_ELICIT_IMPLICIT_H
#define VFM_ELICIT_IMPLICIT_H

#include <stdint.h>

#include "vfm_elicit.h"
#include "vfm_implicit.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vfm_elicit_implicit_t {
  float w0, w1;       /* weight of an unobserved pair (> 0) and of an observed one (>= w0), finite                 */
  int64_t lo, n;      /* the partner field's id range [lo, lo + n) within [0, T), n >= 1: the range of `base`      */
  const double* base; /* [vfm_implicit_base_doubles(d)] the partner field's base block (vfm_implicit_base_f32)     */
} vfm_elicit_implicit_t;

/* Workspace of vfm_elicit_implicit_f32 in bytes: the asked flags [P], the score's operands [n_ops, 4d + 2] and, when a
 * (d + 1) x (d + 1) system does not stay in LDS (lds_dim as in vfm_elicit_solve_t), one triangle per workgroup
 * (min(U, VFM_FOLDIN_SOLVE_SLABS)).  VFM_E_INVALID on negative arguments, d outside [1, VFM_FOLDIN_MAX_D] or
 * lds_dim < -1. */
int64_t vfm_elicit_implicit_workspace_bytes(int64_t U, int64_t P, int64_t n_ops, int32_t d, int32_t lds_dim);

/* Run the sessions of p (read as vfm_elicit_solve_f32 reads it: strategy, seed, reset, write, lds_dim, the out_* arrays)
 * under imp; prior: NULL, or the respondents' field prior [2, d + 1] = mean | precision (include/vfm_implicit_prior.h:
 * every fold is then the PRIOR form, and `reset` starts a respondent at that prior).  A respondent id outside [0, T) asks
 * nothing (every out_row -1); a pool row with a partner outside [lo, lo + n) or an operand outside [0, n_ops) is never
 * asked; a history row with a partner outside [lo, lo + n) makes the respondent's means, factor scales and losses NaN (s_w,
 * a function of the counts, stays finite) from its first fold on, as vfm_foldin_solve_implicit_f32 documents.  Under
 * VFM_RANK_TOP / VARIANCE / MEAN its scores are then NaN and nothing more is asked of it; under VFM_RANK_RANDOM, whose
 * score does not read the posterior, it keeps being asked and every fold stays NaN.
 * U = 0: nothing is launched.  VFM_E_INVALID (nothing launched) wherever vfm_elicit_solve_f32 returns it, and for
 * F != 2, imp NULL, base NULL, w0 <= 0, w1 < w0, a weight that is not finite, n < 1 and a range outside [0, T). */
int vfm_elicit_implicit_f32(const vfm_elicit_solve_t* p, const vfm_elicit_implicit_t* imp, const float* prior,
                            void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VFM_ELICIT_IMPLICIT_H */

/*
 * vfm_bound_prior.h -- C ABI of the bound solves of libvfm_hip.so (gfx950) under a learnt field prior:
 * vfm_foldin_bound_f32 (vfm_bound.h) and vfm_foldin_bound_split_f32 (vfm_bound_sweep.h) with the folded field's prior
 * N(m_c, 1 / lam_c) per coordinate c in [0, d] (0: the first-order weight, 1 .. d: the factors) in place of N(0, 1), the
 * entity block of a hierarchical bound sweep (VFM.fit_bound(learn_priors=True); DESIGN.md §4, "Hierarchical bound
 * sweeps").
 *
 * Per entity each round of vfm_bound.h becomes
 *   D_c       = kl lam_c + (0, sum_r w_r A_r)_c
 *   b_c       = sum_r ((y_r - 1/2) - w_r c_mean,r) u_r,c - (0, 1/2 sum_r w_r C_r)_c + kl lam_c m_c
 *   sigma_c^2 = kl / (kl lam_c + sum_r w_r (A_r,c + M_r,c^2))        (c = 0: sum_r w_r)
 * with H = diag(D) + U^T W U (primal) or K = W^-1 + U D^-1 U^T (dual) solved by the same code, and the xi block
 * unchanged.  With reset, xi^(0) is taken at mu = m, sigma^2 = 1 / lam.  The loss written is B_e with
 *   KL = 1/2 (lam sigma^2 + lam (mu - m)^2 - 1 - log(lam sigma^2))
 * per coordinate, at the written fp32 parameters; VFM_FOLDIN_OBJECTIVE reports the same B_e at the table rows.  An
 * entity without rows (or without chunks) gets the prior: mu = m, sigma = lam^-1/2, loss 0.
 *
 * prior: device pointer to [2, d + 1] fp32, the means then the precisions.  The kernels stage it once per workgroup, in
 * fp64, in LDS; the workspace is that of the parent call.  A precision that is not finite and positive is the
 * caller's to reject (the kernels do not look): it gives NaN rows, as a kl_weight <= 0 would.  With m = 0 and lam = 1 the
 * rows and the losses are the parent call's, bit for bit.  Everything else -- operands, orders of summation, guards,
 * launches, what is written -- is the parent call's: no atomics, no host synchronisation, and an entity's output bytes
 * depend on its own rows, d, the chunk length of the split form and the prior alone.
 *
 * Conventions: those of vfm_foldin.h.  No struct of an existing header changes.
 */
#ifndef VFM_BOUND_PRIOR_H
#define VFM_BOUND_PRIOR_H

#include <stdint.h>

#include "vfm_bound.h"
#include "vfm_bound_sweep.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Workspace of vfm_foldin_bound_prior_f32 in bytes: vfm_foldin_bound_workspace_bytes of the same arguments (the prior
 * is staged in LDS, 2 (d + 1) doubles more per workgroup).  VFM_E_INVALID as there. */
int64_t vfm_foldin_bound_prior_workspace_bytes(int64_t E, int64_t R, int64_t n_ops, int32_t d, int32_t lds_dim);

/* vfm_foldin_bound_f32 under `prior`.  prior == NULL runs vfm_foldin_bound_f32 itself.  VFM_E_INVALID (nothing
 * launched) exactly where vfm_foldin_bound_f32 returns it. */
int vfm_foldin_bound_prior_f32(const vfm_foldin_bound_t* p, const float* prior, void* stream);

/* Workspace of vfm_foldin_bound_split_prior_f32 in bytes: vfm_foldin_bound_split_workspace_bytes of the same
 * arguments.  VFM_E_INVALID as there. */
int64_t vfm_foldin_bound_split_prior_workspace_bytes(int64_t n_chunks, int64_t n_heavy, int64_t R, int64_t n_ops,
                                                     int32_t d, int32_t lds_dim);

/* vfm_foldin_bound_split_f32 under `prior`.  prior == NULL runs vfm_foldin_bound_split_f32 itself.  VFM_E_INVALID
 * (nothing launched) exactly where vfm_foldin_bound_split_f32 returns it. */
int vfm_foldin_bound_split_prior_f32(const vfm_foldin_bound_split_t* p, const float* prior, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VFM_BOUND_PRIOR_H */

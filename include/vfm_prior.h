/*
 * vfm_prior.h -- C ABI of the exact solves of libvfm_hip.so (gfx950) under a learnt field prior: vfm_foldin_solve_f32
 * (vfm_foldin.h) and vfm_foldin_solve_split_f32 (vfm_sweep.h) with the folded field's prior N(m_c, 1 / lam_c) per
 * coordinate c in [0, d] (0: the first-order weight, 1 .. d: the factors) in place of N(0, 1), the entity block of a
 * hierarchical sweep (VFM.fit_exact(learn_priors=True); DESIGN.md §4, "Hierarchical sweeps").
 *
 * Per entity the system of vfm_foldin.h becomes
 *   H = prec (sum_r u_r u_r^T + diag(0, sum_r A_r)) + kl diag(lam),  b = prec (sum_r t_r u_r - (0, 1/2 sum_r C_r)) + kl lam m,
 *   sigma_c^2 = kl / (kl lam_c + prec sum_r (A_r,c + M_r,c^2)),
 * solved in the same primal or dual form by the same code, and the loss written is L_e with
 *   KL = 1/2 (lam sigma^2 + lam (mu - m)^2 - 1 - log(lam sigma^2))
 * per coordinate.  An entity without rows gets the prior: mu = m, sigma = lam^-1/2.
 *
 * prior: device pointer to [2, d + 1] fp32, the means then the precisions.  The kernels stage it once per workgroup, in
 * fp64, in LDS; the workspace is that of the parent call.  A precision that is not finite and positive is the
 * caller's to reject (the kernels do not look): it gives NaN rows, as a kl_weight <= 0 would.  With m = 0 and lam = 1 the
 * rows and the losses are the parent call's, bit for bit.  Everything else -- operands, orders of summation, guards,
 * what is written -- is the parent call's: no atomics, no host synchronisation, and an entity's output bytes depend
 * on its own rows, d, the chunk length of the split form and the prior alone.
 *
 * Conventions: those of vfm_foldin.h.  No struct of an existing header changes.
 */
#ifndef VFM_PRIOR_H
#define VFM_PRIOR_H

#include <stdint.h>

#include "vfm_foldin.h"
#include "vfm_sweep.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Workspace of vfm_foldin_solve_prior_f32 in bytes: vfm_foldin_solve_workspace_bytes of the same arguments (the prior
 * is staged in LDS, 2 (d + 1) doubles more per workgroup).  VFM_E_INVALID as there. */
int64_t vfm_foldin_solve_prior_workspace_bytes(int64_t E, int64_t n_ops, int32_t d, int32_t lds_dim);

/* vfm_foldin_solve_f32 under `prior`.  prior == NULL runs vfm_foldin_solve_f32 itself.  VFM_E_INVALID (nothing
 * launched) exactly where vfm_foldin_solve_f32 returns it. */
int vfm_foldin_solve_prior_f32(const vfm_foldin_solve_t* p, const float* prior, void* stream);

/* Workspace of vfm_foldin_solve_split_prior_f32 in bytes: vfm_foldin_split_workspace_bytes of the same arguments.
 * VFM_E_INVALID as there. */
int64_t vfm_foldin_split_prior_workspace_bytes(int64_t n_chunks, int64_t n_heavy, int64_t n_ops, int32_t d,
                                               int32_t lds_dim);

/* vfm_foldin_solve_split_f32 under `prior`.  prior == NULL runs vfm_foldin_solve_split_f32 itself.  VFM_E_INVALID
 * (nothing launched) exactly where vfm_foldin_solve_split_f32 returns it. */
int vfm_foldin_solve_split_prior_f32(const vfm_foldin_split_t* p, const float* prior, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VFM_PRIOR_H */

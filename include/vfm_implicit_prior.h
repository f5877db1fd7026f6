/*
 * vfm_implicit_prior.h -- C ABI of the implicit-feedback solve of libvfm_hip.so (gfx950) under a learnt field prior:
 * vfm_foldin_solve_implicit_f32 (vfm_implicit.h) with the folded field's prior N(m_c, 1 / lam_c) per coordinate c in
 * [0, d] (0: the first-order weight, 1 .. d: the factors) in place of N(0, 1), the entity block of a hierarchical
 * implicit sweep (VFM.fit_implicit(learn_priors=True); DESIGN.md §4, "Hierarchical implicit sweeps").
 *
 * Per entity the system of vfm_implicit.h becomes
 *   H = kl diag(lam) + prec [ w0 (T_B + diag(0, SA_B)) + dw sum_{r in obs(e)} (u_r u_r^T + diag(0, A_r)) ]
 *   b = prec [ w0 tu_B + sum_{r in obs(e)} (w1 y_r - dw c_mean,r) u_r ] + kl lam m,   theta = H^-1 b
 *   sigma_c^2 = kl / (kl lam_c + prec SB'_c),   SB'_c = w0 SB_B,c + dw sum_obs (A_rc + M_rc^2)   (SB'_0 = w0 n + dw n_e)
 * solved by the same code in the same primal form, and the loss written is
 *   L_e = 1/2 [prec tt' - 2 theta . b_data + (theta^T H theta - kl sum_c lam_c theta_c^2) + prec sum_c sigma_c^2 SB'_c]
 *         + (w0 n + dw n_e) (1/2 log 2 pi - 1/2 log prec) + kl sum_c KL_c
 *   KL_c = 1/2 (lam sigma^2 + lam (theta - m)^2 - 1 - log(lam sigma^2))
 * with b_data = b without the prior's term and theta^T H theta = |L^T theta|^2 off the Cholesky factor.  An entity
 * without observed rows gets the base-only optimum under the prior (not the prior itself: its w0 rows exist).
 *
 * prior: device pointer to [2, d + 1] fp32, the means then the precisions, the folded field's row of the priors, as in
 * vfm_prior.h.  The kernel stages it once per workgroup, in fp64, in LDS (2 (d + 1) doubles in front of the parent's
 * vectors); the workspace and the base (vfm_implicit_base_f32: it does not depend on the prior) are the parent call's.  A
 * precision that is not finite and positive is the caller's to reject (the kernel does not look): it gives NaN rows, as
 * a kl_weight <= 0 would.  With m = 0 and lam = 1 the rows and the losses are the parent call's, bit for bit.  Everything
 * else -- operands, orders of summation, the chunk pass, guards, what is written -- is the parent call's: no atomics, no
 * host synchronisation, and an entity's output bytes depend on its observed rows, the partner catalog, chunk_rows, d,
 * its form and the prior alone.
 *
 * Conventions: those of vfm_foldin.h.  No struct of an existing header changes.
 */
#ifndef VFM_IMPLICIT_PRIOR_H
#define VFM_IMPLICIT_PRIOR_H

#include <stdint.h>

#include "vfm_implicit.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Workspace of vfm_foldin_solve_implicit_prior_f32 in bytes: vfm_implicit_solve_workspace_bytes of the same arguments
 * (the prior is staged in LDS, 2 (d + 1) doubles more per workgroup).  VFM_E_INVALID as there. */
int64_t vfm_implicit_solve_prior_workspace_bytes(int64_t E, int64_t n_chunks, int32_t d, int32_t lds_dim);

/* vfm_foldin_solve_implicit_f32 under `prior`.  prior == NULL runs vfm_foldin_solve_implicit_f32 itself.  VFM_E_INVALID
 * (nothing launched) exactly where vfm_foldin_solve_implicit_f32 returns it. */
int vfm_foldin_solve_implicit_prior_f32(const vfm_implicit_solve_t* p, const float* prior, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VFM_IMPLICIT_PRIOR_H */

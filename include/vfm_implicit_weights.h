/*
 * vfm_implicit_weights.h -- C ABI of the implicit-feedback solve of libvfm_hip.so (gfx950) with a confidence weight per
 * observed pair: vfm_foldin_solve_implicit_f32 (vfm_implicit.h) and its form under a field prior (vfm_implicit_prior.h)
 * in which observed row r weighs w_r >= w0 in place of the one w1 (Hu, Koren & Volinsky's c_ui = 1 + alpha r_ui), the
 * entity block of VFM.fit_implicit(weights=); DESIGN.md §4, "Weighted implicit sweeps".
 *
 * Every unobserved pair keeps (w0, 0).  With g_r = w_r - w0, taken in fp64 from the two fp32 values, the system of
 * vfm_implicit.h becomes
 *   H         = kl I + prec [ w0 (T_B + diag(0, SA_B)) + sum_{r in obs(e)} g_r (u_r u_r^T + diag(0, A_r)) ]
 *   b         = prec [ w0 tu_B + sum_{r in obs(e)} (w_r y_r - g_r c_mean,r) u_r ],   theta = H^-1 b
 *   SB'_c     = w0 SB_B,c + sum_obs g_r (A_rc + M_rc^2)          (c = 0: W_e = w0 n + sum_obs g_r)
 *   sigma_c^2 = kl / (kl + prec SB'_c)
 *   tt'       = w0 tt_B + sum_obs (w_r (y_r - c_mean,r)^2 - w0 c_mean,r^2 + g_r c_var,r)
 * and L_e keeps the expression of vfm_implicit.h with these b, SB', tt' and W_e in place of w0 n + dw n_e.  Under a prior
 * (prior != NULL) kl becomes kl lam_c and b gains kl lam m, exactly as in vfm_implicit_prior.h.  The correction at the
 * observed rows is a weighted Gram instead of dw times an unweighted one: the chunk pass scales the four u_i of a row's
 * 4 x 4 tile by g_r, the per-coordinate sums add g_r A, g_r (A + M^2) and g_r, the row-list form adds g_r, g_r M_i and
 * g_r M_i M_j, and the solve forms w0 base + share.  The base (vfm_implicit_base_f32) does not depend on the weights.
 *
 * weights: device pointer to [R] fp32, row r's weight, in the row order of p->y; it is read where y is, under the same
 * clamps.  THE KERNEL DOES NOT CHECK IT: a weight below w0 or not finite is the caller's to reject, as a prior's
 * precision is (below w0 the system can lose positive definiteness and the rows come out NaN or meaningless; nothing is
 * read or written out of bounds).  vae_amd's Python surface rejects both.  p->w1 is neither read nor checked.
 *
 * Constant weights w_r = w1 give the optimum of the call with that w1, not its bytes: sum_r (g u_r) u_r^T and
 * dw sum_r u_r u_r^T round differently.  An entity whose rows all weigh exactly w0 with target 0 adds exact zeros and
 * gets the bytes of the same entity without rows.  Everything else -- operands, orders of summation, guards, the
 * LDS / slab rule, what is written -- is the parent call's: no atomics, no host synchronisation, and an entity's output
 * bytes depend on its observed rows and their weights, the partner catalog, chunk_rows, d, its form and the prior alone.
 *
 * Conventions: those of vfm_foldin.h.  No struct of an existing header changes.
 */
#ifndef VFM_IMPLICIT_WEIGHTS_H
#define VFM_IMPLICIT_WEIGHTS_H

#include <stdint.h>

#include "vfm_implicit.h"
#include "vfm_implicit_prior.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Workspace of vfm_foldin_solve_implicit_weights_f32 in bytes: vfm_implicit_solve_workspace_bytes of the same arguments
 * (the weights are the caller's array).  VFM_E_INVALID as there. */
int64_t vfm_implicit_solve_weights_workspace_bytes(int64_t E, int64_t n_chunks, int32_t d, int32_t lds_dim);

/* vfm_foldin_solve_implicit_prior_f32 with a weight per observed row.  weights == NULL runs
 * vfm_foldin_solve_implicit_prior_f32(p, prior, stream) itself; prior == NULL is the N(0, 1) prior.  VFM_E_INVALID
 * (nothing launched) exactly where vfm_foldin_solve_implicit_f32 returns it, except that with weights p->w1 is not
 * looked at. */
int vfm_foldin_solve_implicit_weights_f32(const vfm_implicit_solve_t* p, const float* prior, const float* weights,
                                          void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VFM_IMPLICIT_WEIGHTS_H */

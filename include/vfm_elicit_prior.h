/*
 * vfm_elicit_prior.h -- C ABI of the exact, bound and design sessions of libvfm_hip.so (gfx950) under a learnt field
 * prior: vfm_elicit_solve_f32 (vfm_elicit.h), vfm_elicit_bound_f32 (vfm_bound.h), vfm_design_scores_f32 and
 * vfm_design_elicit_f32 (vfm_design.h) with the respondents' field prior N(m_c, 1 / lam_c) per coordinate c in [0, d]
 * (0: the first-order weight, 1 .. d: the factors) in place of N(0, 1): what VFM.fit_exact(learn_priors=True) and
 * VFM.fit_bound(learn_priors=True) learn, read where a cold-start respondent is interviewed ("Sessions
 * under learnt priors").
 *
 * The fold of a round is that of vfm_prior.h (exact, design) or of vfm_bound_prior.h (bound) -- the same body, started
 * from the session's theta_e as in the parent session.  With `reset` a respondent starts at the prior,
 *   mu_c = m_c,  sigma_c = lam_c^-1/2   (stored as sigma for the |.| link, log(expm1(sigma)) for softplus),
 * which is also what round 0 is scored from; it depends on the prior and the link alone.  The design score is taken
 * at the optimum's scales under the prior,
 *   sigma_k^2 = kl / (kl lam_k + prec S_k),  sigma_w^2 = kl / (kl lam_0 + prec n);
 * it reads lam and never m.
 *
 * prior: device pointer to [2, d + 1] fp32, the means then the precisions, of column `field`.  The kernels stage it
 * once per workgroup, in fp64, in LDS in front of everything else (16 (d + 1) bytes more per workgroup); the workspace
 * is that of the parent call.  A precision that is not finite and positive is the caller's to reject (the kernels do
 * not look).  With m = 0 and lam = 1 everything written is the parent call's, bit for bit.  Everything else --
 * operands, orders of summation, guards, launches, what is written -- is the parent call's: no atomics, no host
 * synchronisation.
 *
 * Conventions: those of vfm_elicit.h.  No struct of an existing header changes.
 */
#ifndef VFM_ELICIT_PRIOR_H
#define VFM_ELICIT_PRIOR_H

#include <stdint.h>

#include "vfm_bound.h"
#include "vfm_design.h"
#include "vfm_elicit.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Workspace of vfm_elicit_solve_prior_f32 in bytes: vfm_elicit_solve_workspace_bytes of the same arguments.
 * VFM_E_INVALID as there. */
int64_t vfm_elicit_solve_prior_workspace_bytes(int64_t U, int64_t P, int64_t n_ops, int32_t d, int32_t lds_dim);

/* vfm_elicit_solve_f32 under `prior`.  prior == NULL runs vfm_elicit_solve_f32 itself.  VFM_E_INVALID (nothing
 * launched) exactly where vfm_elicit_solve_f32 returns it. */
int vfm_elicit_solve_prior_f32(const vfm_elicit_solve_t* p, const float* prior, void* stream);

/* Workspace of vfm_elicit_bound_prior_f32 in bytes: vfm_elicit_bound_workspace_bytes of the same arguments.
 * VFM_E_INVALID as there. */
int64_t vfm_elicit_bound_prior_workspace_bytes(int64_t U, int64_t P, int64_t H, int64_t n_ops, int32_t d,
                                               int32_t n_rounds, int32_t lds_dim);

/* vfm_elicit_bound_f32 under `prior`.  prior == NULL runs vfm_elicit_bound_f32 itself.  VFM_E_INVALID (nothing
 * launched) exactly where vfm_elicit_bound_f32 returns it. */
int vfm_elicit_bound_prior_f32(const vfm_elicit_bound_t* p, const float* prior, void* stream);

/* Workspace of vfm_design_scores_prior_f32 and vfm_design_elicit_prior_f32 in bytes: vfm_design_workspace_bytes of the
 * same arguments.  VFM_E_INVALID as there. */
int64_t vfm_design_prior_workspace_bytes(int64_t U, int64_t P, int64_t n_ops, int32_t d, int32_t lds_dim);

/* vfm_design_scores_f32 under `prior`.  prior == NULL runs vfm_design_scores_f32 itself.  VFM_E_INVALID (nothing
 * launched) exactly where vfm_design_scores_f32 returns it. */
int vfm_design_scores_prior_f32(const vfm_design_t* p, const float* prior, void* stream);

/* vfm_design_elicit_f32 under `prior`.  prior == NULL runs vfm_design_elicit_f32 itself.  VFM_E_INVALID (nothing
 * launched) exactly where vfm_design_elicit_f32 returns it. */
int vfm_design_elicit_prior_f32(const vfm_design_t* p, const float* prior, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VFM_ELICIT_PRIOR_H */

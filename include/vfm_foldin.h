/*
 * vfm_foldin.h -- C ABI of the fold-in kernels of libvfm_hip.so (gfx950): fit the variational factors of chosen
 * entities with every other parameter frozen.
 *
 * With all parameters but one entity's theta_e = (mu_e [d], s_e [d], mu_w,e, s_w,e) frozen, the mean-field ELBO splits
 * into independent per-entity problems
 *   L_e = sum_{rows r of e} E_q[ nll(y_r, pred_r) ] + kl_weight (KL(q(w_e) || N(0,1)) + sum_k KL(q(z_e,k) || N(0,1)))
 * and each of them runs its whole Adam optimisation inside one launch: a group of W lanes per entity (lanes own
 * coordinates), theta_e and its Adam moments in registers for all steps, the entity's rows staged in LDS while they fit.
 *
 * nll: Normal with precision link(alpha) (VFM_LIK_NORMAL; sigma_y = sqrt(1 / |alpha|) under the |.| link) or Bernoulli
 * with logits (VFM_LIK_BERNOULLI); sigma = link(s), link = |.|, or softplus with VFM_FLAG_LINK_SOFTPLUS.
 *   VFM_OBJ_CLOSED_FORM (Normal only): E[(y - pred)^2] = (y - E pred)^2 + Var pred over every random variable of the
 *     row, in the closed form of vfm_rank.h.  The frozen fields of a row are folded into an operand once (prep kernel):
 *     with S_Q = sum of the frozen embeddings, M = E S_Q, A = Var S_Q, C = 2 Cov(S_Q, P_Q) (P_Q: their pair term) and
 *     the scalars c_mean, c_var,  E pred = c_mean + mu_w,e + mu_e . M,
 *     Var pred = c_var + sigma_w,e^2 + sum_k (mu_e,k^2 A_k + sigma_e,k^2 (A_k + M_k^2) + mu_e,k C_k).
 *   VFM_OBJ_SAMPLED: the mean over n_samples reparameterised draws of every random variable of the row.  Draw s of
 *     iteration t uses the eps vfm_philox_eps_f32 (vfm_hip.h) writes for (seed, step = t * n_samples + s, one sample):
 *     entity e's eps is keyed on its id, the global bias' on the reserved id, exactly as in training.
 * Optimiser: Adam (beta 0.9 / 0.999, eps 1e-8, bias correction, constant lr), fresh moments, n_steps updates; step t
 * uses the gradient at the iterate of step t - 1.  out_loss = L_e at the final parameters (draw key t = t0 + n_steps).
 *
 * Conventions: those of vfm_hip.h.  Every pointer is DEVICE memory owned by the caller; launch-only, no host
 * synchronisation; the caller owns the workspace (vfm_foldin_workspace_bytes); 0 on success, a negative VFM_E_* code or
 * a positive hipError_t otherwise; arguments are checked before any HIP call; vfm_last_error() describes the last
 * failure on the calling thread.  Tables as in vfm_hip.h: entity_params [T, 2d] = [mu | s], bias_params [T, 2] =
 * [mu_w, s_w], scalars [3] = alpha, global_bias_mean, global_bias_scale.
 */
#ifndef VFM_FOLDIN_H
#define VFM_FOLDIN_H

#include <stdint.h>

#include "vfm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VFM_FOLDIN_MAX_D 512
#define VFM_FOLDIN_MAX_SAMPLES 4
#define VFM_FOLDIN_FIT 0       /* run n_steps Adam updates, write the rows of the entities, out_loss at the end     */
#define VFM_FOLDIN_OBJECTIVE 1 /* n_steps must be 0: out_loss and out_grad at the current parameters, nothing written */

typedef struct vfm_foldin_t {
  int64_t E;          /* folded entities                                                                         */
  int64_t R;          /* rows, sorted (stably) by the folded id                                                  */
  int64_t T;          /* table rows                                                                              */
  int64_t n_ops;      /* closed form: distinct frozen-partner tuples (row operands); 0 for the sampled objective  */
  int32_t F, d;       /* fields (1 .. VFM_MAX_FIELDS), embedding size (1 .. VFM_FOLDIN_MAX_D)                     */
  int32_t col;        /* the folded column of x                                                                  */
  int32_t objective;  /* VFM_OBJ_CLOSED_FORM (VFM_LIK_NORMAL only) or VFM_OBJ_SAMPLED                            */
  int32_t likelihood; /* VFM_LIK_NORMAL / VFM_LIK_BERNOULLI                                                      */
  int32_t flags;      /* 0 or VFM_FLAG_LINK_SOFTPLUS                                                             */
  int32_t mode;       /* VFM_FOLDIN_FIT / VFM_FOLDIN_OBJECTIVE                                                   */
  int32_t n_steps;    /* Adam updates (>= 0)                                                                     */
  int32_t n_samples;  /* sampled objective: draws per iteration, 1 .. VFM_FOLDIN_MAX_SAMPLES                     */
  int32_t reset;      /* 1: start from the prior (mu = 0, sigma = 1) instead of the current rows                 */
  int32_t lds_rows;   /* -1: as many rows per entity staged in LDS as fit; >= 0: at most that many (tests)      */
  int32_t pad0;
  float lr, kl_weight;
  uint64_t seed;      /* Philox key (the model's rng_seed)                                                       */
  int64_t t0;         /* sampled: the draw key of the first iteration (0 for a fit)                              */
  const int64_t* entities; /* [E] folded ids, ascending                                                           */
  const int64_t* row_ptr;  /* [E + 1] offsets of each entity's rows                                                */
  const int64_t* x;        /* [R, F] the rows                                                                     */
  const float* y;          /* [R]                                                                                 */
  const int64_t* op_x;     /* closed form: [n_ops, F] one row of each partner tuple (the folded column is ignored) */
  const int64_t* row_op;   /* closed form: [R] operand of each row                                                */
  float* entity_params;    /* [T, 2d]: read; the rows of `entities` are written by a fit                          */
  float* bias_params;      /* [T, 2]                                                                              */
  const float* scalars;    /* [3]                                                                                 */
  float* out_loss;         /* [E] L_e                                                                             */
  float* out_grad;         /* VFM_FOLDIN_OBJECTIVE: [E, 2d + 2] = [dL/dmu | dL/ds | dL/dmu_w | dL/ds_w], or NULL     */
  void* workspace;
  int64_t workspace_bytes;
} vfm_foldin_t;

/* Workspace of vfm_foldin_f32 in bytes (0 for the sampled objective).  Negative on bad arguments. */
int64_t vfm_foldin_workspace_bytes(int64_t n_ops, int32_t d, int32_t objective);

/* Fold in (or evaluate) the entities of p.  An entity id outside [0, T) gets a NaN loss and is not written; a partner
 * id outside [0, T) makes its rows' entities NaN. */
int vfm_foldin_f32(const vfm_foldin_t* p, void* stream);

/*
 * Exact fold-in (closed form only): the optimum of L_e itself, in one launch, no iterations.
 *
 * With everything else frozen the closed-form L_e is quadratic in the means theta = (mu_w, mu) and separable and convex
 * in each scale, so its one global optimum has a closed form.  With u_r = (1, M_r), t_r = y_r - c_mean,r,
 * prec = link(alpha), kl = kl_weight > 0 and n the rows of e (duplicates counted):
 *   H theta = b,  H = prec (sum_r u_r u_r^T + diag(0, sum_r A_r)) + kl I,  b = prec (sum_r t_r u_r - (0, 1/2 sum_r C_r))
 *   sigma_w^2 = kl / (kl + prec n),   sigma_k^2 = kl / (kl + prec sum_r (A_rk + M_rk^2))
 * stored as s = sigma under |.| and s = log(expm1(sigma)) under softplus.  H = D + prec U^T U (D diagonal, U [n, d + 1]):
 * an entity with n <= d rows is solved in the dual n x n form (Woodbury),
 *   theta = D^-1 b - D^-1 U^T (I / prec + U D^-1 U^T)^-1 U D^-1 b,
 * one with more rows in the primal (d + 1) x (d + 1) form.  One workgroup per entity: fp64 row operands (the prep's sums
 * before their rounding to fp32, links in fp64), sums in fp64 in row-list order, a
 * packed Cholesky factor in LDS while the system fits, else in the workgroup's slab of the workspace.  No atomics, no
 * host synchronisation, and the result does not depend on the entity's current row or on the other entities of the call.
 * out_loss = L_e at the written fp32 parameters, with the arithmetic of vfm_foldin_f32's final pass.
 */
#define VFM_FOLDIN_SOLVE_LDS_DIM 135 /* the largest system kept in LDS (packed fp64 triangle: 73,440 bytes)          */
#define VFM_FOLDIN_SOLVE_SLABS 256   /* workgroups of a launch that may need a workspace slab                        */

typedef struct vfm_foldin_solve_t {
  int64_t E;          /* folded entities                                                                         */
  int64_t R;          /* rows, sorted (stably) by the folded id                                                  */
  int64_t T;          /* table rows                                                                              */
  int64_t n_ops;      /* distinct frozen-partner tuples (row operands)                                           */
  int32_t F, d;       /* fields (1 .. VFM_MAX_FIELDS), embedding size (1 .. VFM_FOLDIN_MAX_D)                     */
  int32_t col;        /* the folded column of op_x                                                               */
  int32_t objective;  /* VFM_OBJ_CLOSED_FORM                                                                     */
  int32_t likelihood; /* VFM_LIK_NORMAL                                                                          */
  int32_t flags;      /* 0 or VFM_FLAG_LINK_SOFTPLUS                                                             */
  int32_t lds_dim;    /* -1: systems stay in LDS while they fit; >= 0: larger ones go to the workspace (tests)  */
  float kl_weight;    /* > 0                                                                                     */
  const int64_t* entities; /* [E] folded ids, ascending                                                           */
  const int64_t* row_ptr;  /* [E + 1] offsets of each entity's rows                                                */
  const float* y;          /* [R]                                                                                 */
  const int64_t* op_x;     /* [n_ops, F] one row of each partner tuple (the folded column is ignored)              */
  const int64_t* row_op;   /* [R] operand of each row                                                             */
  float* entity_params;    /* [T, 2d]: read; the rows of `entities` are written                                   */
  float* bias_params;      /* [T, 2]                                                                              */
  const float* scalars;    /* [3]                                                                                 */
  float* out_loss;         /* [E] L_e                                                                             */
  void* workspace;
  int64_t workspace_bytes;
} vfm_foldin_solve_t;

/* Workspace of vfm_foldin_solve_f32 in bytes: the row operands (fp32 for the loss, as vfm_foldin_f32 keeps them, and
 * unrounded fp64 for the solve), and min(E, VFM_FOLDIN_SOLVE_SLABS) slabs of a packed
 * (d + 1) x (d + 1) fp64 triangle when such a system would not stay in LDS.  Negative on bad arguments. */
int64_t vfm_foldin_solve_workspace_bytes(int64_t E, int64_t n_ops, int32_t d, int32_t lds_dim);

/* Write the exact optimum of every entity of p.  An entity id outside [0, T) gets a NaN loss and is not written; a
 * partner id outside [0, T) makes its rows' entities NaN.  VFM_E_INVALID (nothing launched) for an objective other than
 * VFM_OBJ_CLOSED_FORM, a likelihood other than VFM_LIK_NORMAL, kl_weight <= 0, d > VFM_FOLDIN_MAX_D, a short or
 * misaligned (256 bytes) workspace and the other range checks of vfm_foldin_f32. */
int vfm_foldin_solve_f32(const vfm_foldin_solve_t* p, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VFM_FOLDIN_H */

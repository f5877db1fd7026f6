/*
 * vfm_bound.h -- C ABI of the bound fold-in of libvfm_hip.so (gfx950): the fold-in of vfm_foldin.h for the Bernoulli
 * likelihood ('class' models), by exact solves of the Jaakkola-Jordan quadratic bound instead of Adam on a sampled
 * objective.
 *
 * For y in {0, 1} and the logit f,  nll(y, f) = -y f + log(1 + e^f)  and, for any xi > 0 with
 * lambda(xi) = tanh(xi / 2) / (4 xi),
 *   nll(y, f) <= -(y - 1/2) f + xi / 2 + log(1 + e^-xi) + lambda(xi) (f^2 - xi^2),          equality at f = +-xi.
 * Under q, with the closed-form moments of vfm_foldin.h (E f_r = c_mean,r + theta . u_r, u_r = (1, M_r), Var f_r as
 * written there, c_var,r included), the bound of row r is a Gaussian row of weight w_r = 2 lambda(xi_r) in (0, 1/4] and
 * pseudo-target (y_r - 1/2) / w_r.  With the other entities frozen and kl = kl_weight > 0 the objective of entity e,
 *   B_e(theta, sigma; xi) = sum_r [ -(y_r - 1/2) E f_r + w_r / 2 (E f_r^2 + Var f_r - xi_r^2) + xi_r / 2 + log(1 + e^-xi_r) ]
 *                           + kl (KL(q(w_e) || N(0,1)) + sum_k KL(q(z_e,k) || N(0,1))),
 * is minimised block by block, each block exactly, n_iters rounds of
 *   xi block   xi_r^2 = (E f_r)^2 + Var f_r at the current (theta, sigma);  w_r = tanh(xi_r / 2) / (2 xi_r)
 *              (1/4 - xi_r^2 / 48 for xi_r < 1e-3)
 *   q block    H theta = b,  H = sum_r w_r (u_r u_r^T + diag(0, A_r)) + kl I,
 *              b = sum_r ((y_r - 1/2) - w_r c_mean,r) u_r - (0, 1/2 sum_r w_r C_r),
 *              sigma_w^2 = kl / (kl + sum_r w_r),   sigma_k^2 = kl / (kl + sum_r w_r (A_rk + M_rk^2))
 * H = D + U^T W U (D = kl + (0, sum_r w_r A_r), W = diag(w)): an entity with n <= d rows is solved in the dual form
 * K = W^-1 + U D^-1 U^T,  theta = D^-1 b - D^-1 U^T K^-1 U D^-1 b,  one with more rows in the primal form: the rule, the
 * packed Cholesky factorisation, the LDS / slab placement of the triangle and the rounding of the written row are those
 * of vfm_foldin_solve_f32.  The iterate (theta, sigma^2) stays in fp64 for all rounds and is rounded to fp32 once, at
 * the end.  The start is xi^(0) from the entity's current row, or from the prior (mu = 0, sigma = 1) with reset; the
 * starting row enters through xi^(0) only.
 *
 * With xi at its optimum the row term collapses to a function of the parameters alone,
 *   B_e(theta, sigma) = sum_r [ -(y_r - 1/2) E f_r + xi_r / 2 + log1p(e^-xi_r) ] + kl KL,  xi_r = sqrt((E f_r)^2 + Var f_r),
 * which is the loss reported: an upper bound on L_e of vfm_foldin.h (expected Bernoulli nll + kl KL) that no round
 * increases.  It is evaluated at the written fp32 parameters with fp32 per-row moments (the arithmetic of
 * vfm_foldin_f32's closed-form final pass), the rows added in row order.
 *
 * One workgroup per entity; fp64 row operands from the two prep kernels of vfm_foldin_solve_f32 plus c_var in fp64 from
 * a prep of this unit; every sum in a fixed order that depends on the entity's own rows and d alone.  No atomics, no host
 * synchronisation; an entity's output bytes do not depend on the other entities of the call, on the grid or on where
 * its triangle lives.
 *
 * Conventions: those of vfm_foldin.h.
 */
#ifndef VFM_BOUND_H
#define VFM_BOUND_H

#include <stdint.h>

#include "vfm_foldin.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vfm_foldin_bound_t {
  int64_t E;          /* folded entities                                                                         */
  int64_t R;          /* rows, sorted (stably) by the folded id                                                  */
  int64_t T;          /* table rows                                                                              */
  int64_t n_ops;      /* distinct frozen-partner tuples (row operands)                                           */
  int32_t F, d;       /* fields (1 .. VFM_MAX_FIELDS), embedding size (1 .. VFM_FOLDIN_MAX_D)                     */
  int32_t col;        /* the folded column of op_x                                                               */
  int32_t objective;  /* VFM_OBJ_CLOSED_FORM (the moments of the bound are the closed form's)                    */
  int32_t likelihood; /* VFM_LIK_BERNOULLI                                                                       */
  int32_t flags;      /* 0 or VFM_FLAG_LINK_SOFTPLUS                                                             */
  int32_t lds_dim;    /* as in vfm_foldin_solve_t                                                                */
  float kl_weight;    /* > 0                                                                                     */
  int32_t n_iters;    /* rounds: >= 1 for VFM_FOLDIN_FIT, 0 for VFM_FOLDIN_OBJECTIVE                             */
  int32_t reset;      /* 1: xi^(0) from the prior (mu = 0, sigma = 1) instead of the current rows                */
  int32_t mode;       /* VFM_FOLDIN_FIT: run the rounds, write the rows, out_loss = B_e at the written fp32      */
                      /* parameters; VFM_FOLDIN_OBJECTIVE: nothing written, out_loss = B_e at the current rows   */
  int32_t pad0;
  const int64_t* entities; /* [E] folded ids, ascending                                                           */
  const int64_t* row_ptr;  /* [E + 1] offsets of each entity's rows                                                */
  const float* y;          /* [R] in {0, 1}                                                                       */
  const int64_t* op_x;     /* [n_ops, F] one row of each partner tuple (the folded column is ignored)              */
  const int64_t* row_op;   /* [R] operand of each row                                                             */
  float* entity_params;    /* [T, 2d]: read; the rows of `entities` are written by a fit                          */
  float* bias_params;      /* [T, 2]                                                                              */
  const float* scalars;    /* [3] (alpha is not read: the Bernoulli likelihood has no precision)                  */
  float* out_loss;         /* [E] B_e                                                                             */
  void* workspace;
  int64_t workspace_bytes;
} vfm_foldin_bound_t;

/* Workspace of vfm_foldin_bound_f32 in bytes, each part rounded up to 256: the operand block of
 * vfm_foldin_solve_workspace_bytes (what that function returns without slabs), n_ops doubles of c_var in fp64, R
 * doubles of row weights, and the slabs by the rule of vfm_foldin_solve_workspace_bytes (min(E, VFM_FOLDIN_SOLVE_SLABS)
 * packed (d + 1) x (d + 1) fp64 triangles when such a system would not stay in LDS).  VFM_E_INVALID on negative
 * arguments, d outside [1, VFM_FOLDIN_MAX_D] or lds_dim < -1. */
int64_t vfm_foldin_bound_workspace_bytes(int64_t E, int64_t R, int64_t n_ops, int32_t d, int32_t lds_dim);

/* Fit (or evaluate) the entities of p.  An entity id outside [0, T) gets a NaN loss and is not written; a partner id
 * outside [0, T) makes its rows' entities and their losses NaN; an entity with an empty row range gets the prior
 * (mu = 0, s = link^-1(1)) and loss 0; E = 0: nothing is launched.  VFM_E_INVALID (nothing launched) for everything
 * vfm_foldin_solve_f32 rejects, a likelihood other than VFM_LIK_BERNOULLI, a mode other than the two above, n_iters < 1
 * in VFM_FOLDIN_FIT or != 0 in VFM_FOLDIN_OBJECTIVE, and a short or misaligned (256 bytes) workspace. */
int vfm_foldin_bound_f32(const vfm_foldin_bound_t* p, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VFM_BOUND_H */

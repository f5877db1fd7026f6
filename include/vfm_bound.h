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

#include "vfm_elicit.h"
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

/* ---- The bound field-form session: ask, run the bound's rounds, ask again ----------------------------------------------
 * vfm_elicit_solve_f32 (vfm_elicit.h) for 'class' models: each round's fold is the bound fold-in above instead of the
 * exact optimum of a 'reg' model.  kl_weight > 0, answers and history labels in {0, 1}.
 *
 * Per respondent e of column `field` independently, for round q = 0 .. n_rounds - 1:
 *  1. Score and choose: steps 1-2 of vfm_elicit_solve_f32, unchanged in meaning and in bits (scores under e's CURRENT
 *     posterior; round 0: the table row, or the prior row mu = 0, s = link^-1(1) in fp32 with `reset`; ties to the lower
 *     pool position; NaN never; nothing left: out_row = -1, out_score = out_loss = NaN and nothing more is folded for e).
 *  2. Fold in.  e's rows are its history in the given order, then the asked rows in the order asked; e's posterior becomes
 *     bitwise what vfm_foldin_bound_f32 writes for E = 1, col = field, reset = 0, the same n_iters and kl_weight on exactly
 *     those rows with e's table row holding the current fp32 posterior: xi^(0) at the fp32 posterior read through the
 *     link in fp64, n_iters rounds in fp64, rounded once; out_loss is that call's out_loss, B_e at the rounded parameters.
 *     The next round scores from, and the next fold starts at, those fp32 parameters.
 * A respondent's result does not depend on the other respondents, the grid, the stream or where its triangle is stored.
 * Launches, whatever n_rounds: the score's operand pass, the fold-in's fp32 and fp64 operand passes and the c_var pass over
 * op_x, and one session kernel.  No atomics, no host synchronisation.  hist_ptr must not decrease (each respondent's row
 * weights live at its own offset of the workspace). */
typedef struct vfm_elicit_bound_t {
  uint32_t struct_size; /* sizeof(vfm_elicit_bound_t) of the caller's build; checked (VFM_STRUCT_INIT)                */
  uint32_t abi_version; /* VFM_ABI_VERSION of the caller's build                                                      */
  int64_t U;            /* respondents                                                                                */
  int64_t P;            /* pool rows of all respondents                                                               */
  int64_t H;            /* history rows of all respondents (0: none)                                                  */
  int64_t T;            /* table rows                                                                                 */
  int64_t n_ops;        /* distinct contexts of pool and history (row operands)                                       */
  int32_t F, d;         /* fields (2 .. VFM_MAX_FIELDS), embedding size (1 .. VFM_FOLDIN_MAX_D)                       */
  int32_t field;        /* the respondents' column                                                                    */
  int32_t key_col;      /* the context column whose id keys VFM_RANK_RANDOM                                           */
  int32_t n_rounds;     /* Q, 0 .. VFM_ELICIT_MAX_ROUNDS                                                              */
  int32_t strategy;     /* VFM_RANK_TOP / VARIANCE / MEAN / RANDOM                                                    */
  int32_t flags;        /* 0 or VFM_FLAG_LINK_SOFTPLUS                                                                */
  int32_t reset;        /* 1: round 0 starts from the prior row instead of the respondents' table rows                */
  int32_t write;        /* 1: the respondents' table rows get the final posterior; 0: no table byte changes           */
  int32_t lds_dim;      /* -1: systems up to VFM_FOLDIN_SOLVE_LDS_DIM live in LDS; >= 0: up to that size (tests)      */
  float kl_weight;      /* weight of the KL terms, > 0                                                                */
  int32_t n_iters;      /* rounds of the bound per fold, >= 1                                                         */
  uint64_t seed;        /* Philox key of the strategy's uniforms (seed + q)                                           */
  const int64_t* entities;   /* [U] respondent ids, ascending                                                         */
  const int64_t* pool_ptr;   /* [U + 1] offsets of each respondent's pool rows                                        */
  const int64_t* pool_x;     /* [P, F] the pool rows, in the caller's pool order per respondent                       */
  const float* pool_y;       /* [P] the answer each question would receive, in {0, 1}                                 */
  const int64_t* hist_ptr;   /* [U + 1] offsets of each respondent's history rows, or NULL (H = 0)                    */
  const int64_t* hist_x;     /* [H, F]                                                                                */
  const float* hist_y;       /* [H] in {0, 1}                                                                         */
  const int64_t* op_x;       /* [n_ops, F] one row of each distinct context (column `field` is ignored)               */
  const int64_t* pool_op;    /* [P] operand of each pool row, in [0, n_ops)                                           */
  const int64_t* hist_op;    /* [H] operand of each history row, in [0, n_ops)                                        */
  float* entity_params;      /* [T, 2d]: read; the rows of `entities` are written when `write`                        */
  float* bias_params;        /* [T, 2]                                                                                */
  const float* scalars;      /* [3]                                                                                   */
  int64_t* out_row;          /* [U, Q] the pool row asked (an index into pool_x's rows), or -1                        */
  float* out_score;          /* [U, Q] its score                                                                      */
  float* out_loss;           /* [U, Q] B_e after the round                                                            */
  float* out_theta;          /* NULL, or [U, Q, 2d + 2] = [mu | s | mu_w | s_w] after each round                      */
  float* out_mean;           /* NULL, or [Q + 1, P]: as in vfm_elicit_field_t (both or neither)                       */
  float* out_var;
  void* workspace;
  int64_t workspace_bytes;
} vfm_elicit_bound_t;

/* Workspace of vfm_elicit_bound_f32 in bytes, each part rounded up to 256: the parts of vfm_elicit_solve_workspace_bytes
 * without its slabs (the asked flags [max(P, 1)], the score's operands [n_ops, 4d] and [n_ops, 2] floats, the fold-in's
 * operand block), n_ops doubles of c_var, H + U * n_rounds doubles of row weights (respondent g's at hist_ptr[g] + g *
 * n_rounds, fold row i at offset i), and the slabs by the rule of vfm_foldin_solve_workspace_bytes for U entities.
 * VFM_E_INVALID on negative arguments, d outside [1, VFM_FOLDIN_MAX_D], n_rounds outside [0, VFM_ELICIT_MAX_ROUNDS] or
 * lds_dim < -1. */
int64_t vfm_elicit_bound_workspace_bytes(int64_t U, int64_t P, int64_t H, int64_t n_ops, int32_t d, int32_t n_rounds,
                                         int32_t lds_dim);

/* Run the sessions of p.  The guards are vfm_elicit_solve_f32's: a respondent id outside [0, T) asks nothing (every
 * out_row -1); a pool row with a context id outside [0, T) (or an operand outside [0, n_ops)) has NaN moments and is never
 * asked; a history row whose operand is NaN makes the fold NaN.  U = 0: nothing is launched.  VFM_E_INVALID (nothing
 * launched) for everything vfm_elicit_solve_f32 rejects and n_iters < 1. */
int vfm_elicit_bound_f32(const vfm_elicit_bound_t* p, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VFM_BOUND_H */

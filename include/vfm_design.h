/*
 * vfm_design.h -- C ABI of target-aware elicitation of libvfm_hip.so (gfx950): ask the question that most reduces the
 * predictive variance over a target set (Cohn's ALC; A-optimal design under the mean-field posterior).
 *
 * 'reg' models, kl_weight > 0.  For a respondent e of column `field` with fold rows R (the history in its given order,
 * then the rows asked, in the order asked; n = |R|, duplicates counted) and a target list J_e of contexts, the scales
 * of the exact fold-in's optimum (vfm_foldin.h) do not depend on the answers:
 *     sigma_k^2 = v_k(S_k) = kl / (kl + prec S_k),   S_k = sum_{r in R} a_rk,   a_rk = A_rk + M_rk^2
 *     sigma_w^2 = v_w(n)   = kl / (kl + prec n),     prec = link(alpha), kl = kl_weight
 * with (M_r, A_r) the unrounded fp64 operands of the row's context.  The score of a candidate q is the drop of the mean
 * over J_e of the part of Var pred_j carried by e's scales if q were asked next:
 *     W_k = (1 / |J_e|) sum_{j in J_e} a_jk            (in the list's order; an empty list: W = 0)
 *     score(q) = (v_w(n) - v_w(n + 1)) + sum_{k = 0 .. d - 1} W_k (v_k(S_k) - v_k(S_k + a_qk))
 * fp64 throughout, S added in row order (the bits of the exact fold-in's own sum), the score from the bias term on in
 * k order, rounded to fp32 once.  It does not depend on the answers, on e's current means, on `reset` or on e's table
 * row.  The best question has the highest score; ties go to the lower pool position; NaN is never asked.  A pool row
 * with a context id outside [0, T) or an operand outside [0, n_ops) scores NaN; a target with either makes W NaN, and
 * that respondent asks nothing (out_row = -1, out_score = out_loss = NaN, as when a pool runs out).
 *
 * Conventions: those of vfm_hip.h / vfm_elicit.h.  Every pointer is DEVICE memory owned by the caller; launch-only, no
 * host synchronisation, no atomics; the caller owns the workspace (vfm_design_workspace_bytes, 256-byte aligned); 0 on
 * success, a negative VFM_E_* code or a positive hipError_t otherwise; arguments are checked before any HIP call;
 * vfm_last_error() describes the last failure on the calling thread.
 */
#ifndef VFM_DESIGN_H
#define VFM_DESIGN_H

#include <stdint.h>

#include "vfm_elicit.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vfm_design_t {
  uint32_t struct_size; /* sizeof(vfm_design_t) of the caller's build; checked (VFM_STRUCT_INIT)                      */
  uint32_t abi_version; /* VFM_ABI_VERSION of the caller's build                                                      */
  int64_t U;            /* respondents                                                                                */
  int64_t P;            /* pool rows of all respondents                                                               */
  int64_t H;            /* history rows of all respondents (0: none)                                                  */
  int64_t T;            /* table rows                                                                                 */
  int64_t n_ops;        /* distinct contexts of pool, history and targets (row operands)                              */
  int64_t n_targets;    /* target entries of all respondents (0: none)                                                */
  int32_t F, d;         /* fields (2 .. VFM_MAX_FIELDS), embedding size (1 .. VFM_FOLDIN_MAX_D)                       */
  int32_t field;        /* the respondents' column                                                                    */
  int32_t n_rounds;     /* Q, 0 .. VFM_ELICIT_MAX_ROUNDS (vfm_design_elicit_f32; ignored by vfm_design_scores_f32)    */
  int32_t flags;        /* 0 or VFM_FLAG_LINK_SOFTPLUS                                                                */
  int32_t reset;        /* 1: round 0's moments (out_mean / out_var) are those of the prior; the scores do not care   */
  int32_t write;        /* 1: the respondents' table rows get the final posterior; 0: no table byte changes           */
  int32_t lds_dim;      /* -1: systems up to VFM_FOLDIN_SOLVE_LDS_DIM live in LDS; >= 0: up to that size (tests)      */
  float kl_weight;      /* weight of the KL terms, > 0                                                                */
  const int64_t* entities;   /* [U] respondent ids, ascending                                                         */
  const int64_t* pool_ptr;   /* [U + 1] offsets of each respondent's pool rows                                        */
  const int64_t* pool_x;     /* [P, F] the pool rows, in the caller's pool order per respondent                       */
  const float* pool_y;       /* [P] the answer each question would receive (sessions only)                            */
  const int64_t* hist_ptr;   /* [U + 1] offsets of each respondent's history rows, or NULL (H = 0)                    */
  const int64_t* hist_x;     /* [H, F] (sessions only)                                                                */
  const float* hist_y;       /* [H] (sessions only)                                                                   */
  const int64_t* tgt_ptr;    /* [U + 1] offsets of each respondent's target list                                      */
  const int64_t* tgt_op;     /* [n_targets] operand of each target context                                            */
  const int64_t* op_x;       /* [n_ops, F] one row of each distinct context (column `field` is ignored)               */
  const int64_t* pool_op;    /* [P] operand of each pool row                                                          */
  const int64_t* hist_op;    /* [H] operand of each history row, in [0, n_ops)                                        */
  float* entity_params;      /* [T, 2d]: read; the rows of `entities` are written when `write`                        */
  float* bias_params;        /* [T, 2]                                                                                */
  const float* scalars;      /* [3]                                                                                   */
  int64_t* out_row;          /* [U, Q] the pool row asked (an index into pool_x's rows), or -1                        */
  float* out_score;          /* [U, Q] its score                                                                      */
  float* out_loss;           /* [U, Q] the exact fold-in's out_loss after the round                                   */
  float* out_theta;          /* NULL, or [U, Q, 2d + 2] = [mu | s | mu_w | s_w] after each round                      */
  float* out_mean;           /* NULL, or [Q + 1, P]: as in vfm_elicit_field_t (both or neither)                       */
  float* out_var;
  float* out_pool_score;     /* [P] every pool row's score (vfm_design_scores_f32 only)                               */
  void* workspace;
  int64_t workspace_bytes;
} vfm_design_t;

/* Workspace of both entry points in bytes: vfm_elicit_solve_workspace_bytes' layout (the asked flags [P], the moments'
 * operands [n_ops, 4d + 2], the fold-in's fp32 and fp64 row operands and, when a (d + 1) x (d + 1) system does not fit
 * in LDS, one slab per workgroup).  Negative on bad arguments. */
int64_t vfm_design_workspace_bytes(int64_t U, int64_t P, int64_t n_ops, int32_t d, int32_t lds_dim);

/* The one-round form: out_pool_score [P] = score of every pool row with R = the respondent's history.  n_rounds, reset,
 * write, pool_y, hist_x, hist_y and the session outputs are ignored.  A respondent id outside [0, T): NaN scores.
 * Launches: the fp64 operand pass over op_x and one score kernel. */
int vfm_design_scores_f32(const vfm_design_t* p, void* stream);

/* The sessions: per respondent and round q, score every row not asked yet, ask the best, then fold in -- e's posterior
 * becomes bitwise what vfm_foldin_solve_f32 writes for E = 1, col = field on the history followed by the rows asked so
 * far, and out_loss is that call's out_loss; out_theta, out_mean / out_var and `write` as in vfm_elicit_solve_f32.  A
 * respondent's result does not depend on the other respondents, the grid, the stream or where its triangle is stored.
 * Launches, whatever n_rounds: the three operand passes over op_x and one session kernel. */
int vfm_design_elicit_f32(const vfm_design_t* p, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VFM_DESIGN_H */

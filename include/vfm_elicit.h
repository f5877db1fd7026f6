/*
 * vfm_elicit.h -- C ABI of the elicitation session of libvfm_hip.so (gfx950): an adaptive questionnaire -- ask, fold
 * in, ask again -- for many users in one launch.
 *
 * The reference's last act (vfm.py:1236-1251, --interactive) asks every test user N_QUESTIONS_ASKED questions: pick the
 * next question by a strategy, take the answer, refit the user's parameters alone.  With the items frozen the users are
 * independent, and every round of a user's session depends on that user's own posterior only, so a whole session runs
 * where a whole fold-in runs (vfm_foldin.h): one lane group per user, theta_u in registers over all rounds, the user's
 * rows in LDS.
 *
 * Per user u independently, for round q = 0 .. n_rounds - 1:
 *  1. Score.  Every pool row of u not asked yet gets the closed-form (mean, var, score) of the pair (u, item) under u's
 *     CURRENT posterior (round 0: the table row, or the prior mu = 0, sigma = 1 with `reset`) and the frozen item rows:
 *     bitwise what vfm_predictive_moments_f32 (vfm_rank.h) returns for the pair if u's table row held that posterior;
 *     VFM_RANK_RANDOM: the Philox uniform keyed on (seed + q, u, item).
 *  2. Choose.  The best score; ties go to the lower pool position; a NaN score is never chosen.  Nothing left to ask:
 *     out_row = -1, out_score = out_loss = NaN, and nothing more is folded for u.
 *  3. Fold in.  u's rows are now the history in its given order followed by the asked rows in the order asked: n_steps
 *     Adam updates from the current posterior with fresh moments, bitwise what vfm_foldin_f32 gives for E = 1 on exactly
 *     those rows (the sampled objective with t0 + q (n_steps + 1) as its t0).  The result is round q + 1's posterior.
 *
 * Two-field models: column 0 the users, column 1 the items; the items' rows are frozen (an id of `users` must not
 * appear among the items).  A user's result does not depend on the other users of the launch, the grid or the stream.
 * Launches: one operand pass over op_x (closed form only) and the session kernel, whatever n_rounds.
 *
 * Conventions: those of vfm_hip.h / vfm_foldin.h.  Every pointer is DEVICE memory owned by the caller; launch-only, no
 * host synchronisation; the caller owns the workspace (vfm_elicit_workspace_bytes, 256-byte aligned); 0 on success, a
 * negative VFM_E_* code or a positive hipError_t otherwise; arguments are checked before any HIP call;
 * vfm_last_error() describes the last failure on the calling thread.
 */
#ifndef VFM_ELICIT_H
#define VFM_ELICIT_H

#include <stdint.h>

#include "vfm_foldin.h"
#include "vfm_hip.h"
#include "vfm_rank.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VFM_ELICIT_MAX_ROUNDS 4096

typedef struct vfm_elicit_t {
  uint32_t struct_size; /* sizeof(vfm_elicit_t) of the caller's build; checked (VFM_STRUCT_INIT)                     */
  uint32_t abi_version; /* VFM_ABI_VERSION of the caller's build                                                     */
  int64_t U;            /* users                                                                                     */
  int64_t P;            /* pool rows of all users                                                                    */
  int64_t H;            /* history rows of all users (0: none)                                                       */
  int64_t T;            /* table rows                                                                                */
  int64_t n_ops;        /* closed form: distinct items of pool and history (row operands); 0 for the sampled form    */
  int32_t F, d;         /* fields (must be 2), embedding size (1 .. VFM_FOLDIN_MAX_D)                                */
  int32_t n_rounds;     /* Q, 0 .. VFM_ELICIT_MAX_ROUNDS                                                             */
  int32_t strategy;     /* VFM_RANK_TOP / VARIANCE / MEAN / RANDOM                                                   */
  int32_t objective;    /* VFM_OBJ_CLOSED_FORM (VFM_LIK_NORMAL only) or VFM_OBJ_SAMPLED                              */
  int32_t likelihood;   /* VFM_LIK_NORMAL / VFM_LIK_BERNOULLI                                                        */
  int32_t flags;        /* 0 or VFM_FLAG_LINK_SOFTPLUS                                                               */
  int32_t n_steps;      /* Adam updates per round (>= 0)                                                             */
  int32_t n_samples;    /* sampled objective: draws per iteration, 1 .. VFM_FOLDIN_MAX_SAMPLES                       */
  int32_t reset;        /* 1: round 0 starts from the prior instead of the users' table rows                         */
  int32_t write;        /* 1: the users' table rows get the final posterior; 0: no table byte changes                */
  int32_t lds_rows;     /* -1: as many fold rows per user staged in LDS as fit; >= 0: at most that many (tests)      */
  float lr, kl_weight;
  uint64_t seed;        /* Philox key: the strategy's uniforms (seed + q) and the sampled objective's draws          */
  int64_t t0;           /* sampled: the draw key of round 0's first iteration                                        */
  const int64_t* users;      /* [U] user ids, ascending                                                              */
  const int64_t* pool_ptr;   /* [U + 1] offsets of each user's pool rows                                             */
  const int64_t* pool_items; /* [P] item ids, in the caller's pool order per user                                    */
  const float* pool_y;       /* [P] the answer each question would receive                                           */
  const int64_t* hist_ptr;   /* [U + 1] offsets of each user's history rows, or NULL (H = 0)                         */
  const int64_t* hist_items; /* [H]                                                                                  */
  const float* hist_y;       /* [H]                                                                                  */
  const int64_t* op_x;       /* closed form: [n_ops, 2] the distinct items in column 1 (column 0 is ignored)         */
  const int64_t* pool_op;    /* closed form: [P] operand of each pool row                                            */
  const int64_t* hist_op;    /* closed form: [H] operand of each history row                                         */
  float* entity_params;      /* [T, 2d]: read; the rows of `users` are written when `write`                          */
  float* bias_params;        /* [T, 2]                                                                               */
  const float* scalars;      /* [3]                                                                                  */
  int64_t* out_row;          /* [U, Q] the pool row asked (an index into pool_items), or -1                          */
  float* out_score;          /* [U, Q] its score                                                                     */
  float* out_loss;           /* [U, Q] the fold-in's out_loss after the round                                        */
  float* out_theta;          /* NULL, or [U, Q, 2d + 2] = [mu | s | mu_w | s_w] after each round                     */
  float* out_mean;           /* NULL, or [Q + 1, P]: the logit mean of every pool row as scored before round q; row   */
  float* out_var;            /*   Q is one more scoring pass after the last fold (both or neither).  Rows already     */
                             /*   asked keep being written: the caller masks them with out_row.                      */
  void* workspace;
  int64_t workspace_bytes;
} vfm_elicit_t;

/* Workspace of vfm_elicit_f32 in bytes: the asked flags [P] and, for the closed form, the row operands.  Negative on
 * bad arguments. */
int64_t vfm_elicit_workspace_bytes(int64_t P, int64_t n_ops, int32_t d, int32_t objective);

/* Run the sessions of p.  A user id outside [0, T) asks nothing (every out_row -1); a pool item outside [0, T) has NaN
 * moments and is never asked. */
int vfm_elicit_f32(const vfm_elicit_t* p, void* stream);

/* ---- The field form: sessions for models with any number of fields ----------------------------------------------------
 * A respondent is an entity of column `field` (0 <= field < F, 2 <= F <= VFM_MAX_FIELDS).  A pool row is a full row
 * [F]: column `field` the respondent, the other columns the question's context, whose table rows are frozen (an id of
 * `entities` must not appear in a context column).  key_col, a context column, gives the Philox key of VFM_RANK_RANDOM,
 * as qkey does in vfm_field_moments_f32.
 *
 * Per respondent e independently, for round q = 0 .. n_rounds - 1:
 *  1. Score.  Every pool row of e not asked yet gets (mean, var, score): bitwise what vfm_field_moments_f32 (vfm_rank.h)
 *     returns for that row with this `field`, this `strategy`, seed `seed + q` and qkey = row[key_col], if e's table row
 *     held e's CURRENT posterior (round 0: the table row, or the prior with `reset`).  The rounding is the one stated in
 *     vfm_rank.h: the context operands M, A, A + M^2, C, c_mean, c_var formed in fp64 in column order and rounded once;
 *     the mean chain over d and the variance chain over [mu^2 | sigma^2 | mu] as fp32 fma chains in k order; then
 *     (chain + c_mean) + mu_w and (chain + c_var) + sigma_w^2.
 *  2. Choose.  As vfm_elicit_f32: the best score, ties to the lower pool position, NaN never; nothing left to ask:
 *     out_row = -1, out_score = out_loss = NaN, and nothing more is folded for e.
 *  3. Fold in.  e's rows are its history in the given order, then the asked rows in the order asked: n_steps Adam
 *     updates from the current posterior with fresh moments, bitwise what vfm_foldin_f32 gives for E = 1, col = field on
 *     exactly those rows (the sampled objective with t0 + q (n_steps + 1) as its t0).
 * A respondent's result does not depend on the other respondents, the grid or the stream.  Launches: the operand passes
 * over op_x (the score's operands for both objectives, the fold-in's for the closed form) and one session kernel,
 * whatever n_rounds.  No atomics.  The options and outputs are those of vfm_elicit_t, unchanged in meaning. */
typedef struct vfm_elicit_field_t {
  uint32_t struct_size; /* sizeof(vfm_elicit_field_t) of the caller's build; checked (VFM_STRUCT_INIT)                */
  uint32_t abi_version; /* VFM_ABI_VERSION of the caller's build                                                      */
  int64_t U;            /* respondents                                                                                */
  int64_t P;            /* pool rows of all respondents                                                               */
  int64_t H;            /* history rows of all respondents (0: none)                                                  */
  int64_t T;            /* table rows                                                                                 */
  int64_t n_ops;        /* distinct contexts of pool and history (row operands), both objectives                      */
  int32_t F, d;         /* fields (2 .. VFM_MAX_FIELDS), embedding size (1 .. VFM_FOLDIN_MAX_D)                       */
  int32_t field;        /* the respondents' column                                                                    */
  int32_t key_col;      /* the context column whose id keys VFM_RANK_RANDOM                                           */
  int32_t n_rounds;     /* Q, 0 .. VFM_ELICIT_MAX_ROUNDS                                                              */
  int32_t strategy;     /* VFM_RANK_TOP / VARIANCE / MEAN / RANDOM                                                    */
  int32_t objective;    /* VFM_OBJ_CLOSED_FORM (VFM_LIK_NORMAL only) or VFM_OBJ_SAMPLED                               */
  int32_t likelihood;   /* VFM_LIK_NORMAL / VFM_LIK_BERNOULLI                                                         */
  int32_t flags;        /* 0 or VFM_FLAG_LINK_SOFTPLUS                                                                */
  int32_t n_steps;      /* Adam updates per round (>= 0)                                                              */
  int32_t n_samples;    /* sampled objective: draws per iteration, 1 .. VFM_FOLDIN_MAX_SAMPLES                        */
  int32_t reset;        /* 1: round 0 starts from the prior instead of the respondents' table rows                    */
  int32_t write;        /* 1: the respondents' table rows get the final posterior; 0: no table byte changes           */
  int32_t lds_rows;     /* -1: as many fold rows per respondent staged in LDS as fit; >= 0: at most that many (tests) */
  float lr, kl_weight;
  uint64_t seed;        /* Philox key: the strategy's uniforms (seed + q) and the sampled objective's draws           */
  int64_t t0;           /* sampled: the draw key of round 0's first iteration                                         */
  const int64_t* entities;   /* [U] respondent ids, ascending                                                         */
  const int64_t* pool_ptr;   /* [U + 1] offsets of each respondent's pool rows                                        */
  const int64_t* pool_x;     /* [P, F] the pool rows, in the caller's pool order per respondent                       */
  const float* pool_y;       /* [P] the answer each question would receive                                            */
  const int64_t* hist_ptr;   /* [U + 1] offsets of each respondent's history rows, or NULL (H = 0)                    */
  const int64_t* hist_x;     /* [H, F]                                                                                */
  const float* hist_y;       /* [H]                                                                                   */
  const int64_t* op_x;       /* [n_ops, F] one row of each distinct context (column `field` is ignored)               */
  const int64_t* pool_op;    /* [P] operand of each pool row, in [0, n_ops)                                           */
  const int64_t* hist_op;    /* [H] operand of each history row                                                       */
  float* entity_params;      /* [T, 2d]: read; the rows of `entities` are written when `write`                        */
  float* bias_params;        /* [T, 2]                                                                                */
  const float* scalars;      /* [3]                                                                                   */
  int64_t* out_row;          /* [U, Q] the pool row asked (an index into pool_x's rows), or -1                        */
  float* out_score;          /* [U, Q] its score                                                                      */
  float* out_loss;           /* [U, Q] the fold-in's out_loss after the round                                         */
  float* out_theta;          /* NULL, or [U, Q, 2d + 2] = [mu | s | mu_w | s_w] after each round                      */
  float* out_mean;           /* NULL, or [Q + 1, P]: the logit mean of every pool row as scored before round q; row    */
  float* out_var;            /*   Q is one more scoring pass after the last fold (both or neither).  Rows already      */
                             /*   asked keep being written: the caller masks them with out_row.                       */
  void* workspace;
  int64_t workspace_bytes;
} vfm_elicit_field_t;

/* Workspace of vfm_elicit_field_f32 in bytes: the asked flags [P], the score's operands [n_ops, 4d + 2] and, for the
 * closed form, the fold-in's row operands.  Negative on bad arguments. */
int64_t vfm_elicit_field_workspace_bytes(int64_t P, int64_t n_ops, int32_t d, int32_t objective);

/* Run the sessions of p.  A respondent id outside [0, T) asks nothing (every out_row -1); a pool row with a context id
 * outside [0, T) (or an operand outside [0, n_ops)) has NaN moments and is never asked. */
int vfm_elicit_field_f32(const vfm_elicit_field_t* p, void* stream);

/* ---- The exact field-form session: ask, solve the optimum, ask again ---------------------------------------------------
 * vfm_elicit_field_f32 with the closed-form objective, where each round's n_steps Adam updates are replaced by the exact
 * fold-in (vfm_foldin.h: vfm_foldin_solve_f32): the global optimum of L_e on the respondent's rows, one small symmetric
 * positive definite solve.  No lr, n_steps or starting point.  'reg' models (Normal likelihood), kl_weight > 0.
 *
 * Per respondent e of column `field` independently, for round q = 0 .. n_rounds - 1:
 *  1. Score and choose: steps 1-2 of vfm_elicit_field_f32, unchanged in meaning and in bits (scores under e's CURRENT
 *     posterior; round 0: the table row, or the prior with `reset`; VFM_RANK_RANDOM keyed on (seed + q, row[key_col], e);
 *     ties to the lower pool position; NaN never; nothing left: out_row = -1, out_score = out_loss = NaN and nothing more
 *     is folded for e).
 *  2. Fold in.  e's rows are its history in the given order, then the asked rows in the order asked; e's posterior becomes
 *     bitwise what vfm_foldin_solve_f32 writes for E = 1, col = field on exactly those rows, and out_loss is that call's
 *     out_loss.  The optimum does not depend on the current row, so `reset` affects round 0's scoring only.
 * A respondent's result does not depend on the other respondents, the grid, the stream or where its triangle is stored.
 * Launches, whatever n_rounds: the score's operand pass, the fold-in's fp32 (for the loss) and fp64 operand passes over
 * op_x, and one session kernel.  No atomics, no host synchronisation. */
typedef struct vfm_elicit_solve_t {
  uint32_t struct_size; /* sizeof(vfm_elicit_solve_t) of the caller's build; checked (VFM_STRUCT_INIT)                */
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
  int32_t reset;        /* 1: round 0 is scored from the prior instead of the respondents' table rows                 */
  int32_t write;        /* 1: the respondents' table rows get the final posterior; 0: no table byte changes           */
  int32_t lds_dim;      /* -1: systems up to VFM_FOLDIN_SOLVE_LDS_DIM live in LDS; >= 0: up to that size (tests)      */
  float kl_weight;      /* weight of the KL terms, > 0                                                                */
  uint64_t seed;        /* Philox key of the strategy's uniforms (seed + q)                                           */
  const int64_t* entities;   /* [U] respondent ids, ascending                                                         */
  const int64_t* pool_ptr;   /* [U + 1] offsets of each respondent's pool rows                                        */
  const int64_t* pool_x;     /* [P, F] the pool rows, in the caller's pool order per respondent                       */
  const float* pool_y;       /* [P] the answer each question would receive                                            */
  const int64_t* hist_ptr;   /* [U + 1] offsets of each respondent's history rows, or NULL (H = 0)                    */
  const int64_t* hist_x;     /* [H, F]                                                                                */
  const float* hist_y;       /* [H]                                                                                   */
  const int64_t* op_x;       /* [n_ops, F] one row of each distinct context (column `field` is ignored)               */
  const int64_t* pool_op;    /* [P] operand of each pool row, in [0, n_ops)                                           */
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
  void* workspace;
  int64_t workspace_bytes;
} vfm_elicit_solve_t;

/* Workspace of vfm_elicit_solve_f32 in bytes: the asked flags [P], the score's operands [n_ops, 4d + 2], the fold-in's
 * fp32 and fp64 row operands and, when a (d + 1) x (d + 1) system does not fit in LDS (lds_dim as in the struct), one
 * slab per workgroup (min(U, VFM_FOLDIN_SOLVE_SLABS)).  Negative on bad arguments. */
int64_t vfm_elicit_solve_workspace_bytes(int64_t U, int64_t P, int64_t n_ops, int32_t d, int32_t lds_dim);

/* Run the sessions of p.  A respondent id outside [0, T) asks nothing (every out_row -1); a pool row with a context id
 * outside [0, T) (or an operand outside [0, n_ops)) has NaN moments and is never asked; a history row whose operand is
 * NaN makes the fold NaN, as in vfm_foldin_solve_f32. */
int vfm_elicit_solve_f32(const vfm_elicit_solve_t* p, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VFM_ELICIT_H */

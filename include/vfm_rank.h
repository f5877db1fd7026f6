/*
 * vfm_rank.h -- C ABI of the preference-elicitation kernels of libvfm_hip.so (gfx950): closed-form predictive
 * moments of the mean-field posterior, and a fused catalog ranking (scores by fp32 MFMA, exclusion lists, top k).
 *
 * The caller of the posterior in the reference is select_next_question / predict_proba (vfm.py:1024-1057): it scores
 * (user, item) pairs by the mean probability or the logit variance over S posterior samples.  These entry points give
 * the exact S -> infinity limit of those estimates in one pass.
 *
 * Conventions: those of vfm_hip.h.  Every pointer is DEVICE memory owned by the caller; launch-only, no host
 * synchronisation; the caller owns the workspace (vfm_rank_workspace_bytes); 0 on success, a negative VFM_E_* code or a
 * positive hipError_t otherwise; arguments are checked before any HIP call; vfm_last_error() (vfm_hip.h) describes the
 * last failure on the calling thread.  Tables as in vfm_hip.h: entity_params [T, 2d] = [mu | s],
 * bias_params [T, 2] = [mu_w, s_w], scalars [3] = alpha, global_bias_mean, global_bias_scale; sigma = link(s),
 * link = |.|, or softplus with VFM_FLAG_LINK_SOFTPLUS.
 *
 * Closed form (a_f ~ N(m_f, s_f^2) independent per coordinate k):
 *   E[pred]   = m0 + sum_f mu_w,f + sum_k sum_{f<g} m_f m_g
 *   Var[pred] = sigma0^2 + sum_f sigma_w,f^2 + sum_k [ sum_{f<g} s_f^2 s_g^2 + sum_f s_f^2 (sum_{g!=f} m_g)^2 ]
 * For two fields (u, i) the pair term is sum_k (mu_u^2 sigma_i^2 + sigma_u^2 (mu_i^2 + sigma_i^2)).
 */
#ifndef VFM_RANK_H
#define VFM_RANK_H

#include <stdint.h>

#include "vfm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* scoring strategies (the reference's select_next_question strategies, plus plain top-k) */
#define VFM_RANK_TOP 0      /* score = E[pred]                                                         */
#define VFM_RANK_VARIANCE 1 /* score = Var[pred] (the logit variance of predict_proba)                */
#define VFM_RANK_MEAN 2     /* score = -|E| / sqrt(1 + pi Var / 8): the probit form of -|p_bar - 0.5|  */
#define VFM_RANK_RANDOM 3   /* score = Philox uniform in [0,1) keyed on (seed, user id, item id)     */
#define VFM_RANK_MAX_K 128
#define VFM_RANK_MAX_SPLITS 64

/* Closed-form logit mean and variance of rows x [B, F] (int64 or int32 ids by id_bits), any F <= VFM_MAX_FIELDS.
 * flags: 0 or VFM_FLAG_LINK_SOFTPLUS.  score: NULL, or [B] written with the ranking score of `strategy` (for
 * VFM_RANK_RANDOM keyed on (seed, x[r,0], x[r,1]); F == 2 for VFM_RANK_RANDOM).  For F == 2 the three outputs are
 * bitwise those vfm_rank_items_f32 forms for the same pair.  A row with an id outside [0, T) gets NaN outputs. */
int vfm_predictive_moments_f32(int64_t B, int32_t F, int32_t d, int64_t T, int32_t id_bits, int32_t flags,
                               const void* x, const float* entity_params, const float* bias_params,
                               const float* scalars, int32_t strategy, uint64_t seed, float* logit_mean,
                               float* logit_var, float* score, void* stream);

/* Workspace of vfm_rank_items_f32, in bytes (n_splits = 0: the automatic split count).  Negative on bad arguments. */
int64_t vfm_rank_workspace_bytes(int64_t U, int64_t n_cand, int32_t d, int32_t k, int32_t strategy, int32_t n_splits);

/* Top k candidate items of each query user, two-field model (F must be 2).
 *  users [U] int64 entity ids of the users; candidates: cand [n_cand] int64 entity ids, STRICTLY ASCENDING, or
 *  cand == NULL for the range [item_lo, item_lo + n_cand).  n_cand < 2^31.
 *  Exclusion: excl_ptr [U+1] int64 offsets into excl_items [n_excl] (int64 entity ids, ascending per user); both NULL
 *  (and n_excl 0) for none.  The walk over a user's list advances with the candidates: cost O(list length).
 *  Order: score descending, then item id ascending; NaN scores are never returned.  Bitwise deterministic and
 *  independent of n_splits (1 .. VFM_RANK_MAX_SPLITS, 0 = automatic): every pair's score is one k-ordered fp32 fma
 *  chain (the fp32-input MFMA).
 *  Outputs [U, k]: out_items (entity ids), out_score, out_mean, out_var (the winners' closed-form moments).  Fewer than
 *  k candidates: item -1, score -inf, NaN moments.  flags: 0 or VFM_FLAG_LINK_SOFTPLUS. */
int vfm_rank_items_f32(int64_t U, const int64_t* users, int64_t n_cand, const int64_t* cand, int64_t item_lo,
                       int64_t T, int32_t F, int32_t d, int32_t k, int32_t strategy, int32_t flags, uint64_t seed,
                       int32_t n_splits, const int64_t* excl_ptr, const int64_t* excl_items, int64_t n_excl,
                       const float* entity_params, const float* bias_params, const float* scalars, void* workspace,
                       int64_t workspace_bytes, int64_t* out_items, float* out_score, float* out_mean,
                       float* out_var, void* stream);

/* Workspace of vfm_rank_heldout_f32, in bytes (n_splits = 0: the automatic split count): the packed operands of
 * vfm_rank_items_f32 plus O(n_splits (U + n_pos)), never O(U n_cand).  Negative on bad arguments. */
int64_t vfm_rank_eval_workspace_bytes(int64_t U, int64_t n_cand, int64_t n_pos, int32_t d, int32_t strategy,
                                      int32_t n_splits);

/* Held-out ranking evaluation, two-field model (F must be 2): where each user's held-out positives land in the user's
 * full ranking of the candidates, in the order of vfm_rank_items_f32 (c beats i: score_c > score_i, or equal scores and
 * id_c < id_i; the scores bitwise those of vfm_predictive_moments_f32 for the strategy).
 *  users, cand / item_lo, n_cand, exclusions, strategy, seed, n_splits, flags: as vfm_rank_items_f32.  The eligible
 *  candidates of user u, E_u: the candidates not excluded for u.
 *  Positives: pos_ptr [U+1] int64 offsets into pos_items [n_pos] (int64 entity ids, STRICTLY ASCENDING per user); P_u
 *  the positives of u.  Every positive should lie in E_u (the caller checks: the Python layer raises otherwise).
 *  Outputs, int64: per positive p of u (aligned with pos_items) out_rank[p] = #{c in E_u : c beats p} (p's 0-based
 *  position in u's ranking), out_rank_neg[p] = #{c in E_u \ P_u : c beats p}; per user out_n_eligible[u] = |E_u|,
 *  out_n_neg[u] = |E_u \ P_u|.  Integer counts: bitwise deterministic and independent of n_splits, the grid and the
 *  stream.  A positive with rank < k is item [rank] of vfm_rank_items_f32's list for k; one with rank >= k is not in it.
 *  Scores are assumed finite (a NaN score -- non-finite parameters -- compares false with everything).  Cost: the
 *  ranking's score tiles and scan, a positive compare per candidate, a binary search over P_u for the candidates that
 *  beat u's last positive; O(|P_u|^2) to sort P_u. */
int vfm_rank_heldout_f32(int64_t U, const int64_t* users, int64_t n_cand, const int64_t* cand, int64_t item_lo,
                         int64_t T, int32_t F, int32_t d, int32_t strategy, int32_t flags, uint64_t seed,
                         int32_t n_splits, const int64_t* excl_ptr, const int64_t* excl_items, int64_t n_excl,
                         const int64_t* pos_ptr, const int64_t* pos_items, int64_t n_pos,
                         const float* entity_params, const float* bias_params, const float* scalars, void* workspace,
                         int64_t workspace_bytes, int64_t* out_rank, int64_t* out_rank_neg, int64_t* out_n_eligible,
                         int64_t* out_n_neg, void* stream);

/* ---- One field's catalog ranked for models with any number of fields (the field form) --------------------------------
 * A query is a context: one entity of every field but `field`; c is a candidate entity of `field`.  With S the sum of
 * the context's embeddings and P their pair term, per coordinate k (sums over the context columns q):
 *   M = E S,  A = Var S = sum_q sigma_q^2,  C = 2 Cov(S, P) = 2 sum_q sigma_q^2 (M - mu_q),
 *   c_mean = m0 + sum_q mu_w,q + sum_k E P,  c_var = sigma0^2 + sum_q sigma_w,q^2 + sum_k Var P
 *   E pred   = c_mean + mu_w,c + sum_k mu_c M
 *   Var pred = c_var + sigma_w,c^2 + sum_k [ mu_c^2 A + sigma_c^2 (A + M^2) + mu_c C ]
 * (the closed form above with the context's part separated; Var P is its context-only part).  Over a catalog these are
 * two GEMMs: query [M] . candidate [mu] (K = d), query [A | A + M^2 | C] . candidate [mu^2 | sigma^2 | mu] (K = 3d).
 *
 * Rounding, the bitwise definition of a field-form score: M, A, A + M^2, C per coordinate and c_mean, c_var are formed
 * in fp64 -- sums over the context columns in column order, then for the two constants over the coordinates in k order --
 * and each rounded to fp32 once; the two dot products are fp32 fma chains in k order (the variance chain over
 * [mu^2 | sigma^2 | mu] in that order); mean = (chain + c_mean) + mu_w,c, var = (chain + c_var) + sigma_w,c^2. */

/* Field-form moments of rows x [B, F] (int64 or int32 ids by id_bits): column `field` is the candidate, the other
 * columns its context; 2 <= F <= VFM_MAX_FIELDS.  score: NULL, or [B] written with the ranking score of `strategy`; for
 * VFM_RANK_RANDOM the Philox uniform keyed on (seed, qkey[r], x[r, field]); qkey [B] int64, NULL: the row's position r.
 * The three outputs are bitwise those vfm_rank_field_f32 returns for the same (context, candidate).  A row with an id
 * outside [0, T) gets NaN outputs.  flags: 0 or VFM_FLAG_LINK_SOFTPLUS. */
int vfm_field_moments_f32(int64_t B, int32_t F, int32_t d, int64_t T, int32_t id_bits, int32_t flags, const void* x,
                          int32_t field, const float* entity_params, const float* bias_params, const float* scalars,
                          int32_t strategy, uint64_t seed, const int64_t* qkey, float* logit_mean, float* logit_var,
                          float* score, void* stream);

/* Workspace of vfm_rank_field_f32, in bytes (n_splits = 0: the automatic split count).  Negative on bad arguments. */
int64_t vfm_rank_field_workspace_bytes(int64_t Q, int64_t n_cand, int32_t F, int32_t d, int32_t k, int32_t strategy,
                                       int32_t n_splits);

/* Top k candidates of field `field` for each query context.
 *  ctx [Q, F] int64 entity ids; column `field` is ignored.  qkey [Q] int64: the query's key of VFM_RANK_RANDOM (score =
 *  Philox uniform keyed on (seed, qkey[q], candidate id)); NULL: the query's position q.
 *  cand / cand_lo / n_cand, excl_ptr [Q+1] / excl_items / n_excl, k, the order (score descending, then candidate id
 *  ascending), padding, NaN handling (a context or candidate id outside [0, T): NaN scores, never returned), n_splits:
 *  as the users, items and exclusions of vfm_rank_items_f32.  2 <= F <= VFM_MAX_FIELDS.
 *  Outputs [Q, k]: out_items, out_score, out_mean, out_var: each returned score, mean and variance is bitwise
 *  vfm_field_moments_f32 of the row (context, candidate).  Bitwise deterministic and independent of n_splits, the grid
 *  and the stream. */
int vfm_rank_field_f32(int64_t Q, const int64_t* ctx, int32_t field, const int64_t* qkey, int64_t n_cand,
                       const int64_t* cand, int64_t cand_lo, int64_t T, int32_t F, int32_t d, int32_t k,
                       int32_t strategy, int32_t flags, uint64_t seed, int32_t n_splits, const int64_t* excl_ptr,
                       const int64_t* excl_items, int64_t n_excl, const float* entity_params, const float* bias_params,
                       const float* scalars, void* workspace, int64_t workspace_bytes, int64_t* out_items,
                       float* out_score, float* out_mean, float* out_var, void* stream);

/* Workspace of vfm_rank_heldout_field_f32, in bytes (n_splits = 0: the automatic split count): the packed operands of
 * vfm_rank_field_f32 (both parts, no top-k lists) plus O(n_splits (Q + n_pos)), never O(Q n_cand).  Negative on bad
 * arguments. */
int64_t vfm_rank_eval_field_workspace_bytes(int64_t Q, int64_t n_cand, int64_t n_pos, int32_t F, int32_t d,
                                            int32_t strategy, int32_t n_splits);

/* Held-out ranking evaluation in the field form, 2 <= F <= VFM_MAX_FIELDS: where each query context's held-out
 * positives land in the query's full ranking of the candidates of `field`, in the order of vfm_rank_field_f32 (c beats
 * i: score_c > score_i, or equal scores and id_c < id_i; the scores bitwise those of vfm_field_moments_f32 of the row
 * (context, candidate) for the strategy).
 *  ctx [Q, F], field, qkey, cand / cand_lo / n_cand, the exclusion CSR over the queries, strategy, seed, n_splits, flags:
 *  as vfm_rank_field_f32.  The eligible candidates of query q, E_q: the candidates not excluded for q.
 *  Positives: pos_ptr [Q+1] int64 offsets into pos_items [n_pos] (int64 entity ids of `field`, STRICTLY ASCENDING per
 *  query); P_q the positives of q.  Every positive should lie in E_q (the caller checks: the Python layer raises or
 *  drops).
 *  Outputs, int64: per positive p of q (aligned with pos_items) out_rank[p] = #{c in E_q : c beats p},
 *  out_rank_neg[p] = #{c in E_q \ P_q : c beats p}; per query out_n_eligible[q] = |E_q|, out_n_neg[q] = |E_q \ P_q|.
 *  Integer counts: bitwise deterministic and independent of n_splits, the grid, the stream and the other queries of the
 *  call.  A positive with rank < k is item [rank] of vfm_rank_field_f32's list for k; one with rank >= k is not in it.
 *  A context or candidate id outside [0, T) gives a NaN score, which compares false with everything.  Q == 0: returns
 *  0, nothing is launched.  Cost: the operand packing and score tiles of vfm_rank_field_f32, one 4d-long fp32 chain per
 *  positive, and the scan, sort and merge of vfm_rank_heldout_f32. */
int vfm_rank_heldout_field_f32(int64_t Q, const int64_t* ctx, int32_t field, const int64_t* qkey, int64_t n_cand,
                               const int64_t* cand, int64_t cand_lo, int64_t T, int32_t F, int32_t d, int32_t strategy,
                               int32_t flags, uint64_t seed, int32_t n_splits, const int64_t* excl_ptr,
                               const int64_t* excl_items, int64_t n_excl, const int64_t* pos_ptr,
                               const int64_t* pos_items, int64_t n_pos, const float* entity_params,
                               const float* bias_params, const float* scalars, void* workspace, int64_t workspace_bytes,
                               int64_t* out_rank, int64_t* out_rank_neg, int64_t* out_n_eligible, int64_t* out_n_neg,
                               void* stream);

/* ---- The field form under supplied posteriors --------------------------------------------------------------------------
 * The three entry points above with the parameters of ONE context column taken from the caller instead of the tables: a
 * posterior held outside the model (a session's theta, a what-if, a cold-start respondent) is ranked without writing it
 * into the tables.  Each takes its table form's arguments plus
 *   post_field  the context column whose parameters are supplied: 0 <= post_field < F, post_field != field;
 *   post        [Q, 2d + 2] fp32 ([B, 2d + 2] for the moments), one row per query: [mu (d) | s (d) | mu_w | s_w], s and
 *               s_w the raw stored values (the link of `flags` is applied as for a table row) -- a row of the theta a
 *               session of vfm_elicit.h returns.
 * Query q is the context ctx[q] with the parameters of column post_field taken from post[q].  Every output is bit for
 * bit what the table form returns for query q from tables in which the entity and bias rows of id ctx[q, post_field] hold
 * post[q]: for every strategy, both links, any n_splits, grid and stream, and whatever the other queries of the call are
 * (two queries may carry the same id with different rows: each is its own query).  The id in column post_field keeps
 * its other roles -- it must lie in [0, T) (else a NaN query), it is what exclusion lists and qkey refer to -- but its
 * table rows are never read.  The operand arithmetic and its rounding are those defined above; only the source of one
 * column's row differs.
 * Workspaces: the layouts do not change; vfm_rank_field_workspace_bytes and vfm_rank_eval_field_workspace_bytes serve
 * these calls.  Errors: everything the table forms reject; post_field out of range or equal to field; post == NULL
 * with Q > 0 (B > 0).  Q == 0 (B == 0): returns 0, nothing is launched. */
int vfm_field_moments_post_f32(int64_t B, int32_t F, int32_t d, int64_t T, int32_t id_bits, int32_t flags, const void* x,
                               int32_t field, int32_t post_field, const float* post, const float* entity_params,
                               const float* bias_params, const float* scalars, int32_t strategy, uint64_t seed,
                               const int64_t* qkey, float* logit_mean, float* logit_var, float* score, void* stream);

int vfm_rank_field_post_f32(int64_t Q, const int64_t* ctx, int32_t field, int32_t post_field, const float* post,
                            const int64_t* qkey, int64_t n_cand, const int64_t* cand, int64_t cand_lo, int64_t T,
                            int32_t F, int32_t d, int32_t k, int32_t strategy, int32_t flags, uint64_t seed,
                            int32_t n_splits, const int64_t* excl_ptr, const int64_t* excl_items, int64_t n_excl,
                            const float* entity_params, const float* bias_params, const float* scalars, void* workspace,
                            int64_t workspace_bytes, int64_t* out_items, float* out_score, float* out_mean,
                            float* out_var, void* stream);

int vfm_rank_heldout_field_post_f32(int64_t Q, const int64_t* ctx, int32_t field, int32_t post_field, const float* post,
                                    const int64_t* qkey, int64_t n_cand, const int64_t* cand, int64_t cand_lo, int64_t T,
                                    int32_t F, int32_t d, int32_t strategy, int32_t flags, uint64_t seed,
                                    int32_t n_splits, const int64_t* excl_ptr, const int64_t* excl_items, int64_t n_excl,
                                    const int64_t* pos_ptr, const int64_t* pos_items, int64_t n_pos,
                                    const float* entity_params, const float* bias_params, const float* scalars,
                                    void* workspace, int64_t workspace_bytes, int64_t* out_rank, int64_t* out_rank_neg,
                                    int64_t* out_n_eligible, int64_t* out_n_neg, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VFM_RANK_H */

// vfm_rank_field.hip -- ranking one field's catalog for models with any number of fields (include/vfm_rank.h:
// vfm_field_moments_f32, vfm_rank_field_f32), its held-out evaluation (vfm_rank_heldout_field_f32), and the three under
// supplied posteriors (vfm_*_post_f32: one context column's parameters from a caller's row instead of the tables).
//
// With every field of a row but one fixed (the query's context), the row's closed-form moments are linear resp.
// quadratic in the free entity c (include/vfm_foldin.h):
//   E pred   = c_mean + mu_w,c + sum_k mu_c M
//   Var pred = c_var + sigma_w,c^2 + sum_k [ mu_c^2 A + sigma_c^2 (A + M^2) + mu_c C ]
// so over a catalog they are GEMMs again: query [M] . candidate [mu] (K = d) and query [A | A + M^2 | C] . candidate
// [mu^2 | sigma^2 | mu] (K = 3d).  Only the operands are new:
//   k_field_ctx_prep   a wave per query, lanes over coordinates: fp64 sums over the context columns -> the packed row
//   k_field_cand_prep  the candidates' rows
// The score tiles, the scan with the exclusion cursor, the top k and the split merge are those of the two-field ranking
// (vfm_rank_tile.hpp, vfm_rank_scan.hpp, k_rank of vfm_rank.hip).  Both parts are always packed (the merge recomputes the
// winners' two moments from the query's packed row, whatever the strategy scored).
//
// The held-out evaluation packs the same operands, scores every positive from its query's packed row
// (k_field_pos_score: field_pair_moments again) and hands over to the sort, scan and merge of the two-field evaluation
// (vfm_rank_eval.hpp: vfm::launch_rank_eval, k_rank_eval of vfm_rank_eval.hip).
//
// Compiled with -ffp-contract=off: field_pair_moments' explicit fmaf chains are the MFMA chains of the tile, and the fp64
// operand arithmetic (ctx_coord) rounds the same in k_field_ctx_prep and k_field_moments, bit for bit.  That arithmetic
// lives in vfm_field_ctx.hpp, which the field-form elicitation session (vfm_elicit_field.hip) includes as well.
//
// The posterior forms differ in the operand formation alone: k_field_ctx_prep and k_field_moments are instantiated for
// both row-sources of vfm_field_ctx.hpp (TableRows, PostRows).  Everything downstream works from the packed row.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "vfm_rank.h"
#include "vfm_rank_tile.hpp"
#include "vfm_field_ctx.hpp"         // ctx_coord, ctx_op_var, ctx_consts, ctx_valid, cand_op_var, field_pair_moments
#include "vfm_rank_scan.hpp"
#include "vfm_rank_eval.hpp"

namespace {

constexpr int WAVE = 64;
constexpr int PREP_BLOCK = 256;       // k_field_ctx_prep: four queries per workgroup

// A query's operands read from its packed row (the ranking's workspace)
struct StoredOp {
  const float* row;
  int KA;
  __device__ float mean_op(int k) const { return row[k]; }
  int d;
  __device__ float var_op(int part, int k) const { return row[KA + part * d + k]; }
};

// A query's operands formed on the fly from its row-source (k_field_moments: no workspace)
template <typename ID, typename SRC>
struct TableOp {
  const ID* xr;
  int F, field, d;
  bool sp;
  SRC src;
  __device__ float mean_op(int k) const { return (float)ctx_coord_of(xr, F, field, k, d, sp, src).M; }
  __device__ float var_op(int part, int k) const { return ctx_op_var(ctx_coord_of(xr, F, field, k, d, sp, src), part); }
};

// ---------------------------------------------------------------------------------------------------------------------
// k_field_moments: one thread per row x [B, F]; column `field` is the free entity, the others its context, their
// parameters from rows.at(r); the candidate's always from the tables.
// ---------------------------------------------------------------------------------------------------------------------
template <typename ID, typename SRC>
__global__ __launch_bounds__(256) void k_field_moments(int64_t B, int F, int field, int d, int64_t T, bool sp,
                                                       const ID* __restrict__ x, SRC rows, const float* __restrict__ scal,
                                                       int strat, uint64_t seed, const int64_t* __restrict__ qkey,
                                                       float* __restrict__ out_m, float* __restrict__ out_v,
                                                       float* __restrict__ out_s) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= B) return;
  const ID* xr = x + r * F;
  const int64_t c = (int64_t)xr[field];
  float mean = __builtin_nanf(""), var = __builtin_nanf(""), sc = __builtin_nanf("");
  if (ctx_valid(xr, F, field, T) && c >= 0 && c < T) {
    const SRC src = rows.at(r);
    double cm, cv;
    ctx_consts_of(xr, F, field, d, sp, src, scal, cm, cv);
    for (int k = 0; k < d; ++k) {                 // (in k order, as the prep's ordered lane sum)
      const CtxCoord cc = ctx_coord_of(xr, F, field, k, d, sp, src);
      cm += cc.ep;
      cv += cc.vp;
    }
    field_pair_moments(TableOp<ID, SRC>{xr, F, field, d, sp, src}, rows.ent + c * 2 * d, rows.bias + c * 2, (float)cm,
                       (float)cv, d, sp, mean, var);
    sc = strat == VFM_RANK_RANDOM ? philox_uniform(seed, qkey ? qkey[r] : r, c) : score_of(strat, mean, var);
  }
  out_m[r] = mean;
  out_v[r] = var;
  if (out_s) out_s[r] = sc;
}

// ---------------------------------------------------------------------------------------------------------------------
// k_field_ctx_prep: a wave per query row (rows past Q: zero padding), lanes over coordinates, so every gather of a
// context entity's 8d bytes is coalesced.  Writes the packed row [M .. 0 | A | A + M^2 | C .. 0], the constants
// (c_mean, c_var) -- the coordinates' E P and Var P added in k order: an ordered sum over the lanes of each chunk of 64 --
// and, without caller keys, the query's position as its Philox key.  A context id outside [0, T): a NaN row.  The
// columns' parameters come from rows.at(r): with PostRows the lanes read the query's posterior row as they read a table
// row, 4 bytes per lane and coordinate, contiguous.
// ---------------------------------------------------------------------------------------------------------------------
template <typename SRC>
__global__ __launch_bounds__(PREP_BLOCK) void k_field_ctx_prep(int64_t Q_pad, int64_t Q, const int64_t* __restrict__ ctx,
                                                               int F, int field, int64_t T, int Kp, int KA, int KB,
                                                               int d, bool sp, SRC rows,
                                                               const float* __restrict__ scal, float* __restrict__ op,
                                                               float* __restrict__ con, int64_t* __restrict__ key_out) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t r = (int64_t)blockIdx.x * (PREP_BLOCK / WAVE) + (threadIdx.x >> 6);
  if (r >= Q_pad) return;                                   // (wave-uniform)
  float* row = op + r * Kp;
  const int64_t* xr = ctx + r * F;
  const bool live = r < Q;
  const bool ok = live && ctx_valid(xr, F, field, T);
  if (!ok) {
    const float fill = live ? __builtin_nanf("") : 0.f;
    for (int k = lane; k < Kp; k += WAVE) row[k] = fill;
    if (lane < 2) con[r * 2 + lane] = fill;
  } else {
    const SRC src = rows.at(r);
    double cm, cv;
    ctx_consts_of(xr, F, field, d, sp, src, scal, cm, cv);
    for (int k0 = 0; k0 < d; k0 += WAVE) {
      const int k = k0 + lane;
      CtxCoord cc = {0., 0., 0., 0., 0.};
      if (k < d) {
        cc = ctx_coord_of(xr, F, field, k, d, sp, src);
        row[k] = (float)cc.M;
        row[KA + k] = ctx_op_var(cc, 0);
        row[KA + d + k] = ctx_op_var(cc, 1);
        row[KA + 2 * d + k] = ctx_op_var(cc, 2);
      }
      const int n = min(WAVE, d - k0);
      for (int j = 0; j < n; ++j) {
        cm += __shfl(cc.ep, j);
        cv += __shfl(cc.vp, j);
      }
    }
    for (int k = d + lane; k < KA; k += WAVE) row[k] = 0.f;
    for (int kb = 3 * d + lane; kb < KB; kb += WAVE) row[KA + kb] = 0.f;
    if (lane == 0) {
      con[r * 2] = (float)cm;
      con[r * 2 + 1] = (float)cv;
    }
  }
  if (key_out && live && lane == 0) key_out[r] = r;
}

// ---------------------------------------------------------------------------------------------------------------------
// k_field_cand_prep: the candidates' packed rows [rows_pad, Kp] = [mu .. 0 | mu^2 | sigma^2 | mu .. 0] (zero rows past
// n_cand) and constants (mu_w, sigma_w^2); one thread per value, as k_rank_prep.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_field_cand_prep(int64_t rows_pad, int64_t rows, const int64_t* __restrict__ ids,
                                                         int64_t lo, int64_t T, int Kp, int KA, int d, bool sp,
                                                         const float* __restrict__ ent, const float* __restrict__ bias,
                                                         float* __restrict__ op, float* __restrict__ con) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int W = Kp + 2;
  if (idx >= rows_pad * W) return;
  const int64_t r = idx / W;
  const int k = (int)(idx - r * W);
  float v = 0.f;
  if (r < rows) {
    const int64_t e = ids ? ids[r] : lo + r;
    if (e < 0 || e >= T) {
      v = __builtin_nanf("");
    } else if (k < KA) {
      v = k < d ? op_mean(ent + e * 2 * d, k) : 0.f;
    } else if (k < Kp) {
      const int kb = k - KA;
      v = kb < 3 * d ? cand_op_var(ent + e * 2 * d, kb, d, sp) : 0.f;
    } else if (k == Kp) {
      v = bias[e * 2];
    } else {
      const float sw = link_of(bias[e * 2 + 1], sp);
      v = sw * sw;
    }
  }
  if (k < Kp) op[r * Kp + k] = v;
  else con[r * 2 + (k - Kp)] = v;
}

// The winners' moments of k_rank_merge: the query's packed row and constants against the candidate's table rows
struct FieldMoments {
  const float *uop, *ucon;
  int Kp, KA;
  int64_t T;
  int d;
  bool sp;
  const float *ent, *bias;
  __device__ void operator()(int64_t u, int64_t iid, float& m, float& v) const {
    if (iid >= 0 && iid < T)
      field_pair_moments(StoredOp{uop + u * Kp, KA, d}, ent + iid * 2 * d, bias + iid * 2, ucon[u * 2], ucon[u * 2 + 1], d,
                         sp, m, v);
  }
};

// ---------------------------------------------------------------------------------------------------------------------
// k_field_pos_score: one thread per held-out positive p: its query (the row of pos_ptr holding p) and the strategy's
// score of (the query's context, p) from the query's packed row -- the chains of k_rank_merge<FieldMoments>, hence bit
// for bit the tile's score and k_field_moments' score.  NaN for a context or candidate id outside [0, T).
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(POS_BLOCK) void k_field_pos_score(int64_t Q, int64_t n_pos, const int64_t* __restrict__ ctx,
                                                               int F, int field, const int64_t* __restrict__ keys,
                                                               const int64_t* __restrict__ pos_ptr,
                                                               const int64_t* __restrict__ pos_items, int64_t T, int d,
                                                               bool sp, int strat, uint64_t seed,
                                                               const float* __restrict__ uop,
                                                               const float* __restrict__ ucon, int Kp, int KA,
                                                               const float* __restrict__ ent,
                                                               const float* __restrict__ bias, float* __restrict__ raw,
                                                               int64_t* __restrict__ pusr) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pos) return;
  int64_t row;
  const int64_t q = pos_row_of(pos_ptr, Q, n_pos, p, row);
  pusr[p] = row;
  const int64_t iid = pos_items[p];
  float sc = __builtin_nanf("");
  if (iid >= 0 && iid < T && ctx_valid(ctx + q * F, F, field, T)) {
    if (strat == VFM_RANK_RANDOM) {
      sc = philox_uniform(seed, keys[q], iid);
    } else {
      float m, v;
      field_pair_moments(StoredOp{uop + q * Kp, KA, d}, ent + iid * 2 * d, bias + iid * 2, ucon[q * 2], ucon[q * 2 + 1], d,
                         sp, m, v);
      sc = score_of(strat, m, v);
    }
  }
  raw[p] = sc;
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
// The operand part of a workspace: both operand parts for every strategy (no candidate block for VFM_RANK_RANDOM: no
// tile runs) and the position keys.  Padding, tiles and the split count: op_layout_of.
struct FieldOps {
  int KA, KB, Kp, S, n_tiles;
  int64_t U_pad, C_pad, off_uop, off_iop, off_ucon, off_icon, off_key, end;
};

FieldOps field_ops_of(int64_t Q, int64_t n_cand, int d, int strategy, int n_splits) {
  const OpLayout B = op_layout_of(Q, n_cand, d, strategy, n_splits);
  FieldOps L;
  L.KA = (int)round_up(d, KS);
  L.KB = (int)round_up(3 * (int64_t)d, KS);
  L.Kp = L.KA + L.KB;
  L.S = B.S; L.n_tiles = B.n_tiles; L.U_pad = B.U_pad; L.C_pad = B.C_pad;
  const int64_t c_rows = strategy == VFM_RANK_RANDOM ? 0 : L.C_pad;
  L.off_uop = 0;
  L.off_iop = L.off_uop + round_up(L.U_pad * L.Kp * 4, 256);
  L.off_ucon = L.off_iop + round_up(c_rows * L.Kp * 4, 256);
  L.off_icon = L.off_ucon + round_up(L.U_pad * 2 * 4, 256);
  L.off_key = L.off_icon + round_up(c_rows * 2 * 4, 256);
  L.end = L.off_key + round_up(Q * 8, 256);
  return L;
}

// The ranking's workspace: the operands, then the split lists
struct FieldLayout : FieldOps, ListLayout {};

FieldLayout field_layout_of(int64_t Q, int64_t n_cand, int d, int k, int strategy, int n_splits) {
  FieldLayout L;
  static_cast<FieldOps&>(L) = field_ops_of(Q, n_cand, d, strategy, n_splits);
  static_cast<ListLayout&>(L) = list_layout_of(L.end, L.S, Q, k);
  return L;
}

// The evaluation's workspace: the operands, then the eval tail
struct FieldEvalLayout : FieldOps, EvalTail {};

FieldEvalLayout field_eval_layout_of(int64_t Q, int64_t n_cand, int64_t n_pos, int d, int strategy, int n_splits) {
  FieldEvalLayout L;
  static_cast<FieldOps&>(L) = field_ops_of(Q, n_cand, d, strategy, n_splits);
  static_cast<EvalTail&>(L) = eval_tail_of(L.end, L.S, Q, n_pos);
  return L;
}

// k_field_ctx_prep and k_field_cand_prep into the operand blocks of L.  VFM_RANK_RANDOM: no tile runs, so the candidates
// are never packed; the contexts only where their position keys are needed (ctx_rows false: the caller reads neither the
// packed rows nor, with keys of its own, the position keys).  post: NULL for the table form, else the queries'
// posterior rows of column post_field.
int launch_field_prep(const FieldOps& L, char* ws, int64_t Q, const int64_t* ctx, int F, int field, const int64_t* qkey,
                      int64_t n_cand, const int64_t* cand, int64_t cand_lo, int64_t T, int d, bool sp, int strategy,
                      bool ctx_rows, const float* ent, const float* bias, const float* scal, int post_field,
                      const float* post, hipStream_t st) {
  if (ctx_rows || !qkey) {
    const dim3 grid((unsigned)((L.U_pad + PREP_BLOCK / WAVE - 1) / (PREP_BLOCK / WAVE)));
    float *uop = (float*)(ws + L.off_uop), *ucon = (float*)(ws + L.off_ucon);
    int64_t* key_out = qkey ? (int64_t*)nullptr : (int64_t*)(ws + L.off_key);
    if (post)
      hipLaunchKernelGGL(k_field_ctx_prep<PostRows>, grid, dim3(PREP_BLOCK), 0, st, L.U_pad, Q, ctx, F, field, T, L.Kp,
                         L.KA, L.KB, d, sp, PostRows{ent, bias, post, post_field, d}, scal, uop, ucon, key_out);
    else
      hipLaunchKernelGGL(k_field_ctx_prep<TableRows>, grid, dim3(PREP_BLOCK), 0, st, L.U_pad, Q, ctx, F, field, T, L.Kp,
                         L.KA, L.KB, d, sp, TableRows{ent, bias}, scal, uop, ucon, key_out);
    if (int rc = launch_status("k_field_ctx_prep")) return rc;
  }
  const int64_t ni = L.C_pad * (L.Kp + 2);
  if (strategy != VFM_RANK_RANDOM && ni > 0) {
    hipLaunchKernelGGL(k_field_cand_prep, dim3((unsigned)((ni + 255) / 256)), dim3(256), 0, st, L.C_pad, n_cand, cand,
                       cand_lo, T, L.Kp, L.KA, d, sp, ent, bias, (float*)(ws + L.off_iop), (float*)(ws + L.off_icon));
    if (int rc = launch_status("k_field_cand_prep")) return rc;
  }
  return 0;
}

int check_fields(int32_t F, int32_t field) {
  if (F < 2 || F > VFM_MAX_FIELDS) return vfm::fail(VFM_E_INVALID, "F out of range [2,64]");
  if (field < 0 || field >= F) return vfm::fail(VFM_E_INVALID, "field out of range [0,F)");
  return 0;
}

// The posterior forms' own arguments: the supplied column is a context column
int check_post_field(int32_t F, int32_t field, int32_t post_field) {
  if (post_field < 0 || post_field >= F) return vfm::fail(VFM_E_INVALID, "post_field out of range [0,F)");
  if (post_field == field)
    return vfm::fail(VFM_E_INVALID, "post_field must differ from field: the posterior is a context column's");
  return 0;
}

template <typename ID, typename SRC>
void launch_field_moments(int64_t B, int F, int field, int d, int64_t T, bool sp, const void* x, SRC rows,
                          const float* scal, int strategy, uint64_t seed, const int64_t* qkey, float* m, float* v,
                          float* s, hipStream_t st) {
  hipLaunchKernelGGL((k_field_moments<ID, SRC>), dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, B, F, field, d, T,
                     sp, (const ID*)x, rows, scal, strategy, seed, qkey, m, v, s);
}

// vfm_field_moments_f32 (has_post false) and vfm_field_moments_post_f32
int field_moments_impl(int64_t B, int32_t F, int32_t d, int64_t T, int32_t id_bits, int32_t flags, const void* x,
                       int32_t field, bool has_post, int32_t post_field, const float* post, const float* entity_params,
                       const float* bias_params, const float* scalars, int32_t strategy, uint64_t seed,
                       const int64_t* qkey, float* logit_mean, float* logit_var, float* score, void* stream) {
  if (int rc = check_common(T, d, flags, strategy)) return rc;
  if (int rc = check_fields(F, field)) return rc;
  if (has_post)
    if (int rc = check_post_field(F, field, post_field)) return rc;
  if (B < 0) return vfm::fail(VFM_E_INVALID, "B < 0");
  if (id_bits != 32 && id_bits != 64) return vfm::fail(VFM_E_INVALID, "id_bits must be 32 or 64");
  if (B == 0) return 0;
  if (!x || !entity_params || !bias_params || !scalars || !logit_mean || !logit_var)
    return vfm::fail(VFM_E_INVALID, "null pointer");
  if (has_post && !post) return vfm::fail(VFM_E_INVALID, "null pointer: post");
  const hipStream_t st = (hipStream_t)stream;
  const bool sp = (flags & VFM_FLAG_LINK_SOFTPLUS) != 0;
  const TableRows tab{entity_params, bias_params};
  const PostRows pst{entity_params, bias_params, post, post_field, d};
  if (id_bits == 64) {
    if (has_post)
      launch_field_moments<int64_t>(B, F, field, d, T, sp, x, pst, scalars, strategy, seed, qkey, logit_mean, logit_var,
                                    score, st);
    else
      launch_field_moments<int64_t>(B, F, field, d, T, sp, x, tab, scalars, strategy, seed, qkey, logit_mean, logit_var,
                                    score, st);
  } else {
    if (has_post)
      launch_field_moments<int32_t>(B, F, field, d, T, sp, x, pst, scalars, strategy, seed, qkey, logit_mean, logit_var,
                                    score, st);
    else
      launch_field_moments<int32_t>(B, F, field, d, T, sp, x, tab, scalars, strategy, seed, qkey, logit_mean, logit_var,
                                    score, st);
  }
  return launch_status("k_field_moments");
}

// vfm_rank_field_f32 (has_post false) and vfm_rank_field_post_f32
int rank_field_impl(int64_t Q, const int64_t* ctx, int32_t field, bool has_post, int32_t post_field, const float* post,
                    const int64_t* qkey, int64_t n_cand, const int64_t* cand, int64_t cand_lo, int64_t T, int32_t F,
                    int32_t d, int32_t k, int32_t strategy, int32_t flags, uint64_t seed, int32_t n_splits,
                    const int64_t* excl_ptr, const int64_t* excl_items, int64_t n_excl, const float* entity_params,
                    const float* bias_params, const float* scalars, void* workspace, int64_t workspace_bytes,
                    int64_t* out_items, float* out_score, float* out_mean, float* out_var, void* stream) {
  if (int rc = check_common(T, d, flags, strategy)) return rc;
  if (int rc = check_fields(F, field)) return rc;
  if (has_post)
    if (int rc = check_post_field(F, field, post_field)) return rc;
  if (k < 1 || k > VFM_RANK_MAX_K) return vfm::fail(VFM_E_INVALID, "k out of range [1,128]");
  if (Q < 0) return vfm::fail(VFM_E_INVALID, "Q < 0");
  if (n_cand < 0 || n_cand >= ((int64_t)1 << 31)) return vfm::fail(VFM_E_INVALID, "n_cand out of range [0,2^31)");
  if (n_splits < 0 || n_splits > VFM_RANK_MAX_SPLITS) return vfm::fail(VFM_E_INVALID, "n_splits out of range [0,64]");
  if (!cand && (cand_lo < 0 || cand_lo + n_cand > T)) return vfm::fail(VFM_E_INVALID, "candidate range outside [0,T)");
  if (n_excl < 0 || (n_excl > 0 && (!excl_ptr || !excl_items)))
    return vfm::fail(VFM_E_INVALID, "exclusion lists: excl_ptr and excl_items together, n_excl >= 0");
  if (Q == 0) return 0;
  if (!ctx || !entity_params || !bias_params || !scalars || !workspace || !out_items || !out_score || !out_mean ||
      !out_var)
    return vfm::fail(VFM_E_INVALID, "null pointer");
  if (has_post && !post) return vfm::fail(VFM_E_INVALID, "null pointer: post");
  const FieldLayout L = field_layout_of(Q, n_cand, d, k, strategy, n_splits);
  if (workspace_bytes < L.bytes)
    return vfm::fail(VFM_E_INVALID, "workspace too small (vfm_rank_field_workspace_bytes)");
  if (((uintptr_t)workspace) & 255) return vfm::fail(VFM_E_INVALID, "workspace must be 256-byte aligned");

  const hipStream_t st = (hipStream_t)stream;
  const bool sp = (flags & VFM_FLAG_LINK_SOFTPLUS) != 0;
  char* ws = (char*)workspace;
  float *uop = (float*)(ws + L.off_uop), *iop = (float*)(ws + L.off_iop), *ucon = (float*)(ws + L.off_ucon),
        *icon = (float*)(ws + L.off_icon);
  int64_t* keys = (int64_t*)(ws + L.off_key);
  if (int rc = launch_field_prep(L, ws, Q, ctx, F, field, qkey, n_cand, cand, cand_lo, T, d, sp, strategy, true,
                                 entity_params, bias_params, scalars, post_field, has_post ? post : nullptr, st))
    return rc;
  vfm::RankScan a;
  a.U = Q; a.n_cand = n_cand; a.item_lo = cand_lo; a.n_excl = excl_ptr ? n_excl : 0;
  a.keys = qkey ? qkey : keys; a.cand = cand; a.excl_ptr = excl_ptr; a.excl_items = excl_items;
  a.uop = uop; a.iop = iop; a.ucon = ucon; a.icon = icon;
  a.Kp = L.Kp; a.KA = L.KA; a.KB = L.KB;
  a.ls = (float*)(ws + L.off_ls); a.lc = (int*)(ws + L.off_lc);
  a.k = k; a.n_tiles = L.n_tiles; a.S = L.S; a.seed = seed;
  if (int rc = vfm::launch_rank_scan(a, strategy, (unsigned)(L.U_pad / UT), st)) return rc;
  hipLaunchKernelGGL(k_rank_merge<FieldMoments>, dim3((unsigned)Q), dim3(MERGE_BLOCK), 0, st, Q, k, L.S, a.ls, a.lc, cand,
                     cand_lo, FieldMoments{uop, ucon, L.Kp, L.KA, T, d, sp, entity_params, bias_params}, out_items,
                     out_score, out_mean, out_var);
  return launch_status("k_rank_merge");
}

// vfm_rank_heldout_field_f32 (has_post false) and vfm_rank_heldout_field_post_f32
int rank_heldout_field_impl(int64_t Q, const int64_t* ctx, int32_t field, bool has_post, int32_t post_field,
                            const float* post, const int64_t* qkey, int64_t n_cand, const int64_t* cand, int64_t cand_lo,
                            int64_t T, int32_t F, int32_t d, int32_t strategy, int32_t flags, uint64_t seed,
                            int32_t n_splits, const int64_t* excl_ptr, const int64_t* excl_items, int64_t n_excl,
                            const int64_t* pos_ptr, const int64_t* pos_items, int64_t n_pos, const float* entity_params,
                            const float* bias_params, const float* scalars, void* workspace, int64_t workspace_bytes,
                            int64_t* out_rank, int64_t* out_rank_neg, int64_t* out_n_eligible, int64_t* out_n_neg,
                            void* stream) {
  if (int rc = check_common(T, d, flags, strategy)) return rc;
  if (int rc = check_fields(F, field)) return rc;
  if (has_post)
    if (int rc = check_post_field(F, field, post_field)) return rc;
  if (Q < 0) return vfm::fail(VFM_E_INVALID, "Q < 0");
  if (n_cand < 0 || n_cand >= ((int64_t)1 << 31)) return vfm::fail(VFM_E_INVALID, "n_cand out of range [0,2^31)");
  if (n_pos < 0 || n_pos >= ((int64_t)1 << 40)) return vfm::fail(VFM_E_INVALID, "n_pos out of range [0,2^40)");
  if (n_splits < 0 || n_splits > VFM_RANK_MAX_SPLITS) return vfm::fail(VFM_E_INVALID, "n_splits out of range [0,64]");
  if (!cand && (cand_lo < 0 || cand_lo + n_cand > T)) return vfm::fail(VFM_E_INVALID, "candidate range outside [0,T)");
  if (n_excl < 0 || (n_excl > 0 && (!excl_ptr || !excl_items)))
    return vfm::fail(VFM_E_INVALID, "exclusion lists: excl_ptr and excl_items together, n_excl >= 0");
  if (n_pos > 0 && !pos_items) return vfm::fail(VFM_E_INVALID, "null pointer: pos_items");
  if (Q == 0) return 0;
  if (!ctx || !pos_ptr || !entity_params || !bias_params || !scalars || !workspace || !out_n_eligible || !out_n_neg ||
      (n_pos > 0 && (!out_rank || !out_rank_neg)))
    return vfm::fail(VFM_E_INVALID, "null pointer");
  if (has_post && !post) return vfm::fail(VFM_E_INVALID, "null pointer: post");
  const FieldEvalLayout L = field_eval_layout_of(Q, n_cand, n_pos, d, strategy, n_splits);
  if (workspace_bytes < L.bytes)
    return vfm::fail(VFM_E_INVALID, "workspace too small (vfm_rank_eval_field_workspace_bytes)");
  if (((uintptr_t)workspace) & 255) return vfm::fail(VFM_E_INVALID, "workspace must be 256-byte aligned");

  const hipStream_t st = (hipStream_t)stream;
  const bool sp = (flags & VFM_FLAG_LINK_SOFTPLUS) != 0;
  char* ws = (char*)workspace;
  if (int rc = launch_field_prep(L, ws, Q, ctx, F, field, qkey, n_cand, cand, cand_lo, T, d, sp, strategy,
                                 strategy != VFM_RANK_RANDOM, entity_params, bias_params, scalars, post_field,
                                 has_post ? post : nullptr, st))
    return rc;
  vfm::RankEval a;
  a.U = Q; a.n_cand = n_cand; a.item_lo = cand_lo; a.n_excl = excl_ptr ? n_excl : 0; a.n_pos = n_pos;
  a.keys = qkey ? qkey : (const int64_t*)(ws + L.off_key); a.cand = cand; a.excl_ptr = excl_ptr;
  a.excl_items = excl_items; a.pos_ptr = pos_ptr; a.pos_items = pos_items;
  a.uop = (const float*)(ws + L.off_uop); a.iop = (const float*)(ws + L.off_iop);
  a.ucon = (const float*)(ws + L.off_ucon); a.icon = (const float*)(ws + L.off_icon);
  a.Kp = L.Kp; a.KA = L.KA; a.KB = L.KB;
  eval_tail_into(a, ws, L);
  a.n_tiles = L.n_tiles; a.S = L.S; a.seed = seed;
  a.out_rank = out_rank; a.out_rank_neg = out_rank_neg; a.out_n_eligible = out_n_eligible; a.out_n_neg = out_n_neg;
  if (n_pos > 0) {
    hipLaunchKernelGGL(k_field_pos_score, dim3((unsigned)((n_pos + POS_BLOCK - 1) / POS_BLOCK)), dim3(POS_BLOCK), 0, st,
                       Q, n_pos, ctx, (int)F, (int)field, a.keys, pos_ptr, pos_items, T, (int)d, sp, (int)strategy, seed,
                       a.uop, a.ucon, L.Kp, L.KA, entity_params, bias_params, (float*)(ws + L.off_raw),
                       (int64_t*)(ws + L.off_pusr));
    if (int rc = launch_status("k_field_pos_score")) return rc;
  }
  return vfm::launch_rank_eval(a, strategy, (unsigned)(L.U_pad / UT), st);
}

}  // namespace

extern "C" {

int vfm_field_moments_f32(int64_t B, int32_t F, int32_t d, int64_t T, int32_t id_bits, int32_t flags, const void* x,
                          int32_t field, const float* entity_params, const float* bias_params, const float* scalars,
                          int32_t strategy, uint64_t seed, const int64_t* qkey, float* logit_mean, float* logit_var,
                          float* score, void* stream) {
  return field_moments_impl(B, F, d, T, id_bits, flags, x, field, false, -1, nullptr, entity_params, bias_params,
                            scalars, strategy, seed, qkey, logit_mean, logit_var, score, stream);
}

int vfm_field_moments_post_f32(int64_t B, int32_t F, int32_t d, int64_t T, int32_t id_bits, int32_t flags, const void* x,
                               int32_t field, int32_t post_field, const float* post, const float* entity_params,
                               const float* bias_params, const float* scalars, int32_t strategy, uint64_t seed,
                               const int64_t* qkey, float* logit_mean, float* logit_var, float* score, void* stream) {
  return field_moments_impl(B, F, d, T, id_bits, flags, x, field, true, post_field, post, entity_params, bias_params,
                            scalars, strategy, seed, qkey, logit_mean, logit_var, score, stream);
}

int64_t vfm_rank_field_workspace_bytes(int64_t Q, int64_t n_cand, int32_t F, int32_t d, int32_t k, int32_t strategy,
                                       int32_t n_splits) {
  if (Q < 0 || n_cand < 0 || n_cand >= ((int64_t)1 << 31) || F < 2 || F > VFM_MAX_FIELDS || d < 1 || d > 4096 || k < 1 ||
      k > VFM_RANK_MAX_K || strategy < VFM_RANK_TOP || strategy > VFM_RANK_RANDOM || n_splits < 0 ||
      n_splits > VFM_RANK_MAX_SPLITS)
    return VFM_E_INVALID;
  return field_layout_of(Q, n_cand, d, k, strategy, n_splits).bytes;
}

int vfm_rank_field_f32(int64_t Q, const int64_t* ctx, int32_t field, const int64_t* qkey, int64_t n_cand,
                       const int64_t* cand, int64_t cand_lo, int64_t T, int32_t F, int32_t d, int32_t k,
                       int32_t strategy, int32_t flags, uint64_t seed, int32_t n_splits, const int64_t* excl_ptr,
                       const int64_t* excl_items, int64_t n_excl, const float* entity_params, const float* bias_params,
                       const float* scalars, void* workspace, int64_t workspace_bytes, int64_t* out_items,
                       float* out_score, float* out_mean, float* out_var, void* stream) {
  return rank_field_impl(Q, ctx, field, false, -1, nullptr, qkey, n_cand, cand, cand_lo, T, F, d, k, strategy, flags,
                         seed, n_splits, excl_ptr, excl_items, n_excl, entity_params, bias_params, scalars, workspace,
                         workspace_bytes, out_items, out_score, out_mean, out_var, stream);
}

int vfm_rank_field_post_f32(int64_t Q, const int64_t* ctx, int32_t field, int32_t post_field, const float* post,
                            const int64_t* qkey, int64_t n_cand, const int64_t* cand, int64_t cand_lo, int64_t T,
                            int32_t F, int32_t d, int32_t k, int32_t strategy, int32_t flags, uint64_t seed,
                            int32_t n_splits, const int64_t* excl_ptr, const int64_t* excl_items, int64_t n_excl,
                            const float* entity_params, const float* bias_params, const float* scalars, void* workspace,
                            int64_t workspace_bytes, int64_t* out_items, float* out_score, float* out_mean,
                            float* out_var, void* stream) {
  return rank_field_impl(Q, ctx, field, true, post_field, post, qkey, n_cand, cand, cand_lo, T, F, d, k, strategy, flags,
                         seed, n_splits, excl_ptr, excl_items, n_excl, entity_params, bias_params, scalars, workspace,
                         workspace_bytes, out_items, out_score, out_mean, out_var, stream);
}

int64_t vfm_rank_eval_field_workspace_bytes(int64_t Q, int64_t n_cand, int64_t n_pos, int32_t F, int32_t d,
                                            int32_t strategy, int32_t n_splits) {
  if (!eval_sizes_ok(Q, n_cand, n_pos) || F < 2 || F > VFM_MAX_FIELDS || d < 1 || d > 4096 ||
      strategy < VFM_RANK_TOP || strategy > VFM_RANK_RANDOM || n_splits < 0 || n_splits > VFM_RANK_MAX_SPLITS)
    return VFM_E_INVALID;
  return field_eval_layout_of(Q, n_cand, n_pos, d, strategy, n_splits).bytes;
}

int vfm_rank_heldout_field_f32(int64_t Q, const int64_t* ctx, int32_t field, const int64_t* qkey, int64_t n_cand,
                               const int64_t* cand, int64_t cand_lo, int64_t T, int32_t F, int32_t d, int32_t strategy,
                               int32_t flags, uint64_t seed, int32_t n_splits, const int64_t* excl_ptr,
                               const int64_t* excl_items, int64_t n_excl, const int64_t* pos_ptr,
                               const int64_t* pos_items, int64_t n_pos, const float* entity_params,
                               const float* bias_params, const float* scalars, void* workspace, int64_t workspace_bytes,
                               int64_t* out_rank, int64_t* out_rank_neg, int64_t* out_n_eligible, int64_t* out_n_neg,
                               void* stream) {
  return rank_heldout_field_impl(Q, ctx, field, false, -1, nullptr, qkey, n_cand, cand, cand_lo, T, F, d, strategy,
                                 flags, seed, n_splits, excl_ptr, excl_items, n_excl, pos_ptr, pos_items, n_pos,
                                 entity_params, bias_params, scalars, workspace, workspace_bytes, out_rank, out_rank_neg,
                                 out_n_eligible, out_n_neg, stream);
}

int vfm_rank_heldout_field_post_f32(int64_t Q, const int64_t* ctx, int32_t field, int32_t post_field, const float* post,
                                    const int64_t* qkey, int64_t n_cand, const int64_t* cand, int64_t cand_lo, int64_t T,
                                    int32_t F, int32_t d, int32_t strategy, int32_t flags, uint64_t seed,
                                    int32_t n_splits, const int64_t* excl_ptr, const int64_t* excl_items, int64_t n_excl,
                                    const int64_t* pos_ptr, const int64_t* pos_items, int64_t n_pos,
                                    const float* entity_params, const float* bias_params, const float* scalars,
                                    void* workspace, int64_t workspace_bytes, int64_t* out_rank, int64_t* out_rank_neg,
                                    int64_t* out_n_eligible, int64_t* out_n_neg, void* stream) {
  return rank_heldout_field_impl(Q, ctx, field, true, post_field, post, qkey, n_cand, cand, cand_lo, T, F, d, strategy,
                                 flags, seed, n_splits, excl_ptr, excl_items, n_excl, pos_ptr, pos_items, n_pos,
                                 entity_params, bias_params, scalars, workspace, workspace_bytes, out_rank, out_rank_neg,
                                 out_n_eligible, out_n_neg, stream);
}

}  // extern "C"

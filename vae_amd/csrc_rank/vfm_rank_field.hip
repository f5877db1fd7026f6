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
// packed rows nor, with keys of its own, the position keys).  The table form or, with r.has_post, the queries' posterior
// rows of column r.post_field.
int launch_field_prep(const FieldOps& L, const RankCall& r, bool ctx_rows) {
  char* ws = (char*)r.workspace;
  const bool sp = r.softplus();
  if (ctx_rows || !r.qkey) {
    const dim3 grid((unsigned)((L.U_pad + PREP_BLOCK / WAVE - 1) / (PREP_BLOCK / WAVE)));
    float *uop = (float*)(ws + L.off_uop), *ucon = (float*)(ws + L.off_ucon);
    int64_t* key_out = r.qkey ? (int64_t*)nullptr : (int64_t*)(ws + L.off_key);
    if (r.has_post)
      hipLaunchKernelGGL(k_field_ctx_prep<PostRows>, grid, dim3(PREP_BLOCK), 0, r.stream, L.U_pad, r.Q, r.queries,
                         (int)r.F, (int)r.field, r.T, L.Kp, L.KA, L.KB, (int)r.d, sp,
                         PostRows{r.ent, r.bias, r.post, r.post_field, r.d}, r.scal, uop, ucon, key_out);
    else
      hipLaunchKernelGGL(k_field_ctx_prep<TableRows>, grid, dim3(PREP_BLOCK), 0, r.stream, L.U_pad, r.Q, r.queries,
                         (int)r.F, (int)r.field, r.T, L.Kp, L.KA, L.KB, (int)r.d, sp, TableRows{r.ent, r.bias}, r.scal,
                         uop, ucon, key_out);
    if (int rc = launch_status("k_field_ctx_prep")) return rc;
  }
  const int64_t ni = L.C_pad * (L.Kp + 2);
  if (r.strategy != VFM_RANK_RANDOM && ni > 0) {
    hipLaunchKernelGGL(k_field_cand_prep, dim3((unsigned)((ni + 255) / 256)), dim3(256), 0, r.stream, L.C_pad, r.n_cand,
                       r.cand, r.cand_lo, r.T, L.Kp, L.KA, (int)r.d, sp, r.ent, r.bias, (float*)(ws + L.off_iop),
                       (float*)(ws + L.off_icon));
    if (int rc = launch_status("k_field_cand_prep")) return rc;
  }
  return 0;
}

// The field forms' own conditions: the ranked column and, for the posterior forms, the supplied one (a context column)
int check_fields(int32_t F, int32_t field, bool has_post, int32_t post_field) {
  if (F < 2 || F > VFM_MAX_FIELDS) return vfm::fail(VFM_E_INVALID, "F out of range [2,64]");
  if (field < 0 || field >= F) return vfm::fail(VFM_E_INVALID, "field out of range [0,F)");
  if (!has_post) return 0;
  if (post_field < 0 || post_field >= F) return vfm::fail(VFM_E_INVALID, "post_field out of range [0,F)");
  if (post_field == field)
    return vfm::fail(VFM_E_INVALID, "post_field must differ from field: the posterior is a context column's");
  return 0;
}

// One moments call as vfm_field_moments_f32 / vfm_field_moments_post_f32 received it
struct MomentsCall {
  int64_t B, T;
  int32_t F, d, id_bits, flags, field, post_field, strategy;
  bool has_post;
  const void* x;
  const float *post, *ent, *bias, *scal;
  uint64_t seed;
  const int64_t* qkey;
  float *mean, *var, *score;
  hipStream_t stream;
};

template <typename ID, typename SRC>
void launch_field_moments(const MomentsCall& c, SRC rows) {
  hipLaunchKernelGGL((k_field_moments<ID, SRC>), dim3((unsigned)((c.B + 255) / 256)), dim3(256), 0, c.stream, c.B,
                     (int)c.F, (int)c.field, (int)c.d, c.T, (c.flags & VFM_FLAG_LINK_SOFTPLUS) != 0, (const ID*)c.x, rows,
                     c.scal, (int)c.strategy, c.seed, c.qkey, c.mean, c.var, c.score);
}

int field_moments_call(const MomentsCall& c) {
  if (int rc = check_common(c.T, c.d, c.flags, c.strategy)) return rc;
  if (int rc = check_fields(c.F, c.field, c.has_post, c.post_field)) return rc;
  if (c.B < 0) return vfm::fail(VFM_E_INVALID, "B < 0");
  if (c.id_bits != 32 && c.id_bits != 64) return vfm::fail(VFM_E_INVALID, "id_bits must be 32 or 64");
  if (c.B == 0) return 0;
  if (!c.x || !c.ent || !c.bias || !c.scal || !c.mean || !c.var) return vfm::fail(VFM_E_INVALID, "null pointer");
  if (c.has_post && !c.post) return vfm::fail(VFM_E_INVALID, "null pointer: post");
  const TableRows tab{c.ent, c.bias};
  const PostRows pst{c.ent, c.bias, c.post, c.post_field, c.d};
  if (c.id_bits == 64) {
    if (c.has_post) launch_field_moments<int64_t>(c, pst);
    else launch_field_moments<int64_t>(c, tab);
  } else {
    if (c.has_post) launch_field_moments<int32_t>(c, pst);
    else launch_field_moments<int32_t>(c, tab);
  }
  return launch_status("k_field_moments");
}

// vfm_rank_field_f32 and vfm_rank_field_post_f32 (r.has_post)
int rank_field_call(const RankCall& r) {
  if (int rc = check_common(r.T, r.d, r.flags, r.strategy)) return rc;
  if (int rc = check_fields(r.F, r.field, r.has_post, r.post_field)) return rc;
  if (int rc = check_rank_call(r, RANK_ASK_TOPK | RANK_ASK_FIELD)) return rc;
  if (r.Q == 0) return 0;
  const FieldLayout L = field_layout_of(r.Q, r.n_cand, r.d, r.k, r.strategy, r.n_splits);
  if (int rc = check_rank_workspace(r, L.bytes, "workspace too small (vfm_rank_field_workspace_bytes)")) return rc;

  const char* ws = (const char*)r.workspace;
  if (int rc = launch_field_prep(L, r, true)) return rc;
  return scan_and_merge(r, L, r.qkey ? r.qkey : (const int64_t*)(ws + L.off_key),
                        FieldMoments{(const float*)(ws + L.off_uop), (const float*)(ws + L.off_ucon), L.Kp, L.KA, r.T, r.d,
                                     r.softplus(), r.ent, r.bias});
}

// vfm_rank_heldout_field_f32 and vfm_rank_heldout_field_post_f32 (r.has_post)
int rank_heldout_field_call(const RankCall& r) {
  if (int rc = check_common(r.T, r.d, r.flags, r.strategy)) return rc;
  if (int rc = check_fields(r.F, r.field, r.has_post, r.post_field)) return rc;
  if (int rc = check_rank_call(r, RANK_ASK_HELDOUT | RANK_ASK_FIELD)) return rc;
  if (r.Q == 0) return 0;
  const FieldEvalLayout L = field_eval_layout_of(r.Q, r.n_cand, r.n_pos, r.d, r.strategy, r.n_splits);
  if (int rc = check_rank_workspace(r, L.bytes, "workspace too small (vfm_rank_eval_field_workspace_bytes)")) return rc;

  char* ws = (char*)r.workspace;
  if (int rc = launch_field_prep(L, r, r.strategy != VFM_RANK_RANDOM)) return rc;
  const int64_t* keys = r.qkey ? r.qkey : (const int64_t*)(ws + L.off_key);
  if (r.n_pos > 0) {
    hipLaunchKernelGGL(k_field_pos_score, dim3((unsigned)((r.n_pos + POS_BLOCK - 1) / POS_BLOCK)), dim3(POS_BLOCK), 0,
                       r.stream, r.Q, r.n_pos, r.queries, (int)r.F, (int)r.field, keys, r.pos_ptr, r.pos_items, r.T,
                       (int)r.d, r.softplus(), (int)r.strategy, r.seed, (const float*)(ws + L.off_uop),
                       (const float*)(ws + L.off_ucon), L.Kp, L.KA, r.ent, r.bias, (float*)(ws + L.off_raw),
                       (int64_t*)(ws + L.off_pusr));
    if (int rc = launch_status("k_field_pos_score")) return rc;
  }
  return eval_after_scores(r, L, keys);
}

}  // namespace

extern "C" {

int vfm_field_moments_f32(int64_t B, int32_t F, int32_t d, int64_t T, int32_t id_bits, int32_t flags, const void* x,
                          int32_t field, const float* entity_params, const float* bias_params, const float* scalars,
                          int32_t strategy, uint64_t seed, const int64_t* qkey, float* logit_mean, float* logit_var,
                          float* score, void* stream) {
  return field_moments_call(MomentsCall{B, T, F, d, id_bits, flags, field, -1, strategy, false, x, nullptr,
                                        entity_params, bias_params, scalars, seed, qkey, logit_mean, logit_var, score,
                                        (hipStream_t)stream});
}

int vfm_field_moments_post_f32(int64_t B, int32_t F, int32_t d, int64_t T, int32_t id_bits, int32_t flags, const void* x,
                               int32_t field, int32_t post_field, const float* post, const float* entity_params,
                               const float* bias_params, const float* scalars, int32_t strategy, uint64_t seed,
                               const int64_t* qkey, float* logit_mean, float* logit_var, float* score, void* stream) {
  return field_moments_call(MomentsCall{B, T, F, d, id_bits, flags, field, post_field, strategy, true, x, post,
                                        entity_params, bias_params, scalars, seed, qkey, logit_mean, logit_var, score,
                                        (hipStream_t)stream});
}

int64_t vfm_rank_field_workspace_bytes(int64_t Q, int64_t n_cand, int32_t F, int32_t d, int32_t k, int32_t strategy,
                                       int32_t n_splits) {
  if (Q < 0 || n_cand < 0 || n_cand >= ((int64_t)1 << 31) || F < 2 || F > VFM_MAX_FIELDS || d < 1 || d > 4096 || k < 1 ||
      k > VFM_RANK_MAX_K || strategy < VFM_RANK_TOP || strategy > VFM_RANK_RANDOM || n_splits < 0 ||
      n_splits > VFM_RANK_MAX_SPLITS)
    return VFM_E_INVALID;
  return field_layout_of(Q, n_cand, d, k, strategy, n_splits).bytes;
}

int vfm_rank_field_post_f32(int64_t Q, const int64_t* ctx, int32_t field, int32_t post_field, const float* post,
                            const int64_t* qkey, int64_t n_cand, const int64_t* cand, int64_t cand_lo, int64_t T,
                            int32_t F, int32_t d, int32_t k, int32_t strategy, int32_t flags, uint64_t seed,
                            int32_t n_splits, const int64_t* excl_ptr, const int64_t* excl_items, int64_t n_excl,
                            const float* entity_params, const float* bias_params, const float* scalars, void* workspace,
                            int64_t workspace_bytes, int64_t* out_items, float* out_score, float* out_mean,
                            float* out_var, void* stream) {
  RankCall r;
  r.Q = Q; r.queries = ctx; r.qkey = qkey; r.field = field;
  r.has_post = true; r.post_field = post_field; r.post = post;
  r.n_cand = n_cand; r.cand = cand; r.cand_lo = cand_lo;
  r.excl_ptr = excl_ptr; r.excl_items = excl_items; r.n_excl = n_excl;
  r.T = T; r.F = F; r.d = d; r.ent = entity_params; r.bias = bias_params; r.scal = scalars;
  r.workspace = workspace; r.workspace_bytes = workspace_bytes;
  r.k = k; r.strategy = strategy; r.flags = flags; r.n_splits = n_splits; r.seed = seed;
  r.out_items = out_items; r.out_score = out_score; r.out_mean = out_mean; r.out_var = out_var;
  r.stream = (hipStream_t)stream;
  return rank_field_call(r);
}

int vfm_rank_field_f32(int64_t Q, const int64_t* ctx, int32_t field, const int64_t* qkey, int64_t n_cand,
                       const int64_t* cand, int64_t cand_lo, int64_t T, int32_t F, int32_t d, int32_t k,
                       int32_t strategy, int32_t flags, uint64_t seed, int32_t n_splits, const int64_t* excl_ptr,
                       const int64_t* excl_items, int64_t n_excl, const float* entity_params, const float* bias_params,
                       const float* scalars, void* workspace, int64_t workspace_bytes, int64_t* out_items,
                       float* out_score, float* out_mean, float* out_var, void* stream) {
  RankCall r;
  r.Q = Q; r.queries = ctx; r.qkey = qkey; r.field = field;
  r.n_cand = n_cand; r.cand = cand; r.cand_lo = cand_lo;
  r.excl_ptr = excl_ptr; r.excl_items = excl_items; r.n_excl = n_excl;
  r.T = T; r.F = F; r.d = d; r.ent = entity_params; r.bias = bias_params; r.scal = scalars;
  r.workspace = workspace; r.workspace_bytes = workspace_bytes;
  r.k = k; r.strategy = strategy; r.flags = flags; r.n_splits = n_splits; r.seed = seed;
  r.out_items = out_items; r.out_score = out_score; r.out_mean = out_mean; r.out_var = out_var;
  r.stream = (hipStream_t)stream;
  return rank_field_call(r);
}

int64_t vfm_rank_eval_field_workspace_bytes(int64_t Q, int64_t n_cand, int64_t n_pos, int32_t F, int32_t d,
                                            int32_t strategy, int32_t n_splits) {
  if (!eval_sizes_ok(Q, n_cand, n_pos) || F < 2 || F > VFM_MAX_FIELDS || d < 1 || d > 4096 ||
      strategy < VFM_RANK_TOP || strategy > VFM_RANK_RANDOM || n_splits < 0 || n_splits > VFM_RANK_MAX_SPLITS)
    return VFM_E_INVALID;
  return field_eval_layout_of(Q, n_cand, n_pos, d, strategy, n_splits).bytes;
}

int vfm_rank_heldout_field_post_f32(int64_t Q, const int64_t* ctx, int32_t field, int32_t post_field, const float* post,
                                    const int64_t* qkey, int64_t n_cand, const int64_t* cand, int64_t cand_lo, int64_t T,
                                    int32_t F, int32_t d, int32_t strategy, int32_t flags, uint64_t seed,
                                    int32_t n_splits, const int64_t* excl_ptr, const int64_t* excl_items, int64_t n_excl,
                                    const int64_t* pos_ptr, const int64_t* pos_items, int64_t n_pos,
                                    const float* entity_params, const float* bias_params, const float* scalars,
                                    void* workspace, int64_t workspace_bytes, int64_t* out_rank, int64_t* out_rank_neg,
                                    int64_t* out_n_eligible, int64_t* out_n_neg, void* stream) {
  RankCall r;
  r.Q = Q; r.queries = ctx; r.qkey = qkey; r.field = field;
  r.has_post = true; r.post_field = post_field; r.post = post;
  r.n_cand = n_cand; r.cand = cand; r.cand_lo = cand_lo;
  r.excl_ptr = excl_ptr; r.excl_items = excl_items; r.n_excl = n_excl;
  r.pos_ptr = pos_ptr; r.pos_items = pos_items; r.n_pos = n_pos;
  r.T = T; r.F = F; r.d = d; r.ent = entity_params; r.bias = bias_params; r.scal = scalars;
  r.workspace = workspace; r.workspace_bytes = workspace_bytes;
  r.strategy = strategy; r.flags = flags; r.n_splits = n_splits; r.seed = seed;
  r.out_rank = out_rank; r.out_rank_neg = out_rank_neg; r.out_n_eligible = out_n_eligible; r.out_n_neg = out_n_neg;
  r.stream = (hipStream_t)stream;
  return rank_heldout_field_call(r);
}

int vfm_rank_heldout_field_f32(int64_t Q, const int64_t* ctx, int32_t field, const int64_t* qkey, int64_t n_cand,
                               const int64_t* cand, int64_t cand_lo, int64_t T, int32_t F, int32_t d, int32_t strategy,
                               int32_t flags, uint64_t seed, int32_t n_splits, const int64_t* excl_ptr,
                               const int64_t* excl_items, int64_t n_excl, const int64_t* pos_ptr,
                               const int64_t* pos_items, int64_t n_pos, const float* entity_params,
                               const float* bias_params, const float* scalars, void* workspace, int64_t workspace_bytes,
                               int64_t* out_rank, int64_t* out_rank_neg, int64_t* out_n_eligible, int64_t* out_n_neg,
                               void* stream) {
  RankCall r;
  r.Q = Q; r.queries = ctx; r.qkey = qkey; r.field = field;
  r.n_cand = n_cand; r.cand = cand; r.cand_lo = cand_lo;
  r.excl_ptr = excl_ptr; r.excl_items = excl_items; r.n_excl = n_excl;
  r.pos_ptr = pos_ptr; r.pos_items = pos_items; r.n_pos = n_pos;
  r.T = T; r.F = F; r.d = d; r.ent = entity_params; r.bias = bias_params; r.scal = scalars;
  r.workspace = workspace; r.workspace_bytes = workspace_bytes;
  r.strategy = strategy; r.flags = flags; r.n_splits = n_splits; r.seed = seed;
  r.out_rank = out_rank; r.out_rank_neg = out_rank_neg; r.out_n_eligible = out_n_eligible; r.out_n_neg = out_n_neg;
  r.stream = (hipStream_t)stream;
  return rank_heldout_field_call(r);
}

}  // extern "C"

// vfm_elicit_field_score.hpp -- what the field-form sessions share on the device: the score's operand pass over the
// distinct contexts (k_elicit_ctx_prep), the kernel arguments, the fold rows of a respondent and the two operand views
// of a score (a context's row of the score table, the respondent's candidate operands in LDS).  Used by
// vfm_elicit_field.hip (the Adam session) and vfm_elicit_exact_body.hpp (the exact sessions: vfm_elicit_solve.hip and,
// for out_mean / out_var, vfm_elicit_design.hip), so a score is the same bits in all.  Included inside `namespace vfm { namespace {` of a unit, after vfm_foldin_body.hpp; the unit includes
// vfm_rank_tile.hpp and vfm_field_ctx.hpp at file scope first.
#pragma once

constexpr int WAVE = 64;

// ---------------------------------------------------------------------------------------------------------------------
// k_elicit_ctx_prep: a wave per context row of op_x, lanes over coordinates.  sop [n_ops, 4 d] = [M | A | A + M^2 | C],
// soc [n_ops, 2] = (c_mean, c_var) -- the coordinates' E P and Var P added in k order: an ordered sum over the lanes of
// each chunk of 64, as k_field_ctx_prep and k_field_moments add them.  A context id outside [0, T): a NaN row.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FB) void k_elicit_ctx_prep(int64_t n_ops, const int64_t* __restrict__ opx, int F, int field,
                                                        int64_t T, int d, bool sp, const float* __restrict__ ent,
                                                        const float* __restrict__ bias, const float* __restrict__ scal,
                                                        float* __restrict__ sop, float* __restrict__ soc) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t r = (int64_t)blockIdx.x * (FB / WAVE) + (threadIdx.x >> 6);
  if (r >= n_ops) return;                                   // (wave-uniform)
  float* row = sop + r * 4 * (int64_t)d;
  const int64_t* xr = opx + r * F;
  if (!ctx_valid(xr, F, field, T)) {
    for (int k = lane; k < 4 * d; k += WAVE) row[k] = __builtin_nanf("");
    if (lane < 2) soc[r * 2 + lane] = __builtin_nanf("");
    return;
  }
  double cm, cv;
  ctx_consts(xr, F, field, sp, bias, scal, cm, cv);
  for (int k0 = 0; k0 < d; k0 += WAVE) {
    const int k = k0 + lane;
    CtxCoord cc = {0., 0., 0., 0., 0.};
    if (k < d) {
      cc = ctx_coord(xr, F, field, k, d, sp, ent);
      row[k] = (float)cc.M;
      row[d + k] = ctx_op_var(cc, 0);
      row[2 * d + k] = ctx_op_var(cc, 1);
      row[3 * d + k] = ctx_op_var(cc, 2);
    }
    const int n = min(WAVE, d - k0);
    for (int j = 0; j < n; ++j) {
      cm += __shfl(cc.ep, j);
      cv += __shfl(cc.vp, j);
    }
  }
  if (lane == 0) {
    soc[r * 2] = (float)cm;
    soc[r * 2 + 1] = (float)cv;
  }
}

struct ElicitFieldArgs {
  FoldArgs f;                            // the fold-in's options, tables and operands (its row list is unused)
  int64_t U, P, H, n_ops;
  int32_t Q, strat, write, key_col;
  uint64_t seed;
  const int64_t *ents, *pool_ptr, *pool_x, *hist_ptr, *hist_x, *pool_op, *hist_op;
  const float *pool_y, *hist_y;
  const float *sop, *soc;                // the score's operands [n_ops, 4 d], [n_ops, 2]
  int64_t* out_row;
  float *out_score, *out_loss, *out_theta, *out_mean, *out_var;
  uint8_t* asked;                        // [P] workspace
};

// the fold rows of one respondent: the history slice in its order, then the asked pool rows in the order asked
struct FieldSessionRows {
  const ElicitFieldArgs& a;
  int64_t h0, nh;
  const int64_t* asked;                  // the respondent's row of out_row
  __device__ __forceinline__ int64_t op(int64_t i) const { return i < nh ? a.hist_op[h0 + i] : a.pool_op[asked[i - nh]]; }
  __device__ __forceinline__ float y(int64_t i) const { return i < nh ? a.hist_y[h0 + i] : a.pool_y[asked[i - nh]]; }
  __device__ __forceinline__ int64_t partner(int64_t i, int f) const {       // column f of the row
    return i < nh ? a.hist_x[(h0 + i) * a.f.F + f] : a.pool_x[asked[i - nh] * a.f.F + f];
  }
};

// A context's operands read from its row of the score table
struct CtxRowOp {
  const float* row;
  int d;
  __device__ __forceinline__ float mean_op(int k) const { return row[k]; }
  __device__ __forceinline__ float var_op(int part, int k) const { return row[(part + 1) * d + k]; }
};

// The respondent as the candidate: its operands [mu | mu^2 | sigma^2 | mu_w, sigma_w^2] from the group's LDS copy
struct ThetaCand {
  const float* uth;
  int DP;
  __device__ __forceinline__ float mean_op(int k) const { return uth[k]; }
  __device__ __forceinline__ float var_op(int part, int k) const { return part == 2 ? uth[k] : uth[(part + 1) * DP + k]; }
  __device__ __forceinline__ float mu_w() const { return uth[3 * DP]; }
  __device__ __forceinline__ float var_w() const { return uth[3 * DP + 1]; }
};

// mu^2 and sigma^2 of a coordinate as the ranking forms them (cand_op_var: the ranking side's link, products rounded)
__device__ __forceinline__ void theta_cand_ops(float m, float s, bool sp, float& m2, float& s2) {
#pragma clang fp contract(off)
  const float sg = link_of(s, sp);
  m2 = m * m;
  s2 = sg * sg;
}

inline int64_t sop_bytes(int64_t n_ops, int d) { return round_up(n_ops * 4 * (int64_t)d * 4, 256); }
inline int64_t soc_bytes(int64_t n_ops) { return round_up(n_ops * 2 * 4, 256); }

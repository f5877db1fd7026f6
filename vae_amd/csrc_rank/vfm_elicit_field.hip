// vfm_elicit_field.hip -- elicitation sessions in the field form (include/vfm_elicit.h: vfm_elicit_field_f32): ask,
// fold in and ask again for the entities of one column of a model with any number of fields, every round of every
// respondent in one launch.  A unit of its own beside vfm_elicit.hip (the two-field session, untouched) so that the two
// families of 28 instances compile side by side.
//
// k_elicit_ctx_prep: the score's operand of every distinct context of pool and history, once -- a wave per context,
//   lanes over coordinates (k_field_ctx_prep's arithmetic from vfm_field_ctx.hpp): [M | A | A + M^2 | C] and
//   (c_mean, c_var), the bits vfm_field_moments_f32 forms on the fly.
// k_foldin_prep (closed form only, vfm_foldin_body.hpp): the fold-in's operand [M | A | C], c_mean, c_var of the same
//   contexts.  The two tables are kept apart: they are two definitions (rank-field rounding, contraction off; the
//   fold-in's own sums, contraction on) and nothing shows that they agree in every bit.
// k_elicit_field: k_elicit's layout.  A group of W lanes per respondent (W, CPL by d as shape_of picks them; lane l owns
//   coordinates j W + l); theta_e stays in registers over all rounds, the Adam moments over a round; the fold rows
//   (history, then the asked rows) are staged in LDS while they fit and streamed from the operand table past that; an
//   asked row is APPENDED to the closed form's row sums.  Scoring: lane l scores the pool rows l, l + W, .. whole, one
//   serial k-ordered chain each, from the row's context operand and a per-group LDS copy of the candidate operands of
//   theta_e, [mu | mu^2 | sigma^2 | mu_w, sigma_w^2], refreshed once per round (the link is evaluated d times per round,
//   not d times per pool row); the best (score, position) is reduced over the group by a butterfly of a total order.  The
//   asked flags live in the workspace, the asked order in out_row; both are written by lane 0 and read by the group
//   after a barrier.  No atomics.
//
// Rounding: the rank expressions (vfm_field_ctx.hpp, score_of) pin fp contraction off, the fold-in body
// (vfm_foldin_body.hpp) pins it on, each with a pragma at the top of its body.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "vfm_args.hpp"
#include "vfm_elicit.h"
#include "vfm_rank_tile.hpp"         // score_of, philox_uniform, link_of
#include "vfm_field_ctx.hpp"         // ctx_coord, ctx_op_var, ctx_consts, ctx_valid, field_chain_moments

namespace vfm {
namespace {
#include "vfm_rng.hpp"
#include "vfm_common.hpp"
#include "vfm_foldin_body.hpp"       // FoldArgs, k_foldin_prep, fold_stage_rows, fold_run: k_foldin's body

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

template <int W, int CPL, int LINK, bool SAMPLED>
__global__ __launch_bounds__(FB) void k_elicit_field(const ElicitFieldArgs a) {
  extern __shared__ float lds[];
  constexpr int GPB = FB / W, DP = W * CPL;
  constexpr bool SP = LINK == LINK_SOFTPLUS;
  const FoldArgs& f = a.f;
  const int tid = threadIdx.x, l = tid % W, grp = tid / W;
  const int64_t g = (int64_t)blockIdx.x * GPB + grp;
  const bool live = g < a.U;
  int64_t p0 = 0, np = 0, h0 = 0, nh = 0, e = -1;
  if (live) {
    p0 = min(max(a.pool_ptr[g], (int64_t)0), a.P);
    np = min(max(a.pool_ptr[g + 1], p0), a.P) - p0;
    if (a.hist_ptr) {
      h0 = min(max(a.hist_ptr[g], (int64_t)0), a.H);
      nh = min(max(a.hist_ptr[g + 1], h0), a.H) - h0;
    }
    e = a.ents[g];
  }
  const bool eok = live && e >= 0 && e < f.T;
  const int d = f.d, Q = a.Q, F = f.F;
  const float prec = f.lik == VFM_LIK_NORMAL ? link_f<LINK>(f.scal[0]) : 0.f;
  const float m0 = f.scal[1], sg0 = link_f<LINK>(f.scal[2]);
  const FieldSessionRows rows{a, h0, nh, a.out_row + g * Q};

  // ---- theta_e (coordinates past d: mu = 0, s = prior, never updated)
  float mu[CPL], sp[CPL];
  bool vk[CPL];
#pragma unroll
  for (int j = 0; j < CPL; ++j) {
    const int kc = j * W + l;
    vk[j] = kc < d;
    mu[j] = 0.f;
    sp[j] = prior_s<LINK>();
    if (vk[j] && eok && !f.reset) {
      mu[j] = f.entity[e * 2 * d + kc];
      sp[j] = f.entity[e * 2 * d + d + kc];
    }
  }
  float muw = 0.f, spw = prior_s<LINK>();
  if (eok && !f.reset) { muw = f.bias[e * 2]; spw = f.bias[e * 2 + 1]; }

  // ---- LDS of the group: the fold stage (Ms [cap, DP], Cy [cap]) and theta_e's candidate operands (uth [3 DP + 2])
  float* Ms = lds + (int64_t)grp * ((int64_t)f.cap * (DP + 1) + 3 * DP + 2);
  float* Cy = Ms + (int64_t)f.cap * DP;
  float* uth = Cy + f.cap;

  for (int64_t p = l; p < np; p += W) a.asked[p0 + p] = 0;
  float SA[CPL], SB[CPL], SC[CPL];
  float Scv = 0.f;
#pragma unroll
  for (int j = 0; j < CPL; ++j) SA[j] = SB[j] = SC[j] = 0.f;
  if constexpr (!SAMPLED) {
    if (eok) fold_stage_rows<W, CPL>(f, rows, 0, nh, l, Ms, Cy, SA, SB, SC, Scv);
  }
  int64_t n = nh;

  // every thread of the block runs every round's barriers; a respondent with nothing left to ask skips the work
  // between them
  for (int q = 0; q <= Q; ++q) {
#pragma unroll
    for (int j = 0; j < CPL; ++j)
      if (vk[j]) {
        float m2, s2;
        theta_cand_ops(mu[j], sp[j], SP, m2, s2);
        uth[j * W + l] = mu[j]; uth[DP + j * W + l] = m2; uth[2 * DP + j * W + l] = s2;
      }
    if (l == 0) {
      float m2, s2;
      theta_cand_ops(muw, spw, SP, m2, s2);
      uth[3 * DP] = muw; uth[3 * DP + 1] = s2;
    }
    __syncthreads();                     // (theta_e, the asked flags and the stage are read across the group's lanes)
    if (q == Q && !a.out_mean) break;

    // ---- score: lane l takes the pool rows l, l + W, ..; its best by (score, position)
    float bs = 0.f;
    int64_t bp = -1;
    for (int64_t p = l; p < np; p += W) {
      const bool was = a.asked[p0 + p] != 0;
      if (was && !a.out_mean) continue;
      const int64_t* xr = a.pool_x + (p0 + p) * F;
      const int64_t o = a.pool_op[p0 + p];
      float mean = __builtin_nanf(""), var = __builtin_nanf(""), sc = __builtin_nanf("");
      if (eok && o >= 0 && o < a.n_ops && ctx_valid(xr, F, f.col, f.T)) {
        if (a.strat != VFM_RANK_RANDOM || a.out_mean)
          field_chain_moments(CtxRowOp{a.sop + o * 4 * (int64_t)d, d}, ThetaCand{uth, DP}, a.soc[o * 2], a.soc[o * 2 + 1],
                              d, mean, var);
        sc = a.strat == VFM_RANK_RANDOM ? philox_uniform(a.seed + (uint64_t)q, xr[a.key_col], e)
                                        : score_of(a.strat, mean, var);
      }
      if (a.out_mean) {
        a.out_mean[(int64_t)q * a.P + p0 + p] = mean;
        a.out_var[(int64_t)q * a.P + p0 + p] = var;
      }
      if (!was && sc == sc && (bp < 0 || sc > bs)) { bs = sc; bp = p; }
    }
    if (q == Q) break;

    // ---- choose: a butterfly over the group in the total order (score descending, position ascending)
#pragma unroll
    for (int off = W / 2; off >= 1; off >>= 1) {
      const float os = __shfl_xor(bs, off, W);
      const long long op = __shfl_xor((long long)bp, off, W);
      if (op >= 0 && (bp < 0 || os > bs || (os == bs && op < bp))) { bs = os; bp = op; }
    }
    const bool act = eok && bp >= 0;
    if (live && l == 0) {
      a.out_row[g * Q + q] = act ? p0 + bp : -1;
      a.out_score[g * Q + q] = act ? bs : __builtin_nanf("");
      if (act) a.asked[p0 + bp] = 1;
    }
    __syncthreads();                     // (out_row: the asked row is fold row n from here on)

    // ---- fold in: the asked row appended to the sums and the stage, then the fold-in's own body
    if constexpr (!SAMPLED) {
      if (act) fold_stage_rows<W, CPL>(f, rows, n, n + 1, l, Ms, Cy, SA, SB, SC, Scv);
      __syncthreads();
    }
    if (act) {
      ++n;
      fold_run<W, CPL, LINK, SAMPLED>(
          f, rows, n, e, f.t0 + (int64_t)q * ((int64_t)f.n_steps + 1), l, Ms, Cy, prec, m0, sg0, mu, sp, vk, muw, spw,
          SA, SB, SC, Scv, [&](float loss, const float (&)[CPL], const float (&)[CPL], float, float) {
            if (l == 0) a.out_loss[g * Q + q] = loss;
          });
    } else if (live && l == 0) {
      a.out_loss[g * Q + q] = __builtin_nanf("");
    }
    if (live && a.out_theta) {
      float* to = a.out_theta + (g * Q + q) * (2 * (int64_t)d + 2);
#pragma unroll
      for (int j = 0; j < CPL; ++j)
        if (vk[j]) { to[j * W + l] = mu[j]; to[d + j * W + l] = sp[j]; }
      if (l == 0) { to[2 * d] = muw; to[2 * d + 1] = spw; }
    }
  }

  if (eok && a.write) {
#pragma unroll
    for (int j = 0; j < CPL; ++j)
      if (vk[j]) { f.entity[e * 2 * d + j * W + l] = mu[j]; f.entity[e * 2 * d + d + j * W + l] = sp[j]; }
    if (l == 0) { f.bias[e * 2] = muw; f.bias[e * 2 + 1] = spw; }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
// fold rows per respondent staged in LDS: what the block's stage leaves after every group's copy of theta_e's operands
int lds_cap(const FShape& s) {
  const int DP = s.W * s.CPL, per_group = LDS_BYTES / 4 / (FB / s.W);
  const int c = (per_group - (3 * DP + 2)) / (DP + 1);
  return c < 0 ? 0 : c;
}

template <int W, int CPL, int LINK, bool SAMPLED>
void launch(const ElicitFieldArgs& a, hipStream_t st) {
  constexpr int GPB = FB / W, DP = W * CPL;
  const size_t shm = (size_t)GPB * ((size_t)a.f.cap * (DP + 1) + 3 * DP + 2) * 4;
  hipLaunchKernelGGL((k_elicit_field<W, CPL, LINK, SAMPLED>), dim3((unsigned)((a.U + GPB - 1) / GPB)), dim3(FB), shm, st,
                     a);
}

template <int LINK, bool SAMPLED>
void launch_shape(const FShape& s, const ElicitFieldArgs& a, hipStream_t st) {
  switch (s.W * 16 + s.CPL) {
    case 8 * 16 + 1: launch<8, 1, LINK, SAMPLED>(a, st); break;
    case 16 * 16 + 1: launch<16, 1, LINK, SAMPLED>(a, st); break;
    case 32 * 16 + 1: launch<32, 1, LINK, SAMPLED>(a, st); break;
    case 64 * 16 + 1: launch<64, 1, LINK, SAMPLED>(a, st); break;
    case 64 * 16 + 2: launch<64, 2, LINK, SAMPLED>(a, st); break;
    case 64 * 16 + 4: launch<64, 4, LINK, SAMPLED>(a, st); break;
    default: launch<64, 8, LINK, SAMPLED>(a, st); break;
  }
}

int64_t flags_bytes(int64_t P) { return round_up(P > 0 ? P : 1, 256); }
int64_t sop_bytes(int64_t n_ops, int d) { return round_up(n_ops * 4 * (int64_t)d * 4, 256); }
int64_t soc_bytes(int64_t n_ops) { return round_up(n_ops * 2 * 4, 256); }

}  // namespace
}  // namespace vfm

extern "C" {

int64_t vfm_elicit_field_workspace_bytes(int64_t P, int64_t n_ops, int32_t d, int32_t objective) {
  if (P < 0 || n_ops < 0 || d < 1 || d > VFM_FOLDIN_MAX_D ||
      (objective != VFM_OBJ_CLOSED_FORM && objective != VFM_OBJ_SAMPLED))
    return VFM_E_INVALID;
  int64_t b = vfm::flags_bytes(P) + vfm::sop_bytes(n_ops, d) + vfm::soc_bytes(n_ops);
  if (objective == VFM_OBJ_CLOSED_FORM) b += vfm::ops_off_opc(n_ops, d) + vfm::round_up(n_ops * 2 * 4, 256);
  return b;
}

int vfm_elicit_field_f32(const vfm_elicit_field_t* p, void* stream) {
  using vfm::fail;
  if (!p) return fail(VFM_E_INVALID, "vfm_elicit_field_f32: NULL argument struct");
  if (p->struct_size != (uint32_t)sizeof(vfm_elicit_field_t) || p->abi_version != (uint32_t)VFM_ABI_VERSION)
    return fail(VFM_E_INVALID,
                "vfm_elicit_field_t: struct_size / abi_version differ from this library's (VFM_STRUCT_INIT)");
  if (p->T < 1) return fail(VFM_E_INVALID, "T < 1");
  if (p->F < 2 || p->F > VFM_MAX_FIELDS) return fail(VFM_E_INVALID, "F out of range [2,64]");
  if (p->field < 0 || p->field >= p->F) return fail(VFM_E_INVALID, "field out of range [0,F)");
  if (p->key_col < 0 || p->key_col >= p->F || p->key_col == p->field)
    return fail(VFM_E_INVALID, "key_col must be a context column: in [0,F) and not field");
  if (p->d < 1 || p->d > VFM_FOLDIN_MAX_D) return fail(VFM_E_INVALID, "d out of range [1,512]");
  if (p->U < 0 || p->P < 0 || p->H < 0) return fail(VFM_E_INVALID, "U < 0, P < 0 or H < 0");
  if (p->n_rounds < 0 || p->n_rounds > VFM_ELICIT_MAX_ROUNDS) return fail(VFM_E_INVALID, "n_rounds out of range [0,4096]");
  if (p->strategy < VFM_RANK_TOP || p->strategy > VFM_RANK_RANDOM) return fail(VFM_E_INVALID, "unknown strategy");
  if (p->likelihood != VFM_LIK_NORMAL && p->likelihood != VFM_LIK_BERNOULLI)
    return fail(VFM_E_INVALID, "unknown likelihood");
  if (p->objective == VFM_OBJ_CLOSED_FORM) {
    if (p->likelihood != VFM_LIK_NORMAL) return fail(VFM_E_INVALID, "the closed form needs the Normal likelihood");
  } else if (p->objective == VFM_OBJ_SAMPLED) {
    if (p->n_samples < 1 || p->n_samples > VFM_FOLDIN_MAX_SAMPLES)
      return fail(VFM_E_INVALID, "n_samples out of range [1,4]");
  } else {
    return fail(VFM_E_INVALID, "unknown objective");
  }
  if (p->n_ops < 0 || (p->P + p->H > 0 && p->n_ops < 1)) return fail(VFM_E_INVALID, "n_ops out of range");
  if (p->flags & ~VFM_FLAG_LINK_SOFTPLUS) return fail(VFM_E_INVALID, "flags: only VFM_FLAG_LINK_SOFTPLUS is accepted");
  if (p->n_steps < 0) return fail(VFM_E_INVALID, "n_steps must be >= 0");
  if (p->t0 < 0 || p->t0 + (int64_t)(p->n_rounds + 1) * ((int64_t)p->n_steps + 1) >=
                       ((int64_t)1 << 60) / VFM_FOLDIN_MAX_SAMPLES)
    return fail(VFM_E_INVALID, "t0 out of range");
  if (!(p->lr >= 0.f) || !(p->kl_weight >= 0.f)) return fail(VFM_E_INVALID, "lr and kl_weight must be >= 0");
  if ((p->out_mean == nullptr) != (p->out_var == nullptr))
    return fail(VFM_E_INVALID, "out_mean and out_var: both or neither");
  if (p->U == 0) return 0;
  if (!p->entities || !p->pool_ptr || !p->entity_params || !p->bias_params || !p->scalars ||
      (p->P > 0 && (!p->pool_x || !p->pool_y)) || (p->H > 0 && (!p->hist_ptr || !p->hist_x || !p->hist_y)) ||
      (p->n_rounds > 0 && (!p->out_row || !p->out_score || !p->out_loss)))
    return fail(VFM_E_INVALID, "null pointer");
  if ((p->P + p->H > 0 && !p->op_x) || (p->P > 0 && !p->pool_op) || (p->H > 0 && !p->hist_op))
    return fail(VFM_E_INVALID, "op_x, pool_op and hist_op needed");
  const bool cf = p->objective == VFM_OBJ_CLOSED_FORM;
  const int64_t n_ops = p->n_ops;
  const int64_t ws = vfm_elicit_field_workspace_bytes(p->P, n_ops, p->d, p->objective);
  if (ws < 0 || p->workspace_bytes < ws || !p->workspace)
    return fail(VFM_E_INVALID, "workspace too small (vfm_elicit_field_workspace_bytes)");
  if (((uintptr_t)p->workspace) & 255) return fail(VFM_E_INVALID, "workspace must be 256-byte aligned");

  const hipStream_t st = (hipStream_t)stream;
  const bool sp = (p->flags & VFM_FLAG_LINK_SOFTPLUS) != 0;
  const vfm::FShape s = vfm::shape_of(p->d);
  const int DP = s.W * s.CPL;
  vfm::ElicitFieldArgs a;
  vfm::FoldArgs& f = a.f;
  f.E = p->U; f.R = 0; f.T = p->T;
  f.F = p->F; f.d = p->d; f.col = p->field; f.lik = p->likelihood; f.S = cf ? 1 : p->n_samples;
  f.n_steps = p->n_steps; f.reset = p->reset ? 1 : 0; f.mode = VFM_FOLDIN_FIT; f.cap = 0;
  f.lr = p->lr; f.klw = p->kl_weight; f.t0 = p->t0;
  f.key.seed_lo = (uint32_t)p->seed; f.key.seed_hi = (uint32_t)(p->seed >> 32);
  f.key.step_lo = f.key.step_hi = 0; f.key.chunk_off = 0;
  f.ent = nullptr; f.ptr = nullptr; f.x = nullptr; f.row_op = nullptr; f.y = nullptr;
  f.ops = nullptr; f.opc = nullptr;
  f.entity = p->entity_params; f.bias = p->bias_params; f.scal = p->scalars;
  f.loss = nullptr; f.grad = nullptr;
  a.U = p->U; a.P = p->P; a.H = p->H; a.n_ops = n_ops; a.Q = p->n_rounds; a.strat = p->strategy;
  a.write = p->write ? 1 : 0; a.key_col = p->key_col; a.seed = p->seed;
  a.ents = p->entities; a.pool_ptr = p->pool_ptr; a.pool_x = p->pool_x; a.pool_y = p->pool_y;
  a.hist_ptr = p->H > 0 ? p->hist_ptr : nullptr; a.hist_x = p->hist_x; a.hist_y = p->hist_y;
  a.pool_op = p->pool_op; a.hist_op = p->hist_op;
  a.out_row = p->out_row; a.out_score = p->out_score; a.out_loss = p->out_loss; a.out_theta = p->out_theta;
  a.out_mean = p->out_mean; a.out_var = p->out_var;
  char* w = (char*)p->workspace;
  a.asked = (uint8_t*)w;
  w += vfm::flags_bytes(p->P);
  float* sop = (float*)w;
  w += vfm::sop_bytes(n_ops, p->d);
  float* soc = (float*)w;
  w += vfm::soc_bytes(n_ops);
  a.sop = sop; a.soc = soc;
  if (n_ops > 0) {
    const unsigned nb = (unsigned)((n_ops + vfm::FB / vfm::WAVE - 1) / (vfm::FB / vfm::WAVE));
    hipLaunchKernelGGL(vfm::k_elicit_ctx_prep, dim3(nb), dim3(vfm::FB), 0, st, n_ops, p->op_x, (int)p->F, (int)p->field,
                       p->T, (int)p->d, sp, p->entity_params, p->bias_params, p->scalars, sop, soc);
    if (int rc = launch_status("k_elicit_ctx_prep")) return rc;
  }
  if (cf) {
    float* ops = (float*)w;
    float* opc = (float*)(w + vfm::ops_off_opc(n_ops, p->d));
    f.ops = ops; f.opc = opc;
    const int cap = vfm::lds_cap(s);
    f.cap = p->lds_rows < 0 ? cap : (p->lds_rows < cap ? p->lds_rows : cap);
    if (n_ops > 0) {
      const unsigned nb = (unsigned)((n_ops + vfm::FB - 1) / vfm::FB);
      if (sp)
        hipLaunchKernelGGL(vfm::k_foldin_prep<vfm::LINK_SOFTPLUS>, dim3(nb), dim3(vfm::FB), 0, st, n_ops, (int)p->F, p->d,
                           DP, (int)p->field, p->T, p->op_x, p->entity_params, p->bias_params, p->scalars, ops, opc);
      else
        hipLaunchKernelGGL(vfm::k_foldin_prep<vfm::LINK_ABS>, dim3(nb), dim3(vfm::FB), 0, st, n_ops, (int)p->F, p->d, DP,
                           (int)p->field, p->T, p->op_x, p->entity_params, p->bias_params, p->scalars, ops, opc);
      if (int rc = launch_status("k_foldin_prep")) return rc;
    }
    if (sp) vfm::launch_shape<vfm::LINK_SOFTPLUS, false>(s, a, st);
    else vfm::launch_shape<vfm::LINK_ABS, false>(s, a, st);
  } else {
    if (sp) vfm::launch_shape<vfm::LINK_SOFTPLUS, true>(s, a, st);
    else vfm::launch_shape<vfm::LINK_ABS, true>(s, a, st);
  }
  return launch_status("k_elicit_field");
}

}  // extern "C"

// vfm_elicit.hip -- elicitation sessions (include/vfm_elicit.h): ask, fold in and ask again, every round of every
// user's session in one launch.
//
// k_foldin_prep (closed form only, vfm_foldin_body.hpp): the row operand of every distinct item of pool and history,
//   once -- the items are frozen.
// k_elicit: k_foldin's layout.  A group of W lanes per user (W, CPL by d as shape_of picks them; lane l owns coordinates
//   j W + l); theta_u stays in registers over all rounds, the Adam moments over a round; the fold rows (history, then
//   the asked rows) are staged in LDS while they fit and streamed from the operand table past that.  The row sums of
//   the closed form are sequential in row order, so an asked row is APPENDED to them (fold_stage_rows over [n, n + 1)):
//   the same chains as the full recomputation.  Scoring parallelises the other way: a pair's score is a serial
//   k-ordered chain, so lane l scores the pool rows l, l + W, .. whole, reading theta_u from a per-group LDS copy in the
//   table's layout [mu | s | mu_w, s_w] that is refreshed after each fold; the best (score, position) is reduced over
//   the group by a butterfly of a total order, so every lane ends with the same winner.  The asked flags live in the
//   workspace, the asked order in out_row; both are written by lane 0 and read by the group after a barrier.  No atomics.
//
// Rounding: one kernel reproduces two definitions.  The pair functions of vfm_rank_tile.hpp (pair_moments, op_var,
// score_of) are defined under fp contraction off, the fold-in body of vfm_foldin_body.hpp under contraction on; each
// pins its mode with a pragma at the top of its body (decided by the front end, so inlining does not change it).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "vfm_args.hpp"
#include "vfm_elicit.h"
#include "vfm_rank_tile.hpp"         // pair_moments, score_of, philox_uniform: the scores of k_moments, bit for bit

namespace vfm {
namespace {
#include "vfm_rng.hpp"
#include "vfm_common.hpp"
#include "vfm_foldin_body.hpp"       // FoldArgs, k_foldin_prep, fold_stage_rows, fold_run: k_foldin's body

struct ElicitArgs {
  FoldArgs f;                            // the fold-in's options, tables and operands (its row list is unused)
  int64_t U, P;
  int32_t Q, strat, write;
  uint64_t seed;
  const int64_t *users, *pool_ptr, *pool_items, *hist_ptr, *hist_items, *pool_op, *hist_op;
  const float *pool_y, *hist_y;
  int64_t H;
  int64_t* out_row;
  float *out_score, *out_loss, *out_theta, *out_mean, *out_var;
  uint8_t* asked;                        // [P] workspace
};

// the fold rows of one user: the history slice in its order, then the asked pool rows in the order asked
struct SessionRows {
  const ElicitArgs& a;
  int64_t h0, nh;
  const int64_t* asked;                  // the user's row of out_row
  __device__ __forceinline__ int64_t op(int64_t i) const { return i < nh ? a.hist_op[h0 + i] : a.pool_op[asked[i - nh]]; }
  __device__ __forceinline__ float y(int64_t i) const { return i < nh ? a.hist_y[h0 + i] : a.pool_y[asked[i - nh]]; }
  __device__ __forceinline__ int64_t partner(int64_t i, int) const {
    return i < nh ? a.hist_items[h0 + i] : a.pool_items[asked[i - nh]];
  }
};

template <int W, int CPL, int LINK, bool SAMPLED>
__global__ __launch_bounds__(FB) void k_elicit(const ElicitArgs a) {
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
    e = a.users[g];
  }
  const bool eok = live && e >= 0 && e < f.T;
  const int d = f.d, Q = a.Q;
  const float prec = f.lik == VFM_LIK_NORMAL ? link_f<LINK>(f.scal[0]) : 0.f;
  const float m0 = f.scal[1], sg0 = link_f<LINK>(f.scal[2]);
  const float sg0r = link_of(f.scal[2], SP);             // (the ranking side's form of the same link)
  const SessionRows rows{a, h0, nh, a.out_row + g * Q};

  // ---- theta_u (coordinates past d: mu = 0, s = prior, never updated)
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

  // ---- LDS of the group: the fold stage (Ms [cap, DP], Cy [cap]) and theta_u in the table's layout (uth [2 DP + 2])
  float* Ms = lds + (int64_t)grp * ((int64_t)f.cap * (DP + 1) + 2 * DP + 2);
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

  // every thread of the block runs every round's barriers; a user with nothing left to ask skips the work between them
  for (int q = 0; q <= Q; ++q) {
#pragma unroll
    for (int j = 0; j < CPL; ++j)
      if (vk[j]) { uth[j * W + l] = mu[j]; uth[d + j * W + l] = sp[j]; }
    if (l == 0) { uth[2 * d] = muw; uth[2 * d + 1] = spw; }
    __syncthreads();                     // (theta_u, the asked flags and the stage are read across the group's lanes)
    if (q == Q && !a.out_mean) break;

    // ---- score: lane l takes the pool rows l, l + W, ..; its best by (score, position)
    float bs = 0.f;
    int64_t bp = -1;
    for (int64_t p = l; p < np; p += W) {
      const bool was = a.asked[p0 + p] != 0;
      if (was && !a.out_mean) continue;
      const int64_t it = a.pool_items[p0 + p];
      float mean = __builtin_nanf(""), var = __builtin_nanf(""), sc = __builtin_nanf("");
      if (eok && it >= 0 && it < f.T) {
        if (a.strat != VFM_RANK_RANDOM || a.out_mean)
          pair_moments(uth, f.entity + it * 2 * d, uth + 2 * d, f.bias + it * 2, m0, sg0r, d, SP, mean, var);
        sc = a.strat == VFM_RANK_RANDOM ? philox_uniform(a.seed + (uint64_t)q, e, it) : score_of(a.strat, mean, var);
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
// fold rows per user staged in LDS: what the block's stage leaves after every group's copy of theta_u
int lds_cap(const FShape& s) {
  const int DP = s.W * s.CPL, per_group = LDS_BYTES / 4 / (FB / s.W);
  const int c = (per_group - (2 * DP + 2)) / (DP + 1);
  return c < 0 ? 0 : c;
}

template <int W, int CPL, int LINK, bool SAMPLED>
void launch(const ElicitArgs& a, hipStream_t st) {
  constexpr int GPB = FB / W, DP = W * CPL;
  const size_t shm = (size_t)GPB * ((size_t)a.f.cap * (DP + 1) + 2 * DP + 2) * 4;
  hipLaunchKernelGGL((k_elicit<W, CPL, LINK, SAMPLED>), dim3((unsigned)((a.U + GPB - 1) / GPB)), dim3(FB), shm, st, a);
}

template <int LINK, bool SAMPLED>
void launch_shape(const FShape& s, const ElicitArgs& a, hipStream_t st) {
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

}  // namespace
}  // namespace vfm

extern "C" {

int64_t vfm_elicit_workspace_bytes(int64_t P, int64_t n_ops, int32_t d, int32_t objective) {
  if (P < 0 || n_ops < 0 || d < 1 || d > VFM_FOLDIN_MAX_D ||
      (objective != VFM_OBJ_CLOSED_FORM && objective != VFM_OBJ_SAMPLED))
    return VFM_E_INVALID;
  int64_t b = vfm::flags_bytes(P);
  if (objective == VFM_OBJ_CLOSED_FORM) b += vfm::ops_off_opc(n_ops, d) + vfm::round_up(n_ops * 2 * 4, 256);
  return b;
}

int vfm_elicit_f32(const vfm_elicit_t* p, void* stream) {
  using vfm::fail;
  if (!p) return fail(VFM_E_INVALID, "vfm_elicit_f32: NULL argument struct");
  if (p->struct_size != (uint32_t)sizeof(vfm_elicit_t) || p->abi_version != (uint32_t)VFM_ABI_VERSION)
    return fail(VFM_E_INVALID, "vfm_elicit_t: struct_size / abi_version differ from this library's (VFM_STRUCT_INIT)");
  if (p->T < 1) return fail(VFM_E_INVALID, "T < 1");
  if (p->F != 2) return fail(VFM_E_INVALID, "elicitation sessions: two-field models only (F must be 2)");
  if (p->d < 1 || p->d > VFM_FOLDIN_MAX_D) return fail(VFM_E_INVALID, "d out of range [1,512]");
  if (p->U < 0 || p->P < 0 || p->H < 0) return fail(VFM_E_INVALID, "U < 0, P < 0 or H < 0");
  if (p->n_rounds < 0 || p->n_rounds > VFM_ELICIT_MAX_ROUNDS) return fail(VFM_E_INVALID, "n_rounds out of range [0,4096]");
  if (p->strategy < VFM_RANK_TOP || p->strategy > VFM_RANK_RANDOM) return fail(VFM_E_INVALID, "unknown strategy");
  if (p->likelihood != VFM_LIK_NORMAL && p->likelihood != VFM_LIK_BERNOULLI)
    return fail(VFM_E_INVALID, "unknown likelihood");
  if (p->objective == VFM_OBJ_CLOSED_FORM) {
    if (p->likelihood != VFM_LIK_NORMAL) return fail(VFM_E_INVALID, "the closed form needs the Normal likelihood");
    if (p->n_ops < 0 || (p->P + p->H > 0 && p->n_ops < 1)) return fail(VFM_E_INVALID, "n_ops out of range");
  } else if (p->objective == VFM_OBJ_SAMPLED) {
    if (p->n_samples < 1 || p->n_samples > VFM_FOLDIN_MAX_SAMPLES)
      return fail(VFM_E_INVALID, "n_samples out of range [1,4]");
  } else {
    return fail(VFM_E_INVALID, "unknown objective");
  }
  if (p->flags & ~VFM_FLAG_LINK_SOFTPLUS) return fail(VFM_E_INVALID, "flags: only VFM_FLAG_LINK_SOFTPLUS is accepted");
  if (p->n_steps < 0) return fail(VFM_E_INVALID, "n_steps must be >= 0");
  if (p->t0 < 0 || p->t0 + (int64_t)(p->n_rounds + 1) * ((int64_t)p->n_steps + 1) >=
                       ((int64_t)1 << 60) / VFM_FOLDIN_MAX_SAMPLES)
    return fail(VFM_E_INVALID, "t0 out of range");
  if (!(p->lr >= 0.f) || !(p->kl_weight >= 0.f)) return fail(VFM_E_INVALID, "lr and kl_weight must be >= 0");
  if ((p->out_mean == nullptr) != (p->out_var == nullptr))
    return fail(VFM_E_INVALID, "out_mean and out_var: both or neither");
  if (p->U == 0) return 0;
  if (!p->users || !p->pool_ptr || !p->entity_params || !p->bias_params || !p->scalars ||
      (p->P > 0 && (!p->pool_items || !p->pool_y)) || (p->H > 0 && (!p->hist_ptr || !p->hist_items || !p->hist_y)) ||
      (p->n_rounds > 0 && (!p->out_row || !p->out_score || !p->out_loss)))
    return fail(VFM_E_INVALID, "null pointer");
  const bool cf = p->objective == VFM_OBJ_CLOSED_FORM;
  const int64_t n_ops = cf ? p->n_ops : 0;
  if (cf && ((p->P + p->H > 0 && !p->op_x) || (p->P > 0 && !p->pool_op) || (p->H > 0 && !p->hist_op)))
    return fail(VFM_E_INVALID, "closed form: op_x, pool_op and hist_op needed");
  const int64_t ws = vfm_elicit_workspace_bytes(p->P, n_ops, p->d, p->objective);
  if (ws < 0 || p->workspace_bytes < ws || !p->workspace)
    return fail(VFM_E_INVALID, "workspace too small (vfm_elicit_workspace_bytes)");
  if (((uintptr_t)p->workspace) & 255) return fail(VFM_E_INVALID, "workspace must be 256-byte aligned");

  const hipStream_t st = (hipStream_t)stream;
  const bool sp = (p->flags & VFM_FLAG_LINK_SOFTPLUS) != 0;
  const vfm::FShape s = vfm::shape_of(p->d);
  const int DP = s.W * s.CPL;
  vfm::ElicitArgs a;
  vfm::FoldArgs& f = a.f;
  f.E = p->U; f.R = 0; f.T = p->T;
  f.F = 2; f.d = p->d; f.col = 0; f.lik = p->likelihood; f.S = cf ? 1 : p->n_samples;
  f.n_steps = p->n_steps; f.reset = p->reset ? 1 : 0; f.mode = VFM_FOLDIN_FIT; f.cap = 0;
  f.lr = p->lr; f.klw = p->kl_weight; f.t0 = p->t0;
  f.key.seed_lo = (uint32_t)p->seed; f.key.seed_hi = (uint32_t)(p->seed >> 32);
  f.key.step_lo = f.key.step_hi = 0; f.key.chunk_off = 0;
  f.ent = nullptr; f.ptr = nullptr; f.x = nullptr; f.row_op = nullptr; f.y = nullptr;
  f.ops = nullptr; f.opc = nullptr;
  f.entity = p->entity_params; f.bias = p->bias_params; f.scal = p->scalars;
  f.loss = nullptr; f.grad = nullptr;
  a.U = p->U; a.P = p->P; a.H = p->H; a.Q = p->n_rounds; a.strat = p->strategy; a.write = p->write ? 1 : 0;
  a.seed = p->seed;
  a.users = p->users; a.pool_ptr = p->pool_ptr; a.pool_items = p->pool_items; a.pool_y = p->pool_y;
  a.hist_ptr = p->H > 0 ? p->hist_ptr : nullptr; a.hist_items = p->hist_items; a.hist_y = p->hist_y;
  a.pool_op = p->pool_op; a.hist_op = p->hist_op;
  a.out_row = p->out_row; a.out_score = p->out_score; a.out_loss = p->out_loss; a.out_theta = p->out_theta;
  a.out_mean = p->out_mean; a.out_var = p->out_var;
  char* w = (char*)p->workspace;
  a.asked = (uint8_t*)w;
  if (cf) {
    float* ops = (float*)(w + vfm::flags_bytes(p->P));
    float* opc = (float*)(w + vfm::flags_bytes(p->P) + vfm::ops_off_opc(n_ops, p->d));
    f.ops = ops; f.opc = opc;
    const int cap = vfm::lds_cap(s);
    f.cap = p->lds_rows < 0 ? cap : (p->lds_rows < cap ? p->lds_rows : cap);
    if (n_ops > 0) {
      const unsigned nb = (unsigned)((n_ops + vfm::FB - 1) / vfm::FB);
      if (sp)
        hipLaunchKernelGGL(vfm::k_foldin_prep<vfm::LINK_SOFTPLUS>, dim3(nb), dim3(vfm::FB), 0, st, n_ops, 2, p->d, DP, 0,
                           p->T, p->op_x, p->entity_params, p->bias_params, p->scalars, ops, opc);
      else
        hipLaunchKernelGGL(vfm::k_foldin_prep<vfm::LINK_ABS>, dim3(nb), dim3(vfm::FB), 0, st, n_ops, 2, p->d, DP, 0,
                           p->T, p->op_x, p->entity_params, p->bias_params, p->scalars, ops, opc);
      if (int rc = launch_status("k_foldin_prep")) return rc;
    }
    if (sp) vfm::launch_shape<vfm::LINK_SOFTPLUS, false>(s, a, st);
    else vfm::launch_shape<vfm::LINK_ABS, false>(s, a, st);
  } else {
    if (sp) vfm::launch_shape<vfm::LINK_SOFTPLUS, true>(s, a, st);
    else vfm::launch_shape<vfm::LINK_ABS, true>(s, a, st);
  }
  return launch_status("k_elicit");
}

}  // extern "C"

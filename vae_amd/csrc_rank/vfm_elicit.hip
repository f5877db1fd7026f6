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

#include <type_traits>

#include "vfm_args.hpp"
#include "vfm_elicit.h"
#include "vfm_rank_tile.hpp"         // pair_moments, score_of, philox_uniform: the scores of k_moments, bit for bit

namespace vfm {
namespace {
#include "vfm_rng.hpp"
#include "vfm_common.hpp"
#include "vfm_foldin_body.hpp"       // FoldArgs, k_foldin_prep, fold_stage_rows, fold_run: k_foldin's body
#include "vfm_elicit_host.hpp"       // what the two session entry points share on the host

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
  using namespace vfm;
  if (int rc = check_session_struct(p, "vfm_elicit_f32: NULL argument struct",
                                    "vfm_elicit_t: struct_size / abi_version differ from this library's (VFM_STRUCT_INIT)"))
    return rc;
  if (p->F != 2) return fail(VFM_E_INVALID, "elicitation sessions: two-field models only (F must be 2)");
  if (int rc = check_session_options(p, false)) return rc;
  if (p->U == 0) return 0;
  if (!p->users || (p->P > 0 && !p->pool_items) || (p->H > 0 && !p->hist_items) || session_pointers_missing(p))
    return fail(VFM_E_INVALID, "null pointer");
  const bool cf = p->objective == VFM_OBJ_CLOSED_FORM;
  const int64_t n_ops = cf ? p->n_ops : 0;
  if (cf && ((p->P + p->H > 0 && !p->op_x) || (p->P > 0 && !p->pool_op) || (p->H > 0 && !p->hist_op)))
    return fail(VFM_E_INVALID, "closed form: op_x, pool_op and hist_op needed");
  if (int rc = check_session_workspace(p, vfm_elicit_workspace_bytes(p->P, n_ops, p->d, p->objective),
                                       "workspace too small (vfm_elicit_workspace_bytes)"))
    return rc;

  const hipStream_t st = (hipStream_t)stream;
  const bool sp = (p->flags & VFM_FLAG_LINK_SOFTPLUS) != 0;
  const FShape sh = shape_of(p->d);
  const auto theta_floats = [](int DP) { return 2 * DP + 2; };      // (the group's copy of theta_u: the table's layout)
  ElicitArgs a = session_args<ElicitArgs>(p, 2, 0);
  a.users = p->users; a.pool_items = p->pool_items; a.hist_items = p->hist_items;
  FoldArgs& f = a.f;
  if (cf) {
    char* w = (char*)p->workspace + flags_bytes(p->P);
    float* ops = (float*)w;
    float* opc = (float*)(w + ops_off_opc(n_ops, p->d));
    f.ops = ops; f.opc = opc;
    f.cap = lds_cap(sh, theta_floats(sh.W * sh.CPL), p->lds_rows);
    if (int rc = launch_foldin_prep(sp, f, n_ops, p->op_x, ops, opc, st)) return rc;
  }
  launch_session(sh, sp, !cf, a, st, theta_floats, [](auto w, auto c, auto link, auto sampled) {
    return k_elicit<decltype(w)::value, decltype(c)::value, decltype(link)::value, decltype(sampled)::value>;
  });
  return launch_status("k_elicit");
}

}  // extern "C"

// vfm_elicit_field.hip -- elicitation sessions in the field form (include/vfm_elicit.h: vfm_elicit_field_f32): ask,
// fold in and ask again for the entities of one column of a model with any number of fields, every round of every
// respondent in one launch.  A unit of its own beside vfm_elicit.hip (the two-field session, untouched) so that the two
// families of 28 instances compile side by side.
//
// k_elicit_ctx_prep (vfm_elicit_field_score.hpp, with the kernel arguments, the fold rows and the score's operand
//   views, shared with the exact session of vfm_elicit_solve.hip): the score's operand of every distinct context of
//   pool and history, once -- a wave per context,
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

#include <type_traits>

#include "vfm_args.hpp"
#include "vfm_elicit.h"
#include "vfm_rank_tile.hpp"         // score_of, philox_uniform, link_of
#include "vfm_field_ctx.hpp"         // ctx_coord, ctx_op_var, ctx_consts, ctx_valid, field_chain_moments

namespace vfm {
namespace {
#include "vfm_rng.hpp"
#include "vfm_common.hpp"
#include "vfm_foldin_body.hpp"       // FoldArgs, k_foldin_prep, fold_stage_rows, fold_run: k_foldin's body
#include "vfm_elicit_host.hpp"       // what the two session entry points share on the host
#include "vfm_elicit_field_score.hpp" // k_elicit_ctx_prep, ElicitFieldArgs, FieldSessionRows, the score's operand views

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
  using namespace vfm;
  if (int rc = check_session_struct(
          p, "vfm_elicit_field_f32: NULL argument struct",
          "vfm_elicit_field_t: struct_size / abi_version differ from this library's (VFM_STRUCT_INIT)"))
    return rc;
  if (p->F < 2 || p->F > VFM_MAX_FIELDS) return fail(VFM_E_INVALID, "F out of range [2,64]");
  if (p->field < 0 || p->field >= p->F) return fail(VFM_E_INVALID, "field out of range [0,F)");
  if (p->key_col < 0 || p->key_col >= p->F || p->key_col == p->field)
    return fail(VFM_E_INVALID, "key_col must be a context column: in [0,F) and not field");
  if (int rc = check_session_options(p, true)) return rc;
  if (p->U == 0) return 0;
  if (!p->entities || (p->P > 0 && !p->pool_x) || (p->H > 0 && !p->hist_x) || session_pointers_missing(p))
    return fail(VFM_E_INVALID, "null pointer");
  if ((p->P + p->H > 0 && !p->op_x) || (p->P > 0 && !p->pool_op) || (p->H > 0 && !p->hist_op))
    return fail(VFM_E_INVALID, "op_x, pool_op and hist_op needed");
  const bool cf = p->objective == VFM_OBJ_CLOSED_FORM;
  const int64_t n_ops = p->n_ops;
  if (int rc = check_session_workspace(p, vfm_elicit_field_workspace_bytes(p->P, n_ops, p->d, p->objective),
                                       "workspace too small (vfm_elicit_field_workspace_bytes)"))
    return rc;

  const hipStream_t st = (hipStream_t)stream;
  const bool sp = (p->flags & VFM_FLAG_LINK_SOFTPLUS) != 0;
  const FShape sh = shape_of(p->d);
  char* w = (char*)p->workspace + flags_bytes(p->P);
  float* sop = (float*)w;
  w += sop_bytes(n_ops, p->d);
  float* soc = (float*)w;
  w += soc_bytes(n_ops);
  const auto theta_floats = [](int DP) { return 3 * DP + 2; };      // (the group's copy of theta_e: the candidate operands)
  ElicitFieldArgs a = session_args<ElicitFieldArgs>(p, p->F, p->field);
  a.ents = p->entities; a.pool_x = p->pool_x; a.hist_x = p->hist_x;
  a.n_ops = n_ops; a.key_col = p->key_col; a.sop = sop; a.soc = soc;
  FoldArgs& f = a.f;
  if (n_ops > 0) {
    const unsigned nb = (unsigned)((n_ops + FB / WAVE - 1) / (FB / WAVE));
    hipLaunchKernelGGL(k_elicit_ctx_prep, dim3(nb), dim3(FB), 0, st, n_ops, p->op_x, (int)p->F, (int)p->field, p->T,
                       (int)p->d, sp, p->entity_params, p->bias_params, p->scalars, sop, soc);
    if (int rc = launch_status("k_elicit_ctx_prep")) return rc;
  }
  if (cf) {
    float* ops = (float*)w;
    float* opc = (float*)(w + ops_off_opc(n_ops, p->d));
    f.ops = ops; f.opc = opc;
    f.cap = lds_cap(sh, theta_floats(sh.W * sh.CPL), p->lds_rows);
    if (int rc = launch_foldin_prep(sp, f, n_ops, p->op_x, ops, opc, st)) return rc;
  }
  launch_session(sh, sp, !cf, a, st, theta_floats, [](auto w, auto c, auto link, auto sampled) {
    return k_elicit_field<decltype(w)::value, decltype(c)::value, decltype(link)::value, decltype(sampled)::value>;
  });
  return launch_status("k_elicit_field");
}

}  // extern "C"

// vfm_elicit_design.hip -- target-aware elicitation (include/vfm_design.h): the question asked is the one that most
// reduces the predictive variance over the respondent's target contexts (csrc_rank/vfm_design_score.hpp holds the
// score and the two walks).
//
// k_design_score: the one-round form.  One workgroup of FB threads per respondent in a grid-stride loop; S from the
//   history, W and v(S) formed once into LDS (3 d doubles); thread t then scores the pool rows t, t + FB, .. whole.
// k_elicit_design<W, CPL, LINK>: the sessions, in k_elicit_solve's layout -- theta_e in LDS (pf of solve_body) over all
//   rounds, the same choose-reduction with the same total order, solve_body unchanged after every answer, `write` /
//   out_theta / out_mean / out_var as there.  W is formed once per respondent into LDS; S is walked again every round
//   INTO solve_body's own scale-sum vector (SBd, sm + 6 (d + 1) + 1), after the barrier that ends every round (the
//   caller's side of solve_body's contract): phase A leaves the same bits there; v(S) is refreshed beside W.  The moments
//   (out_mean / out_var) are those of vfm_elicit_solve_f32, computed only when asked for.
//
// Operand passes, once, over an operand table that also holds the target contexts: k_elicit_ctx_prep (the moments'
// operands), k_foldin_prep and k_foldin_solve_prep.  No atomics, no host synchronisation.
//
// LDS of a session block: k_elicit_solve's plus 2 d doubles (W, v(S)).  Everything a respondent reads from LDS or its
// slab is written for that respondent first.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "vfm_args.hpp"
#include "vfm_design.h"
#include "vfm_launch.hpp"            // launch_status
#include "vfm_rank_tile.hpp"         // link_of
#include "vfm_field_ctx.hpp"         // ctx_valid, field_chain_moments

namespace vfm {
namespace {
#include "vfm_rng.hpp"
#include "vfm_common.hpp"
#include "vfm_foldin_body.hpp"       // FoldArgs, k_foldin_prep, fold_stage_rows, the host side
#include "vfm_foldin_solve_body.hpp" // solve_body, k_foldin_solve_prep, the operand block and the slabs
#include "vfm_elicit_host.hpp"       // the checks the session entry points share
#include "vfm_elicit_field_score.hpp" // k_elicit_ctx_prep, ElicitFieldArgs, FieldSessionRows, the moments' operand views
#include "vfm_design_score.hpp"      // design_walk_S, design_walk_W, design_v, design_score, design_better

struct DesignArgs {
  ElicitFieldArgs e;                     // (e.f.cap = 0; e.strat, e.key_col, e.seed unused)
  const double* ops64;                   // [n_ops, 3, d]  M | A | C, unrounded
  const double* cm64;                    // [n_ops]        c_mean
  double* slab;                          // [gridDim.x, slab_elems] or NULL when every system stays in LDS
  int64_t slab_elems;
  int32_t cap_dim;                       // systems up to this size live in LDS
  int64_t n_targets;
  const int64_t *tgt_ptr, *tgt_op;
  float* out_pool_score;                 // [P] (k_design_score)
};

constexpr int NW = FB / WAVE;            // waves of a block

// bytes of a session block's LDS past k_foldin_solve's: W and v(S), the waves' winners, the moments' candidate operands
__host__ __device__ inline int64_t design_tail_bytes(int d, int DP) {
  return 2 * (int64_t)d * 8 + NW * 8 + NW * 4 + (3 * (int64_t)DP + 2) * 4;
}

// the history slice of a respondent as the rows of design_walk_S
struct HistOps {
  const int64_t* o;
  __device__ __forceinline__ int64_t op(int64_t i) const { return o[i]; }
};

template <int LINK>
__global__ __launch_bounds__(FB) void k_design_score(const DesignArgs s) {
  extern __shared__ double sm[];
  const ElicitFieldArgs& a = s.e;
  const FoldArgs& f = a.f;
  const int tid = threadIdx.x, d = f.d, F = f.F;
  double *S = sm, *Wt = sm + d, *vS = sm + 2 * d;
  const double prec = link_d<LINK>(f.scal[0]), kl = f.klw;

  for (int64_t g = blockIdx.x; g < a.U; g += gridDim.x) {
    const int64_t p0 = min(max(a.pool_ptr[g], (int64_t)0), a.P);
    const int64_t np = min(max(a.pool_ptr[g + 1], p0), a.P) - p0;
    int64_t h0 = 0, nh = 0;
    if (a.hist_ptr) {
      h0 = min(max(a.hist_ptr[g], (int64_t)0), a.H);
      nh = min(max(a.hist_ptr[g + 1], h0), a.H) - h0;
    }
    const int64_t t0 = min(max(s.tgt_ptr[g], (int64_t)0), s.n_targets);
    const int64_t nt = min(max(s.tgt_ptr[g + 1], t0), s.n_targets) - t0;
    const int64_t e = a.ents[g];
    const bool eok = e >= 0 && e < f.T;

    design_walk_S(s.ops64, a.n_ops, d, HistOps{a.hist_op + h0}, nh, S);
    design_walk_W(s.ops64, a.n_ops, d, s.tgt_op + t0, nt, Wt);
    for (int k = tid; k < d; k += FB) vS[k] = design_v(kl, prec, S[k]);       // (the thread that wrote S[k])
    __syncthreads();

    for (int64_t p = tid; p < np; p += FB) {
      const int64_t o = a.pool_op[p0 + p];
      float sc = __builtin_nanf("");
      if (eok && o >= 0 && o < a.n_ops && ctx_valid(a.pool_x + (p0 + p) * F, F, f.col, f.T))
        sc = design_score(S, Wt, vS, (double)nh, s.ops64 + o * 3 * (int64_t)d, d, kl, prec);
      s.out_pool_score[p0 + p] = sc;
    }
    __syncthreads();                     // (S, W, v(S) are rewritten by the next respondent)
  }
}

template <int W, int CPL, int LINK>
__global__ __launch_bounds__(FB) void k_elicit_design(const DesignArgs s) {
  extern __shared__ double sm[];
  constexpr int DP = W * CPL;
  constexpr bool SP = LINK == LINK_SOFTPLUS;
  const ElicitFieldArgs& a = s.e;
  const FoldArgs& f = a.f;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int d = f.d, d1 = d + 1, Q = a.Q, F = f.F;
  double* Sv = sm + 6 * d1 + 1;          // S: coordinates 1 .. d of solve_body's scale sums (SBd)
  float* pf = (float*)(sm + 7 * d1);     // theta_e: mu_w, mu [d] | s_w, s [d]  (solve_body's)
  double* Hl = sm + 8 * d1;
  double* Wt = Hl + tri(s.cap_dim);                         // [d] the target weights
  double* vS = Wt + d;                                      // [d] v(S)
  long long* rpos = (long long*)(vS + d);                   // [NW] the waves' winners
  float* rsc = (float*)(rpos + NW);                         // [NW]
  float* uth = rsc + NW;                                    // [3 DP + 2] the moments' candidate operands of theta_e
  double* Hg = s.slab ? s.slab + (int64_t)blockIdx.x * s.slab_elems : nullptr;
  const float precf = link_f<LINK>(f.scal[0]);
  const double prec = link_d<LINK>(f.scal[0]), kl = f.klw;

  for (int64_t g = blockIdx.x; g < a.U; g += gridDim.x) {
    const int64_t p0 = min(max(a.pool_ptr[g], (int64_t)0), a.P);
    const int64_t np = min(max(a.pool_ptr[g + 1], p0), a.P) - p0;
    int64_t h0 = 0, nh = 0;
    if (a.hist_ptr) {
      h0 = min(max(a.hist_ptr[g], (int64_t)0), a.H);
      nh = min(max(a.hist_ptr[g + 1], h0), a.H) - h0;
    }
    const int64_t t0 = min(max(s.tgt_ptr[g], (int64_t)0), s.n_targets);
    const int64_t nt = min(max(s.tgt_ptr[g + 1], t0), s.n_targets) - t0;
    const int64_t e = a.ents[g];
    const bool eok = e >= 0 && e < f.T;                     // (block-uniform)
    const FieldSessionRows rows{a, h0, nh, a.out_row + g * Q};

    // ---- theta_e: the table row, or the prior; the target weights, once
    for (int c = tid; c < d1; c += FB) {
      float m = 0.f, sp = prior_s<LINK>();
      if (eok && !f.reset) {
        m = c == 0 ? f.bias[e * 2] : f.entity[e * 2 * d + (c - 1)];
        sp = c == 0 ? f.bias[e * 2 + 1] : f.entity[e * 2 * d + d + (c - 1)];
      }
      pf[c] = m;
      pf[d1 + c] = sp;
    }
    design_walk_W(s.ops64, a.n_ops, d, s.tgt_op + t0, nt, Wt);
    for (int64_t p = tid; p < np; p += FB) a.asked[p0 + p] = 0;
    int64_t n = nh;
    __syncthreads();

    const auto put_theta = [&](int q) {                     // theta_e after round q, by every thread
      if (!a.out_theta) return;
      float* to = a.out_theta + (g * Q + q) * (2 * (int64_t)d + 2);
      for (int k = tid; k < d; k += FB) { to[k] = pf[1 + k]; to[d + k] = pf[d1 + 1 + k]; }
      if (tid == 0) { to[2 * d] = pf[0]; to[2 * d + 1] = pf[d1]; }
    };

    for (int q = 0; q <= Q; ++q) {
      if (a.out_mean) {
        for (int k = tid; k < d; k += FB) {
          float m2, s2;
          theta_cand_ops(pf[1 + k], pf[d1 + 1 + k], SP, m2, s2);
          uth[k] = pf[1 + k]; uth[DP + k] = m2; uth[2 * DP + k] = s2;
        }
        if (tid == 0) {
          float m2, s2;
          theta_cand_ops(pf[0], pf[d1], SP, m2, s2);
          uth[3 * DP] = pf[0]; uth[3 * DP + 1] = s2;
        }
      }
      if (q < Q) {                       // S over the n fold rows so far, in row order, and v(S)
        design_walk_S(s.ops64, a.n_ops, d, rows, n, Sv);
        for (int k = tid; k < d; k += FB) vS[k] = design_v(kl, prec, Sv[k]);  // (the thread that wrote Sv[k])
      }
      __syncthreads();                   // (S, v(S), uth and the asked flags are read across the block)
      if (q == Q && !a.out_mean) break;

      // ---- score: thread t takes the pool rows t, t + FB, ..; its best by (score, position)
      float bs = 0.f;
      long long bp = -1;
      for (int64_t p = tid; p < np; p += FB) {
        const bool was = a.asked[p0 + p] != 0;
        if (was && !a.out_mean) continue;
        const int64_t* xr = a.pool_x + (p0 + p) * F;
        const int64_t o = a.pool_op[p0 + p];
        const bool ok = eok && o >= 0 && o < a.n_ops && ctx_valid(xr, F, f.col, f.T);
        if (a.out_mean) {
          float mean = __builtin_nanf(""), var = __builtin_nanf("");
          if (ok)
            field_chain_moments(CtxRowOp{a.sop + o * 4 * (int64_t)d, d}, ThetaCand{uth, DP}, a.soc[o * 2], a.soc[o * 2 + 1],
                                d, mean, var);
          a.out_mean[(int64_t)q * a.P + p0 + p] = mean;
          a.out_var[(int64_t)q * a.P + p0 + p] = var;
        }
        if (was || q == Q || !ok) continue;
        const float sc = design_score(Sv, Wt, vS, (double)n, s.ops64 + o * 3 * (int64_t)d, d, kl, prec);
        if (sc == sc && (bp < 0 || sc > bs)) { bs = sc; bp = p; }
      }
      if (q == Q) break;

      // ---- choose: a butterfly over the wave, then the waves' winners in wave order; a total order
#pragma unroll
      for (int off = WAVE / 2; off >= 1; off >>= 1) {
        const float os = __shfl_xor(bs, off, WAVE);
        const long long op = __shfl_xor(bp, off, WAVE);
        if (design_better(os, op, bs, bp)) { bs = os; bp = op; }
      }
      if (lane == 0) { rsc[wv] = bs; rpos[wv] = bp; }
      __syncthreads();
      bs = rsc[0]; bp = rpos[0];
#pragma unroll
      for (int w = 1; w < NW; ++w)
        if (design_better(rsc[w], rpos[w], bs, bp)) { bs = rsc[w]; bp = rpos[w]; }
      const bool act = eok && bp >= 0;   // (block-uniform)
      if (tid == 0) {
        a.out_row[g * Q + q] = act ? p0 + bp : -1;
        a.out_score[g * Q + q] = act ? bs : __builtin_nanf("");
        if (act) a.asked[p0 + bp] = 1;
        else a.out_loss[g * Q + q] = __builtin_nanf("");
      }
      __syncthreads();                   // (out_row: the asked row is fold row n from here on)

      // ---- fold in: the optimum over the history and the rows asked so far, from the rows themselves
      if (act) {
        ++n;
        const int m = solve_dim(n, d);
        solve_body<W, CPL, LINK>(f, s.ops64, s.cm64, rows, n, sm, m <= s.cap_dim ? Hl : Hg, precf, prec,
                                 a.out_loss + g * Q + q, [&](const float*) { put_theta(q); });
      } else {
        put_theta(q);
      }
      __syncthreads();                   // (solve_body's contract: its LDS -- SBd, by the next round's walk -- is written again)
    }

    if (eok && a.write) {
      for (int k = tid; k < d; k += FB) {
        f.entity[e * 2 * d + k] = pf[1 + k];
        f.entity[e * 2 * d + d + k] = pf[d1 + 1 + k];
      }
      if (tid == 0) { f.bias[e * 2] = pf[0]; f.bias[e * 2 + 1] = pf[d1]; }
    }
    __syncthreads();                     // (pf and W are rewritten by the next respondent)
  }
}

void launch_sessions(const FShape& sh, bool sp, const DesignArgs& s, unsigned grid, hipStream_t st) {
  for_link(sp, [&](auto link) {
    for_shape(sh, [&](auto w, auto c) {
      constexpr int DP = decltype(w)::value * decltype(c)::value;
      const size_t shm = (size_t)lds_doubles(s.e.f.d, s.cap_dim) * 8 + (size_t)design_tail_bytes(s.e.f.d, DP);
      const auto k = k_elicit_design<decltype(w)::value, decltype(c)::value, decltype(link)::value>;
      // (more than 64 KiB of dynamic LDS: state the size; a runtime that needs no opt-in ignores it)
      (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
      (void)hipGetLastError();
      hipLaunchKernelGGL(k, dim3(grid), dim3(FB), shm, st, s);
    });
  });
}

// workspace: [asked flags | the moments' operands | their constants | the fold-in's operand block and slabs]
inline int64_t off_fold(int64_t P, int64_t n_ops, int d) { return flags_bytes(P) + sop_bytes(n_ops, d) + soc_bytes(n_ops); }

// the checks of both entry points, in the order they are reported; session: vfm_design_elicit_f32
int check_design(const vfm_design_t* p, bool session, const char* null_msg) {
  if (int rc = check_session_struct(p, null_msg,
                                    "vfm_design_t: struct_size / abi_version differ from this library's (VFM_STRUCT_INIT)"))
    return rc;
  if (p->F < 2 || p->F > VFM_MAX_FIELDS) return fail(VFM_E_INVALID, "F out of range [2,64]");
  if (p->field < 0 || p->field >= p->F) return fail(VFM_E_INVALID, "field out of range [0,F)");
  if (p->d < 1 || p->d > VFM_FOLDIN_MAX_D) return fail(VFM_E_INVALID, "d out of range [1,512]");
  if (p->U < 0 || p->P < 0 || p->H < 0 || p->n_targets < 0) return fail(VFM_E_INVALID, "U < 0, P < 0, H < 0 or n_targets < 0");
  if (session && (p->n_rounds < 0 || p->n_rounds > VFM_ELICIT_MAX_ROUNDS))
    return fail(VFM_E_INVALID, "n_rounds out of range [0,4096]");
  if (p->n_ops < 0 || (p->P + p->H + p->n_targets > 0 && p->n_ops < 1)) return fail(VFM_E_INVALID, "n_ops out of range");
  if (p->flags & ~VFM_FLAG_LINK_SOFTPLUS) return fail(VFM_E_INVALID, "flags: only VFM_FLAG_LINK_SOFTPLUS is accepted");
  if (p->lds_dim < -1) return fail(VFM_E_INVALID, "lds_dim: -1 or >= 0");
  if (!(p->kl_weight > 0.f) || !(p->kl_weight <= 3.0e38f))
    return fail(VFM_E_INVALID, "kl_weight must be > 0 and finite (the prior is what makes the scales finite)");
  if (session && (p->out_mean == nullptr) != (p->out_var == nullptr))
    return fail(VFM_E_INVALID, "out_mean and out_var: both or neither");
  if (p->U == 0) return 0;
  if (!p->entities || !p->tgt_ptr || (p->P > 0 && !p->pool_x) || (p->n_targets > 0 && !p->tgt_op))
    return fail(VFM_E_INVALID, "null pointer");
  if (session ? ((p->H > 0 && !p->hist_x) || session_pointers_missing(p))
              : (!p->pool_ptr || !p->entity_params || !p->bias_params || !p->scalars || (p->H > 0 && !p->hist_ptr) ||
                 (p->P > 0 && !p->out_pool_score)))
    return fail(VFM_E_INVALID, "null pointer");
  if ((p->n_ops > 0 && !p->op_x) || (p->P > 0 && !p->pool_op) || (p->H > 0 && !p->hist_op))
    return fail(VFM_E_INVALID, "op_x, pool_op and hist_op needed");
  return check_session_workspace(p, vfm_design_workspace_bytes(p->U, p->P, p->n_ops, p->d, p->lds_dim),
                                 "workspace too small (vfm_design_workspace_bytes)");
}

// the kernel arguments of both entry points; w: the fold-in's operand block in the workspace
DesignArgs design_args(const vfm_design_t* p, bool session, char*& w, float*& sop, float*& soc) {
  w = (char*)p->workspace + flags_bytes(p->P);
  sop = (float*)w;
  w += sop_bytes(p->n_ops, p->d);
  soc = (float*)w;
  w += soc_bytes(p->n_ops);              // (w: the fold-in's operand block)
  DesignArgs s = {};
  ElicitFieldArgs& a = s.e;
  a.f = fill_fold_args(p->U, p->T, p->F, p->d, p->field, VFM_LIK_NORMAL, 1, 0, session && p->reset ? 1 : 0, VFM_FOLDIN_FIT,
                       0.f, p->kl_weight, 0, 0, p->entity_params, p->bias_params, p->scalars);
  a.U = p->U; a.P = p->P; a.H = p->H; a.n_ops = p->n_ops;
  a.Q = session ? p->n_rounds : 0; a.write = session && p->write ? 1 : 0;
  a.ents = p->entities; a.pool_ptr = p->pool_ptr; a.pool_x = p->pool_x; a.pool_y = p->pool_y;
  a.hist_ptr = p->H > 0 ? p->hist_ptr : nullptr; a.hist_x = p->hist_x; a.hist_y = p->hist_y;
  a.pool_op = p->pool_op; a.hist_op = p->hist_op;
  a.sop = sop; a.soc = soc;
  if (session) {
    a.out_row = p->out_row; a.out_score = p->out_score; a.out_loss = p->out_loss; a.out_theta = p->out_theta;
    a.out_mean = p->out_mean; a.out_var = p->out_var;
  }
  a.asked = (uint8_t*)p->workspace;
  a.f.ops = (const float*)w;
  a.f.opc = (const float*)(w + ops_off_opc(p->n_ops, p->d));
  s.ops64 = (const double*)(w + off_ops64(p->n_ops, p->d));
  s.cm64 = (const double*)(w + off_cm64(p->n_ops, p->d));
  s.cap_dim = cap_dim_of(p->d, p->lds_dim);
  s.n_targets = p->n_targets; s.tgt_ptr = p->tgt_ptr; s.tgt_op = p->tgt_op;
  s.out_pool_score = p->out_pool_score;
  return s;
}

}  // namespace
}  // namespace vfm

extern "C" {

int64_t vfm_design_workspace_bytes(int64_t U, int64_t P, int64_t n_ops, int32_t d, int32_t lds_dim) {
  if (U < 0 || P < 0 || n_ops < 0 || d < 1 || d > VFM_FOLDIN_MAX_D || lds_dim < -1) return VFM_E_INVALID;
  int64_t b = vfm::off_fold(P, n_ops, d) + vfm::off_slabs(n_ops, d);
  if (d + 1 > vfm::cap_dim_of(d, lds_dim))
    b += (U < VFM_FOLDIN_SOLVE_SLABS ? U : VFM_FOLDIN_SOLVE_SLABS) * vfm::slab_bytes(d);
  return b;
}

int vfm_design_scores_f32(const vfm_design_t* p, void* stream) {
  using namespace vfm;
  if (int rc = check_design(p, false, "vfm_design_scores_f32: NULL argument struct")) return rc;
  if (p->U == 0 || p->P == 0) return 0;
  const hipStream_t st = (hipStream_t)stream;
  const bool sp = (p->flags & VFM_FLAG_LINK_SOFTPLUS) != 0;
  char* w;
  float *sop, *soc;
  const DesignArgs s = design_args(p, false, w, sop, soc);
  const FoldArgs& f = s.e.f;
  const unsigned nb = (unsigned)((p->n_ops + FB - 1) / FB);
  const int64_t gmax = (int64_t)1 << 20;
  const unsigned grid = (unsigned)(p->U < gmax ? p->U : gmax);
  int rc = 0;
  for_link(sp, [&](auto link) {
    hipLaunchKernelGGL(k_foldin_solve_prep<decltype(link)::value>, dim3(nb), dim3(FB), 0, st, p->n_ops, f.F, f.d, f.col, f.T,
                       p->op_x, f.entity, f.bias, f.scal, (double*)s.ops64, (double*)s.cm64);
    rc = launch_status("k_foldin_solve_prep");
    if (rc) return;
    hipLaunchKernelGGL(k_design_score<decltype(link)::value>, dim3(grid), dim3(FB), (size_t)3 * f.d * 8, st, s);
    rc = launch_status("k_design_score");
  });
  return rc;
}

int vfm_design_elicit_f32(const vfm_design_t* p, void* stream) {
  using namespace vfm;
  if (int rc = check_design(p, true, "vfm_design_elicit_f32: NULL argument struct")) return rc;
  if (p->U == 0) return 0;
  const hipStream_t st = (hipStream_t)stream;
  const bool sp = (p->flags & VFM_FLAG_LINK_SOFTPLUS) != 0;
  const FShape sh = shape_of(p->d);
  char* w;
  float *sop, *soc;
  DesignArgs s = design_args(p, true, w, sop, soc);
  const bool slabs = p->d + 1 > s.cap_dim;
  s.slab = slabs ? (double*)(w + off_slabs(p->n_ops, p->d)) : nullptr;
  s.slab_elems = slab_bytes(p->d) / 8;
  const int64_t gmax = slabs ? VFM_FOLDIN_SOLVE_SLABS : ((int64_t)1 << 20);
  const unsigned grid = (unsigned)(p->U < gmax ? p->U : gmax);

  if (p->n_ops > 0) {
    const unsigned nb = (unsigned)((p->n_ops + NW - 1) / NW);
    hipLaunchKernelGGL(k_elicit_ctx_prep, dim3(nb), dim3(FB), 0, st, p->n_ops, p->op_x, (int)p->F, (int)p->field, p->T,
                       (int)p->d, sp, p->entity_params, p->bias_params, p->scalars, sop, soc);
    if (int rc = launch_status("k_elicit_ctx_prep")) return rc;
    if (int rc = launch_solve_preps(sp, s.e.f, p->n_ops, p->op_x, w, st)) return rc;
  }
  launch_sessions(sh, sp, s, grid, st);
  return launch_status("k_elicit_design");
}

}  // extern "C"

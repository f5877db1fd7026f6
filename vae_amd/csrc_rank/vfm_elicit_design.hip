// vfm_elicit_design.hip -- target-aware elicitation (include/vfm_design.h): the question asked is the one that most
// reduces the predictive variance over the respondent's target contexts (csrc_rank/vfm_design_score.hpp holds the
// score and the two walks).
//
// k_design_score: the one-round form.  One workgroup of FB threads per respondent in a grid-stride loop; S from the
//   history, W and v(S) formed once into LDS (3 d doubles); thread t then scores the pool rows t, t + FB, .. whole.
// k_elicit_design<W, CPL, LINK>: the sessions -- the session loop of vfm_elicit_exact_body.hpp (exact_session: the
//   layout, the choice, the fold-in by solve_body, `write` / out_theta / out_mean / out_var, the operand passes and the
//   host path are there) with DesignScore.  W is formed once per respondent into LDS; S is walked again every round
//   INTO solve_body's own scale-sum vector (SBd, sm + 6 (d + 1) + 1), after the barrier that ends every round (the
//   caller's side of solve_body's contract): phase A leaves the same bits there; v(S) is refreshed beside W.  The moments
//   (out_mean / out_var) are those of vfm_elicit_solve_f32, computed only when asked for, and with them the candidate
//   operands of theta_e.
//
// The operand table also holds the target contexts.  No atomics, no host synchronisation.
//
// LDS of a session block: k_elicit_solve's plus 2 d doubles (W, v(S)) between the triangle and the waves' winners.
//
// vfm_design_scores_prior_f32 and vfm_design_elicit_prior_f32 (include/vfm_elicit_prior.h) run the PRIOR = true
// instantiations (k_design_score<LINK, true>, k_elicit_design_prior): the respondents' field prior staged in LDS in
// front, the score's v under its precisions (vfm_design_score.hpp), one more pointer among the kernel's arguments; the
// instantiations without it are the parents', unchanged.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "vfm_args.hpp"
#include "vfm_design.h"
#include "vfm_elicit_prior.h"
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
#include "vfm_elicit_exact_body.hpp" // ElicitSolveArgs, exact_session, the host side of the exact sessions
#include "vfm_design_score.hpp"      // design_walk_S, design_walk_W, design_v, design_score

struct DesignArgs : ElicitSolveArgs {     // (e.strat, e.key_col, e.seed unused)
  int64_t n_targets;
  const int64_t *tgt_ptr, *tgt_op;
  float* out_pool_score;                 // [P] (k_design_score)
};

// the history slice of a respondent as the rows of design_walk_S
struct HistOps {
  const int64_t* o;
  __device__ __forceinline__ int64_t op(int64_t i) const { return o[i]; }
};

template <int LINK, bool PRIOR>
__device__ __forceinline__ void design_score_pass(const DesignArgs& s, const float* __restrict__ prior) {
  extern __shared__ double sm_all[];
  const ElicitFieldArgs& a = s.e;
  const FoldArgs& f = a.f;
  const int tid = threadIdx.x, d = f.d;
  double* sm = sm_all + (PRIOR ? 2 * (d + 1) : 0);         // (the prior in front: mean | precision [2, d + 1])
  const double* lam = PRIOR ? sm_all + (d + 1) : nullptr;
  double *S = sm, *Wt = sm + d, *vS = sm + 2 * d;
  const double prec = link_d<LINK>(f.scal[0]), kl = f.klw;
  if constexpr (PRIOR) {
    stage_prior(prior, sm_all, d + 1);
    __syncthreads();
  }

  for (int64_t g = blockIdx.x; g < a.U; g += gridDim.x) {
    const RespondentRanges r = respondent_ranges(a, g);
    int64_t t0, nt;
    clamped_range(s.tgt_ptr, g, s.n_targets, t0, nt);
    const int64_t e = a.ents[g];
    const bool eok = e >= 0 && e < f.T;

    design_walk_S(s.ops64, a.n_ops, d, HistOps{a.hist_op + r.h0}, r.nh, S);
    design_walk_W(s.ops64, a.n_ops, d, s.tgt_op + t0, nt, Wt);
    design_put_v<PRIOR>(kl, prec, S, d, vS, lam);          // (the thread that wrote S[k])
    __syncthreads();

    for (int64_t p = tid; p < r.np; p += FB) {
      const int64_t o = a.pool_op[r.p0 + p];
      float sc = __builtin_nanf("");
      if (pool_row_ok(a, r.p0 + p, o, eok))
        sc = design_score<PRIOR>(S, Wt, vS, (double)r.nh, s.ops64 + o * 3 * (int64_t)d, d, kl, prec, lam);
      s.out_pool_score[r.p0 + p] = sc;
    }
    __syncthreads();                     // (S, W, v(S) are rewritten by the next respondent)
  }
}

template <int LINK>
__global__ __launch_bounds__(FB) void k_design_score(const DesignArgs s) {
  design_score_pass<LINK, false>(s, nullptr);
}

template <int LINK>
__global__ __launch_bounds__(FB) void k_design_score_prior(const DesignArgs s, const float* __restrict__ prior) {
  design_score_pass<LINK, true>(s, prior);
}

// the questions scored by the drop of the targets' variance that the respondent's scales carry
template <bool PRIOR>
struct DesignScoreT {
  using Args = DesignArgs;
  static constexpr bool THETA_OPS_EVERY_ROUND = false, ROUND_END_BARRIER = true;
  __host__ __device__ static int64_t lds_doubles(int d) { return 2 * (int64_t)d; }

  const DesignArgs& s;
  double *Sv, *Wt, *vS;                  // S: coordinates 1 .. d of solve_body's scale sums (SBd) | [d] W | [d] v(S)
  double prec, kl;
  const double* lam;                     // PRIOR: the prior's precisions [d + 1] in LDS
  __device__ __forceinline__ DesignScoreT(const Args& s_, double* sm, double* own, double prec_, const double* pr)
      : s(s_), Sv(sm + 6 * (s_.e.f.d + 1) + 1), Wt(own), vS(own + s_.e.f.d), prec(prec_), kl(s_.e.f.klw),
        lam(PRIOR ? pr + (s_.e.f.d + 1) : nullptr) {}

  __device__ __forceinline__ void begin_respondent(int64_t g) const {          // the target weights, once
    int64_t t0, nt;
    clamped_range(s.tgt_ptr, g, s.n_targets, t0, nt);
    design_walk_W(s.ops64, s.e.n_ops, s.e.f.d, s.tgt_op + t0, nt, Wt);
  }

  __device__ __forceinline__ void begin_round(int q, const FieldSessionRows& rows, int64_t n) const {
    if (q == s.e.Q) return;              // S over the n fold rows so far, in row order, and v(S)
    const int d = s.e.f.d;
    design_walk_S(s.ops64, s.e.n_ops, d, rows, n, Sv);
    design_put_v<PRIOR>(kl, prec, Sv, d, vS, lam);         // (the thread that wrote Sv[k])
  }

  template <int DP>
  __device__ __forceinline__ float pool_row(int q, int64_t p0, int64_t p, bool was, bool eok, int64_t, int64_t n,
                                            const float* uth) const {
    const ElicitFieldArgs& a = s.e;
    const int d = a.f.d;
    const int64_t o = a.pool_op[p0 + p];
    const bool ok = pool_row_ok(a, p0 + p, o, eok);
    float mean = __builtin_nanf(""), var = __builtin_nanf("");
    if (a.out_mean && ok) pool_row_moments<DP>(a, o, uth, mean, var);
    put_moments(a, q, p0, p, mean, var);
    if (was || q == a.Q || !ok) return __builtin_nanf("");
    return design_score<PRIOR>(Sv, Wt, vS, (double)n, s.ops64 + o * 3 * (int64_t)d, d, kl, prec, lam);
  }
};
using DesignScore = DesignScoreT<false>;

template <int W, int CPL, int LINK>
__global__ __launch_bounds__(FB) void k_elicit_design(const DesignArgs s) {
  exact_session<DesignScore, W, CPL, LINK>(s);
}

template <int W, int CPL, int LINK>
__global__ __launch_bounds__(FB) void k_elicit_design_prior(const DesignArgs s, const float* __restrict__ prior) {
  exact_session<DesignScoreT<true>, W, CPL, LINK, SolveFold, true>(s, prior);
}

// the checks of both entry points, in the order they are reported; session: vfm_design_elicit_f32
int check_design(const vfm_design_t* p, bool session, const char* null_msg) {
  if (int rc = check_session_struct(p, null_msg,
                                    "vfm_design_t: struct_size / abi_version differ from this library's (VFM_STRUCT_INIT)"))
    return rc;
  if (int rc = check_exact_field(p)) return rc;
  if (int rc = check_exact_sizes(p, p->n_targets >= 0, "U < 0, P < 0, H < 0 or n_targets < 0", session)) return rc;
  if (int rc = check_exact_options(p, p->P + p->H + p->n_targets,
                                   "kl_weight must be > 0 and finite (the prior is what makes the scales finite)", session))
    return rc;
  if (p->U == 0) return 0;
  if (!p->entities || !p->tgt_ptr || (p->P > 0 && !p->pool_x) || (p->n_targets > 0 && !p->tgt_op))
    return fail(VFM_E_INVALID, "null pointer");
  if (session ? ((p->H > 0 && !p->hist_x) || session_pointers_missing(p))
              : (!p->pool_ptr || !p->entity_params || !p->bias_params || !p->scalars || (p->H > 0 && !p->hist_ptr) ||
                 (p->P > 0 && !p->out_pool_score)))
    return fail(VFM_E_INVALID, "null pointer");
  return check_exact_operands(p, p->n_ops > 0, "workspace too small (vfm_design_workspace_bytes)");
}

// the kernel arguments of both entry points; returns the grid of the session kernel
unsigned design_args(const vfm_design_t* p, bool session, DesignArgs& s) {
  const unsigned grid = exact_session_args(p, session, 0, s);
  s.n_targets = p->n_targets; s.tgt_ptr = p->tgt_ptr; s.tgt_op = p->tgt_op;
  s.out_pool_score = p->out_pool_score;
  return grid;
}

}  // namespace
}  // namespace vfm

static int design_scores_call(const vfm_design_t* p, const float* prior, void* stream);
static int design_elicit_call(const vfm_design_t* p, const float* prior, void* stream);

extern "C" {

int64_t vfm_design_workspace_bytes(int64_t U, int64_t P, int64_t n_ops, int32_t d, int32_t lds_dim) {
  return vfm::exact_session_workspace_bytes(U, P, n_ops, d, lds_dim);
}

int64_t vfm_design_prior_workspace_bytes(int64_t U, int64_t P, int64_t n_ops, int32_t d, int32_t lds_dim) {
  return vfm_design_workspace_bytes(U, P, n_ops, d, lds_dim);          // (the prior lives in LDS, not in the workspace)
}

int vfm_design_scores_f32(const vfm_design_t* p, void* stream) { return design_scores_call(p, nullptr, stream); }

int vfm_design_scores_prior_f32(const vfm_design_t* p, const float* prior, void* stream) {
  return design_scores_call(p, prior, stream);
}

int vfm_design_elicit_f32(const vfm_design_t* p, void* stream) { return design_elicit_call(p, nullptr, stream); }

int vfm_design_elicit_prior_f32(const vfm_design_t* p, const float* prior, void* stream) {
  return design_elicit_call(p, prior, stream);
}

}  // extern "C"

// both one-round entry points: prior == NULL is vfm_design_scores_f32
static int design_scores_call(const vfm_design_t* p, const float* prior, void* stream) {
  using namespace vfm;
  if (int rc = check_design(p, false, "vfm_design_scores_f32: NULL argument struct")) return rc;
  if (p->U == 0 || p->P == 0) return 0;
  const hipStream_t st = (hipStream_t)stream;
  const bool sp = (p->flags & VFM_FLAG_LINK_SOFTPLUS) != 0;
  DesignArgs s;
  design_args(p, false, s);              // (no system is solved: the session's grid and slabs are not used)
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
    if (prior)
      hipLaunchKernelGGL(k_design_score_prior<decltype(link)::value>, dim3(grid), dim3(FB),
                         (size_t)(3 * f.d + 2 * (f.d + 1)) * 8, st, s, prior);
    else
      hipLaunchKernelGGL(k_design_score<decltype(link)::value>, dim3(grid), dim3(FB), (size_t)3 * f.d * 8, st, s);
    rc = launch_status("k_design_score");
  });
  return rc;
}

// both session entry points: prior == NULL is vfm_design_elicit_f32
static int design_elicit_call(const vfm_design_t* p, const float* prior, void* stream) {
  using namespace vfm;
  if (int rc = check_design(p, true, "vfm_design_elicit_f32: NULL argument struct")) return rc;
  if (p->U == 0) return 0;
  const hipStream_t st = (hipStream_t)stream;
  const bool sp = (p->flags & VFM_FLAG_LINK_SOFTPLUS) != 0;
  DesignArgs s;
  const unsigned grid = design_args(p, true, s);
  if (int rc = launch_exact_session_preps(p, sp, s, st)) return rc;
  if (prior) {
    launch_exact_session<DesignScoreT<true>>(sp, s, grid, st, [](auto w, auto c, auto link) {
      return k_elicit_design_prior<decltype(w)::value, decltype(c)::value, decltype(link)::value>;
    }, 2 * (int64_t)(p->d + 1), prior);
  } else {
    launch_exact_session<DesignScore>(sp, s, grid, st, [](auto w, auto c, auto link) {
      return k_elicit_design<decltype(w)::value, decltype(c)::value, decltype(link)::value>;
    });
  }
  return launch_status("k_elicit_design");
}

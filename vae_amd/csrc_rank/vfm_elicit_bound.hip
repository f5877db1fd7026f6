// vfm_elicit_bound.hip -- the bound field-form elicitation session (include/vfm_bound.h: vfm_elicit_bound_f32): ask,
// run the Jaakkola-Jordan rounds of the respondent's bound, ask again -- every round of every respondent of a 'class'
// model in one launch.
//
// k_elicit_bound<W, CPL, LINK> is the session loop of vfm_elicit_exact_body.hpp (exact_session: the layout, the choice,
// the operand passes and the host path are there) with MomentScore (vfm_elicit_moment_score.hpp: k_elicit_solve's
// scores) and BoundFold where k_elicit_solve has SolveFold: the fold of a round is bound_body of
// vfm_foldin_bound_body.hpp, k_foldin_bound's per-entity work, started at theta_e in LDS (the fp32 posterior the round
// was scored from) instead of a table row.  The scales of the iterate sit behind the LDS triangle as in k_foldin_bound;
// respondent g's row weights at wrow[h0 + g Q + i] for fold row i, a range no other workgroup touches while hist_ptr
// does not decrease.
//
// vfm_elicit_bound_prior_f32 (include/vfm_elicit_prior.h) runs k_elicit_bound_prior, the PRIOR = true instantiation of the
// same session loop: the respondents' field prior staged in LDS in front, bound_body<.., true> as the fold (still from
// theta_e: prior_start stays false, `reset` is the session's own prior row), one more pointer among the kernel's
// arguments; k_elicit_bound is the instantiation without it, unchanged.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "vfm_args.hpp"
#include "vfm_bound.h"
#include "vfm_elicit_prior.h"
#include "vfm_launch.hpp"            // launch_status
#include "vfm_rank_tile.hpp"         // score_of, philox_uniform, link_of
#include "vfm_field_ctx.hpp"         // ctx_valid, field_chain_moments

namespace vfm {
namespace {
#include "vfm_rng.hpp"
#include "vfm_common.hpp"
#include "vfm_foldin_body.hpp"       // FoldArgs, k_foldin_prep, fold_stage_rows, the host side
#include "vfm_foldin_solve_body.hpp" // chol_solve, put_params, k_foldin_solve_prep, the operand block and the slabs
#include "vfm_foldin_bound_body.hpp" // bound_body, k_foldin_bound_prep
#include "vfm_elicit_host.hpp"       // the checks the session entry points share
#include "vfm_elicit_field_score.hpp" // k_elicit_ctx_prep, ElicitFieldArgs, FieldSessionRows, the score's operand views
#include "vfm_elicit_exact_body.hpp" // ElicitSolveArgs, exact_session, the host side of the exact sessions
#include "vfm_elicit_moment_score.hpp" // MomentScore

struct ElicitBoundArgs : ElicitSolveArgs {   // (e.f.n_steps: the rounds of the bound per fold)
  const double* cv64;                    // [n_ops]        c_var
  double* wrow;                          // [H + U Q]      w_r of the round in flight
};

// the fold of a round: n_iters rounds of the bound from theta_e
struct BoundFold {
  static constexpr bool ALL_PAIRS = false;
  __host__ __device__ static int64_t lds_doubles(int d) { return d + 1; }
  template <int W, int CPL, int LINK, bool PRIOR, class Rows, class Store>
  __device__ __forceinline__ static void run(const ElicitBoundArgs& s, const FoldArgs& f, const Rows& rows, int64_t n,
                                             int64_t g, double* sm, double* Hm, double* sg2, float, double, float* loss,
                                             Store&& store, const double* pr) {
    bound_body<W, CPL, LINK, PRIOR>(f, s.ops64, s.cm64, s.cv64, s.wrow + rows.h0 + g * s.e.Q, rows, n, false, sm, Hm, sg2,
                                    loss, store, pr);
  }
};

template <int W, int CPL, int LINK>
__global__ __launch_bounds__(FB) void k_elicit_bound(const ElicitBoundArgs s) {
  exact_session<MomentScore, W, CPL, LINK, BoundFold>(s);
}

template <int W, int CPL, int LINK>
__global__ __launch_bounds__(FB) void k_elicit_bound_prior(const ElicitBoundArgs s, const float* __restrict__ prior) {
  exact_session<MomentScore, W, CPL, LINK, BoundFold, true>(s, prior);
}

// workspace: [the exact session's parts up to its slabs | c_var | the row weights | the slabs]
inline int64_t off_bound_cv(int64_t P, int64_t n_ops, int d) { return off_fold(P, n_ops, d) + off_slabs(n_ops, d); }
inline int64_t off_bound_wrow(int64_t P, int64_t n_ops, int d) { return off_bound_cv(P, n_ops, d) + round_up(n_ops * 8, 256); }
inline int64_t off_session_slabs(int64_t U, int64_t P, int64_t H, int64_t n_ops, int d, int Q) {
  return off_bound_wrow(P, n_ops, d) + round_up((H + U * Q) * 8, 256);
}

}  // namespace
}  // namespace vfm

static int elicit_bound_call(const vfm_elicit_bound_t* p, const float* prior, void* stream);

extern "C" {

int64_t vfm_elicit_bound_workspace_bytes(int64_t U, int64_t P, int64_t H, int64_t n_ops, int32_t d, int32_t n_rounds,
                                         int32_t lds_dim) {
  if (U < 0 || P < 0 || H < 0 || n_ops < 0 || d < 1 || d > VFM_FOLDIN_MAX_D || n_rounds < 0 ||
      n_rounds > VFM_ELICIT_MAX_ROUNDS || lds_dim < -1)
    return VFM_E_INVALID;
  return vfm::off_session_slabs(U, P, H, n_ops, d, n_rounds) + vfm::slabs_bytes(U, d, lds_dim);
}

int64_t vfm_elicit_bound_prior_workspace_bytes(int64_t U, int64_t P, int64_t H, int64_t n_ops, int32_t d,
                                               int32_t n_rounds, int32_t lds_dim) {
  return vfm_elicit_bound_workspace_bytes(U, P, H, n_ops, d, n_rounds, lds_dim);     // (the prior lives in LDS)
}

int vfm_elicit_bound_f32(const vfm_elicit_bound_t* p, void* stream) { return elicit_bound_call(p, nullptr, stream); }

int vfm_elicit_bound_prior_f32(const vfm_elicit_bound_t* p, const float* prior, void* stream) {
  return elicit_bound_call(p, prior, stream);
}

}  // extern "C"

// both entry points: prior == NULL is vfm_elicit_bound_f32
static int elicit_bound_call(const vfm_elicit_bound_t* p, const float* prior, void* stream) {
  using namespace vfm;
  if (int rc = check_session_struct(
          p, "vfm_elicit_bound_f32: NULL argument struct",
          "vfm_elicit_bound_t: struct_size / abi_version differ from this library's (VFM_STRUCT_INIT)"))
    return rc;
  if (int rc = check_exact_field(p)) return rc;
  if (p->key_col < 0 || p->key_col >= p->F || p->key_col == p->field)
    return fail(VFM_E_INVALID, "key_col must be a context column: in [0,F) and not field");
  if (int rc = check_exact_sizes(p, true, "U < 0, P < 0 or H < 0", true)) return rc;
  if (p->strategy < VFM_RANK_TOP || p->strategy > VFM_RANK_RANDOM) return fail(VFM_E_INVALID, "unknown strategy");
  if (int rc = check_exact_options(
          p, p->P + p->H, "kl_weight must be > 0 and finite (the prior is what makes the system positive definite)", true))
    return rc;
  if (p->n_iters < 1) return fail(VFM_E_INVALID, "n_iters must be >= 1");
  if (p->U == 0) return 0;
  if (!p->entities || (p->P > 0 && !p->pool_x) || (p->H > 0 && !p->hist_x) || session_pointers_missing(p))
    return fail(VFM_E_INVALID, "null pointer");
  if ((p->P + p->H > 0 && !p->op_x) || (p->P > 0 && !p->pool_op) || (p->H > 0 && !p->hist_op))
    return fail(VFM_E_INVALID, "op_x, pool_op and hist_op needed");
  if (int rc = check_session_workspace(
          p, vfm_elicit_bound_workspace_bytes(p->U, p->P, p->H, p->n_ops, p->d, p->n_rounds, p->lds_dim),
          "workspace too small (vfm_elicit_bound_workspace_bytes)"))
    return rc;

  const hipStream_t st = (hipStream_t)stream;
  const bool sp = (p->flags & VFM_FLAG_LINK_SOFTPLUS) != 0;
  ElicitBoundArgs s;
  exact_session_args(p, true, p->seed, s);
  s.e.strat = p->strategy; s.e.key_col = p->key_col;
  s.e.f.n_steps = p->n_iters;
  char* w = (char*)p->workspace;
  double* cv64 = (double*)(w + off_bound_cv(p->P, p->n_ops, p->d));
  s.cv64 = cv64;
  s.wrow = (double*)(w + off_bound_wrow(p->P, p->n_ops, p->d));
  const unsigned grid = place_slabs(p->d, p->lds_dim, p->U,
                                    w + off_session_slabs(p->U, p->P, p->H, p->n_ops, p->d, p->n_rounds),
                                    (int64_t)1 << 20, s.sl);
  if (int rc = launch_exact_session_preps(p, sp, s, st)) return rc;
  if (p->n_ops > 0)
    if (int rc = launch_bound_prep(sp, s.e.f, p->n_ops, p->op_x, cv64, st)) return rc;
  if (prior) {
    launch_exact_session<MomentScore, BoundFold>(sp, s, grid, st, [](auto w_, auto c, auto link) {
      return k_elicit_bound_prior<decltype(w_)::value, decltype(c)::value, decltype(link)::value>;
    }, 2 * (int64_t)(p->d + 1), prior);
  } else {
    launch_exact_session<MomentScore, BoundFold>(sp, s, grid, st, [](auto w_, auto c, auto link) {
      return k_elicit_bound<decltype(w_)::value, decltype(c)::value, decltype(link)::value>;
    });
  }
  return launch_status("k_elicit_bound");
}

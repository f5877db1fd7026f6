// vfm_elicit_solve.hip -- the exact field-form elicitation session (include/vfm_elicit.h: vfm_elicit_solve_f32): ask,
// solve the respondent's closed-form optimum, ask again -- every round of every respondent in one launch.
//
// k_elicit_solve<W, CPL, LINK> is the session loop of vfm_elicit_exact_body.hpp (exact_session: the layout, the choice,
// the fold-in by solve_body, the operand passes and the host path are there) with MomentScore: a pool row is scored
// whole by its predictive moments at theta_e (field_chain_moments / score_of / philox_uniform: vfm_elicit_field.hip's
// scores, bit for bit), whose candidate operands are therefore refreshed every round.  The score keeps nothing in LDS
// and writes none of solve_body's, so a round ends without a barrier.
//
// vfm_elicit_solve_prior_f32 (include/vfm_elicit_prior.h) runs k_elicit_solve_prior, the PRIOR = true instantiation of the
// same session loop: the respondents' field prior staged in LDS in front, one more pointer among the kernel's
// arguments; k_elicit_solve is the instantiation without it, unchanged.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "vfm_args.hpp"
#include "vfm_elicit.h"
#include "vfm_elicit_prior.h"
#include "vfm_launch.hpp"            // launch_status
#include "vfm_rank_tile.hpp"         // score_of, philox_uniform, link_of
#include "vfm_field_ctx.hpp"         // ctx_valid, field_chain_moments

namespace vfm {
namespace {
#include "vfm_rng.hpp"
#include "vfm_common.hpp"
#include "vfm_foldin_body.hpp"       // FoldArgs, k_foldin_prep, fold_stage_rows, the host side
#include "vfm_foldin_solve_body.hpp" // solve_body, k_foldin_solve_prep, the operand block and the slabs
#include "vfm_elicit_host.hpp"       // the checks the session entry points share
#include "vfm_elicit_field_score.hpp" // k_elicit_ctx_prep, ElicitFieldArgs, FieldSessionRows, the score's operand views
#include "vfm_elicit_exact_body.hpp" // ElicitSolveArgs, exact_session, the host side of the exact sessions
#include "vfm_elicit_moment_score.hpp" // MomentScore

template <int W, int CPL, int LINK>
__global__ __launch_bounds__(FB) void k_elicit_solve(const ElicitSolveArgs s) {
  exact_session<MomentScore, W, CPL, LINK>(s);
}

template <int W, int CPL, int LINK>
__global__ __launch_bounds__(FB) void k_elicit_solve_prior(const ElicitSolveArgs s, const float* __restrict__ prior) {
  exact_session<MomentScore, W, CPL, LINK, SolveFold, true>(s, prior);
}

}  // namespace
}  // namespace vfm

static int elicit_solve_call(const vfm_elicit_solve_t* p, const float* prior, void* stream);

extern "C" {

int64_t vfm_elicit_solve_workspace_bytes(int64_t U, int64_t P, int64_t n_ops, int32_t d, int32_t lds_dim) {
  return vfm::exact_session_workspace_bytes(U, P, n_ops, d, lds_dim);
}

int64_t vfm_elicit_solve_prior_workspace_bytes(int64_t U, int64_t P, int64_t n_ops, int32_t d, int32_t lds_dim) {
  return vfm_elicit_solve_workspace_bytes(U, P, n_ops, d, lds_dim);    // (the prior lives in LDS, not in the workspace)
}

int vfm_elicit_solve_f32(const vfm_elicit_solve_t* p, void* stream) { return elicit_solve_call(p, nullptr, stream); }

int vfm_elicit_solve_prior_f32(const vfm_elicit_solve_t* p, const float* prior, void* stream) {
  return elicit_solve_call(p, prior, stream);
}

}  // extern "C"

// both entry points: prior == NULL is vfm_elicit_solve_f32
static int elicit_solve_call(const vfm_elicit_solve_t* p, const float* prior, void* stream) {
  using namespace vfm;
  if (int rc = check_session_struct(
          p, "vfm_elicit_solve_f32: NULL argument struct",
          "vfm_elicit_solve_t: struct_size / abi_version differ from this library's (VFM_STRUCT_INIT)"))
    return rc;
  if (int rc = check_exact_field(p)) return rc;
  if (p->key_col < 0 || p->key_col >= p->F || p->key_col == p->field)
    return fail(VFM_E_INVALID, "key_col must be a context column: in [0,F) and not field");
  if (int rc = check_exact_sizes(p, true, "U < 0, P < 0 or H < 0", true)) return rc;
  if (p->strategy < VFM_RANK_TOP || p->strategy > VFM_RANK_RANDOM) return fail(VFM_E_INVALID, "unknown strategy");
  if (int rc = check_exact_options(
          p, p->P + p->H, "kl_weight must be > 0 and finite (the prior is what makes the system positive definite)", true))
    return rc;
  if (p->U == 0) return 0;
  if (!p->entities || (p->P > 0 && !p->pool_x) || (p->H > 0 && !p->hist_x) || session_pointers_missing(p))
    return fail(VFM_E_INVALID, "null pointer");
  if (int rc = check_exact_operands(p, p->P + p->H > 0, "workspace too small (vfm_elicit_solve_workspace_bytes)")) return rc;

  const hipStream_t st = (hipStream_t)stream;
  const bool sp = (p->flags & VFM_FLAG_LINK_SOFTPLUS) != 0;
  ElicitSolveArgs s;
  const unsigned grid = exact_session_args(p, true, p->seed, s);
  s.e.strat = p->strategy; s.e.key_col = p->key_col;
  if (int rc = launch_exact_session_preps(p, sp, s, st)) return rc;
  if (prior) {
    launch_exact_session<MomentScore>(sp, s, grid, st, [](auto w, auto c, auto link) {
      return k_elicit_solve_prior<decltype(w)::value, decltype(c)::value, decltype(link)::value>;
    }, 2 * (int64_t)(p->d + 1), prior);
  } else {
    launch_exact_session<MomentScore>(sp, s, grid, st, [](auto w, auto c, auto link) {
      return k_elicit_solve<decltype(w)::value, decltype(c)::value, decltype(link)::value>;
    });
  }
  return launch_status("k_elicit_solve");
}

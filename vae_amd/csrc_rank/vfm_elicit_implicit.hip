// vfm_elicit_implicit.hip -- the implicit field-form elicitation session (include/vfm_elicit_implicit.h:
// vfm_elicit_implicit_f32): ask, solve the respondent's optimum over every (respondent, partner) pair, ask again -- every
// round of every respondent of a two-field 'reg' model in one launch.
//
// k_elicit_implicit<W, CPL, LINK> is the session loop of vfm_elicit_exact_body.hpp (exact_session: the layout, the choice
// and the host path are there) with MomentScore (vfm_elicit_moment_score.hpp: k_elicit_solve's scores) and ImplicitFold
// where k_elicit_solve has SolveFold: the fold of a round is implicit_body of vfm_implicit_body.hpp, k_implicit_solve's
// per-entity work in its row-list form, over the respondent's history followed by the rows asked so far.  Fold row r is a
// history row (r < n_hist) or the pool row out_row[g Q + r - n_hist]; its partner is the other column of that row, its
// target hist_y / pool_y, its weight w1.  A partner's operands are read from the fp32 tables where they are used, as
// ObservedRows of vfm_implicit.hip reads them: the fold has no operand block and no k_foldin_solve_prep pass -- only
// k_elicit_ctx_prep (the score's operands) runs before the session.  The system is always the primal (d + 1) x (d + 1)
// one (ALL_PAIRS: exact_session's LDS / slab rule with m = d + 1), its base block assembled once before the call by
// vfm_implicit_base_f32: the partner field is frozen over the session.  Sums: a thread per coordinate and a thread per
// triangle element, fold rows in order, then w0 base + dw share -- k_implicit_solve's, so a round's posterior is that
// kernel's bits.  No atomics, no host sync.
//
// k_elicit_implicit_prior is the PRIOR = true instantiation of the same session loop: the respondents' field prior staged
// in LDS in front, implicit_body<.., true, ..> as the fold, one more pointer among the kernel's arguments.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "vfm_args.hpp"
#include "vfm_elicit.h"
#include "vfm_elicit_implicit.h"
#include "vfm_launch.hpp"            // launch_status
#include "vfm_rank_tile.hpp"         // score_of, philox_uniform, link_of
#include "vfm_field_ctx.hpp"         // ctx_valid, field_chain_moments

namespace vfm {
namespace {
#include "vfm_rng.hpp"
#include "vfm_common.hpp"
#include "vfm_foldin_body.hpp"       // FoldArgs, fill_fold_args, the host side
#include "vfm_foldin_solve_body.hpp" // chol_solve, put_params, the slabs
#include "vfm_implicit_body.hpp"     // implicit_body, ListShare, obs_t, obs_q
#include "vfm_elicit_host.hpp"       // the checks the session entry points share
#include "vfm_elicit_field_score.hpp" // k_elicit_ctx_prep, ElicitFieldArgs, FieldSessionRows, the score's operand views
#include "vfm_elicit_exact_body.hpp" // ElicitSolveArgs, exact_session, the host side of the exact sessions
#include "vfm_elicit_moment_score.hpp" // MomentScore

struct ElicitImplicitArgs : ElicitSolveArgs {   // (ops64, cm64, e.f.ops, e.f.opc: NULL, the fold has no operand block)
  double w0, w1;
  int64_t lo, n;                         // the partner field's id range, the range of base
  const double* base;                    // [imp_doubles(d)]
};

// is id j a partner the base block covers?
__device__ __forceinline__ bool in_base(const ElicitImplicitArgs& s, int64_t j) { return j >= s.lo && j < s.lo + s.n; }

// the observed rows of a respondent for coord_sums / list_elem: the session's fold rows, one weight w1
struct ImplicitSessionRows {
  const ElicitImplicitArgs& s;
  const FieldSessionRows& rows;
  __device__ __forceinline__ int64_t id(int64_t r) const {
    const int64_t j = rows.partner(r, 1 - s.e.f.col);
    return in_base(s, j) ? j : -1;
  }
  __device__ __forceinline__ double t(int64_t r, double cm) const { return obs_t(s.w0, s.w1, (double)rows.y(r), cm); }
  __device__ __forceinline__ double q(int64_t r, double cm, double cv) const {
    return obs_q(s.w0, s.w1, (double)rows.y(r), cm, cv);
  }
};

// the fold of a round: the optimum of the respondent's share of J_imp over its n fold rows
struct ImplicitFold {
  static constexpr bool ALL_PAIRS = true;
  __host__ __device__ static int64_t lds_doubles(int) { return 0; }
  __device__ __forceinline__ static bool pool_ok(const ElicitImplicitArgs& s, int64_t row) {
    return in_base(s, s.e.pool_x[row * s.e.f.F + (1 - s.e.f.col)]);
  }
  template <int W, int CPL, int LINK, bool PRIOR, class Rows, class Store>
  __device__ __forceinline__ static void run(const ElicitImplicitArgs& s, const FoldArgs& f, const Rows& rows, int64_t n,
                                             int64_t, double* sm, double* Hm, double*, float, double prec, float* loss,
                                             Store&& store, const double* pr) {
    const ImplicitSessionRows irows{s, rows};
    implicit_body<LINK, PRIOR, false>(ListShare<LINK, false, FoldArgs, ImplicitSessionRows>{f, irows, n}, f.d, s.base,
                                      (double)f.klw, s.w0, s.w1 - s.w0, prec, sm, Hm, loss, store, pr);
  }
};

template <int W, int CPL, int LINK>
__global__ __launch_bounds__(FB) void k_elicit_implicit(const ElicitImplicitArgs s) {
  exact_session<MomentScore, W, CPL, LINK, ImplicitFold>(s);
}

template <int W, int CPL, int LINK>
__global__ __launch_bounds__(FB) void k_elicit_implicit_prior(const ElicitImplicitArgs s, const float* __restrict__ prior) {
  exact_session<MomentScore, W, CPL, LINK, ImplicitFold, true>(s, prior);
}

}  // namespace
}  // namespace vfm

extern "C" {

// workspace: [asked flags | the moments' operands | their constants | the slabs]
int64_t vfm_elicit_implicit_workspace_bytes(int64_t U, int64_t P, int64_t n_ops, int32_t d, int32_t lds_dim) {
  if (U < 0 || P < 0 || n_ops < 0 || d < 1 || d > VFM_FOLDIN_MAX_D || lds_dim < -1) return VFM_E_INVALID;
  return vfm::off_fold(P, n_ops, d) + vfm::slabs_bytes(U, d, lds_dim);
}

int vfm_elicit_implicit_f32(const vfm_elicit_solve_t* p, const vfm_elicit_implicit_t* imp, const float* prior,
                            void* stream) {
  using namespace vfm;
  if (int rc = check_session_struct(
          p, "vfm_elicit_implicit_f32: NULL argument struct",
          "vfm_elicit_solve_t: struct_size / abi_version differ from this library's (VFM_STRUCT_INIT)"))
    return rc;
  if (int rc = check_exact_field(p)) return rc;
  if (p->F != 2) return fail(VFM_E_INVALID, "the implicit session needs a two-field model (F = 2)");
  if (p->key_col < 0 || p->key_col >= p->F || p->key_col == p->field)
    return fail(VFM_E_INVALID, "key_col must be a context column: in [0,F) and not field");
  if (int rc = check_exact_sizes(p, true, "U < 0, P < 0 or H < 0", true)) return rc;
  if (p->strategy < VFM_RANK_TOP || p->strategy > VFM_RANK_RANDOM) return fail(VFM_E_INVALID, "unknown strategy");
  if (int rc = check_exact_options(
          p, p->P + p->H, "kl_weight must be > 0 and finite (the prior is what makes the system positive definite)", true))
    return rc;
  if (!imp) return fail(VFM_E_INVALID, "vfm_elicit_implicit_f32: NULL vfm_elicit_implicit_t");
  if (!(imp->w0 > 0.f) || !(imp->w0 <= 3.0e38f)) return fail(VFM_E_INVALID, "w0 must be > 0 and finite");
  if (!(imp->w1 >= imp->w0) || !(imp->w1 <= 3.0e38f)) return fail(VFM_E_INVALID, "w1 must be >= w0 and finite");
  if (imp->n < 1 || imp->lo < 0 || imp->lo > p->T || imp->n > p->T - imp->lo)
    return fail(VFM_E_INVALID, "the partner range [lo, lo + n) must lie in [0, T) with n >= 1");
  if (!imp->base) return fail(VFM_E_INVALID, "null pointer (base)");
  if (p->U == 0) return 0;
  if (!p->entities || (p->P > 0 && !p->pool_x) || (p->H > 0 && !p->hist_x) || session_pointers_missing(p))
    return fail(VFM_E_INVALID, "null pointer");
  if ((p->P + p->H > 0 && !p->op_x) || (p->P > 0 && !p->pool_op) || (p->H > 0 && !p->hist_op))
    return fail(VFM_E_INVALID, "op_x, pool_op and hist_op needed");
  if (int rc = check_session_workspace(p, vfm_elicit_implicit_workspace_bytes(p->U, p->P, p->n_ops, p->d, p->lds_dim),
                                       "workspace too small (vfm_elicit_implicit_workspace_bytes)"))
    return rc;

  const hipStream_t st = (hipStream_t)stream;
  const bool sp = (p->flags & VFM_FLAG_LINK_SOFTPLUS) != 0;
  ElicitImplicitArgs s;
  const unsigned grid = exact_session_args(p, true, p->seed, s, false);     // (no operand block)
  s.e.strat = p->strategy; s.e.key_col = p->key_col;
  s.w0 = imp->w0; s.w1 = imp->w1; s.lo = imp->lo; s.n = imp->n; s.base = imp->base;
  if (p->n_ops > 0) {
    const unsigned nb = (unsigned)((p->n_ops + NW - 1) / NW);
    hipLaunchKernelGGL(k_elicit_ctx_prep, dim3(nb), dim3(FB), 0, st, p->n_ops, p->op_x, (int)p->F, (int)p->field, p->T,
                       (int)p->d, sp, p->entity_params, p->bias_params, p->scalars, (float*)s.e.sop, (float*)s.e.soc);
    if (int rc = launch_status("k_elicit_ctx_prep")) return rc;
  }
  if (prior) {
    launch_exact_session<MomentScore, ImplicitFold>(sp, s, grid, st, [](auto w, auto c, auto link) {
      return k_elicit_implicit_prior<decltype(w)::value, decltype(c)::value, decltype(link)::value>;
    }, 2 * (int64_t)(p->d + 1), prior);
  } else {
    launch_exact_session<MomentScore, ImplicitFold>(sp, s, grid, st, [](auto w, auto c, auto link) {
      return k_elicit_implicit<decltype(w)::value, decltype(c)::value, decltype(link)::value>;
    });
  }
  return launch_status("k_elicit_implicit");
}

}  // extern "C"

// vfm_foldin_solve.hip -- exact fold-in (include/vfm_foldin.h, vfm_foldin_solve_f32): the closed-form optimum of every
// folded entity in one launch.
//
// k_foldin_solve: one workgroup of FB threads per entity (a grid-stride loop over the entities).  Phases A-E are
//   solve_body of vfm_foldin_solve_body.hpp, which the exact elicitation sessions (vfm_elicit_exact_body.hpp) run on a
//   respondent's rows round after round.  Per entity, with the
//   row operands M_r, A_r, C_r, c_mean,r in fp64 (k_foldin_solve_prep: k_foldin_prep's sums, kept unrounded, with the
//   links in fp64 -- rounded to fp32 they would move the optimum by about 1e-7, more than the last fp32 bit of the rows
//   written) and everything in fp64:
//   A  a thread per coordinate walks the entity's rows in row-list order: D = kl + prec sum_r A_r, b, sum_r (A_r + M_r^2)
//   B  the system: n <= d rows -> the dual K = I / prec + U D^-1 U^T [n, n] (a wave per pair of rows, lanes over the
//      coordinates) with right-hand side U D^-1 b; more rows -> the primal H [d + 1, d + 1] (a thread per element, rows
//      in order) with right-hand side b.  Packed lower triangle, in LDS while it fits, else in the workgroup's slab.
//   C  Cholesky, left-looking, a thread per row, one barrier per column; the right-hand side rides along as one more
//      row, so the forward substitution is part of the factorisation.  Then the backward substitution, column by column.
//   D  theta (dual: D^-1 b - D^-1 U^T z), the scales from their closed forms, rounded to fp32 and written.
//   E  wave 0 evaluates L_e at the written fp32 parameters: the closed form of fold_run's final pass restated (fp32
//      chains in row order, the same lane groups), so the loss is comparable with vfm_foldin_f32's.
// Every sum has a fixed order that depends on the entity's rows alone: no atomics, no host sync, the same bits
// whichever other entities share the launch and wherever the triangle lives.
//
// vfm_foldin_solve_prior_f32 (include/vfm_prior.h) is the PRIOR = true instantiation of the same kernel: the folded
// field's prior [2, d + 1] = mean | precision is staged once per workgroup in fp64 in LDS in front of solve_body's
// vectors; the instantiation without it is the parent's, unchanged.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "vfm_args.hpp"
#include "vfm_foldin.h"
#include "vfm_prior.h"
#include "vfm_launch.hpp"            // launch_status

namespace vfm {
namespace {
#include "vfm_rng.hpp"
#include "vfm_common.hpp"

#include "vfm_foldin_body.hpp"       // FoldArgs, k_foldin_prep, fold_stage_rows, the host side
#include "vfm_foldin_solve_body.hpp" // solve_body (phases A-E), k_foldin_solve_prep, the operand block and the slabs

struct SolveArgs {
  FoldArgs f;                            // (cap = 0: fold_stage_rows stages nothing; f.ops / f.opc: the fp32 operands of the loss)
  const double* ops64;                   // [n_ops, 3, d]  M | A | C, unrounded
  const double* cm64;                    // [n_ops]        c_mean
  SolveSlabs sl;                         // the slabs and the LDS rule of the triangle
  const float* prior;                    // [2, d + 1] mean | precision of the folded field (PRIOR instantiations only)
};

template <int W, int CPL, int LINK, bool PRIOR>
__global__ __launch_bounds__(FB) void k_foldin_solve(const SolveArgs s) {
#pragma clang fp contract(on)
  extern __shared__ double sm_all[];
  const FoldArgs& a = s.f;
  const int tid = threadIdx.x;
  const int d = a.d, d1 = d + 1;
  double* sm = sm_all + (PRIOR ? 2 * d1 : 0);              // (the prior in front: lds_doubles_prior)
  const double* pr = PRIOR ? sm_all : nullptr;
  if constexpr (PRIOR) {
    stage_prior(s.prior, sm_all, d1);
    __syncthreads();
  }
  double* Hl = sm + 8 * d1;              // (past solve_body's vectors and fp32 parameters)
  double* Hg = s.sl.slab ? s.sl.slab + (int64_t)blockIdx.x * s.sl.slab_elems : nullptr;
  const float precf = link_f<LINK>(a.scal[0]);
  const double prec = link_d<LINK>(a.scal[0]);

  for (int64_t g = blockIdx.x; g < a.E; g += gridDim.x) {
    const int64_t r0 = min(max(a.ptr[g], (int64_t)0), a.R);
    const int64_t n = min(max(a.ptr[g + 1], r0), a.R) - r0;
    const int64_t e = a.ent[g];
    const int m = solve_dim(n, d);
    double* Hm = m <= s.sl.cap_dim ? Hl : Hg;
    if (e < 0 || e >= a.T || !Hm) {      // (block-uniform)
      if (tid == 0) a.loss[g] = __builtin_nanf("");
      continue;
    }
    const ListRows rows{a, r0};
    // phases A-E (vfm_foldin_solve_body.hpp); the table row is written where the parameters are published
    solve_body<W, CPL, LINK, PRIOR>(a, s.ops64, s.cm64, rows, n, sm, Hm, precf, prec, a.loss + g, [&](const float* pf) {
      for (int k = tid; k < d; k += FB) {
        a.entity[e * 2 * d + k] = pf[1 + k];
        a.entity[e * 2 * d + d + k] = pf[d1 + 1 + k];
      }
      if (tid == 0) {
        a.bias[e * 2] = pf[0];
        a.bias[e * 2 + 1] = pf[d1];
      }
    }, pr);
    __syncthreads();                     // (pf is rewritten by the next entity)
  }
}

template <bool PRIOR>
void launch(const FShape& f, bool sp, const SolveArgs& s, unsigned grid, size_t shm, hipStream_t st) {
  for_link(sp, [&](auto link) {
    for_shape(f, [&](auto w, auto c) {
      launch_lds(k_foldin_solve<decltype(w)::value, decltype(c)::value, decltype(link)::value, PRIOR>, grid, shm, st, s);
    });
  });
}

}  // namespace
}  // namespace vfm

static int solve_call(const vfm_foldin_solve_t* p, const float* prior, void* stream);

extern "C" {

int64_t vfm_foldin_solve_workspace_bytes(int64_t E, int64_t n_ops, int32_t d, int32_t lds_dim) {
  if (E < 0 || n_ops < 0 || d < 1 || d > VFM_FOLDIN_MAX_D || lds_dim < -1) return VFM_E_INVALID;
  return vfm::off_slabs(n_ops, d) + vfm::slabs_bytes(E, d, lds_dim);
}

int64_t vfm_foldin_solve_prior_workspace_bytes(int64_t E, int64_t n_ops, int32_t d, int32_t lds_dim) {
  return vfm_foldin_solve_workspace_bytes(E, n_ops, d, lds_dim);       // (the prior lives in LDS, not in the workspace)
}

int vfm_foldin_solve_f32(const vfm_foldin_solve_t* p, void* stream) { return solve_call(p, nullptr, stream); }

int vfm_foldin_solve_prior_f32(const vfm_foldin_solve_t* p, const float* prior, void* stream) {
  return solve_call(p, prior, stream);
}

}  // extern "C"

// both entry points: prior == NULL is vfm_foldin_solve_f32
static int solve_call(const vfm_foldin_solve_t* p, const float* prior, void* stream) {
  if (!p) return vfm::fail(VFM_E_INVALID, "vfm_foldin_solve_f32: NULL argument struct");
  const int64_t ws = vfm_foldin_solve_workspace_bytes(p->E, p->n_ops, p->d, p->lds_dim);
  const auto own = [&]() -> const char* {
    if (p->objective != VFM_OBJ_CLOSED_FORM)
      return "the exact fold-in solves the closed-form objective only (VFM_OBJ_CLOSED_FORM)";
    return p->likelihood != VFM_LIK_NORMAL ? "the closed form needs the Normal likelihood" : nullptr;
  };
  if (int rc = vfm::check_solve(p, p->row_ptr, true, ws, "vfm_foldin_solve_workspace_bytes", own)) return rc;
  if (p->E == 0) return 0;

  const hipStream_t st = (hipStream_t)stream;
  const bool sp = (p->flags & VFM_FLAG_LINK_SOFTPLUS) != 0;
  const vfm::FShape f = vfm::shape_of(p->d);
  vfm::SolveArgs s;
  vfm::fill_solve_args(s, p, VFM_LIK_NORMAL, 0, 0, VFM_FOLDIN_FIT);
  s.f.ptr = p->row_ptr;
  char* w = (char*)p->workspace;
  const unsigned grid =
      vfm::place_slabs(p->d, p->lds_dim, p->E, w + vfm::off_slabs(p->n_ops, p->d), (int64_t)1 << 20, s.sl);
  s.prior = prior;
  const size_t shm = (size_t)(prior ? vfm::lds_doubles_prior(p->d, s.sl.cap_dim) : vfm::lds_doubles(p->d, s.sl.cap_dim)) * 8;

  if (p->n_ops > 0) {
    if (int rc = vfm::launch_solve_preps(sp, s.f, p->n_ops, p->op_x, w, st)) return rc;
  }
  if (prior) vfm::launch<true>(f, sp, s, grid, shm, st);
  else vfm::launch<false>(f, sp, s, grid, shm, st);
  return launch_status("k_foldin_solve");
}

// vfm_foldin_bound.hip -- bound fold-in (include/vfm_bound.h, vfm_foldin_bound_f32): the fold-in of a 'class' model by
// exact solves of the Jaakkola-Jordan bound of the Bernoulli likelihood, every folded entity in one launch.
//
// k_foldin_bound_prep: c_var of operand o in fp64 -- k_foldin_prep's sum, not rounded to fp32, the links of the fp32
//   table values in fp64, summed as k_foldin_solve_prep sums c_mean (a thread per operand, the coordinates in order).
// k_foldin_bound: one workgroup of FB threads per entity (a grid-stride loop over the entities, the slab cap of
//   k_foldin_solve).  The iterate theta [d + 1], sigma_w^2, sigma_k^2 [d] stays in LDS in fp64 for all rounds.  Per round:
//   X  a wave per row, lanes over the coordinates: E f_r and Var f_r from the fp64 operands (wave_sum_d, a fixed
//      butterfly), xi_r^2 = (E f_r)^2 + Var f_r, w_r = tanh(xi_r / 2) / (2 xi_r) (the series below 1e-3) -> the workspace
//      at the row's own index
//   A  a thread per coordinate walks the rows in row-list order: D = kl + sum_r w_r A_r, b, sum_r w_r,
//      sum_r w_r (A_r + M_r^2)
//   B  the system: n <= d rows -> the dual K = W^-1 + U D^-1 U^T (a wave per pair of rows), right-hand side U D^-1 b;
//      more rows -> the primal H = D + U^T W U (a thread per element, rows in order), right-hand side b
//   C  chol_solve of vfm_foldin_solve_body.hpp, as it stands
//   then theta (dual: D^-1 b - D^-1 U^T z) and the scales' closed forms, kept in fp64
//   After the last round:
//   D  put_params of vfm_foldin_solve_body.hpp (prec = 1: the weights are inside the sums) and the table write
//   E  wave 0 evaluates B_e at the written fp32 parameters: per row the fp32 moments of the closed-form final pass
//      (fold_stage_rows over that row alone, the same lane groups), xi = sqrtf(.), the rows added in row order in fp64.
//   VFM_FOLDIN_OBJECTIVE runs E alone, at the table row.
// The per-entity work (the start from the fp32 parameters in LDS, the rounds, D's rounding and E) is bound_body of
// vfm_foldin_bound_body.hpp, shared with the bound elicitation session (vfm_elicit_bound.hip); this kernel loads the
// entity's table row into LDS for it and writes the table row from its store step.
// Every sum has a fixed order that depends on the entity's rows and d alone: no atomics, no host sync, the same bits
// whichever other entities share the launch and wherever the triangle lives.
//
// vfm_foldin_bound_prior_f32 (include/vfm_bound_prior.h) is the PRIOR = true instantiation of the same kernel: the folded
// field's prior [2, d + 1] = mean | precision is staged once per workgroup in fp64 in LDS in front of bound_body's
// vectors; the instantiation without it is the parent's, unchanged.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "vfm_args.hpp"
#include "vfm_bound.h"
#include "vfm_bound_prior.h"
#include "vfm_launch.hpp"            // launch_status

namespace vfm {
namespace {
#include "vfm_rng.hpp"
#include "vfm_common.hpp"

#include "vfm_foldin_body.hpp"       // FoldArgs, k_foldin_prep, fold_stage_rows, the host side
#include "vfm_foldin_solve_body.hpp" // k_foldin_solve_prep, chol_solve, put_params, the operand block and the slabs
#include "vfm_foldin_bound_body.hpp" // k_foldin_bound_prep, bound_body, bound_loss

struct BoundArgs {
  FoldArgs f;                            // (cap = 0; n_steps: the rounds; f.ops / f.opc: the fp32 operands of the loss)
  const double* ops64;                   // [n_ops, 3, d]  M | A | C, unrounded
  const double* cm64;                    // [n_ops]        c_mean
  const double* cv64;                    // [n_ops]        c_var
  double* wrow;                          // [R]            w_r of the round in flight
  SolveSlabs sl;                         // the slabs and the LDS rule of the triangle
  const float* prior;                    // [2, d + 1] mean | precision of the folded field (PRIOR instantiations only)
};

template <int W, int CPL, int LINK, bool PRIOR>
__global__ __launch_bounds__(FB) void k_foldin_bound(const BoundArgs s) {
#pragma clang fp contract(on)
  extern __shared__ double sm_all[];
  const FoldArgs& a = s.f;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int d = a.d, d1 = d + 1;
  double* sm = sm_all + (PRIOR ? 2 * d1 : 0);              // (the prior in front: lds_doubles_prior's rule)
  const double* pr = PRIOR ? sm_all : nullptr;
  if constexpr (PRIOR) {
    stage_prior(s.prior, sm_all, d1);
    __syncthreads();
  }
  float* pf = (float*)(sm + 7 * d1);     // the fp32 parameters: mu_w, mu [d] | s_w, s [d]  (bound_body's)
  double* Hl = sm + 8 * d1;              // the triangle while it fits
  double* sg2 = Hl + tri(s.sl.cap_dim);  // sigma_w^2, sigma_k^2 [d]
  double* Hg = s.sl.slab ? s.sl.slab + (int64_t)blockIdx.x * s.sl.slab_elems : nullptr;

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
    float* erow = a.entity + e * 2 * (int64_t)d;

    // ---- the fp32 parameters at the entity's row: where B_e is evaluated, or where xi^(0) is taken
    if (a.mode == VFM_FOLDIN_OBJECTIVE || !a.reset) {
      for (int c = tid; c < d1; c += FB) {
        pf[c] = c ? erow[c - 1] : a.bias[e * 2];
        pf[d1 + c] = c ? erow[d + c - 1] : a.bias[e * 2 + 1];
      }
    }
    __syncthreads();

    if (a.mode == VFM_FOLDIN_OBJECTIVE) {
      if (wv == 0) bound_loss<W, CPL, LINK, PRIOR>(a, rows, n, pf, lane, a.loss + g, pr);
    } else {
      bound_body<W, CPL, LINK, PRIOR>(a, s.ops64, s.cm64, s.cv64, s.wrow + r0, rows, n, a.reset != 0, sm, Hm, sg2, a.loss + g,
                               [&](const float*) {           // the table row, rounded once
                                 for (int k = tid; k < d; k += FB) {
                                   erow[k] = pf[1 + k];
                                   erow[d + k] = pf[d1 + 1 + k];
                                 }
                                 if (tid == 0) {
                                   a.bias[e * 2] = pf[0];
                                   a.bias[e * 2 + 1] = pf[d1];
                                 }
                               }, pr);
    }
    __syncthreads();                     // (pf and the iterate are rewritten by the next entity)
  }
}

template <bool PRIOR>
void launch(const FShape& f, bool sp, const BoundArgs& s, unsigned grid, size_t shm, hipStream_t st) {
  for_link(sp, [&](auto link) {
    for_shape(f, [&](auto w, auto c) {
      launch_lds(k_foldin_bound<decltype(w)::value, decltype(c)::value, decltype(link)::value, PRIOR>, grid, shm, st, s);
    });
  });
}

}  // namespace
}  // namespace vfm

static int bound_call(const vfm_foldin_bound_t* p, const float* prior, void* stream);

extern "C" {

int64_t vfm_foldin_bound_workspace_bytes(int64_t E, int64_t R, int64_t n_ops, int32_t d, int32_t lds_dim) {
  if (E < 0 || R < 0 || n_ops < 0 || d < 1 || d > VFM_FOLDIN_MAX_D || lds_dim < -1) return VFM_E_INVALID;
  return vfm::off_bound_own(R, n_ops, d) + vfm::slabs_bytes(E, d, lds_dim);
}

int64_t vfm_foldin_bound_prior_workspace_bytes(int64_t E, int64_t R, int64_t n_ops, int32_t d, int32_t lds_dim) {
  return vfm_foldin_bound_workspace_bytes(E, R, n_ops, d, lds_dim);    // (the prior lives in LDS, not in the workspace)
}

int vfm_foldin_bound_f32(const vfm_foldin_bound_t* p, void* stream) { return bound_call(p, nullptr, stream); }

int vfm_foldin_bound_prior_f32(const vfm_foldin_bound_t* p, const float* prior, void* stream) {
  return bound_call(p, prior, stream);
}

}  // extern "C"

// both entry points: prior == NULL is vfm_foldin_bound_f32
static int bound_call(const vfm_foldin_bound_t* p, const float* prior, void* stream) {
  if (!p) return vfm::fail(VFM_E_INVALID, "vfm_foldin_bound_f32: NULL argument struct");
  const int64_t ws = vfm_foldin_bound_workspace_bytes(p->E, p->R, p->n_ops, p->d, p->lds_dim);
  const auto own = [&]() -> const char* {
    if (p->objective != VFM_OBJ_CLOSED_FORM)
      return "the bound fold-in uses the closed-form moments only (VFM_OBJ_CLOSED_FORM)";
    if (p->likelihood != VFM_LIK_BERNOULLI) return "the bound fold-in needs the Bernoulli likelihood (VFM_LIK_BERNOULLI)";
    if (p->mode != VFM_FOLDIN_FIT && p->mode != VFM_FOLDIN_OBJECTIVE) return "mode: VFM_FOLDIN_FIT or VFM_FOLDIN_OBJECTIVE";
    if (p->mode == VFM_FOLDIN_FIT && p->n_iters < 1) return "n_iters must be >= 1 for a fit";
    return p->mode == VFM_FOLDIN_OBJECTIVE && p->n_iters != 0 ? "n_iters must be 0 in VFM_FOLDIN_OBJECTIVE" : nullptr;
  };
  if (int rc = vfm::check_solve(p, p->row_ptr, true, ws, "vfm_foldin_bound_workspace_bytes", own)) return rc;
  if (p->E == 0) return 0;

  const hipStream_t st = (hipStream_t)stream;
  const bool sp = (p->flags & VFM_FLAG_LINK_SOFTPLUS) != 0;
  const vfm::FShape f = vfm::shape_of(p->d);
  vfm::BoundArgs s;
  vfm::fill_bound_args(s, p, p->mode);
  s.f.ptr = p->row_ptr;
  char* w = (char*)p->workspace;
  const unsigned grid = vfm::place_slabs(p->d, p->lds_dim, p->E, w + vfm::off_bound_own(p->R, p->n_ops, p->d),
                                         (int64_t)1 << 20, s.sl);
  s.prior = prior;
  const size_t shm = (size_t)(vfm::bound_lds_doubles(p->d, s.sl.cap_dim) + (prior ? 2 * (int64_t)(p->d + 1) : 0)) * 8;

  if (p->n_ops > 0) {
    if (int rc = vfm::launch_solve_preps(sp, s.f, p->n_ops, p->op_x, w, st)) return rc;
    if (int rc = vfm::launch_bound_prep(sp, s.f, p->n_ops, p->op_x, const_cast<double*>(s.cv64), st)) return rc;
  }
  if (prior) vfm::launch<true>(f, sp, s, grid, shm, st);
  else vfm::launch<false>(f, sp, s, grid, shm, st);
  return launch_status("k_foldin_bound");
}

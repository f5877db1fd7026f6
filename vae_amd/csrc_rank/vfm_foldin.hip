// vfm_foldin.hip -- fold-in (include/vfm_foldin.h): fit chosen entities' variational factors with the model frozen.
//
// k_foldin_prep (closed form only): one thread per distinct frozen-partner tuple; the tuple's row operand
//   M = E S_Q, A = Var S_Q, C = 2 Cov(S_Q, P_Q) per coordinate (fp64 sums, stored fp32) and c_mean, c_var.
// k_foldin: a group of W lanes per folded entity (W = 8 .. 64 by d; lane l owns coordinates j W + l, j < CPL).  theta_e
//   and its Adam moments stay in registers for all n_steps; the entity's rows are read once to form the row-independent
//   sums (sum_r A_r, sum_r B_r, sum_r C_r, sum_r c_var,r) and staged in LDS (M_r and c_mean,r - y_r) while they fit,
//   the rest streamed from the operand table.  Per step and row the closed form needs ONE group reduction (mu_e . M_r);
//   the variance's gradient is linear in the row sums.  The sampled objective regenerates the partners' draws every
//   step (Philox, keyed as in training) and needs one reduction per row and draw.  No atomics, no host sync; rows are
//   visited in their order in the sorted row list, so an entity's result does not depend on the other entities.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "vfm_args.hpp"
#include "vfm_foldin.h"
#include "vfm_launch.hpp"            // launch_status

namespace vfm {
namespace {
#include "vfm_rng.hpp"
#include "vfm_common.hpp"

#include "vfm_foldin_body.hpp"       // FoldArgs, k_foldin_prep, the per-entity body (shared with the sessions), the host side

// ---------------------------------------------------------------------------------------------------------------------
// k_foldin
// ---------------------------------------------------------------------------------------------------------------------
template <int W, int CPL, int LINK, bool SAMPLED>
__global__ __launch_bounds__(FB) void k_foldin(const FoldArgs a) {
  extern __shared__ float lds[];
  constexpr int GPB = FB / W, DP = W * CPL;
  const int tid = threadIdx.x, l = tid % W, grp = tid / W;
  const int64_t g = (int64_t)blockIdx.x * GPB + grp;
  const bool live = g < a.E;
  int64_t r0 = 0, n = 0, e = 0;
  if (live) {
    r0 = min(max(a.ptr[g], (int64_t)0), a.R);
    n = min(max(a.ptr[g + 1], r0), a.R) - r0;
    e = a.ent[g];
  }
  const bool eok = e >= 0 && e < a.T;
  const int d = a.d;
  const float prec = a.lik == VFM_LIK_NORMAL ? link_f<LINK>(a.scal[0]) : 0.f;
  const float m0 = a.scal[1], sg0 = link_f<LINK>(a.scal[2]);
  const ListRows rows{a, r0};

  // ---- theta_e (coordinates past d: mu = 0, s = prior, never updated)
  float mu[CPL], sp[CPL];
  bool vk[CPL];
#pragma unroll
  for (int j = 0; j < CPL; ++j) {
    const int kc = j * W + l;
    vk[j] = kc < d;
    mu[j] = 0.f;
    sp[j] = prior_s<LINK>();
    if (vk[j] && eok && !a.reset) {
      mu[j] = a.entity[e * 2 * d + kc];
      sp[j] = a.entity[e * 2 * d + d + kc];
    }
  }
  float muw = 0.f, spw = prior_s<LINK>();
  if (eok && !a.reset) { muw = a.bias[e * 2]; spw = a.bias[e * 2 + 1]; }

  // ---- closed form: row-independent sums, rows staged in LDS
  float SA[CPL], SB[CPL], SC[CPL];
  float Scv = 0.f;
  float* Ms = lds + (int64_t)grp * a.cap * (DP + 1);
  float* Cy = Ms + (int64_t)a.cap * DP;
  if constexpr (!SAMPLED) {
#pragma unroll
    for (int j = 0; j < CPL; ++j) SA[j] = SB[j] = SC[j] = 0.f;
    fold_stage_rows<W, CPL>(a, rows, 0, n, l, Ms, Cy, SA, SB, SC, Scv);
    __syncthreads();                     // (the stage is read across lanes of the group below; the only barrier)
  }

  fold_run<W, CPL, LINK, SAMPLED>(
      a, rows, n, e, a.t0, l, Ms, Cy, prec, m0, sg0, mu, sp, vk, muw, spw, SA, SB, SC, Scv,
      [&](float loss, const float (&gm)[CPL], const float (&gs)[CPL], float gmw, float gsw) {
        if (live && l == 0) a.loss[g] = eok ? loss : __builtin_nanf("");
        if (live && a.mode == VFM_FOLDIN_OBJECTIVE && a.grad) {
          float* go = a.grad + g * (2 * (int64_t)d + 2);
#pragma unroll
          for (int j = 0; j < CPL; ++j)
            if (vk[j]) { go[j * W + l] = gm[j]; go[d + j * W + l] = gs[j]; }
          if (l == 0) { go[2 * d] = gmw; go[2 * d + 1] = gsw; }
        }
      });

  if (live && eok && a.mode == VFM_FOLDIN_FIT) {
#pragma unroll
    for (int j = 0; j < CPL; ++j)
      if (vk[j]) { a.entity[e * 2 * d + j * W + l] = mu[j]; a.entity[e * 2 * d + d + j * W + l] = sp[j]; }
    if (l == 0) { a.bias[e * 2] = muw; a.bias[e * 2 + 1] = spw; }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
void launch(const FShape& s, bool sp, bool sampled, const FoldArgs& a, hipStream_t st) {
  for_link(sp, [&](auto link) {
    for_shape(s, [&](auto w, auto c) {
      constexpr int W = decltype(w)::value, CPL = decltype(c)::value, LINK = decltype(link)::value, GPB = FB / W;
      const dim3 grid((unsigned)((a.E + GPB - 1) / GPB));
      const size_t shm = (size_t)GPB * a.cap * (W * CPL + 1) * 4;      // (sampled: cap = 0)
      if (sampled) hipLaunchKernelGGL((k_foldin<W, CPL, LINK, true>), grid, dim3(FB), shm, st, a);
      else hipLaunchKernelGGL((k_foldin<W, CPL, LINK, false>), grid, dim3(FB), shm, st, a);
    });
  });
}

}  // namespace
}  // namespace vfm

extern "C" {

int64_t vfm_foldin_workspace_bytes(int64_t n_ops, int32_t d, int32_t objective) {
  if (n_ops < 0 || d < 1 || d > VFM_FOLDIN_MAX_D || (objective != VFM_OBJ_CLOSED_FORM && objective != VFM_OBJ_SAMPLED))
    return VFM_E_INVALID;
  if (objective == VFM_OBJ_SAMPLED) return 0;
  return vfm::ops_off_opc(n_ops, d) + vfm::round_up(n_ops * 2 * 4, 256);
}

int vfm_foldin_f32(const vfm_foldin_t* p, void* stream) {
  using vfm::fail;
  if (!p) return fail(VFM_E_INVALID, "vfm_foldin_f32: NULL argument struct");
  if (p->T < 1) return fail(VFM_E_INVALID, "T < 1");
  if (p->d < 1 || p->d > VFM_FOLDIN_MAX_D) return fail(VFM_E_INVALID, "d out of range [1,512]");
  if (p->F < 1 || p->F > VFM_MAX_FIELDS) return fail(VFM_E_INVALID, "F out of range [1,64]");
  if (p->col < 0 || p->col >= p->F) return fail(VFM_E_INVALID, "col out of range [0,F)");
  if (p->E < 0 || p->R < 0) return fail(VFM_E_INVALID, "E < 0 or R < 0");
  if (p->likelihood != VFM_LIK_NORMAL && p->likelihood != VFM_LIK_BERNOULLI)
    return fail(VFM_E_INVALID, "unknown likelihood");
  if (p->objective == VFM_OBJ_CLOSED_FORM) {
    if (p->likelihood != VFM_LIK_NORMAL) return fail(VFM_E_INVALID, "the closed form needs the Normal likelihood");
    if (p->n_ops < 0 || (p->R > 0 && p->n_ops < 1)) return fail(VFM_E_INVALID, "n_ops out of range");
  } else if (p->objective == VFM_OBJ_SAMPLED) {
    if (p->n_samples < 1 || p->n_samples > VFM_FOLDIN_MAX_SAMPLES)
      return fail(VFM_E_INVALID, "n_samples out of range [1,4]");
  } else {
    return fail(VFM_E_INVALID, "unknown objective");
  }
  if (p->flags & ~VFM_FLAG_LINK_SOFTPLUS) return fail(VFM_E_INVALID, "flags: only VFM_FLAG_LINK_SOFTPLUS is accepted");
  if (p->mode != VFM_FOLDIN_FIT && p->mode != VFM_FOLDIN_OBJECTIVE) return fail(VFM_E_INVALID, "unknown mode");
  if (p->n_steps < 0 || (p->mode == VFM_FOLDIN_OBJECTIVE && p->n_steps != 0))
    return fail(VFM_E_INVALID, "n_steps: >= 0, and 0 in the objective mode");
  if (p->t0 < 0 || p->t0 + (int64_t)p->n_steps >= ((int64_t)1 << 60) / VFM_FOLDIN_MAX_SAMPLES)
    return fail(VFM_E_INVALID, "t0 out of range");
  if (!(p->lr >= 0.f) || !(p->kl_weight >= 0.f)) return fail(VFM_E_INVALID, "lr and kl_weight must be >= 0");
  if (p->E == 0) return 0;
  if (!p->entities || !p->row_ptr || !p->entity_params || !p->bias_params || !p->scalars || !p->out_loss ||
      (p->R > 0 && (!p->x || !p->y)))
    return fail(VFM_E_INVALID, "null pointer");
  const bool cf = p->objective == VFM_OBJ_CLOSED_FORM;
  const int64_t n_ops = cf ? p->n_ops : 0;
  if (cf && p->R > 0 && (!p->op_x || !p->row_op)) return fail(VFM_E_INVALID, "closed form: op_x and row_op needed");
  const int64_t ws = vfm_foldin_workspace_bytes(n_ops, p->d, p->objective);
  if (cf && (p->workspace_bytes < ws || (ws > 0 && !p->workspace)))
    return fail(VFM_E_INVALID, "workspace too small (vfm_foldin_workspace_bytes)");
  if (cf && ws > 0 && (((uintptr_t)p->workspace) & 255)) return fail(VFM_E_INVALID, "workspace must be 256-byte aligned");

  const hipStream_t st = (hipStream_t)stream;
  const bool sp = (p->flags & VFM_FLAG_LINK_SOFTPLUS) != 0;
  const vfm::FShape s = vfm::shape_of(p->d);
  vfm::FoldArgs a = vfm::fill_fold_args(p->E, p->T, p->F, p->d, p->col, p->likelihood, cf ? 1 : p->n_samples, p->n_steps,
                                        p->reset ? 1 : 0, p->mode, p->lr, p->kl_weight, p->t0, p->seed,
                                        p->entity_params, p->bias_params, p->scalars);
  a.R = p->R; a.ent = p->entities; a.ptr = p->row_ptr; a.x = p->x; a.row_op = p->row_op; a.y = p->y;
  a.loss = p->out_loss; a.grad = p->out_grad;
  if (cf) {
    char* w = (char*)p->workspace;
    float* ops = (float*)w;
    float* opc = (float*)(w + vfm::ops_off_opc(n_ops, p->d));
    a.ops = ops; a.opc = opc;
    a.cap = vfm::lds_cap(s, 0, p->lds_rows);
    if (int rc = vfm::launch_foldin_prep(sp, a, n_ops, p->op_x, ops, opc, st)) return rc;
  }
  vfm::launch(s, sp, !cf, a, st);
  return launch_status("k_foldin");
}

}  // extern "C"

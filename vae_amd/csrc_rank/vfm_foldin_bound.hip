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
// Every sum has a fixed order that depends on the entity's rows and d alone: no atomics, no host sync, the same bits
// whichever other entities share the launch and wherever the triangle lives.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "vfm_args.hpp"
#include "vfm_bound.h"
#include "vfm_launch.hpp"            // launch_status

namespace vfm {
namespace {
#include "vfm_rng.hpp"
#include "vfm_common.hpp"

#include "vfm_foldin_body.hpp"       // FoldArgs, k_foldin_prep, fold_stage_rows, the host side
#include "vfm_foldin_solve_body.hpp" // k_foldin_solve_prep, chol_solve, put_params, the operand block and the slabs

struct BoundArgs {
  FoldArgs f;                            // (cap = 0; n_steps: the rounds; f.ops / f.opc: the fp32 operands of the loss)
  const double* ops64;                   // [n_ops, 3, d]  M | A | C, unrounded
  const double* cm64;                    // [n_ops]        c_mean
  const double* cv64;                    // [n_ops]        c_var
  double* wrow;                          // [R]            w_r of the round in flight
  SolveSlabs sl;                         // the slabs and the LDS rule of the triangle
};

// LDS of a block in doubles: the exact fold-in's and sigma_w^2, sigma_k^2 [d] behind the triangle
__host__ __device__ inline int64_t bound_lds_doubles(int d, int cap_dim) { return lds_doubles(d, cap_dim) + d + 1; }

inline int64_t off_cv64(int64_t n_ops, int d) { return off_slabs(n_ops, d); }
inline int64_t off_wrow(int64_t n_ops, int d) { return off_cv64(n_ops, d) + round_up(n_ops * 8, 256); }
inline int64_t off_bound_slabs(int64_t R, int64_t n_ops, int d) { return off_wrow(n_ops, d) + round_up(R * 8, 256); }

template <int LINK>
__global__ __launch_bounds__(FB) void k_foldin_bound_prep(int64_t n_ops, int F, int d, int col, int64_t T,
                                                          const int64_t* __restrict__ opx, const float* __restrict__ ent,
                                                          const float* __restrict__ bias, const float* __restrict__ scal,
                                                          double* __restrict__ cvo) {
#pragma clang fp contract(on)
  const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= n_ops) return;
  const int64_t* xr = opx + o * F;
  bool ok = true;
  for (int f = 0; f < F; ++f) ok = ok && (f == col || (xr[f] >= 0 && xr[f] < T));
  if (!ok) {
    cvo[o] = __builtin_nan("");
    return;
  }
  const double sg0 = link_d<LINK>(scal[2]);
  double cv = sg0 * sg0;
  for (int f = 0; f < F; ++f) {
    if (f == col) continue;
    const double sw = link_d<LINK>(bias[xr[f] * 2 + 1]);
    cv += sw * sw;
  }
  for (int k = 0; k < d; ++k) {
    double sm = 0., ss = 0., sss = 0.;
    for (int f = 0; f < F; ++f) {
      if (f == col) continue;
      const float* row = ent + xr[f] * 2 * (int64_t)d;
      const double m = row[k], sg = link_d<LINK>(row[d + k]), s2 = sg * sg;
      sm += m; ss += s2; sss += s2 * s2;
    }
    double lin = 0.;
    for (int f = 0; f < F; ++f) {
      if (f == col) continue;
      const float* row = ent + xr[f] * 2 * (int64_t)d;
      const double m = row[k], sg = link_d<LINK>(row[d + k]), oth = sm - m;
      lin += sg * sg * oth * oth;
    }
    cv += 0.5 * (ss * ss - sss) + lin;
  }
  cvo[o] = cv;
}

// phase E: B_e at the fp32 parameters pf = [mu_w, mu [d] | s_w, s [d]] (LDS), by wave 0; its 64 / W lane groups all
// hold this entity, lane l of a group owns coordinates j W + l
template <int W, int CPL, int LINK, class Rows>
__device__ __forceinline__ void bound_loss(const FoldArgs& a, const Rows& rows, int64_t n, const float* pf, int lane,
                                           float* loss) {
#pragma clang fp contract(on)
  constexpr int DP = W * CPL;
  const int d = a.d, d1 = d + 1, l = lane % W;
  float mu[CPL], sg[CPL];
  bool vk[CPL];
#pragma unroll
  for (int j = 0; j < CPL; ++j) {
    const int kc = j * W + l;
    vk[j] = kc < d;
    mu[j] = vk[j] ? pf[1 + kc] : 0.f;
    sg[j] = link_f<LINK>(vk[j] ? pf[d1 + 1 + kc] : prior_s<LINK>());
  }
  const float muw = pf[0], sgw = link_f<LINK>(pf[d1]);
  double lsum = 0.0;
  for (int64_t i = 0; i < n; ++i) {
    float SA[CPL], SB[CPL], SC[CPL], Scv = 0.f;
#pragma unroll
    for (int j = 0; j < CPL; ++j) SA[j] = SB[j] = SC[j] = 0.f;
    fold_stage_rows<W, CPL>(a, rows, i, i + 1, l, nullptr, nullptr, SA, SB, SC, Scv);   // (a.cap = 0: nothing staged)
    const int64_t o = rows.op(i);
    float p = 0.f;
#pragma unroll
    for (int j = 0; j < CPL; ++j) p = fmaf(mu[j], a.ops[o * 3 * DP + j * W + l], p);
    const float Ef = (a.opc[o * 2] + muw) + group_sum<W>(p);
    float vq = 0.f;
#pragma unroll
    for (int j = 0; j < CPL; ++j) vq += fmaf(mu[j] * mu[j], SA[j], fmaf(sg[j] * sg[j], SB[j], mu[j] * SC[j]));
    const float Vf = (Scv + sgw * sgw) + group_sum<W>(vq);
    float x2 = fmaf(Ef, Ef, Vf);
    x2 = x2 < 0.f ? 0.f : x2;            // (a NaN stays a NaN)
    const float xi = sqrtf(x2);
    const float t = -(rows.y(i) - 0.5f) * Ef + 0.5f * xi + log1pf(expf(-xi));
    lsum += (double)t;
  }
  float klq = 0.f;
#pragma unroll
  for (int j = 0; j < CPL; ++j)
    if (vk[j]) klq += kl_std_normal(mu[j], sg[j]);
  klq = group_sum<W>(klq) + kl_std_normal(muw, sgw);
  if (lane == 0) *loss = (float)(lsum + (double)a.klw * (double)klq);
}

template <int W, int CPL, int LINK>
__global__ __launch_bounds__(FB) void k_foldin_bound(const BoundArgs s) {
#pragma clang fp contract(on)
  extern __shared__ double sm[];
  const FoldArgs& a = s.f;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int d = a.d, d1 = d + 1;
  double* Dd = sm;                       // D                                  [d + 1]  (0: the first-order weight)
  double* Di = Dd + d1;                  // 1 / D
  double* bv = Di + d1;                  // primal: b; dual: D^-1 b
  double* yv = bv + d1;                  // the right-hand side, then L^-1 of it; between two rounds: theta
  double* dv = yv + d1;                  // 1 / L_jj
  double* xv = dv + d1;                  // the solution of the system
  double* SBd = xv + d1;                 // sum_r w_r, sum_r w_r (A_rk + M_rk^2)
  float* pf = (float*)(SBd + d1);        // the fp32 parameters: mu_w, mu [d] | s_w, s [d]
  double* Hl = sm + 8 * d1;              // the triangle while it fits
  double* sg2 = Hl + tri(s.sl.cap_dim);  // sigma_w^2, sigma_k^2 [d]
  double* th = yv;
  double* Hg = s.sl.slab ? s.sl.slab + (int64_t)blockIdx.x * s.sl.slab_elems : nullptr;
  const double kl = a.klw;
  const int64_t os = 3 * (int64_t)d;     // stride of an fp64 operand

  for (int64_t g = blockIdx.x; g < a.E; g += gridDim.x) {
    const int64_t r0 = min(max(a.ptr[g], (int64_t)0), a.R);
    const int64_t n = min(max(a.ptr[g + 1], r0), a.R) - r0;
    const int64_t e = a.ent[g];
    const bool dual = n <= d;
    const int m = solve_dim(n, d);
    double* Hm = m <= s.sl.cap_dim ? Hl : Hg;
    if (e < 0 || e >= a.T || !Hm) {      // (block-uniform)
      if (tid == 0) a.loss[g] = __builtin_nanf("");
      continue;
    }
    const ListRows rows{a, r0};
    float* erow = a.entity + e * 2 * (int64_t)d;

    if (a.mode == VFM_FOLDIN_OBJECTIVE) {
      for (int c = tid; c < d1; c += FB) {
        pf[c] = c ? erow[c - 1] : a.bias[e * 2];
        pf[d1 + c] = c ? erow[d + c - 1] : a.bias[e * 2 + 1];
      }
    } else {
      // ---- the start: xi^(0) is taken at the entity's row, or at the prior
      for (int c = tid; c < d1; c += FB) {
        double t0 = 0., v0 = 1.;
        if (!a.reset) {
          const double sg = link_d<LINK>(c ? erow[d + c - 1] : a.bias[e * 2 + 1]);
          t0 = c ? erow[c - 1] : a.bias[e * 2];
          v0 = sg * sg;
        }
        th[c] = t0;
        sg2[c] = v0;
      }
      __syncthreads();

      for (int it = 0; it < a.n_steps; ++it) {
        // ---- X: the rows' weights at the current iterate
        for (int64_t i = wv; i < n; i += FB / 64) {
          const int64_t o = rows.op(i);
          const double* op = s.ops64 + o * os;
          double pe = 0., pv = 0.;
          for (int k = lane; k < d; k += 64) {
            const double M = op[k], A = op[d + k], C = op[2 * d + k], mu = th[k + 1];
            pe += mu * M;
            pv += mu * mu * A + sg2[k + 1] * (A + M * M) + mu * C;
          }
          pe = wave_sum_d(pe);
          pv = wave_sum_d(pv);
          const double Ef = s.cm64[o] + th[0] + pe;
          const double Vf = s.cv64[o] + sg2[0] + pv;
          double x2 = Ef * Ef + Vf;
          x2 = x2 < 0. ? 0. : x2;        // (a NaN stays a NaN)
          const double xi = sqrt(x2);
          const double w = xi < 1e-3 ? 0.25 - x2 / 48.0 : tanh(0.5 * xi) / (2.0 * xi);
          if (lane == 0) s.wrow[r0 + i] = w;
        }
        __syncthreads();

        // ---- A: the weighted row sums of each coordinate
        for (int c = tid; c < d1; c += FB) {
          double SA = 0., SB = 0., SC = 0., bM = 0.;
          if (c == 0) {
            for (int64_t i = 0; i < n; ++i) {
              const double w = s.wrow[r0 + i];
              SB += w;
              bM += ((double)rows.y(i) - 0.5) - w * s.cm64[rows.op(i)];
            }
          } else {
            for (int64_t i = 0; i < n; ++i) {
              const int64_t o = rows.op(i);
              const double* op = s.ops64 + o * os + (c - 1);
              const double M = op[0], A = op[d], C = op[2 * d], w = s.wrow[r0 + i];
              const double t = ((double)rows.y(i) - 0.5) - w * s.cm64[o];
              SA += w * A;
              SB += w * (A + M * M);
              SC += w * C;
              bM += t * M;
            }
          }
          const double D = kl + SA, b = bM - 0.5 * SC;
          Dd[c] = D;
          Di[c] = 1.0 / D;
          bv[c] = dual ? b / D : b;
          SBd[c] = SB;
        }
        __syncthreads();

        // ---- B: the system and its right-hand side
        if (dual) {
          const int64_t np = tri(m);
          for (int64_t p = wv; p < np; p += FB / 64) {
            int i, j;
            tri_decode(p, i, j);
            const double* Mi = s.ops64 + rows.op(i) * os;
            const double* Mj = s.ops64 + rows.op(j) * os;
            double acc = 0.;
            for (int k = lane; k < d; k += 64) acc += Mi[k] * Mj[k] * Di[k + 1];
            acc = wave_sum_d(acc);
            if (lane == 0) Hm[p] = acc + Di[0] + (i == j ? 1.0 / s.wrow[r0 + i] : 0.0);
          }
          for (int i = wv; i < m; i += FB / 64) {
            const double* Mi = s.ops64 + rows.op(i) * os;
            double acc = 0.;
            for (int k = lane; k < d; k += 64) acc += Mi[k] * bv[k + 1];
            acc = wave_sum_d(acc);
            if (lane == 0) yv[i] = acc + bv[0];
          }
        } else {
          const int64_t np = tri(d1);
          for (int64_t p = tid; p < np; p += FB) {
            int i, j;
            tri_decode(p, i, j);
            double acc = 0.;
            if (i == 0) {
              for (int64_t r = 0; r < n; ++r) acc += s.wrow[r0 + r];
            } else if (j == 0) {
              for (int64_t r = 0; r < n; ++r) acc += s.wrow[r0 + r] * s.ops64[rows.op(r) * os + (i - 1)];
            } else {
              for (int64_t r = 0; r < n; ++r) {
                const double* op = s.ops64 + rows.op(r) * os;
                acc += s.wrow[r0 + r] * op[i - 1] * op[j - 1];
              }
            }
            Hm[p] = acc + (i == j ? Dd[i] : 0.0);
          }
          for (int c = tid; c < d1; c += FB) yv[c] = bv[c];
        }
        __syncthreads();

        // ---- C: the factorisation and the two substitutions
        chol_solve(Hm, yv, dv, xv, m);

        // ---- the iterate, in fp64: the means and the scales' closed forms
        for (int c = tid; c < d1; c += FB) {
          double t;
          if (dual) {
            double acc = 0.;
            if (c == 0) {
              for (int i = 0; i < m; ++i) acc += xv[i];
            } else {
              for (int i = 0; i < m; ++i) acc += s.ops64[rows.op(i) * os + (c - 1)] * xv[i];
            }
            t = bv[c] - Di[c] * acc;
          } else {
            t = xv[c];
          }
          th[c] = t;
          sg2[c] = kl / (kl + SBd[c]);
        }
        __syncthreads();
      }

      // ---- D: rounded to fp32 once and written
      for (int c = tid; c < d1; c += FB) put_params<LINK>(pf, d1, c, th[c], kl, 1.0, SBd[c]);
      __syncthreads();
      for (int k = tid; k < d; k += FB) {
        erow[k] = pf[1 + k];
        erow[d + k] = pf[d1 + 1 + k];
      }
      if (tid == 0) {
        a.bias[e * 2] = pf[0];
        a.bias[e * 2 + 1] = pf[d1];
      }
    }
    __syncthreads();

    // ---- E: B_e at the fp32 parameters
    if (wv == 0) bound_loss<W, CPL, LINK>(a, rows, n, pf, lane, a.loss + g);
    __syncthreads();                     // (pf and the iterate are rewritten by the next entity)
  }
}

void launch(const FShape& f, bool sp, const BoundArgs& s, unsigned grid, size_t shm, hipStream_t st) {
  for_link(sp, [&](auto link) {
    for_shape(f, [&](auto w, auto c) {
      const auto k = k_foldin_bound<decltype(w)::value, decltype(c)::value, decltype(link)::value>;
      // (more than 64 KiB of dynamic LDS: state the size; a runtime that needs no opt-in ignores it)
      (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
      (void)hipGetLastError();
      hipLaunchKernelGGL(k, dim3(grid), dim3(FB), shm, st, s);
    });
  });
}

}  // namespace
}  // namespace vfm

extern "C" {

int64_t vfm_foldin_bound_workspace_bytes(int64_t E, int64_t R, int64_t n_ops, int32_t d, int32_t lds_dim) {
  if (E < 0 || R < 0 || n_ops < 0 || d < 1 || d > VFM_FOLDIN_MAX_D || lds_dim < -1) return VFM_E_INVALID;
  return vfm::off_bound_slabs(R, n_ops, d) + vfm::slabs_bytes(E, d, lds_dim);
}

int vfm_foldin_bound_f32(const vfm_foldin_bound_t* p, void* stream) {
  using vfm::fail;
  if (!p) return fail(VFM_E_INVALID, "vfm_foldin_bound_f32: NULL argument struct");
  if (p->T < 1) return fail(VFM_E_INVALID, "T < 1");
  if (p->d < 1 || p->d > VFM_FOLDIN_MAX_D) return fail(VFM_E_INVALID, "d out of range [1,512]");
  if (p->F < 1 || p->F > VFM_MAX_FIELDS) return fail(VFM_E_INVALID, "F out of range [1,64]");
  if (p->col < 0 || p->col >= p->F) return fail(VFM_E_INVALID, "col out of range [0,F)");
  if (p->E < 0 || p->R < 0) return fail(VFM_E_INVALID, "E < 0 or R < 0");
  if (p->objective != VFM_OBJ_CLOSED_FORM)
    return fail(VFM_E_INVALID, "the bound fold-in uses the closed-form moments only (VFM_OBJ_CLOSED_FORM)");
  if (p->likelihood != VFM_LIK_BERNOULLI)
    return fail(VFM_E_INVALID, "the bound fold-in needs the Bernoulli likelihood (VFM_LIK_BERNOULLI)");
  if (p->n_ops < 0 || (p->R > 0 && p->n_ops < 1)) return fail(VFM_E_INVALID, "n_ops out of range");
  if (p->flags & ~VFM_FLAG_LINK_SOFTPLUS) return fail(VFM_E_INVALID, "flags: only VFM_FLAG_LINK_SOFTPLUS is accepted");
  if (p->lds_dim < -1) return fail(VFM_E_INVALID, "lds_dim: -1 or >= 0");
  if (!(p->kl_weight > 0.f) || !(p->kl_weight <= 3.0e38f))
    return fail(VFM_E_INVALID, "kl_weight must be > 0 and finite (the prior is what makes the system positive definite)");
  if (p->mode != VFM_FOLDIN_FIT && p->mode != VFM_FOLDIN_OBJECTIVE)
    return fail(VFM_E_INVALID, "mode: VFM_FOLDIN_FIT or VFM_FOLDIN_OBJECTIVE");
  if (p->mode == VFM_FOLDIN_FIT && p->n_iters < 1) return fail(VFM_E_INVALID, "n_iters must be >= 1 for a fit");
  if (p->mode == VFM_FOLDIN_OBJECTIVE && p->n_iters != 0)
    return fail(VFM_E_INVALID, "n_iters must be 0 in VFM_FOLDIN_OBJECTIVE");
  if (p->E == 0) return 0;
  if (!p->entities || !p->row_ptr || !p->entity_params || !p->bias_params || !p->scalars || !p->out_loss ||
      (p->R > 0 && (!p->y || !p->op_x || !p->row_op)))
    return fail(VFM_E_INVALID, "null pointer");
  const int64_t ws = vfm_foldin_bound_workspace_bytes(p->E, p->R, p->n_ops, p->d, p->lds_dim);
  if (p->workspace_bytes < ws || (ws > 0 && !p->workspace))
    return fail(VFM_E_INVALID, "workspace too small (vfm_foldin_bound_workspace_bytes)");
  if (ws > 0 && (((uintptr_t)p->workspace) & 255)) return fail(VFM_E_INVALID, "workspace must be 256-byte aligned");

  const hipStream_t st = (hipStream_t)stream;
  const bool sp = (p->flags & VFM_FLAG_LINK_SOFTPLUS) != 0;
  const vfm::FShape f = vfm::shape_of(p->d);
  vfm::BoundArgs s;
  vfm::FoldArgs& a = s.f;
  a = vfm::fill_fold_args(p->E, p->T, p->F, p->d, p->col, VFM_LIK_BERNOULLI, 1, p->n_iters, p->reset != 0, p->mode, 0.f,
                          p->kl_weight, 0, 0, p->entity_params, p->bias_params, p->scalars);
  a.R = p->R; a.ent = p->entities; a.ptr = p->row_ptr; a.row_op = p->row_op; a.y = p->y;
  a.loss = p->out_loss;
  char* w = (char*)p->workspace;
  a.ops = (float*)w;
  a.opc = (float*)(w + vfm::ops_off_opc(p->n_ops, p->d));
  s.ops64 = (double*)(w + vfm::off_ops64(p->n_ops, p->d));
  s.cm64 = (double*)(w + vfm::off_cm64(p->n_ops, p->d));
  double* cv64 = (double*)(w + vfm::off_cv64(p->n_ops, p->d));
  s.cv64 = cv64;
  s.wrow = (double*)(w + vfm::off_wrow(p->n_ops, p->d));
  const unsigned grid = vfm::place_slabs(p->d, p->lds_dim, p->E, w + vfm::off_bound_slabs(p->R, p->n_ops, p->d),
                                         (int64_t)1 << 20, s.sl);
  const size_t shm = (size_t)vfm::bound_lds_doubles(p->d, s.sl.cap_dim) * 8;

  if (p->n_ops > 0) {
    if (int rc = vfm::launch_solve_preps(sp, a, p->n_ops, p->op_x, w, st)) return rc;
    const unsigned nb = (unsigned)((p->n_ops + vfm::FB - 1) / vfm::FB);
    vfm::for_link(sp, [&](auto link) {
      hipLaunchKernelGGL(vfm::k_foldin_bound_prep<decltype(link)::value>, dim3(nb), dim3(vfm::FB), 0, st, p->n_ops, a.F,
                         a.d, a.col, a.T, p->op_x, a.entity, a.bias, a.scal, cv64);
    });
    if (int rc = launch_status("k_foldin_bound_prep")) return rc;
  }
  vfm::launch(f, sp, s, grid, shm, st);
  return launch_status("k_foldin_bound");
}

}  // extern "C"

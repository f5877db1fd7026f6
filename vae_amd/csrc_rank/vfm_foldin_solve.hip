// vfm_foldin_solve.hip -- exact fold-in (include/vfm_foldin.h, vfm_foldin_solve_f32): the closed-form optimum of every
// folded entity in one launch.
//
// k_foldin_solve: one workgroup of FB threads per entity (a grid-stride loop over the entities).  Per entity, with the
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

#include "vfm_foldin_body.hpp"       // FoldArgs, k_foldin_prep, fold_stage_rows, the host side

struct SolveArgs {
  FoldArgs f;                            // (cap = 0: fold_stage_rows stages nothing; f.ops / f.opc: the fp32 operands of the loss)
  const double* ops64;                   // [n_ops, 3, d]  M | A | C, unrounded
  const double* cm64;                    // [n_ops]        c_mean
  double* slab;                          // [gridDim.x, slab_elems] or NULL when every system stays in LDS
  int64_t slab_elems;
  int32_t cap_dim;                       // systems up to this size live in LDS
};

__host__ __device__ inline int64_t tri(int64_t m) { return m * (m + 1) / 2; }

// (i, j), j <= i, of packed index p = i (i + 1) / 2 + j
__device__ __forceinline__ void tri_decode(int64_t p, int& i, int& j) {
  int r = (int)((sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
  while (tri(r + 1) <= p) ++r;
  while (tri(r) > p) --r;
  i = r;
  j = (int)(p - tri(r));
}

// all-reduce over the wave, a fixed butterfly: every lane ends with the same bits
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// LDS of a block in doubles: seven vectors of d + 1, the fp32 parameters (2 (d + 1) floats), the triangle
__host__ __device__ inline int64_t lds_doubles(int d, int cap_dim) { return 8 * (int64_t)(d + 1) + tri(cap_dim); }

template <int LINK>
__device__ __forceinline__ double link_d(float s) { return LINK == LINK_ABS ? fabs((double)s) : softplus_d((double)s); }

// k_foldin_prep's operand o in fp64: the same sums, not rounded to fp32, the links of the fp32 table values in fp64
template <int LINK>
__global__ __launch_bounds__(FB) void k_foldin_solve_prep(int64_t n_ops, int F, int d, int col, int64_t T,
                                                          const int64_t* __restrict__ opx, const float* __restrict__ ent,
                                                          const float* __restrict__ bias, const float* __restrict__ scal,
                                                          double* __restrict__ ops, double* __restrict__ cmo) {
#pragma clang fp contract(on)
  const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= n_ops) return;
  const int64_t* xr = opx + o * F;
  bool ok = true;
  for (int f = 0; f < F; ++f) ok = ok && (f == col || (xr[f] >= 0 && xr[f] < T));
  double* out = ops + o * 3 * (int64_t)d;
  if (!ok) {
    for (int k = 0; k < 3 * d; ++k) out[k] = __builtin_nan("");
    cmo[o] = __builtin_nan("");
    return;
  }
  double cm = scal[1];
  for (int f = 0; f < F; ++f)
    if (f != col) cm += bias[xr[f] * 2];
  for (int k = 0; k < d; ++k) {
    double sm = 0., smm = 0., ss = 0.;
    for (int f = 0; f < F; ++f) {
      if (f == col) continue;
      const float* row = ent + xr[f] * 2 * (int64_t)d;
      const double m = row[k], sg = link_d<LINK>(row[d + k]);
      sm += m; smm += m * m; ss += sg * sg;
    }
    double cov = 0.;
    for (int f = 0; f < F; ++f) {
      if (f == col) continue;
      const float* row = ent + xr[f] * 2 * (int64_t)d;
      const double m = row[k], sg = link_d<LINK>(row[d + k]);
      cov += sg * sg * (sm - m);
    }
    cm += 0.5 * (sm * sm - smm);
    out[k] = sm;
    out[d + k] = ss;
    out[2 * d + k] = 2.0 * cov;
  }
  cmo[o] = cm;
}

template <int W, int CPL, int LINK>
__global__ __launch_bounds__(FB) void k_foldin_solve(const SolveArgs s) {
#pragma clang fp contract(on)
  extern __shared__ double sm[];
  constexpr int DP = W * CPL;
  const FoldArgs& a = s.f;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int d = a.d, d1 = d + 1;
  double* Dd = sm;                       // D                                  [d + 1]  (0: the first-order weight)
  double* Di = Dd + d1;                  // 1 / D
  double* bv = Di + d1;                  // primal: b; dual: D^-1 b
  double* yv = bv + d1;                  // the right-hand side, then L^-1 of it
  double* dv = yv + d1;                  // 1 / L_jj
  double* xv = dv + d1;                  // the solution of the system
  double* SBd = xv + d1;                 // n, sum_r (A_rk + M_rk^2)
  float* pf = (float*)(SBd + d1);        // the fp32 parameters written: mu_w, mu [d] | s_w, s [d]
  double* Hl = SBd + 2 * d1;
  double* Hg = s.slab ? s.slab + (int64_t)blockIdx.x * s.slab_elems : nullptr;
  const float precf = link_f<LINK>(a.scal[0]);
  const double prec = link_d<LINK>(a.scal[0]), kl = a.klw;
  const int64_t os = 3 * (int64_t)d;     // stride of an fp64 operand

  for (int64_t g = blockIdx.x; g < a.E; g += gridDim.x) {
    const int64_t r0 = min(max(a.ptr[g], (int64_t)0), a.R);
    const int64_t n = min(max(a.ptr[g + 1], r0), a.R) - r0;
    const int64_t e = a.ent[g];
    const bool dual = n <= d;
    const int m = dual ? (int)n : d1;
    double* Hm = m <= s.cap_dim ? Hl : Hg;
    if (e < 0 || e >= a.T || !Hm) {      // (block-uniform)
      if (tid == 0) a.loss[g] = __builtin_nanf("");
      continue;
    }
    const ListRows rows{a, r0};

    // ---- A: the row sums of each coordinate
    for (int c = tid; c < d1; c += FB) {
      double SA = 0., SB = 0., SC = 0., bM = 0.;
      if (c == 0) {
        for (int64_t i = 0; i < n; ++i) bM += (double)rows.y(i) - s.cm64[rows.op(i)];
        SB = (double)n;
      } else {
        for (int64_t i = 0; i < n; ++i) {
          const int64_t o = rows.op(i);
          const double* op = s.ops64 + o * os + (c - 1);
          const double M = op[0], A = op[d], C = op[2 * d];
          const double t = (double)rows.y(i) - s.cm64[o];
          SA += A;
          SB += A + M * M;
          SC += C;
          bM += t * M;
        }
      }
      const double D = kl + prec * SA, b = prec * (bM - 0.5 * SC);
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
        if (lane == 0) Hm[p] = acc + Di[0] + (i == j ? 1.0 / prec : 0.0);
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
          acc = (double)n;
        } else if (j == 0) {
          for (int64_t r = 0; r < n; ++r) acc += s.ops64[rows.op(r) * os + (i - 1)];
        } else {
          for (int64_t r = 0; r < n; ++r) {
            const double* op = s.ops64 + rows.op(r) * os;
            acc += op[i - 1] * op[j - 1];
          }
        }
        Hm[p] = prec * acc + (i == j ? Dd[i] : 0.0);
      }
      for (int c = tid; c < d1; c += FB) yv[c] = bv[c];
    }
    __syncthreads();

    // ---- C: L L^T = system (row i of L: thread i mod FB; row m: the right-hand side), one barrier per column
    for (int j = 0; j < m; ++j) {
      const double* Lj = Hm + tri(j);
      int i = j + 1 + (tid - (j + 1) % FB + FB) % FB;        // the first row below j that this thread owns
      if (i <= m) {
        double sjj = Lj[j];
        for (int k = 0; k < j; ++k) sjj -= Lj[k] * Lj[k];
        const double rinv = 1.0 / sqrt(sjj);
        if (i == j + 1) dv[j] = rinv;
        for (; i <= m; i += FB) {
          double* Li = i < m ? Hm + tri(i) : yv;
          double sij = Li[j];
          for (int k = 0; k < j; ++k) sij -= Li[k] * Lj[k];
          Li[j] = sij * rinv;
        }
      }
      __syncthreads();
    }
    // L^T x = yv, from the last column back
    for (int j = m - 1; j >= 0; --j) {
      const double xj = yv[j] * dv[j];
      const double* Lj = Hm + tri(j);
      for (int i = tid; i < j; i += FB) yv[i] -= Lj[i] * xj;
      if (tid == 0) xv[j] = xj;
      __syncthreads();
    }

    // ---- D: the means and the scales, rounded to fp32
    for (int c = tid; c < d1; c += FB) {
      double th;
      if (dual) {
        double acc = 0.;
        if (c == 0) {
          for (int i = 0; i < m; ++i) acc += xv[i];
        } else {
          for (int i = 0; i < m; ++i) acc += s.ops64[rows.op(i) * os + (c - 1)] * xv[i];
        }
        th = bv[c] - Di[c] * acc;
      } else {
        th = xv[c];
      }
      const double sg = sqrt(kl / (kl + prec * SBd[c]));
      pf[c] = (float)th;
      pf[d1 + c] = (float)(LINK == LINK_ABS ? sg : log(expm1(sg)));
    }
    __syncthreads();
    for (int k = tid; k < d; k += FB) {
      a.entity[e * 2 * d + k] = pf[1 + k];
      a.entity[e * 2 * d + d + k] = pf[d1 + 1 + k];
    }
    if (tid == 0) {
      a.bias[e * 2] = pf[0];
      a.bias[e * 2 + 1] = pf[d1];
    }

    // ---- E: L_e at the written parameters (wave 0; its 64 / W lane groups all hold this entity).  The last pass of
    // fold_run's closed form, expression for expression: fp32 chains in row order, lane l of a group owns j W + l
    if (wv == 0) {
      const int l = lane % W;
      float mu[CPL], sg[CPL], SA[CPL], SB[CPL], SC[CPL];
      bool vk[CPL];
#pragma unroll
      for (int j = 0; j < CPL; ++j) {
        const int kc = j * W + l;
        vk[j] = kc < d;
        mu[j] = vk[j] ? pf[1 + kc] : 0.f;
        sg[j] = link_f<LINK>(vk[j] ? pf[d1 + 1 + kc] : prior_s<LINK>());
        SA[j] = SB[j] = SC[j] = 0.f;
      }
      const float muw = pf[0], sgw = link_f<LINK>(pf[d1]);
      float Scv = 0.f, rsq = 0.f;
      fold_stage_rows<W, CPL>(a, rows, 0, n, l, nullptr, nullptr, SA, SB, SC, Scv);     // (a.cap = 0: nothing staged)
      for (int64_t i = 0; i < n; ++i) {
        const int64_t o = rows.op(i);
        float p = 0.f;
#pragma unroll
        for (int j = 0; j < CPL; ++j) p = fmaf(mu[j], a.ops[o * 3 * DP + j * W + l], p);
        const float res = ((a.opc[o * 2] - rows.y(i)) + muw) + group_sum<W>(p);
        rsq = fmaf(res, res, rsq);
      }
      float vq = 0.f, klq = 0.f;
#pragma unroll
      for (int j = 0; j < CPL; ++j) {
        vq += fmaf(mu[j] * mu[j], SA[j], fmaf(sg[j] * sg[j], SB[j], mu[j] * SC[j]));
        if (vk[j]) klq += kl_std_normal(mu[j], sg[j]);
      }
      vq = group_sum<W>(vq);
      klq = group_sum<W>(klq) + kl_std_normal(muw, sgw);
      const double sumv = (double)Scv + (double)n * sgw * sgw + vq;
      const double lsum = 0.5 * precf * ((double)rsq + sumv) + (double)n * ((double)LOG_2PI_HALF - 0.5 * log((double)precf));
      if (lane == 0) a.loss[g] = (float)(lsum + (double)a.klw * (double)klq);
    }
    __syncthreads();                     // (pf is rewritten by the next entity)
  }
}

void launch(const FShape& f, bool sp, const SolveArgs& s, unsigned grid, size_t shm, hipStream_t st) {
  for_link(sp, [&](auto link) {
    for_shape(f, [&](auto w, auto c) {
      const auto k = k_foldin_solve<decltype(w)::value, decltype(c)::value, decltype(link)::value>;
      // (more than 64 KiB of dynamic LDS: state the size; a runtime that needs no opt-in ignores it)
      (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
      (void)hipGetLastError();
      hipLaunchKernelGGL(k, dim3(grid), dim3(FB), shm, st, s);
    });
  });
}

inline int cap_dim_of(int d, int lds_dim) {
  const int fit = d + 1 < VFM_FOLDIN_SOLVE_LDS_DIM ? d + 1 : VFM_FOLDIN_SOLVE_LDS_DIM;
  return lds_dim < 0 || lds_dim > fit ? fit : lds_dim;
}

inline int64_t slab_bytes(int d) { return round_up(tri(d + 1) * 8, 256); }

// workspace: [fp32 operands | their constants | fp64 operands | fp64 c_mean | slabs]
inline int64_t off_ops64(int64_t n_ops, int d) { return ops_off_opc(n_ops, d) + round_up(n_ops * 2 * 4, 256); }
inline int64_t off_cm64(int64_t n_ops, int d) { return off_ops64(n_ops, d) + round_up(n_ops * 3 * d * 8, 256); }
inline int64_t off_slabs(int64_t n_ops, int d) { return off_cm64(n_ops, d) + round_up(n_ops * 8, 256); }

}  // namespace
}  // namespace vfm

extern "C" {

int64_t vfm_foldin_solve_workspace_bytes(int64_t E, int64_t n_ops, int32_t d, int32_t lds_dim) {
  if (E < 0 || n_ops < 0 || d < 1 || d > VFM_FOLDIN_MAX_D || lds_dim < -1) return VFM_E_INVALID;
  int64_t b = vfm::off_slabs(n_ops, d);
  if (d + 1 > vfm::cap_dim_of(d, lds_dim))
    b += (E < VFM_FOLDIN_SOLVE_SLABS ? E : VFM_FOLDIN_SOLVE_SLABS) * vfm::slab_bytes(d);
  return b;
}

int vfm_foldin_solve_f32(const vfm_foldin_solve_t* p, void* stream) {
  using vfm::fail;
  if (!p) return fail(VFM_E_INVALID, "vfm_foldin_solve_f32: NULL argument struct");
  if (p->T < 1) return fail(VFM_E_INVALID, "T < 1");
  if (p->d < 1 || p->d > VFM_FOLDIN_MAX_D) return fail(VFM_E_INVALID, "d out of range [1,512]");
  if (p->F < 1 || p->F > VFM_MAX_FIELDS) return fail(VFM_E_INVALID, "F out of range [1,64]");
  if (p->col < 0 || p->col >= p->F) return fail(VFM_E_INVALID, "col out of range [0,F)");
  if (p->E < 0 || p->R < 0) return fail(VFM_E_INVALID, "E < 0 or R < 0");
  if (p->objective != VFM_OBJ_CLOSED_FORM)
    return fail(VFM_E_INVALID, "the exact fold-in solves the closed-form objective only (VFM_OBJ_CLOSED_FORM)");
  if (p->likelihood != VFM_LIK_NORMAL) return fail(VFM_E_INVALID, "the closed form needs the Normal likelihood");
  if (p->n_ops < 0 || (p->R > 0 && p->n_ops < 1)) return fail(VFM_E_INVALID, "n_ops out of range");
  if (p->flags & ~VFM_FLAG_LINK_SOFTPLUS) return fail(VFM_E_INVALID, "flags: only VFM_FLAG_LINK_SOFTPLUS is accepted");
  if (p->lds_dim < -1) return fail(VFM_E_INVALID, "lds_dim: -1 or >= 0");
  if (!(p->kl_weight > 0.f) || !(p->kl_weight <= 3.0e38f))
    return fail(VFM_E_INVALID, "kl_weight must be > 0 and finite (the prior is what makes the system positive definite)");
  if (p->E == 0) return 0;
  if (!p->entities || !p->row_ptr || !p->entity_params || !p->bias_params || !p->scalars || !p->out_loss ||
      (p->R > 0 && (!p->y || !p->op_x || !p->row_op)))
    return fail(VFM_E_INVALID, "null pointer");
  const int64_t ws = vfm_foldin_solve_workspace_bytes(p->E, p->n_ops, p->d, p->lds_dim);
  if (p->workspace_bytes < ws || (ws > 0 && !p->workspace))
    return fail(VFM_E_INVALID, "workspace too small (vfm_foldin_solve_workspace_bytes)");
  if (ws > 0 && (((uintptr_t)p->workspace) & 255)) return fail(VFM_E_INVALID, "workspace must be 256-byte aligned");

  const hipStream_t st = (hipStream_t)stream;
  const bool sp = (p->flags & VFM_FLAG_LINK_SOFTPLUS) != 0;
  const vfm::FShape f = vfm::shape_of(p->d);
  vfm::SolveArgs s;
  vfm::FoldArgs& a = s.f;
  a = vfm::fill_fold_args(p->E, p->T, p->F, p->d, p->col, VFM_LIK_NORMAL, 1, 0, 0, VFM_FOLDIN_FIT, 0.f, p->kl_weight, 0, 0,
                          p->entity_params, p->bias_params, p->scalars);
  a.R = p->R; a.ent = p->entities; a.ptr = p->row_ptr; a.row_op = p->row_op; a.y = p->y;
  a.loss = p->out_loss;
  char* w = (char*)p->workspace;
  const int64_t off_opc = vfm::ops_off_opc(p->n_ops, p->d);
  float* ops = (float*)w;
  float* opc = (float*)(w + off_opc);
  a.ops = ops; a.opc = opc;
  s.cap_dim = vfm::cap_dim_of(p->d, p->lds_dim);
  const bool slabs = p->d + 1 > s.cap_dim;
  double* ops64 = (double*)(w + vfm::off_ops64(p->n_ops, p->d));
  double* cm64 = (double*)(w + vfm::off_cm64(p->n_ops, p->d));
  s.ops64 = ops64; s.cm64 = cm64;
  s.slab = slabs ? (double*)(w + vfm::off_slabs(p->n_ops, p->d)) : nullptr;
  s.slab_elems = vfm::slab_bytes(p->d) / 8;
  const int64_t gmax = slabs ? VFM_FOLDIN_SOLVE_SLABS : ((int64_t)1 << 20);
  const unsigned grid = (unsigned)(p->E < gmax ? p->E : gmax);
  const size_t shm = (size_t)vfm::lds_doubles(p->d, s.cap_dim) * 8;

  if (p->n_ops > 0) {
    if (int rc = vfm::launch_foldin_prep(sp, a, p->n_ops, p->op_x, ops, opc, st)) return rc;
    const unsigned nb = (unsigned)((p->n_ops + vfm::FB - 1) / vfm::FB);
    vfm::for_link(sp, [&](auto link) {
      hipLaunchKernelGGL(vfm::k_foldin_solve_prep<decltype(link)::value>, dim3(nb), dim3(vfm::FB), 0, st, p->n_ops, p->F,
                         p->d, p->col, p->T, p->op_x, p->entity_params, p->bias_params, p->scalars, ops64, cm64);
    });
    if (int rc = launch_status("k_foldin_solve_prep")) return rc;
  }
  vfm::launch(f, sp, s, grid, shm, st);
  return launch_status("k_foldin_solve");
}

}  // extern "C"

// vfm_foldin_split.hip -- the split exact solve (include/vfm_sweep.h, vfm_foldin_solve_split_f32): the exact fold-in of
// vfm_foldin_solve.hip for entities with many rows, their primal system assembled by one workgroup per chunk of rows.
//
// The operands are k_foldin_prep's and k_foldin_solve_prep's (launch_solve_preps).  Then, on one stream:
//   k_split_assemble   a workgroup per chunk.  The packed lower triangle of sum_r u_r u_r^T, u_r = (1, M_r), in 4 x 4
//                      register tiles: a thread owns a tile and walks the chunk's rows in order (8 loads, 16 fp64 FMAs a
//                      row; the lanes of a wave hold neighbouring tiles of one tile row, so the u_i are one address
//                      and the u_j consecutive).  Then a thread per coordinate for sum A, sum (A + M^2), sum t u, sum C
//                      (phase A of solve_body on the chunk's rows).  All into the chunk's slab:
//                      [triangle tri(d + 1) | SA [d + 1] | SB [d + 1] | sum t u [d + 1] | SC [d]].
//   k_split_solve      a workgroup per entity: the slabs of its chunks added in chunk order, D = kl + prec SA,
//                      H = prec T + diag(D), b = prec (sum t u - SC / 2), then chol_solve and put_params of
//                      vfm_foldin_solve_body.hpp (phases C and D of solve_body), the row written as k_foldin_solve does.
//   k_split_loss       a wave per chunk: the chunk's share of sum_r res_r^2 + sum_r c_var,r + sum_k (mu^2 SA + sigma^2 SB
//                      + mu SC) at the written fp32 row, fold_stage_rows and the residual chain of solve_body's phase E
//   k_split_loss_sum   a thread per entity: the shares in chunk order in fp64, the sigma_w, precision and KL terms
// Every sum has a fixed order that depends on the entity's rows, the chunk length and d alone: no atomics, no host sync.
//
// vfm_foldin_solve_split_prior_f32 (include/vfm_prior.h) runs the PRIOR = true instantiations of k_split_solve and
// k_split_loss_sum: the folded field's prior [2, d + 1] = mean | precision staged once per workgroup in LDS
// (D = kl lam + prec SA, b += kl lam m, the scales and the KL to that prior).  The preps, k_split_assemble and
// k_split_loss do not depend on the prior; the instantiations without it are the parent's, unchanged.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "vfm_args.hpp"
#include "vfm_sweep.h"
#include "vfm_prior.h"
#include "vfm_launch.hpp"            // launch_status

namespace vfm {
namespace {
#include "vfm_rng.hpp"
#include "vfm_common.hpp"

#include "vfm_foldin_body.hpp"       // FoldArgs, k_foldin_prep, fold_stage_rows, the host side
#include "vfm_foldin_solve_body.hpp" // tri, tri_decode, chol_solve, put_params, k_foldin_solve_prep, the operand block

constexpr int TL = 4;                    // edge of a register tile of the triangle

struct SplitArgs {
  FoldArgs f;                            // (E, R, T, d, klw, ent, row_op, y, ops / opc: the fp32 operands of the loss, loss)
  const double* ops64;                   // [n_ops, 3, d]  M | A | C, unrounded
  const double* cm64;                    // [n_ops]        c_mean
  const int64_t* chunk_ptr;              // [E + 1]
  const int64_t* chunks;                 // [n_chunks, 3]  entity number, first row, rows
  double* part;                          // [n_chunks, part_elems]
  double* lpart;                         // [n_chunks]     the chunks' shares of the loss
  SolveSlabs sl;                         // the slabs of k_split_solve's workgroups and the LDS rule of the triangle
  int64_t n_ops, n_chunks, part_elems;
  const float* prior;                    // [2, d + 1] mean | precision of the folded field (PRIOR instantiations only)
};

// chunk q's rows, clamped to [0, R)
__device__ __forceinline__ void chunk_rows_of(const SplitArgs& s, int64_t q, int64_t& r0, int64_t& n) {
  r0 = min(max(s.chunks[q * 3 + 1], (int64_t)0), s.f.R);
  n = min(max(s.chunks[q * 3 + 2], (int64_t)0), s.f.R - r0);
}

// entity g's chunks, clamped to the table
__device__ __forceinline__ void chunks_of(const SplitArgs& s, int64_t g, int64_t& c0, int64_t& c1) {
  c0 = min(max(s.chunk_ptr[g], (int64_t)0), s.n_chunks);
  c1 = min(max(s.chunk_ptr[g + 1], c0), s.n_chunks);
}

__global__ __launch_bounds__(FB) void k_split_assemble(const SplitArgs s) {
#pragma clang fp contract(on)
  const FoldArgs& a = s.f;
  const int tid = threadIdx.x;
  const int d = a.d, d1 = d + 1;
  const int64_t os = 3 * (int64_t)d;
  const int nb = (d1 + TL - 1) / TL;
  const int64_t nblk = tri(nb), nt = tri(d1);
  const double qnan = __builtin_nan("");

  for (int64_t q = blockIdx.x; q < s.n_chunks; q += gridDim.x) {
    int64_t r0, n;
    chunk_rows_of(s, q, r0, n);
    double* P = s.part + q * s.part_elems;

    // ---- the triangle, a 4 x 4 tile per thread, rows in order
    for (int64_t b = tid; b < nblk; b += FB) {
      int bi, bj;
      tri_decode(b, bi, bj);
      const int i0 = bi * TL, j0 = bj * TL;
      int xi[TL], xj[TL];                // column of M behind u_i (clamped into the row), u_0 = 1, u past d = 0
#pragma unroll
      for (int t = 0; t < TL; ++t) {
        xi[t] = min(max(i0 + t - 1, 0), d - 1);
        xj[t] = min(max(j0 + t - 1, 0), d - 1);
      }
      double acc[TL][TL];
#pragma unroll
      for (int u = 0; u < TL; ++u)
#pragma unroll
        for (int v = 0; v < TL; ++v) acc[u][v] = 0.;
      bool bad = false;
      for (int64_t r = 0; r < n; ++r) {
        const int64_t o = a.row_op[r0 + r];
        if (o < 0 || o >= s.n_ops) { bad = true; continue; }      // (uniform over the block)
        const double* M = s.ops64 + o * os;
        double ui[TL], uj[TL];
#pragma unroll
        for (int t = 0; t < TL; ++t) {
          const double vi = M[xi[t]], vj = M[xj[t]];
          ui[t] = i0 + t == 0 ? 1.0 : i0 + t < d1 ? vi : 0.0;
          uj[t] = j0 + t == 0 ? 1.0 : j0 + t < d1 ? vj : 0.0;
        }
#pragma unroll
        for (int u = 0; u < TL; ++u)
#pragma unroll
          for (int v = 0; v < TL; ++v) acc[u][v] += ui[u] * uj[v];
      }
#pragma unroll
      for (int u = 0; u < TL; ++u)
#pragma unroll
        for (int v = 0; v < TL; ++v) {
          const int i = i0 + u, j = j0 + v;
          if (i < d1 && j <= i) P[tri(i) + j] = bad ? qnan : acc[u][v];
        }
    }

    // ---- the row sums of each coordinate (solve_body's phase A on the chunk's rows)
    for (int c = tid; c < d1; c += FB) {
      double SA = 0., SB = 0., SC = 0., bM = 0.;
      bool bad = false;
      if (c == 0) {
        for (int64_t r = 0; r < n; ++r) {
          const int64_t o = a.row_op[r0 + r];
          if (o < 0 || o >= s.n_ops) { bad = true; continue; }
          bM += (double)a.y[r0 + r] - s.cm64[o];
        }
        SB = (double)n;
      } else {
        for (int64_t r = 0; r < n; ++r) {
          const int64_t o = a.row_op[r0 + r];
          if (o < 0 || o >= s.n_ops) { bad = true; continue; }
          const double* op = s.ops64 + o * os + (c - 1);
          const double M = op[0], A = op[d], C = op[2 * d];
          const double t = (double)a.y[r0 + r] - s.cm64[o];
          SA += A;
          SB += A + M * M;
          SC += C;
          bM += t * M;
        }
      }
      P[nt + c] = bad ? qnan : SA;
      P[nt + d1 + c] = bad ? qnan : SB;
      P[nt + 2 * d1 + c] = bad ? qnan : bM;
      if (c > 0) P[nt + 3 * d1 + c - 1] = bad ? qnan : SC;
    }
  }
}

template <int LINK, bool PRIOR>
__global__ __launch_bounds__(FB) void k_split_solve(const SplitArgs s) {
#pragma clang fp contract(on)
  extern __shared__ double sm_all[];
  const FoldArgs& a = s.f;
  const int tid = threadIdx.x;
  const int d = a.d, d1 = d + 1;
  double* sm = sm_all + (PRIOR ? 2 * d1 : 0);              // (the prior in front: lds_doubles_prior)
  const double* pr = sm_all;                               // (PRIOR only) m [d + 1] | lam [d + 1]
  if constexpr (PRIOR) {
    stage_prior(s.prior, sm_all, d1);
    __syncthreads();
  }
  double* Dd = sm;                       // solve_body's layout: D | . | . | right-hand side | 1 / L_jj | solution | SB | fp32
  double* yv = Dd + 3 * d1;
  double* dv = yv + d1;
  double* xv = dv + d1;
  double* SBd = xv + d1;
  float* pf = (float*)(SBd + d1);
  double* Hl = sm + 8 * d1;
  double* Hg = s.sl.slab ? s.sl.slab + (int64_t)blockIdx.x * s.sl.slab_elems : nullptr;
  double* Hm = d1 <= s.sl.cap_dim ? Hl : Hg;
  const double prec = link_d<LINK>(a.scal[0]);
  const double kl = a.klw;
  const int64_t nt = tri(d1);

  for (int64_t g = blockIdx.x; g < a.E; g += gridDim.x) {
    const int64_t e = a.ent[g];
    if (e < 0 || e >= a.T || !Hm) continue;                // (block-uniform; k_split_loss_sum writes the NaN loss)
    int64_t c0, c1;
    chunks_of(s, g, c0, c1);
    for (int c = tid; c < d1; c += FB) {
      double SA = 0., SB = 0., SC = 0., bM = 0.;
      for (int64_t q = c0; q < c1; ++q) {
        const double* V = s.part + q * s.part_elems + nt;
        SA += V[c];
        SB += V[d1 + c];
        bM += V[2 * d1 + c];
        if (c > 0) SC += V[3 * d1 + c - 1];
      }
      if constexpr (PRIOR) {
        const double kll = kl * pr[d1 + c], b0 = prec * (bM - 0.5 * SC);
        Dd[c] = kll + prec * SA;
        yv[c] = b0 + kll * pr[c];
      } else {
        Dd[c] = kl + prec * SA;
        yv[c] = prec * (bM - 0.5 * SC);
      }
      SBd[c] = SB;
    }
    __syncthreads();
    for (int64_t p = tid; p < nt; p += FB) {
      int i, j;
      tri_decode(p, i, j);
      double acc = 0.;
      for (int64_t q = c0; q < c1; ++q) acc += s.part[q * s.part_elems + p];
      Hm[p] = prec * acc + (i == j ? Dd[i] : 0.0);
    }
    __syncthreads();
    chol_solve(Hm, yv, dv, xv, d1);
    for (int c = tid; c < d1; c += FB) {
      if constexpr (PRIOR) put_params<LINK, true>(pf, d1, c, xv[c], kl, prec, SBd[c], kl * pr[d1 + c]);
      else put_params<LINK>(pf, d1, c, xv[c], kl, prec, SBd[c]);
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
    __syncthreads();                     // (the vectors and pf are rewritten by the next entity)
  }
}

// a chunk's rows for fold_stage_rows, the operand clamped into the table (a row whose operand is outside it has made
// the entity's row NaN in the assembly already)
struct SplitRows {
  const FoldArgs& a;
  int64_t r0, n_ops;
  __device__ __forceinline__ int64_t op(int64_t i) const { return min(max(a.row_op[r0 + i], (int64_t)0), n_ops - 1); }
  __device__ __forceinline__ float y(int64_t i) const { return a.y[r0 + i]; }
};

template <int W, int CPL, int LINK>
__global__ __launch_bounds__(64) void k_split_loss(const SplitArgs s) {
#pragma clang fp contract(on)
  constexpr int DP = W * CPL;
  const FoldArgs& a = s.f;
  const int lane = threadIdx.x, l = lane % W;
  const int d = a.d;
  for (int64_t q = blockIdx.x; q < s.n_chunks; q += gridDim.x) {
    const int64_t g = s.chunks[q * 3];
    int64_t r0, n;
    chunk_rows_of(s, q, r0, n);
    const int64_t e = g >= 0 && g < a.E ? a.ent[g] : -1;
    if (e < 0 || e >= a.T || s.n_ops < 1) {                // (wave-uniform)
      if (lane == 0) s.lpart[q] = 0.;
      continue;
    }
    float mu[CPL], sg[CPL], SA[CPL], SB[CPL], SC[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      const int kc = j * W + l;
      const bool vk = kc < d;
      mu[j] = vk ? a.entity[e * 2 * d + kc] : 0.f;
      sg[j] = link_f<LINK>(vk ? a.entity[e * 2 * d + d + kc] : prior_s<LINK>());
      SA[j] = SB[j] = SC[j] = 0.f;
    }
    const float muw = a.bias[e * 2];
    float Scv = 0.f, rsq = 0.f;
    const SplitRows rows{a, r0, s.n_ops};
    fold_stage_rows<W, CPL>(a, rows, 0, n, l, nullptr, nullptr, SA, SB, SC, Scv);     // (a.cap = 0: nothing staged)
    for (int64_t i = 0; i < n; ++i) {
      const int64_t o = rows.op(i);
      float p = 0.f;
#pragma unroll
      for (int j = 0; j < CPL; ++j) p = fmaf(mu[j], a.ops[o * 3 * DP + j * W + l], p);
      const float res = ((a.opc[o * 2] - rows.y(i)) + muw) + group_sum<W>(p);
      rsq = fmaf(res, res, rsq);
    }
    float vq = 0.f;
#pragma unroll
    for (int j = 0; j < CPL; ++j) vq += fmaf(mu[j] * mu[j], SA[j], fmaf(sg[j] * sg[j], SB[j], mu[j] * SC[j]));
    vq = group_sum<W>(vq);
    if (lane == 0) s.lpart[q] = ((double)rsq + (double)Scv) + (double)vq;
  }
}

template <int LINK, bool PRIOR>
__global__ __launch_bounds__(FB) void k_split_loss_sum(const SplitArgs s) {
#pragma clang fp contract(on)
  const FoldArgs& a = s.f;
  const int d = a.d;
  __shared__ float prs[PRIOR ? 2 * (VFM_FOLDIN_MAX_D + 1) : 1];          // (PRIOR) m [d + 1] | sqrt(lam) [d + 1]
  if constexpr (PRIOR) {
    for (int c = threadIdx.x; c <= d; c += FB) {
      prs[c] = s.prior[c];
      prs[d + 1 + c] = sqrtf(s.prior[d + 1 + c]);
    }
    __syncthreads();
  }
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= a.E) return;
  const int64_t e = a.ent[g];
  if (e < 0 || e >= a.T) {
    a.loss[g] = __builtin_nanf("");
    return;
  }
  int64_t c0, c1;
  chunks_of(s, g, c0, c1);
  double sum = 0.;
  int64_t n = 0;
  for (int64_t q = c0; q < c1; ++q) {
    int64_t r0, nq;
    chunk_rows_of(s, q, r0, nq);
    sum += s.lpart[q];
    n += nq;
  }
  const float precf = link_f<LINK>(a.scal[0]);
  const float muw = a.bias[e * 2], sgw = link_f<LINK>(a.bias[e * 2 + 1]);
  double klq;
  if constexpr (PRIOR) {
    klq = kl_prior_normal(muw, sgw, prs[0], prs[d + 1]);
    for (int k = 0; k < d; ++k)
      klq += kl_prior_normal(a.entity[e * 2 * d + k], link_f<LINK>(a.entity[e * 2 * d + d + k]), prs[1 + k], prs[d + 2 + k]);
  } else {
    klq = kl_std_normal(muw, sgw);
    for (int k = 0; k < d; ++k) klq += kl_std_normal(a.entity[e * 2 * d + k], link_f<LINK>(a.entity[e * 2 * d + d + k]));
  }
  const double sumv = sum + (double)n * sgw * sgw;
  const double lsum = 0.5 * precf * sumv + (double)n * ((double)LOG_2PI_HALF - 0.5 * log((double)precf));
  a.loss[g] = (float)(lsum + (double)a.klw * klq);
}

}  // namespace
}  // namespace vfm

static int split_call(const vfm_foldin_split_t* p, const float* prior, void* stream);

extern "C" {

int64_t vfm_foldin_split_workspace_bytes(int64_t n_chunks, int64_t n_heavy, int64_t n_ops, int32_t d, int32_t lds_dim) {
  const int64_t lim = (int64_t)1 << 40;                    // (every product below stays under 2^62)
  if (n_chunks < 0 || n_heavy < 0 || n_ops < 0 || n_chunks > lim || n_heavy > lim || n_ops > lim || d < 1 ||
      d > VFM_FOLDIN_MAX_D || lds_dim < -1)
    return VFM_E_INVALID;
  return vfm::off_slabs(n_ops, d) + vfm::part_bytes(n_chunks, d) + vfm::lpart_bytes(n_chunks) +
         vfm::slabs_bytes(n_heavy, d, lds_dim);
}

int64_t vfm_foldin_split_prior_workspace_bytes(int64_t n_chunks, int64_t n_heavy, int64_t n_ops, int32_t d,
                                               int32_t lds_dim) {
  // (the prior lives in LDS, not in the workspace)
  return vfm_foldin_split_workspace_bytes(n_chunks, n_heavy, n_ops, d, lds_dim);
}

int vfm_foldin_solve_split_f32(const vfm_foldin_split_t* p, void* stream) { return split_call(p, nullptr, stream); }

int vfm_foldin_solve_split_prior_f32(const vfm_foldin_split_t* p, const float* prior, void* stream) {
  return split_call(p, prior, stream);
}

}  // extern "C"

// both entry points: prior == NULL is vfm_foldin_solve_split_f32
static int split_call(const vfm_foldin_split_t* p, const float* prior, void* stream) {
  if (!p) return vfm::fail(VFM_E_INVALID, "vfm_foldin_solve_split_f32: NULL argument struct");
  const int64_t ws = vfm_foldin_split_workspace_bytes(p->n_chunks, p->E, p->n_ops, p->d, p->lds_dim);
  const auto own = [&]() -> const char* { return p->n_chunks < 0 ? "n_chunks < 0" : nullptr; };
  if (int rc = vfm::check_solve(p, p->chunk_ptr, p->n_chunks <= 0 || p->chunks, ws, "vfm_foldin_split_workspace_bytes", own))
    return rc;
  if (p->E == 0) return 0;

  const hipStream_t st = (hipStream_t)stream;
  const bool sp = (p->flags & VFM_FLAG_LINK_SOFTPLUS) != 0;
  const vfm::FShape f = vfm::shape_of(p->d);
  vfm::SplitArgs s = {};
  vfm::fill_solve_args(s, p, VFM_LIK_NORMAL, 0, 0, VFM_FOLDIN_FIT);
  const vfm::FoldArgs& a = s.f;
  char* w = (char*)p->workspace;
  const vfm::SplitGrids grid = vfm::place_split(s, p, w + vfm::off_slabs(p->n_ops, p->d));
  s.prior = prior;
  const size_t shm = (size_t)(prior ? vfm::lds_doubles_prior(p->d, s.sl.cap_dim) : vfm::lds_doubles(p->d, s.sl.cap_dim)) * 8;

  if (p->n_ops > 0) {
    if (int rc = vfm::launch_solve_preps(sp, a, p->n_ops, p->op_x, w, st)) return rc;
  }
  if (p->n_chunks > 0) {
    hipLaunchKernelGGL(vfm::k_split_assemble, dim3(grid.c), dim3(vfm::FB), 0, st, s);
    if (int rc = launch_status("k_split_assemble")) return rc;
  }
  vfm::for_link(sp, [&](auto link) {
    const auto k = prior ? vfm::k_split_solve<decltype(link)::value, true> : vfm::k_split_solve<decltype(link)::value, false>;
    vfm::launch_lds(k, grid.e, shm, st, s);
  });
  if (int rc = launch_status("k_split_solve")) return rc;
  if (p->n_chunks > 0) {
    vfm::for_link(sp, [&](auto link) {
      vfm::for_shape(f, [&](auto wd, auto c) {
        hipLaunchKernelGGL((vfm::k_split_loss<decltype(wd)::value, decltype(c)::value, decltype(link)::value>),
                           dim3(grid.c), dim3(64), 0, st, s);
      });
    });
    if (int rc = launch_status("k_split_loss")) return rc;
  }
  vfm::for_link(sp, [&](auto link) {
    const auto k = prior ? vfm::k_split_loss_sum<decltype(link)::value, true> : vfm::k_split_loss_sum<decltype(link)::value, false>;
    hipLaunchKernelGGL(k, dim3((unsigned)((p->E + vfm::FB - 1) / vfm::FB)), dim3(vfm::FB), 0, st, s);
  });
  return launch_status("k_split_loss_sum");
}

// vfm_foldin_bound_split.hip -- the split bound rounds (include/vfm_bound_sweep.h, vfm_foldin_bound_split_f32): the bound
// fold-in of vfm_foldin_bound.hip for entities with many rows, each round's primal system assembled by one workgroup per
// chunk of rows.  It is k_split_assemble's idea (vfm_foldin_split.hip) with a weight per row that changes every round.
//
// The operands are launch_solve_preps' and launch_bound_prep's.  Then, on one stream:
//   k_bsplit_start     a thread per (entity, coordinate): the fp64 iterate theta | sigma^2 from the entity's fp32 row
//                      through the link in fp64, or mu = 0, sigma^2 = 1 with reset (bound_body's start)
//   and per round
//   k_bsplit_assemble  a workgroup per chunk.  Its entity's iterate staged in LDS (2 (d + 1) doubles); phase X of
//                      bound_body on the chunk's rows, a wave per row, w_r into the workspace at the row's own index;
//                      after a barrier the packed lower triangle of sum_r w_r u_r u_r^T in the 4 x 4 register tiles of
//                      k_split_assemble (w_r u_i formed once per row and tile row), then a thread per coordinate for
//                      sum w A, sum w (A + M^2) (coordinate 0: sum w), sum ((y - 1/2) - w c_mean) u, sum w C.  All into
//                      the chunk's slab: [triangle tri(d + 1) | SA [d + 1] | SB [d + 1] | b [d + 1] | SC [d]].
//   k_bsplit_solve     a workgroup per entity: the slabs of its chunks added in chunk order, D = kl + SA,
//                      H = T + diag(D), b - (0, SC / 2), chol_solve of vfm_foldin_solve_body.hpp as it stands; theta and
//                      sigma^2 = kl / (kl + SB) back to the iterate; on the last round put_params (prec = 1) and the
//                      table row, as k_foldin_bound writes it: the iterate is rounded to fp32 once
//   then
//   k_bsplit_loss      a wave per chunk: each row's term of bound_loss at the written fp32 row, the rows added in row
//                      order in fp64
//   k_bsplit_loss_sum  a thread per entity: the chunks' shares in chunk order, plus kl KL
// Rounds are separated by kernel boundaries: no atomics, no host sync, no cooperative launch, no grid-wide barrier.
// Every sum has a fixed order that depends on the entity's rows, the chunk length and d alone.
//
// vfm_foldin_bound_split_prior_f32 (include/vfm_bound_prior.h) runs the PRIOR = true instantiations of k_bsplit_start (the
// reset start mu = m, sigma^2 = 1 / lam), k_bsplit_solve (D = kl lam + SA, b += kl lam m, sigma^2 = kl / (kl lam + SB); the
// prior [2, d + 1] = mean | precision staged once per workgroup in fp64 in LDS) and k_bsplit_loss_sum (the KL to that
// prior).  The preps, k_bsplit_assemble and k_bsplit_loss do not read the prior; the instantiations without it are the
// parent's, unchanged.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "vfm_args.hpp"
#include "vfm_bound_sweep.h"
#include "vfm_bound_prior.h"
#include "vfm_launch.hpp"            // launch_status

namespace vfm {
namespace {
#include "vfm_rng.hpp"
#include "vfm_common.hpp"

#include "vfm_foldin_body.hpp"       // FoldArgs, k_foldin_prep, fold_stage_rows, the host side
#include "vfm_foldin_solve_body.hpp" // tri, tri_decode, wave_sum_d, chol_solve, put_params, the operand block, the slabs
#include "vfm_foldin_bound_body.hpp" // k_foldin_bound_prep, launch_bound_prep

constexpr int TL = 4;                    // edge of a register tile of the triangle (k_split_assemble's)

struct BSplitArgs {
  FoldArgs f;                            // (E, R, T, d, klw, reset, ent, row_op, y, ops / opc: the fp32 operands of the loss)
  const double* ops64;                   // [n_ops, 3, d]  M | A | C, unrounded
  const double* cm64;                    // [n_ops]        c_mean
  const double* cv64;                    // [n_ops]        c_var
  double* wrow;                          // [R]            w_r of the round in flight
  double* iter;                          // [E, 2 (d + 1)] theta | sigma^2
  const int64_t* chunk_ptr;              // [E + 1]
  const int64_t* chunks;                 // [n_chunks, 3]  entity number, first row, rows
  double* part;                          // [n_chunks, part_elems]
  double* lpart;                         // [n_chunks]     the chunks' shares of the loss
  SolveSlabs sl;                         // the slabs of k_bsplit_solve's workgroups and the LDS rule of the triangle
  int64_t n_ops, n_chunks, part_elems;
  int32_t last;                          // k_bsplit_solve: the last round, the table row is written
  const float* prior;                    // [2, d + 1] mean | precision of the folded field (PRIOR instantiations only)
};

// chunk q's rows, clamped to [0, R)
__device__ __forceinline__ void chunk_rows_of(const BSplitArgs& s, int64_t q, int64_t& r0, int64_t& n) {
  r0 = min(max(s.chunks[q * 3 + 1], (int64_t)0), s.f.R);
  n = min(max(s.chunks[q * 3 + 2], (int64_t)0), s.f.R - r0);
}

// entity g's chunks, clamped to the table
__device__ __forceinline__ void chunks_of(const BSplitArgs& s, int64_t g, int64_t& c0, int64_t& c1) {
  c0 = min(max(s.chunk_ptr[g], (int64_t)0), s.n_chunks);
  c1 = min(max(s.chunk_ptr[g + 1], c0), s.n_chunks);
}

template <int LINK, bool PRIOR>
__global__ __launch_bounds__(FB) void k_bsplit_start(const BSplitArgs s) {
#pragma clang fp contract(on)
  const FoldArgs& a = s.f;
  const int d = a.d, d1 = d + 1;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.E * d1) return;
  const int64_t g = i / d1;
  const int c = (int)(i - g * d1);
  const int64_t e = a.ent[g];
  double t0 = 0., v0 = 1.;
  if constexpr (PRIOR) {                 // (the fp32 prior read in fp64)
    t0 = (double)s.prior[c];
    v0 = 1.0 / (double)s.prior[d1 + c];
  }
  if (!a.reset && e >= 0 && e < a.T) {
    const float m = c ? a.entity[e * 2 * d + c - 1] : a.bias[e * 2];
    const float sf = c ? a.entity[e * 2 * d + d + c - 1] : a.bias[e * 2 + 1];
    const double sg = link_d<LINK>(sf);
    t0 = m;
    v0 = sg * sg;
  }
  s.iter[g * 2 * d1 + c] = t0;
  s.iter[g * 2 * d1 + d1 + c] = v0;
}

__global__ __launch_bounds__(FB) void k_bsplit_assemble(const BSplitArgs s) {
#pragma clang fp contract(on)
  __shared__ double it[2 * (VFM_FOLDIN_MAX_D + 1)];        // the entity's iterate: theta [d + 1] | sigma^2 [d + 1]
  const FoldArgs& a = s.f;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int d = a.d, d1 = d + 1;
  const int64_t os = 3 * (int64_t)d;
  const int nb = (d1 + TL - 1) / TL;
  const int64_t nblk = tri(nb), nt = tri(d1);
  const double qnan = __builtin_nan("");
  const double* th = it;
  const double* sg2 = it + d1;

  for (int64_t q = blockIdx.x; q < s.n_chunks; q += gridDim.x) {
    int64_t r0, n;
    chunk_rows_of(s, q, r0, n);
    const int64_t g = s.chunks[q * 3];
    const bool okg = g >= 0 && g < a.E;                    // (block-uniform; a chunk of no entity: a NaN slab, no weights)
    double* P = s.part + q * s.part_elems;
    if (!okg) {
      for (int64_t p = tid; p < s.part_elems; p += FB) P[p] = qnan;
      continue;
    }
    for (int c = tid; c < 2 * d1; c += FB) it[c] = s.iter[g * 2 * d1 + c];
    __syncthreads();

    // ---- X: the rows' weights at the iterate (bound_body's phase X on the chunk's rows)
    for (int64_t r = wv; r < n; r += FB / 64) {
      const int64_t o = a.row_op[r0 + r];
      double w = qnan;
      if (o >= 0 && o < s.n_ops) {                         // (wave-uniform)
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
        x2 = x2 < 0. ? 0. : x2;          // (a NaN stays a NaN)
        const double xi = sqrt(x2);
        w = xi < 1e-3 ? 0.25 - x2 / 48.0 : tanh(0.5 * xi) / (2.0 * xi);
      }
      if (lane == 0) s.wrow[r0 + r] = w;
    }
    __syncthreads();                     // (the weights are read back by the whole workgroup)

    // ---- the weighted triangle, a 4 x 4 tile per thread, rows in order
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
        const double w = s.wrow[r0 + r];
        double wu[TL], uj[TL];
#pragma unroll
        for (int t = 0; t < TL; ++t) {
          const double vi = M[xi[t]], vj = M[xj[t]];
          const double ui = i0 + t == 0 ? 1.0 : i0 + t < d1 ? vi : 0.0;
          wu[t] = w * ui;
          uj[t] = j0 + t == 0 ? 1.0 : j0 + t < d1 ? vj : 0.0;
        }
#pragma unroll
        for (int u = 0; u < TL; ++u)
#pragma unroll
          for (int v = 0; v < TL; ++v) acc[u][v] += wu[u] * uj[v];
      }
#pragma unroll
      for (int u = 0; u < TL; ++u)
#pragma unroll
        for (int v = 0; v < TL; ++v) {
          const int i = i0 + u, j = j0 + v;
          if (i < d1 && j <= i) P[tri(i) + j] = bad ? qnan : acc[u][v];
        }
    }

    // ---- the weighted row sums of each coordinate (bound_body's phase A on the chunk's rows)
    for (int c = tid; c < d1; c += FB) {
      double SA = 0., SB = 0., SC = 0., bM = 0.;
      bool bad = false;
      if (c == 0) {
        for (int64_t r = 0; r < n; ++r) {
          const int64_t o = a.row_op[r0 + r];
          if (o < 0 || o >= s.n_ops) { bad = true; continue; }
          const double w = s.wrow[r0 + r];
          SB += w;
          bM += ((double)a.y[r0 + r] - 0.5) - w * s.cm64[o];
        }
      } else {
        for (int64_t r = 0; r < n; ++r) {
          const int64_t o = a.row_op[r0 + r];
          if (o < 0 || o >= s.n_ops) { bad = true; continue; }
          const double* op = s.ops64 + o * os + (c - 1);
          const double M = op[0], A = op[d], C = op[2 * d], w = s.wrow[r0 + r];
          const double t = ((double)a.y[r0 + r] - 0.5) - w * s.cm64[o];
          SA += w * A;
          SB += w * (A + M * M);
          SC += w * C;
          bM += t * M;
        }
      }
      P[nt + c] = bad ? qnan : SA;
      P[nt + d1 + c] = bad ? qnan : SB;
      P[nt + 2 * d1 + c] = bad ? qnan : bM;
      if (c > 0) P[nt + 3 * d1 + c - 1] = bad ? qnan : SC;
    }
    __syncthreads();                     // (the iterate in LDS is rewritten by the next chunk)
  }
}

template <int LINK, bool PRIOR>
__global__ __launch_bounds__(FB) void k_bsplit_solve(const BSplitArgs s) {
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
  const double kl = a.klw;
  const int64_t nt = tri(d1);

  for (int64_t g = blockIdx.x; g < a.E; g += gridDim.x) {
    const int64_t e = a.ent[g];
    if (e < 0 || e >= a.T || !Hm) continue;                // (block-uniform; k_bsplit_loss_sum writes the NaN loss)
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
        const double kll = kl * pr[d1 + c], b0 = bM - 0.5 * SC;
        Dd[c] = kll + SA;
        yv[c] = b0 + kll * pr[c];
      } else {
        Dd[c] = kl + SA;
        yv[c] = bM - 0.5 * SC;
      }
      SBd[c] = SB;
    }
    __syncthreads();
    for (int64_t p = tid; p < nt; p += FB) {
      int i, j;
      tri_decode(p, i, j);
      double acc = 0.;
      for (int64_t q = c0; q < c1; ++q) acc += s.part[q * s.part_elems + p];
      Hm[p] = acc + (i == j ? Dd[i] : 0.0);
    }
    __syncthreads();
    chol_solve(Hm, yv, dv, xv, d1);
    double* itg = s.iter + g * 2 * d1;
    for (int c = tid; c < d1; c += FB) {
      itg[c] = xv[c];
      if constexpr (PRIOR) {
        const double kll = kl * pr[d1 + c];
        itg[d1 + c] = kl / (kll + SBd[c]);
        if (s.last) put_params<LINK, true>(pf, d1, c, xv[c], kl, 1.0, SBd[c], kll);
      } else {
        itg[d1 + c] = kl / (kl + SBd[c]);
        if (s.last) put_params<LINK>(pf, d1, c, xv[c], kl, 1.0, SBd[c]);
      }
    }
    __syncthreads();
    if (s.last) {                        // the table row, rounded once
      for (int k = tid; k < d; k += FB) {
        a.entity[e * 2 * d + k] = pf[1 + k];
        a.entity[e * 2 * d + d + k] = pf[d1 + 1 + k];
      }
      if (tid == 0) {
        a.bias[e * 2] = pf[0];
        a.bias[e * 2 + 1] = pf[d1];
      }
    }
    __syncthreads();                     // (the vectors and pf are rewritten by the next entity)
  }
}

// a chunk's rows for fold_stage_rows, the operand clamped into the table (a row whose operand is outside it has made
// the entity's row NaN in the assembly already)
struct BSplitRows {
  const FoldArgs& a;
  int64_t r0, n_ops;
  __device__ __forceinline__ int64_t op(int64_t i) const { return min(max(a.row_op[r0 + i], (int64_t)0), n_ops - 1); }
  __device__ __forceinline__ float y(int64_t i) const { return a.y[r0 + i]; }
};

template <int W, int CPL, int LINK>
__global__ __launch_bounds__(64) void k_bsplit_loss(const BSplitArgs s) {
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
    float mu[CPL], sg[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      const int kc = j * W + l;
      const bool vk = kc < d;
      mu[j] = vk ? a.entity[e * 2 * d + kc] : 0.f;
      sg[j] = link_f<LINK>(vk ? a.entity[e * 2 * d + d + kc] : prior_s<LINK>());
    }
    const float muw = a.bias[e * 2], sgw = link_f<LINK>(a.bias[e * 2 + 1]);
    const BSplitRows rows{a, r0, s.n_ops};
    double lsum = 0.0;
    for (int64_t i = 0; i < n; ++i) {    // (bound_loss's row term, expression for expression)
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
      x2 = x2 < 0.f ? 0.f : x2;          // (a NaN stays a NaN)
      const float xi = sqrtf(x2);
      const float t = -(rows.y(i) - 0.5f) * Ef + 0.5f * xi + log1pf(expf(-xi));
      lsum += (double)t;
    }
    if (lane == 0) s.lpart[q] = lsum;
  }
}

template <int LINK, bool PRIOR>
__global__ __launch_bounds__(FB) void k_bsplit_loss_sum(const BSplitArgs s) {
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
  for (int64_t q = c0; q < c1; ++q) sum += s.lpart[q];
  double klq;
  if constexpr (PRIOR) {
    klq = kl_prior_normal(a.bias[e * 2], link_f<LINK>(a.bias[e * 2 + 1]), prs[0], prs[d + 1]);
    for (int k = 0; k < d; ++k)
      klq += kl_prior_normal(a.entity[e * 2 * d + k], link_f<LINK>(a.entity[e * 2 * d + d + k]), prs[1 + k], prs[d + 2 + k]);
  } else {
    klq = kl_std_normal(a.bias[e * 2], link_f<LINK>(a.bias[e * 2 + 1]));
    for (int k = 0; k < d; ++k) klq += kl_std_normal(a.entity[e * 2 * d + k], link_f<LINK>(a.entity[e * 2 * d + d + k]));
  }
  a.loss[g] = (float)(sum + (double)a.klw * klq);
}

// the workspace: [operand block | c_var | row weights | iterate | chunk slabs | loss partials | solve slabs]
// (vfm_foldin_bound_body.hpp: off_cv64, off_wrow, off_bound_own -- the iterate; vfm_foldin_solve_body.hpp: the rest)
inline int64_t off_part(int64_t n_heavy, int64_t R, int64_t n_ops, int d) {
  return off_bound_own(R, n_ops, d) + round_up(n_heavy * 2 * (int64_t)(d + 1) * 8, 256);
}

}  // namespace
}  // namespace vfm

static int bsplit_call(const vfm_foldin_bound_split_t* p, const float* prior, void* stream);

extern "C" {

int64_t vfm_foldin_bound_split_workspace_bytes(int64_t n_chunks, int64_t n_heavy, int64_t R, int64_t n_ops, int32_t d,
                                               int32_t lds_dim) {
  const int64_t lim = (int64_t)1 << 40;                    // (every product below stays under 2^62)
  if (n_chunks < 0 || n_heavy < 0 || R < 0 || n_ops < 0 || n_chunks > lim || n_heavy > lim || R > lim || n_ops > lim ||
      d < 1 || d > VFM_FOLDIN_MAX_D || lds_dim < -1)
    return VFM_E_INVALID;
  return vfm::off_part(n_heavy, R, n_ops, d) + vfm::part_bytes(n_chunks, d) + vfm::lpart_bytes(n_chunks) +
         vfm::slabs_bytes(n_heavy, d, lds_dim);
}

int64_t vfm_foldin_bound_split_prior_workspace_bytes(int64_t n_chunks, int64_t n_heavy, int64_t R, int64_t n_ops,
                                                     int32_t d, int32_t lds_dim) {
  // (the prior lives in LDS, not in the workspace)
  return vfm_foldin_bound_split_workspace_bytes(n_chunks, n_heavy, R, n_ops, d, lds_dim);
}

int vfm_foldin_bound_split_f32(const vfm_foldin_bound_split_t* p, void* stream) { return bsplit_call(p, nullptr, stream); }

int vfm_foldin_bound_split_prior_f32(const vfm_foldin_bound_split_t* p, const float* prior, void* stream) {
  return bsplit_call(p, prior, stream);
}

}  // extern "C"

// both entry points: prior == NULL is vfm_foldin_bound_split_f32
static int bsplit_call(const vfm_foldin_bound_split_t* p, const float* prior, void* stream) {
  if (!p) return vfm::fail(VFM_E_INVALID, "vfm_foldin_bound_split_f32: NULL argument struct");
  const int64_t ws = vfm_foldin_bound_split_workspace_bytes(p->n_chunks, p->E, p->R, p->n_ops, p->d, p->lds_dim);
  const auto own = [&]() -> const char* {
    if (p->n_chunks < 0) return "n_chunks < 0";
    return p->n_iters < 1 ? "n_iters must be >= 1" : nullptr;
  };
  if (int rc = vfm::check_solve(p, p->chunk_ptr, p->n_chunks <= 0 || p->chunks, ws, "vfm_foldin_bound_split_workspace_bytes",
                                own))
    return rc;
  if (p->E == 0) return 0;

  const hipStream_t st = (hipStream_t)stream;
  const bool sp = (p->flags & VFM_FLAG_LINK_SOFTPLUS) != 0;
  const vfm::FShape f = vfm::shape_of(p->d);
  vfm::BSplitArgs s = {};
  vfm::fill_bound_args(s, p, VFM_FOLDIN_FIT);
  const vfm::FoldArgs& a = s.f;
  char* w = (char*)p->workspace;
  s.iter = (double*)(w + vfm::off_bound_own(p->R, p->n_ops, p->d));
  const vfm::SplitGrids grid = vfm::place_split(s, p, w + vfm::off_part(p->E, p->R, p->n_ops, p->d));
  s.prior = prior;
  const size_t shm = (size_t)(prior ? vfm::lds_doubles_prior(p->d, s.sl.cap_dim) : vfm::lds_doubles(p->d, s.sl.cap_dim)) * 8;

  if (p->n_ops > 0) {
    if (int rc = vfm::launch_solve_preps(sp, a, p->n_ops, p->op_x, w, st)) return rc;
    if (int rc = vfm::launch_bound_prep(sp, a, p->n_ops, p->op_x, const_cast<double*>(s.cv64), st)) return rc;
  }
  const int64_t n_it = p->E * (int64_t)(p->d + 1);
  vfm::for_link(sp, [&](auto link) {
    const auto k = prior ? vfm::k_bsplit_start<decltype(link)::value, true> : vfm::k_bsplit_start<decltype(link)::value, false>;
    hipLaunchKernelGGL(k, dim3((unsigned)((n_it + vfm::FB - 1) / vfm::FB)), dim3(vfm::FB), 0, st, s);
  });
  if (int rc = launch_status("k_bsplit_start")) return rc;
  for (int it = 0; it < p->n_iters; ++it) {
    s.last = it == p->n_iters - 1;
    if (p->n_chunks > 0) {
      hipLaunchKernelGGL(vfm::k_bsplit_assemble, dim3(grid.c), dim3(vfm::FB), 0, st, s);
      if (int rc = launch_status("k_bsplit_assemble")) return rc;
    }
    vfm::for_link(sp, [&](auto link) {
      const auto k = prior ? vfm::k_bsplit_solve<decltype(link)::value, true> : vfm::k_bsplit_solve<decltype(link)::value, false>;
      vfm::launch_lds(k, grid.e, shm, st, s);
    });
    if (int rc = launch_status("k_bsplit_solve")) return rc;
  }
  if (p->n_chunks > 0) {
    vfm::for_link(sp, [&](auto link) {
      vfm::for_shape(f, [&](auto wd, auto c) {
        hipLaunchKernelGGL((vfm::k_bsplit_loss<decltype(wd)::value, decltype(c)::value, decltype(link)::value>),
                           dim3(grid.c), dim3(64), 0, st, s);
      });
    });
    if (int rc = launch_status("k_bsplit_loss")) return rc;
  }
  vfm::for_link(sp, [&](auto link) {
    const auto k = prior ? vfm::k_bsplit_loss_sum<decltype(link)::value, true> : vfm::k_bsplit_loss_sum<decltype(link)::value, false>;
    hipLaunchKernelGGL(k, dim3((unsigned)((p->E + vfm::FB - 1) / vfm::FB)), dim3(vfm::FB), 0, st, s);
  });
  return launch_status("k_bsplit_loss_sum");
}

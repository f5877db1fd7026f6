// vfm_implicit.hip -- the implicit-feedback solves (include/vfm_implicit.h): the exact fold-in of vfm_foldin_solve.hip
// over every (entity, partner) pair of a two-field model, the unobserved pairs through one Gram block of the partner field.
//
//   k_implicit_base      a workgroup per chunk of the partner field's ids.  share_of(): the packed lower triangle of
//                        sum_j u_j u_j^T, u_j = (1, mu_j), in the 4 x 4 register tiles of k_split_assemble
//                        (vfm_foldin_split.hip: a thread owns a tile and walks the rows in order), then a thread per
//                        coordinate for sum A, sum (A + M^2), sum t u and, thread 0, sum q: the chunk's slab
//                        [triangle tri(d + 1) | SA [d + 1] | SB [d + 1] | sum t u [d + 1] | sum q].  The catalog's rows
//                        have t = -c_mean and q = c_mean^2 + c_var (a row with y = 0 and weight 1).
//   k_implicit_base_sum  a thread per element of the block: the chunks' slabs added in chunk order.
//   k_implicit_chunks    (chunk form) a workgroup per chunk of an entity's observed rows, share_of() again: the sums are
//                        unweighted but for t = w1 y - dw c_mean and q = w1 (y - c_mean)^2 - w0 c_mean^2 + dw c_var.
//   k_implicit_solve     a workgroup per entity: the entity's own share -- its chunks' slabs added in chunk order, or
//                        (row-list form) accumulated here, a thread per coordinate and a thread per triangle element,
//                        rows in order, as solve_body's phases A and B --, then H = kl I + prec (w0 base + dw share),
//                        chol_solve and put_params of vfm_foldin_solve_body.hpp, the row written as k_split_solve
//                        writes it (the same LDS / slab rule), and L_e from the system: theta^T H theta = |L^T theta|^2
//                        off the factor, a thread per column, the d + 1 terms added by thread 0 in order.
// The operands of a partner j are read from the fp32 tables where they are used (F = 2: M = mu_j, A = link(s_j)^2 in
// fp64, C = 0, c_mean = m_0 + mu_w,j, c_var = link(s_0)^2 + link(s_w,j)^2): there is no operand block.  Every sum has a
// fixed order that depends on the entity's rows, the catalog, chunk_rows and d alone: no atomics, no host sync.
//
// vfm_foldin_solve_implicit_prior_f32 (include/vfm_implicit_prior.h) is the PRIOR = true instantiation of k_implicit_solve:
// the folded field's prior [2, d + 1] = mean | precision is staged once per workgroup in fp64 in LDS in front of the
// vectors (lds_doubles_prior), H = kl diag(lam) + ..., b += kl lam m, sigma_c^2 = kl / (kl lam_c + prec SB'_c) and the KL
// of the loss is to that prior; at m = 0, lam = 1 every expression rounds as with PRIOR off.  The base and the chunk pass do
// not depend on the prior; the instantiation without it is the parent's, unchanged.
//
// vfm_foldin_solve_implicit_weights_f32 (include/vfm_implicit_weights.h) is the WROW = true instantiation of
// k_implicit_chunks and k_implicit_solve: observed row r has the weight w[r] (read where y[r] is, under the same clamps)
// and g_r = w[r] - w0 in fp64.  The share of the observed rows is then a weighted one -- share_of() scales the four u_i
// of a row by g_r before the 16 products of its tile, coord_sums() adds g_r A, g_r (A + M^2) and, for coordinate 0,
// g_r, phase B of the row-list form adds g_r, g_r M_i and g_r M_i M_j -- and the solve forms w0 base + share where it
// forms w0 base + dw share without it.  Rows and chunks are walked in the same order.  Everything of WROW sits under
// `if constexpr`: the instantiations without it are the parent's, unchanged, and PRIOR combines with it.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "vfm_args.hpp"
#include "vfm_implicit.h"
#include "vfm_implicit_prior.h"
#include "vfm_implicit_weights.h"
#include "vfm_launch.hpp"            // launch_status

namespace vfm {
namespace {
#include "vfm_rng.hpp"
#include "vfm_common.hpp"

#include "vfm_foldin_body.hpp"       // FB, for_link, round_up, softplus_d, LOG_2PI_HALF
#include "vfm_foldin_solve_body.hpp" // tri, tri_decode, link_d, chol_solve, put_params, the slab rule, launch_lds
#include "vfm_implicit_body.hpp"     // partner_consts, coord_sums, list_elem, implicit_body: the per-entity text of the solve

constexpr int TL = 4;                    // edge of a register tile of the triangle

struct ImpArgs {
  int64_t E, R, T, n_chunks;
  int64_t lo, n;                         // the partner field's id range (k_implicit_base: the range summed)
  int64_t chunk_rows;                    // k_implicit_base only
  int32_t d;
  double kl, w0, w1;
  const int64_t *ent, *row_ptr, *chunk_ptr, *chunks, *partner;
  const float* y;
  const double* base;                    // [part_elems]
  double* part;                          // [n_chunks, part_elems]
  int64_t part_elems;
  float *entity, *bias;
  const float* scal;
  float* loss;
  SolveSlabs sl;
  const float* prior;                    // [2, d + 1] mean | precision of the folded field (PRIOR instantiation only)
  const float* w;                        // [R] weight of each observed row, >= w0 (WROW instantiations only)
};

__host__ __device__ inline int64_t imp_doubles(int d) { return tri(d + 1) + 3 * (int64_t)(d + 1) + 1; }

// the ids [first, first + n) of the catalog: y = 0, weight 1
struct CatalogRows {
  int64_t first;
  __device__ __forceinline__ int64_t id(int64_t r) const { return first + r; }
  __device__ __forceinline__ double t(int64_t, double cm) const { return -cm; }
  __device__ __forceinline__ double q(int64_t, double cm, double cv) const { return cm * cm + cv; }
};

// the observed rows [r0, r0 + n) of one entity: a partner outside the base's range is -1.  WROW: row r weighs s.w[r0 + r]
// in place of s.w1, and g(r) is what it weighs above an unobserved pair
template <bool WROW>
struct ObservedRows {
  const ImpArgs& s;
  int64_t r0;
  __device__ __forceinline__ int64_t id(int64_t r) const {
    const int64_t j = s.partner[r0 + r];
    return j >= s.lo && j < s.lo + s.n ? j : -1;
  }
  __device__ __forceinline__ double g(int64_t r) const { return (double)s.w[r0 + r] - s.w0; }
  __device__ __forceinline__ double t(int64_t r, double cm) const {
    if constexpr (WROW) return (double)s.w[r0 + r] * (double)s.y[r0 + r] - g(r) * cm;
    else return obs_t(s.w0, s.w1, (double)s.y[r0 + r], cm);
  }
  __device__ __forceinline__ double q(int64_t r, double cm, double cv) const {
    if constexpr (WROW) {
      const double res = (double)s.y[r0 + r] - cm;
      // the two squares in statements of their own: neither fuses into the difference, so a row of weight w0 and
      // target 0 adds exactly 0 (res = -cm) and an entity of such rows is the entity without rows, bit for bit
      const double a = (double)s.w[r0 + r] * res * res;
      const double b = s.w0 * cm * cm;
      return a - b + g(r) * cv;
    } else {
      return obs_q(s.w0, s.w1, (double)s.y[r0 + r], cm, cv);
    }
  }
};

// the slab P of n rows, by the whole workgroup: [triangle | SA | SB | sum t u | sum q], NaN where a row is bad.
// WROW: the triangle of sum g u u^T, the four u_i of a row scaled by g once
template <int LINK, bool WROW = false, class Rows>
__device__ __forceinline__ void share_of(const ImpArgs& s, const Rows& rows, int64_t n, double* P) {
#pragma clang fp contract(on)
  const int tid = threadIdx.x;
  const int d = s.d, d1 = d + 1;
  const int nb = (d1 + TL - 1) / TL;
  const int64_t nblk = tri(nb), nt = tri(d1);
  const double qnan = __builtin_nan("");

  // ---- the triangle, a 4 x 4 tile per thread, rows in order
  for (int64_t b = tid; b < nblk; b += FB) {
    int bi, bj;
    tri_decode(b, bi, bj);
    const int i0 = bi * TL, j0 = bj * TL;
    int xi[TL], xj[TL];                  // column of mu behind u_i (clamped into the row), u_0 = 1, u past d = 0
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
      const int64_t j = rows.id(r);
      if (j < 0) { bad = true; continue; }                         // (uniform over the block)
      const float* M = s.entity + j * 2 * (int64_t)d;
      double ui[TL], uj[TL];
#pragma unroll
      for (int t = 0; t < TL; ++t) {
        const double vi = M[xi[t]], vj = M[xj[t]];
        ui[t] = i0 + t == 0 ? 1.0 : i0 + t < d1 ? vi : 0.0;
        uj[t] = j0 + t == 0 ? 1.0 : j0 + t < d1 ? vj : 0.0;
      }
      if constexpr (WROW) {
        const double g = rows.g(r);
#pragma unroll
        for (int t = 0; t < TL; ++t) ui[t] *= g;
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

  // ---- the row sums of each coordinate
  for (int c = tid; c < d1; c += FB) {
    double SA, SB, bM, tt;
    const bool ok = coord_sums<LINK, WROW>(s, rows, n, c, SA, SB, bM, tt);
    P[nt + c] = ok ? SA : qnan;
    P[nt + d1 + c] = ok || c == 0 ? SB : qnan;                     // (the row count stays: sigma_w is a function of it)
    P[nt + 2 * d1 + c] = ok ? bM : qnan;
    if (c == 0) P[nt + 3 * d1] = ok ? tt : qnan;
  }
}

template <int LINK>
__global__ __launch_bounds__(FB) void k_implicit_base(const ImpArgs s) {
  for (int64_t q = blockIdx.x; q < s.n_chunks; q += gridDim.x) {
    const int64_t r0 = q * s.chunk_rows;
    const int64_t n = min(s.chunk_rows, s.n - r0);
    share_of<LINK>(s, CatalogRows{s.lo + r0}, n, s.part + q * s.part_elems);
  }
}

__global__ __launch_bounds__(FB) void k_implicit_base_sum(const double* __restrict__ part, int64_t n_chunks,
                                                          int64_t elems, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= elems) return;
  double acc = 0.;
  for (int64_t q = 0; q < n_chunks; ++q) acc += part[q * elems + i];
  out[i] = acc;
}

// chunk q's rows, clamped to [0, R)
__device__ __forceinline__ void chunk_rows_of(const ImpArgs& s, int64_t q, int64_t& r0, int64_t& n) {
  r0 = min(max(s.chunks[q * 3 + 1], (int64_t)0), s.R);
  n = min(max(s.chunks[q * 3 + 2], (int64_t)0), s.R - r0);
}

template <int LINK, bool WROW>
__global__ __launch_bounds__(FB) void k_implicit_chunks(const ImpArgs s) {
  for (int64_t q = blockIdx.x; q < s.n_chunks; q += gridDim.x) {
    int64_t r0, n;
    chunk_rows_of(s, q, r0, n);
    share_of<LINK, WROW>(s, ObservedRows<WROW>{s, r0}, n, s.part + q * s.part_elems);
  }
}

// the share of entity g's observed rows for implicit_body: its chunks' slabs [c0, c1) added in chunk order (chunk form),
// or its row list accumulated where it is used (row-list form: ListShare's two calls)
template <int LINK, bool WROW>
struct EntityShare {
  const ImpArgs& s;
  const ObservedRows<WROW>& rows;
  int64_t c0, c1, n;
  __device__ __forceinline__ void coord(int c, double& SA, double& SB, double& bM, double& tt) const {
#pragma clang fp contract(on)
    if (s.chunk_ptr) {
      const int d1 = s.d + 1;
      for (int64_t q = c0; q < c1; ++q) {
        const double* V = s.part + q * s.part_elems + tri(d1);
        SA += V[c];
        SB += V[d1 + c];
        bM += V[2 * d1 + c];
        if (c == 0) tt += V[3 * d1];
      }
    } else {
      ListShare<LINK, WROW, ImpArgs, ObservedRows<WROW>>{s, rows, n}.coord(c, SA, SB, bM, tt);
    }
  }
  __device__ __forceinline__ double elem(int64_t p, int i, int j) const {
#pragma clang fp contract(on)
    if (s.chunk_ptr) {
      double acc = 0.;
      for (int64_t q = c0; q < c1; ++q) acc += s.part[q * s.part_elems + p];
      return acc;
    }
    return list_elem<WROW>(s, rows, n, i, j);
  }
};

template <int LINK, bool PRIOR, bool WROW>
__global__ __launch_bounds__(FB) void k_implicit_solve(const ImpArgs s) {
#pragma clang fp contract(on)
  extern __shared__ double sm_all[];
  const int tid = threadIdx.x;
  const int d = s.d, d1 = d + 1;
  double* sm = sm_all + (PRIOR ? 2 * d1 : 0);              // (the prior in front: lds_doubles_prior)
  const double* pr = PRIOR ? sm_all : nullptr;             // m [d + 1] | lam [d + 1]
  if constexpr (PRIOR) {
    stage_prior(s.prior, sm_all, d1);
    __syncthreads();
  }
  double* Hl = sm + 8 * d1;
  double* Hg = s.sl.slab ? s.sl.slab + (int64_t)blockIdx.x * s.sl.slab_elems : nullptr;
  double* Hm = d1 <= s.sl.cap_dim ? Hl : Hg;
  const double prec = link_d<LINK>(s.scal[0]);
  const double kl = s.kl, w0 = s.w0, dw = s.w1 - s.w0;

  for (int64_t g = blockIdx.x; g < s.E; g += gridDim.x) {
    const int64_t e = s.ent[g];
    if (e < 0 || e >= s.T || !Hm) {                          // (block-uniform)
      if (tid == 0) s.loss[g] = __builtin_nanf("");
      continue;
    }
    // the entity's observed rows: its chunks' slabs [c0, c1), or its row list [r0, r0 + n)
    int64_t c0 = 0, c1 = 0, r0 = 0, n = 0;
    if (s.chunk_ptr) {
      c0 = min(max(s.chunk_ptr[g], (int64_t)0), s.n_chunks);
      c1 = min(max(s.chunk_ptr[g + 1], c0), s.n_chunks);
    } else {
      r0 = min(max(s.row_ptr[g], (int64_t)0), s.R);
      n = min(max(s.row_ptr[g + 1] - r0, (int64_t)0), s.R - r0);
    }
    const ObservedRows<WROW> rows{s, r0};
    // phases A-E (vfm_implicit_body.hpp); the row is written where the fp32 parameters are published
    implicit_body<LINK, PRIOR, WROW>(EntityShare<LINK, WROW>{s, rows, c0, c1, n}, d, s.base, kl, w0, dw, prec, sm, Hm,
                                     s.loss + g, [&](const float* pf) {
      for (int k = tid; k < d; k += FB) {
        s.entity[e * 2 * d + k] = pf[1 + k];
        s.entity[e * 2 * d + d + k] = pf[d1 + 1 + k];
      }
      if (tid == 0) {
        s.bias[e * 2] = pf[0];
        s.bias[e * 2 + 1] = pf[d1];
      }
    }, pr);
    __syncthreads();                     // (the vectors and pf are rewritten by the next entity)
  }
}

inline int64_t imp_part_bytes(int64_t n_chunks, int d) { return round_up(n_chunks * imp_doubles(d) * 8, 256); }

}  // namespace
}  // namespace vfm

static int implicit_solve_call(const vfm_implicit_solve_t* p, const float* prior, const float* weights, void* stream);

extern "C" {

int64_t vfm_implicit_base_doubles(int32_t d) {
  if (d < 1 || d > VFM_FOLDIN_MAX_D) return VFM_E_INVALID;
  return vfm::imp_doubles(d);
}

int64_t vfm_implicit_base_workspace_bytes(int64_t n, int64_t chunk_rows, int32_t d) {
  const int64_t lim = (int64_t)1 << 40;                    // (every product below stays under 2^62)
  if (n < 1 || n > lim || chunk_rows < 1 || d < 1 || d > VFM_FOLDIN_MAX_D) return VFM_E_INVALID;
  return vfm::imp_part_bytes((n - 1) / chunk_rows + 1, d);
}

int64_t vfm_implicit_solve_workspace_bytes(int64_t E, int64_t n_chunks, int32_t d, int32_t lds_dim) {
  const int64_t lim = (int64_t)1 << 40;
  if (E < 0 || n_chunks < 0 || E > lim || n_chunks > lim || d < 1 || d > VFM_FOLDIN_MAX_D || lds_dim < -1)
    return VFM_E_INVALID;
  return vfm::imp_part_bytes(n_chunks, d) + vfm::slabs_bytes(E, d, lds_dim);
}

int vfm_implicit_base_f32(const vfm_implicit_base_t* p, void* stream) {
  using vfm::fail;
  if (!p) return fail(VFM_E_INVALID, "vfm_implicit_base_f32: NULL argument struct");
  if (p->T < 1) return fail(VFM_E_INVALID, "T < 1");
  if (p->d < 1 || p->d > VFM_FOLDIN_MAX_D) return fail(VFM_E_INVALID, "d out of range [1,512]");
  if (p->n < 1 || p->lo < 0 || p->lo > p->T || p->n > p->T - p->lo)
    return fail(VFM_E_INVALID, "the id range [lo, lo + n) must lie in [0, T) with n >= 1");
  if (p->chunk_rows < 1) return fail(VFM_E_INVALID, "chunk_rows < 1");
  if (p->flags & ~VFM_FLAG_LINK_SOFTPLUS) return fail(VFM_E_INVALID, "flags: only VFM_FLAG_LINK_SOFTPLUS is accepted");
  if (!p->entity_params || !p->bias_params || !p->scalars || !p->out_base) return fail(VFM_E_INVALID, "null pointer");
  const int64_t ws = vfm_implicit_base_workspace_bytes(p->n, p->chunk_rows, p->d);
  if (ws < 0) return fail(VFM_E_INVALID, "sizes out of range (vfm_implicit_base_workspace_bytes)");
  if (p->workspace_bytes < ws || !p->workspace)
    return fail(VFM_E_INVALID, "workspace too small (vfm_implicit_base_workspace_bytes)");
  if (((uintptr_t)p->workspace) & 255) return fail(VFM_E_INVALID, "workspace must be 256-byte aligned");

  const hipStream_t st = (hipStream_t)stream;
  vfm::ImpArgs s = {};
  s.T = p->T; s.lo = p->lo; s.n = p->n; s.chunk_rows = p->chunk_rows; s.d = p->d;
  s.n_chunks = (p->n - 1) / p->chunk_rows + 1;
  s.part = (double*)p->workspace; s.part_elems = vfm::imp_doubles(p->d);
  s.entity = const_cast<float*>(p->entity_params); s.bias = const_cast<float*>(p->bias_params); s.scal = p->scalars;
  const int64_t gcap = (int64_t)1 << 20;
  const unsigned grid = (unsigned)(s.n_chunks < gcap ? s.n_chunks : gcap);
  vfm::for_link((p->flags & VFM_FLAG_LINK_SOFTPLUS) != 0, [&](auto link) {
    hipLaunchKernelGGL(vfm::k_implicit_base<decltype(link)::value>, dim3(grid), dim3(vfm::FB), 0, st, s);
  });
  if (int rc = launch_status("k_implicit_base")) return rc;
  hipLaunchKernelGGL(vfm::k_implicit_base_sum, dim3((unsigned)((s.part_elems + vfm::FB - 1) / vfm::FB)), dim3(vfm::FB), 0,
                     st, s.part, s.n_chunks, s.part_elems, p->out_base);
  return launch_status("k_implicit_base_sum");
}

int64_t vfm_implicit_solve_prior_workspace_bytes(int64_t E, int64_t n_chunks, int32_t d, int32_t lds_dim) {
  return vfm_implicit_solve_workspace_bytes(E, n_chunks, d, lds_dim);  // (the prior lives in LDS, not in the workspace)
}

int vfm_foldin_solve_implicit_f32(const vfm_implicit_solve_t* p, void* stream) {
  return implicit_solve_call(p, nullptr, nullptr, stream);
}

int vfm_foldin_solve_implicit_prior_f32(const vfm_implicit_solve_t* p, const float* prior, void* stream) {
  return implicit_solve_call(p, prior, nullptr, stream);
}

int64_t vfm_implicit_solve_weights_workspace_bytes(int64_t E, int64_t n_chunks, int32_t d, int32_t lds_dim) {
  return vfm_implicit_solve_workspace_bytes(E, n_chunks, d, lds_dim);  // (the weights are the caller's array)
}

int vfm_foldin_solve_implicit_weights_f32(const vfm_implicit_solve_t* p, const float* prior, const float* weights,
                                          void* stream) {
  return implicit_solve_call(p, prior, weights, stream);
}

}  // extern "C"

// the three entry points: prior == NULL is vfm_foldin_solve_implicit_f32, weights == NULL the call of one w1; with
// weights p->w1 is neither read nor checked
static int implicit_solve_call(const vfm_implicit_solve_t* p, const float* prior, const float* weights, void* stream) {
  using vfm::fail;
  if (!p) return fail(VFM_E_INVALID, "vfm_foldin_solve_implicit_f32: NULL argument struct");
  if (p->T < 1) return fail(VFM_E_INVALID, "T < 1");
  if (p->d < 1 || p->d > VFM_FOLDIN_MAX_D) return fail(VFM_E_INVALID, "d out of range [1,512]");
  if (p->E < 0 || p->R < 0) return fail(VFM_E_INVALID, "E < 0 or R < 0");
  if (p->n_chunks < 0) return fail(VFM_E_INVALID, "n_chunks < 0");
  if (p->n < 1 || p->lo < 0 || p->lo > p->T || p->n > p->T - p->lo)
    return fail(VFM_E_INVALID, "the partner range [lo, lo + n) must lie in [0, T) with n >= 1");
  if (p->flags & ~VFM_FLAG_LINK_SOFTPLUS) return fail(VFM_E_INVALID, "flags: only VFM_FLAG_LINK_SOFTPLUS is accepted");
  if (p->lds_dim < -1) return fail(VFM_E_INVALID, "lds_dim: -1 or >= 0");
  if (!(p->kl_weight > 0.f) || !(p->kl_weight <= 3.0e38f))
    return fail(VFM_E_INVALID, "kl_weight must be > 0 and finite (the prior is what makes the system positive definite)");
  if (!(p->w0 > 0.f) || !(p->w0 <= 3.0e38f)) return fail(VFM_E_INVALID, "w0 must be > 0 and finite");
  if (!weights && (!(p->w1 >= p->w0) || !(p->w1 <= 3.0e38f))) return fail(VFM_E_INVALID, "w1 must be >= w0 and finite");
  if (p->E == 0) return 0;
  if ((p->row_ptr != nullptr) == (p->chunk_ptr != nullptr))
    return fail(VFM_E_INVALID, "one of row_ptr (row-list form) and chunk_ptr (chunk form) must be given");
  if (p->row_ptr && p->n_chunks != 0) return fail(VFM_E_INVALID, "n_chunks must be 0 in the row-list form");
  if (!p->entities || !p->base || !p->entity_params || !p->bias_params || !p->scalars || !p->out_loss ||
      (p->n_chunks > 0 && !p->chunks) || (p->R > 0 && (!p->y || !p->partner)))
    return fail(VFM_E_INVALID, "null pointer");
  const int64_t ws = vfm_implicit_solve_workspace_bytes(p->E, p->n_chunks, p->d, p->lds_dim);
  if (ws < 0) return fail(VFM_E_INVALID, "sizes out of range (vfm_implicit_solve_workspace_bytes)");
  if (p->workspace_bytes < ws || (ws > 0 && !p->workspace))
    return fail(VFM_E_INVALID, "workspace too small (vfm_implicit_solve_workspace_bytes)");
  if (ws > 0 && (((uintptr_t)p->workspace) & 255)) return fail(VFM_E_INVALID, "workspace must be 256-byte aligned");

  const hipStream_t st = (hipStream_t)stream;
  const bool sp = (p->flags & VFM_FLAG_LINK_SOFTPLUS) != 0;
  vfm::ImpArgs s = {};
  s.E = p->E; s.R = p->R; s.T = p->T; s.n_chunks = p->n_chunks; s.lo = p->lo; s.n = p->n; s.d = p->d;
  s.kl = p->kl_weight; s.w0 = p->w0; s.w1 = weights ? p->w0 : p->w1;
  s.ent = p->entities; s.row_ptr = p->row_ptr; s.chunk_ptr = p->chunk_ptr; s.chunks = p->chunks;
  s.partner = p->partner; s.y = p->y; s.base = p->base;
  s.part = (double*)p->workspace; s.part_elems = vfm::imp_doubles(p->d);
  s.entity = p->entity_params; s.bias = p->bias_params; s.scal = p->scalars; s.loss = p->out_loss;
  s.prior = prior;
  s.w = weights;
  const int64_t gcap = (int64_t)1 << 20;
  const unsigned grid_e = vfm::place_slabs(p->d, p->lds_dim, p->E, (char*)p->workspace + vfm::imp_part_bytes(p->n_chunks, p->d),
                                           gcap, s.sl);
  const size_t shm = (size_t)(prior ? vfm::lds_doubles_prior(p->d, s.sl.cap_dim) : vfm::lds_doubles(p->d, s.sl.cap_dim)) * 8;

  if (p->n_chunks > 0) {
    const unsigned grid_c = (unsigned)(p->n_chunks < gcap ? p->n_chunks : gcap);
    vfm::for_link(sp, [&](auto link) {
      constexpr int L = decltype(link)::value;
      if (weights) hipLaunchKernelGGL((vfm::k_implicit_chunks<L, true>), dim3(grid_c), dim3(vfm::FB), 0, st, s);
      else hipLaunchKernelGGL((vfm::k_implicit_chunks<L, false>), dim3(grid_c), dim3(vfm::FB), 0, st, s);
    });
    if (int rc = launch_status("k_implicit_chunks")) return rc;
  }
  vfm::for_link(sp, [&](auto link) {
    constexpr int L = decltype(link)::value;
    if (prior && weights) vfm::launch_lds(vfm::k_implicit_solve<L, true, true>, grid_e, shm, st, s);
    else if (prior) vfm::launch_lds(vfm::k_implicit_solve<L, true, false>, grid_e, shm, st, s);
    else if (weights) vfm::launch_lds(vfm::k_implicit_solve<L, false, true>, grid_e, shm, st, s);
    else vfm::launch_lds(vfm::k_implicit_solve<L, false, false>, grid_e, shm, st, s);
  });
  return launch_status("k_implicit_solve");
}

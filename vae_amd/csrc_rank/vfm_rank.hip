// vfm_rank.hip -- preference elicitation (include/vfm_rank.h): closed-form predictive moments (k_moments) and the
// fused catalog ranking (k_rank_prep -> k_rank -> k_rank_merge).  The scan k_rank is instantiated here only; the
// field-form ranking (vfm_rank_field.hip) launches it through vfm::launch_rank_scan with operands of its own.
//
// Compiled with -ffp-contract=off: every fused multiply-add below is an explicit fmaf, so the pair moments of
// k_moments, the MFMA chains of k_rank and the recomputation in k_rank_merge round the same way, bit for bit.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "vfm_rank.h"
#include "vfm_rank_tile.hpp"        // pair scores, operand packing (k_rank_prep), the MFMA score tile
#include "vfm_rank_scan.hpp"        // the scan launch other operand forms share, k_rank_merge, the list workspace

namespace {

constexpr int KR = 16;        // k <= KR: the running top k is kept in registers (branch-free insertion)

// ---------------------------------------------------------------------------------------------------------------------
// k_moments: one thread per row.  F == 2: the pair chains above; general F: per coordinate in fp64
//   sum_{f<g} m_f m_g = ((sum m)^2 - sum m^2) / 2,  Var = sum_{f<g} s_f^2 s_g^2 + sum_f s_f^2 (sum_{g!=f} m_g)^2
// ---------------------------------------------------------------------------------------------------------------------
template <typename ID>
__global__ __launch_bounds__(256) void k_moments(int64_t B, int F, int d, int64_t T, bool sp, const ID* __restrict__ x,
                                                 const float* __restrict__ ent, const float* __restrict__ bias,
                                                 const float* __restrict__ scal, int strat, uint64_t seed,
                                                 float* __restrict__ out_m, float* __restrict__ out_v,
                                                 float* __restrict__ out_s) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= B) return;
  const ID* xr = x + r * F;
  bool ok = true;
  for (int f = 0; f < F; ++f) ok = ok && (int64_t)xr[f] >= 0 && (int64_t)xr[f] < T;
  float mean = __builtin_nanf(""), var = __builtin_nanf(""), sc = __builtin_nanf("");
  if (ok) {
    const float m0 = scal[1], sg0 = link_of(scal[2], sp);
    if (F == 2) {
      const int64_t u = (int64_t)xr[0], i = (int64_t)xr[1];
      pair_moments(ent + u * 2 * d, ent + i * 2 * d, bias + u * 2, bias + i * 2, m0, sg0, d, sp, mean, var);
      sc = strat == VFM_RANK_RANDOM ? philox_uniform(seed, u, i) : score_of(strat, mean, var);
    } else {
      double em = (double)m0, ev = (double)sg0 * (double)sg0;
      for (int f = 0; f < F; ++f) {
        const int64_t e = (int64_t)xr[f];
        const double sw = (double)link_of(bias[e * 2 + 1], sp);
        em += (double)bias[e * 2];
        ev += sw * sw;
      }
      for (int k = 0; k < d; ++k) {
        double sm = 0., smm = 0., ss = 0., sss = 0.;
        for (int f = 0; f < F; ++f) {
          const float* row = ent + (int64_t)xr[f] * 2 * d;
          const double m = row[k], s = link_of(row[d + k], sp), s2 = s * s;
          sm += m; smm += m * m; ss += s2; sss += s2 * s2;
        }
        double lin = 0.;
        for (int f = 0; f < F; ++f) {
          const float* row = ent + (int64_t)xr[f] * 2 * d;
          const double m = row[k], s = link_of(row[d + k], sp), o = sm - m;
          lin += s * s * o * o;
        }
        em += 0.5 * (sm * sm - smm);
        ev += 0.5 * (ss * ss - sss) + lin;
      }
      mean = (float)em;
      var = (float)ev;
      sc = score_of(strat, mean, var);
    }
  }
  out_m[r] = mean;
  out_v[r] = var;
  if (out_s) out_s[r] = sc;
}

struct RankArgs {
  int64_t U, n_cand, item_lo, n_excl;
  const int64_t *users, *cand, *excl_ptr, *excl_items;
  TileOps ops;
  float* ls;
  int* lc;
  int k, n_tiles, S;
  uint64_t seed;
};

// ---------------------------------------------------------------------------------------------------------------------
// k_rank: workgroup (user tile of 256, item split).  Per tile of 64 candidates the four waves form the 256 x 64 score
// block (score_tile, vfm_rank_tile.hpp) in an LDS image [item][user] and each thread then walks its own user's column in
// item order: exclusion cursor, then comparison with its running k-th best, rare survivors inserted into the user's
// sorted list (registers for k <= KR, else the workspace; one list per split, written to the workspace at the end).
// ---------------------------------------------------------------------------------------------------------------------
template <int STRAT>
__global__ __launch_bounds__(256, 2) void k_rank(RankArgs a) {
  __shared__ TileSmem sm;
  __shared__ float ci_m[IT], ci_v[IT];
  const int tid = threadIdx.x;
  const int64_t u0 = (int64_t)blockIdx.x * UT, u = u0 + tid;
  const int s = blockIdx.y;
  const bool uvalid = u < a.U;
  const int t_lo = (int)((int64_t)s * a.n_tiles / a.S), t_hi = (int)((int64_t)(s + 1) * a.n_tiles / a.S);
  float* Ls = a.ls + ((int64_t)s * a.U + (uvalid ? u : 0)) * a.k;
  int* Lc = a.lc + ((int64_t)s * a.U + (uvalid ? u : 0)) * a.k;
  float thr_s = -INFINITY;
  int thr_c = INT32_MAX;
  const bool in_regs = a.k <= KR;
  float rs[KR];
  int rc[KR];
#pragma unroll
  for (int p = 0; p < KR; ++p) { rs[p] = -INFINITY; rc[p] = INT32_MAX; }
  int64_t cx = 0, cx_end = 0, ex = INT64_MAX, uid = 0;
  if (uvalid) {
    if (!in_regs)
      for (int p = 0; p < a.k; ++p) { Ls[p] = -INFINITY; Lc[p] = INT32_MAX; }
    if (a.excl_ptr) {
      cx = min(max(a.excl_ptr[u], (int64_t)0), a.n_excl);
      cx_end = min(max(a.excl_ptr[u + 1], cx), a.n_excl);
      ex = cx < cx_end ? a.excl_items[cx] : INT64_MAX;
    }
    uid = a.users[u];
  }
  float ucm[2], ucv[2];
  tile_user_consts<STRAT>(a.ops, u0, tid, ucm, ucv);
  for (int t = t_lo; t < t_hi; ++t) {
    const int64_t c0 = (int64_t)t * IT;
    if constexpr (STRAT != VFM_RANK_RANDOM) score_tile<STRAT>(a.ops, sm, ci_m, ci_v, u0, c0, tid, ucm, ucv);
    if (uvalid) {
      const int jn = (int)min((int64_t)IT, a.n_cand - c0);
      for (int j = 0; j < jn; ++j) {
        const int c = (int)(c0 + j);
        const int64_t id = a.cand ? a.cand[c] : a.item_lo + c;
        while (ex < id) {
          ++cx;
          ex = cx < cx_end ? a.excl_items[cx] : INT64_MAX;
        }
        if (ex == id) continue;
        float sc;
        if constexpr (STRAT == VFM_RANK_RANDOM) sc = philox_uniform(a.seed, uid, id);
        else sc = sm.S[j][tid];
        if (!beats(sc, c, thr_s, thr_c)) continue;
        if (in_regs) {                  // (a wave whose lanes insert at different items pays ~4 KR VALU ops, no memory)
#pragma unroll
          for (int p = KR - 1; p >= 1; --p) {
            const bool bp = beats(sc, c, rs[p - 1], rc[p - 1]), bq = beats(sc, c, rs[p], rc[p]);
            rs[p] = bp ? rs[p - 1] : (bq ? sc : rs[p]);
            rc[p] = bp ? rc[p - 1] : (bq ? c : rc[p]);
          }
          if (beats(sc, c, rs[0], rc[0])) { rs[0] = sc; rc[0] = c; }
#pragma unroll
          for (int p = 0; p < KR; ++p)
            if (p == a.k - 1) { thr_s = rs[p]; thr_c = rc[p]; }
          continue;
        }
        int p = a.k - 1;
        while (p > 0) {
          const float ps = Ls[p - 1];
          const int pc = Lc[p - 1];
          if (!beats(sc, c, ps, pc)) break;
          Ls[p] = ps;
          Lc[p] = pc;
          --p;
        }
        Ls[p] = sc;
        Lc[p] = c;
        thr_s = Ls[a.k - 1];
        thr_c = Lc[a.k - 1];
      }
    }
  }
  if (in_regs && uvalid) {
#pragma unroll
    for (int p = 0; p < KR; ++p)
      if (p < a.k) { Ls[p] = rs[p]; Lc[p] = rc[p]; }
  }
}

// The winners' moments of k_rank_merge (vfm_rank_scan.hpp) for two fields: pair_moments straight from the tables
struct PairMoments {
  const int64_t* users;
  int64_t T;
  int d;
  bool sp;
  const float *ent, *bias, *scal;
  __device__ void operator()(int64_t u, int64_t iid, float& m, float& v) const {
    const int64_t uid = users[u];
    if (uid >= 0 && uid < T && iid >= 0 && iid < T)
      pair_moments(ent + uid * 2 * d, ent + iid * 2 * d, bias + uid * 2, bias + iid * 2, scal[1], link_of(scal[2], sp), d,
                   sp, m, v);
  }
};

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
struct Layout : OpLayout, ListLayout {};

Layout layout_of(int64_t U, int64_t n_cand, int d, int k, int strategy, int n_splits) {
  Layout L;
  static_cast<OpLayout&>(L) = op_layout_of(U, n_cand, d, strategy, n_splits);
  static_cast<ListLayout&>(L) = list_layout_of(L.end, L.S, U, k);
  return L;
}

int launch_scan(const RankArgs& a, int strategy, dim3 grid, hipStream_t st) {
  switch (strategy) {
    case VFM_RANK_TOP: hipLaunchKernelGGL(k_rank<VFM_RANK_TOP>, grid, dim3(256), 0, st, a); break;
    case VFM_RANK_VARIANCE: hipLaunchKernelGGL(k_rank<VFM_RANK_VARIANCE>, grid, dim3(256), 0, st, a); break;
    case VFM_RANK_MEAN: hipLaunchKernelGGL(k_rank<VFM_RANK_MEAN>, grid, dim3(256), 0, st, a); break;
    default: hipLaunchKernelGGL(k_rank<VFM_RANK_RANDOM>, grid, dim3(256), 0, st, a); break;
  }
  return launch_status("k_rank");
}

}  // namespace

int vfm::launch_rank_scan(const RankScan& r, int strategy, unsigned n_query_tiles, hipStream_t st) {
  RankArgs a;
  a.U = r.U; a.n_cand = r.n_cand; a.item_lo = r.item_lo; a.n_excl = r.n_excl;
  a.users = r.keys; a.cand = r.cand; a.excl_ptr = r.excl_ptr; a.excl_items = r.excl_items;
  a.ops = TileOps{r.uop, r.iop, r.ucon, r.icon, r.Kp, r.KA, r.KB};
  a.ls = r.ls; a.lc = r.lc;
  a.k = r.k; a.n_tiles = r.n_tiles; a.S = r.S; a.seed = r.seed;
  return launch_scan(a, strategy, dim3(n_query_tiles, (unsigned)r.S), st);
}

extern "C" {

int vfm_predictive_moments_f32(int64_t B, int32_t F, int32_t d, int64_t T, int32_t id_bits, int32_t flags,
                               const void* x, const float* entity_params, const float* bias_params,
                               const float* scalars, int32_t strategy, uint64_t seed, float* logit_mean,
                               float* logit_var, float* score, void* stream) {
  if (int rc = check_common(T, d, flags, strategy)) return rc;
  if (B < 0) return vfm::fail(VFM_E_INVALID, "B < 0");
  if (F < 1 || F > VFM_MAX_FIELDS) return vfm::fail(VFM_E_INVALID, "F out of range [1,64]");
  if (id_bits != 32 && id_bits != 64) return vfm::fail(VFM_E_INVALID, "id_bits must be 32 or 64");
  if (strategy == VFM_RANK_RANDOM && F != 2) return vfm::fail(VFM_E_INVALID, "the random score needs two fields");
  if (B == 0) return 0;
  if (!x || !entity_params || !bias_params || !scalars || !logit_mean || !logit_var)
    return vfm::fail(VFM_E_INVALID, "null pointer");
  const hipStream_t st = (hipStream_t)stream;
  const bool sp = (flags & VFM_FLAG_LINK_SOFTPLUS) != 0;
  const unsigned nb = (unsigned)((B + 255) / 256);
  if (id_bits == 64)
    hipLaunchKernelGGL(k_moments<int64_t>, dim3(nb), dim3(256), 0, st, B, F, d, T, sp, (const int64_t*)x, entity_params,
                       bias_params, scalars, strategy, seed, logit_mean, logit_var, score);
  else
    hipLaunchKernelGGL(k_moments<int32_t>, dim3(nb), dim3(256), 0, st, B, F, d, T, sp, (const int32_t*)x, entity_params,
                       bias_params, scalars, strategy, seed, logit_mean, logit_var, score);
  return launch_status("k_moments");
}

int64_t vfm_rank_workspace_bytes(int64_t U, int64_t n_cand, int32_t d, int32_t k, int32_t strategy, int32_t n_splits) {
  if (U < 0 || n_cand < 0 || n_cand >= ((int64_t)1 << 31) || d < 1 || d > 4096 || k < 1 || k > VFM_RANK_MAX_K ||
      strategy < VFM_RANK_TOP || strategy > VFM_RANK_RANDOM || n_splits < 0 || n_splits > VFM_RANK_MAX_SPLITS)
    return VFM_E_INVALID;
  return layout_of(U, n_cand, d, k, strategy, n_splits).bytes;
}

int vfm_rank_items_f32(int64_t U, const int64_t* users, int64_t n_cand, const int64_t* cand, int64_t item_lo,
                       int64_t T, int32_t F, int32_t d, int32_t k, int32_t strategy, int32_t flags, uint64_t seed,
                       int32_t n_splits, const int64_t* excl_ptr, const int64_t* excl_items, int64_t n_excl,
                       const float* entity_params, const float* bias_params, const float* scalars, void* workspace,
                       int64_t workspace_bytes, int64_t* out_items, float* out_score, float* out_mean,
                       float* out_var, void* stream) {
  RankCall r;
  r.Q = U; r.queries = users;
  r.n_cand = n_cand; r.cand = cand; r.cand_lo = item_lo;
  r.excl_ptr = excl_ptr; r.excl_items = excl_items; r.n_excl = n_excl;
  r.T = T; r.F = F; r.d = d; r.ent = entity_params; r.bias = bias_params; r.scal = scalars;
  r.workspace = workspace; r.workspace_bytes = workspace_bytes;
  r.k = k; r.strategy = strategy; r.flags = flags; r.n_splits = n_splits; r.seed = seed;
  r.out_items = out_items; r.out_score = out_score; r.out_mean = out_mean; r.out_var = out_var;
  r.stream = (hipStream_t)stream;
  if (int rc = check_common(T, d, flags, strategy)) return rc;
  if (F != 2) return vfm::fail(VFM_E_INVALID, "rank_items: two-field models only (F == 2)");
  if (int rc = check_rank_call(r, RANK_ASK_TOPK)) return rc;
  if (U == 0) return 0;
  const Layout L = layout_of(U, n_cand, d, k, strategy, n_splits);
  if (int rc = check_rank_workspace(r, L.bytes, "workspace too small (vfm_rank_workspace_bytes)")) return rc;

  if (strategy != VFM_RANK_RANDOM)
    if (int rc = launch_rank_prep(L, r)) return rc;
  return scan_and_merge(r, L, users, PairMoments{users, T, d, r.softplus(), entity_params, bias_params, scalars});
}

}  // extern "C"

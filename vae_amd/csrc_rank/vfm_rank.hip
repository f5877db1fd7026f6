// vfm_rank.hip -- preference elicitation (include/vfm_rank.h): closed-form predictive moments (k_moments) and the
// fused catalog ranking (k_rank_prep -> k_rank -> k_rank_merge).
//
// Compiled with -ffp-contract=off: every fused multiply-add below is an explicit fmaf, so the pair moments of
// k_moments, the MFMA chains of k_rank and the recomputation in k_rank_merge round the same way, bit for bit.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "vfm_rank.h"

namespace vfm {
int fail(int code, const char* msg);          // (vfm_abi.hip: the thread's vfm_last_error() text)
int fail_hip(hipError_t e, const char* where);
}  // namespace vfm

namespace {

constexpr int UT = 256;       // users per workgroup (one per thread in the top-k scan)
constexpr int IT = 64;        // candidate items per tile
constexpr int KS = 16;        // K values per LDS stage (operand rows are padded to a multiple of KS with zeros)
constexpr int KR = 16;        // k <= KR: the running top k is kept in registers (branch-free insertion)
constexpr int MERGE_BLOCK = 256;
constexpr float PI_OVER_8 = 0.39269908169872414f;

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float link_of(float s, bool softplus) {
  if (!softplus) return fabsf(s);
  return s > 0.f ? s + log1pf(expf(-s)) : log1pf(expf(s));
}

__device__ __forceinline__ float score_of(int strat, float m, float v) {
  if (strat == VFM_RANK_TOP) return m;
  if (strat == VFM_RANK_VARIANCE) return v;
  return -fabsf(m) / sqrtf(1.0f + PI_OVER_8 * v);
}

// Philox4x32-10 (as vfm_rng.hpp), one uniform in [0,1) with 24 bits per (seed, user, item)
__device__ __forceinline__ float philox_uniform(uint64_t seed, int64_t user, int64_t item) {
  uint32_t c0 = (uint32_t)item, c1 = (uint32_t)((uint64_t)item >> 32), c2 = (uint32_t)user,
           c3 = (uint32_t)((uint64_t)user >> 32), k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return (float)(c0 >> 8) * (1.0f / 16777216.0f);
}

// The K operands of one entity row (the GEMM forms of the closed form):
//   mean part:     user mu_u[k]                       item mu_i[k]
//   variance part: user [mu_u^2 | sigma_u^2]           item [sigma_i^2 | mu_i^2 + sigma_i^2]
__device__ __forceinline__ float op_mean(const float* row, int k) { return row[k]; }
__device__ __forceinline__ float op_var(const float* row, int kb, int d, bool item, bool sp) {
  const int k = kb < d ? kb : kb - d;
  const float m = row[k], s = link_of(row[d + k], sp);
  if (!item) return kb < d ? m * m : s * s;
  return kb < d ? s * s : m * m + s * s;
}

// Closed-form moments of the pair (u, i): the same fp32 chains, in the same k order, as the MFMA accumulation of k_rank
__device__ void pair_moments(const float* eu, const float* ei, const float* bu, const float* bi, float m0, float sg0,
                             int d, bool sp, float& mean, float& var) {
  float am = 0.f, av = 0.f;
  for (int k = 0; k < d; ++k) am = fmaf(op_mean(eu, k), op_mean(ei, k), am);
  for (int kb = 0; kb < 2 * d; ++kb) av = fmaf(op_var(eu, kb, d, false, sp), op_var(ei, kb, d, true, sp), av);
  const float sgu = link_of(bu[1], sp), sgi = link_of(bi[1], sp);
  mean = (am + (m0 + bu[0])) + bi[0];
  var = (av + (sg0 * sg0 + sgu * sgu)) + sgi * sgi;
}

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

// ---------------------------------------------------------------------------------------------------------------------
// k_rank_prep: the packed operand rows [rows_pad, Kp] (zero padded: users past U, items past n_cand, k past each part)
// and the per-row constants [rows_pad, 2]: user (m0 + mu_w, sigma0^2 + sigma_w^2), item (mu_w, sigma_w^2).
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rank_prep(int64_t rows_pad, int64_t rows, const int64_t* __restrict__ ids,
                                                   int64_t lo, int64_t T, int Kp, int KA, int d, bool item, bool sp,
                                                   const float* __restrict__ ent, const float* __restrict__ bias,
                                                   const float* __restrict__ scal, float* __restrict__ op,
                                                   float* __restrict__ con) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int W = Kp + 2;
  if (idx >= rows_pad * W) return;
  const int64_t r = idx / W;
  const int k = (int)(idx - r * W);
  float v = 0.f;
  if (r < rows) {
    const int64_t e = ids ? ids[r] : lo + r;
    if (e < 0 || e >= T) {
      v = __builtin_nanf("");           // (never read out of the tables; the pair's score is NaN and never returned)
    } else if (k < KA) {
      v = k < d ? op_mean(ent + e * 2 * d, k) : 0.f;
    } else if (k < Kp) {
      const int kb = k - KA;
      v = kb < 2 * d ? op_var(ent + e * 2 * d, kb, d, item, sp) : 0.f;
    } else if (k == Kp) {
      v = item ? bias[e * 2] : scal[1] + bias[e * 2];
    } else {
      const float sw = link_of(bias[e * 2 + 1], sp), sg0 = link_of(scal[2], sp);
      v = item ? sw * sw : sg0 * sg0 + sw * sw;
    }
  }
  if (k < Kp) op[r * Kp + k] = v;
  else con[r * 2 + (k - Kp)] = v;
}

struct RankArgs {
  int64_t U, n_cand, item_lo, n_excl;
  const int64_t *users, *cand, *excl_ptr, *excl_items;
  const float *uop, *iop, *ucon, *icon;
  float* ls;
  int* lc;
  int Kp, KA, KB, k, n_tiles, S;
  uint64_t seed;
};

__device__ __forceinline__ bool beats(float s, int c, float ts, int tc) { return s > ts || (s == ts && c < tc); }

// ---------------------------------------------------------------------------------------------------------------------
// k_rank: workgroup (user tile of 256, item split).  Per tile of 64 candidates the four waves form the 256 x 64 score
// block with v_mfma_f32_32x32x2_f32 (wave w: users 64w .. 64w+63 x all 64 items, 2 x 2 blocks of 32 x 32; items on the
// A / row side, users on the B / column side), operands staged k-major in LDS per KS values of K.  The scores go to an
// LDS image [item][user] (aliasing the operand stage) and each thread then walks its own user's column in item order:
// exclusion cursor, then comparison with its running k-th best, rare survivors inserted into the user's sorted list
// (registers for k <= KR, else the workspace; one list per split, written to the workspace at the end).
// ---------------------------------------------------------------------------------------------------------------------
template <int STRAT>
__global__ __launch_bounds__(256, 2) void k_rank(RankArgs a) {
  __shared__ union {
    struct {
      float A[KS][IT + 4];
      float B[KS][UT + 4];
    } op;
    float S[IT][UT];
  } sm;
  __shared__ float ci_m[IT], ci_v[IT];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
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
  float ucm[2] = {0.f, 0.f}, ucv[2] = {0.f, 0.f};
  if constexpr (STRAT != VFM_RANK_RANDOM) {
    for (int ub = 0; ub < 2; ++ub) {
      const int64_t uc = u0 + w * 64 + ub * 32 + (lane & 31);
      ucm[ub] = a.ucon[uc * 2];
      ucv[ub] = a.ucon[uc * 2 + 1];
    }
  }
  for (int t = t_lo; t < t_hi; ++t) {
    const int64_t c0 = (int64_t)t * IT;
    if constexpr (STRAT != VFM_RANK_RANDOM) {
      f32x16 accm[2][2], accv[2][2];
      for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) { accm[i][j] = (f32x16)(0.f); accv[i][j] = (f32x16)(0.f); }
      if (tid < IT) { ci_m[tid] = a.icon[(c0 + tid) * 2]; ci_v[tid] = a.icon[(c0 + tid) * 2 + 1]; }
#pragma unroll
      for (int part = 0; part < 2; ++part) {
        const int K = part == 0 ? a.KA : a.KB, off = part == 0 ? 0 : a.KA;
        if ((part == 0 && STRAT == VFM_RANK_VARIANCE) || (part == 1 && STRAT == VFM_RANK_TOP)) continue;
        for (int k0 = 0; k0 < K; k0 += KS) {
          __syncthreads();
          {
            const int r = tid >> 2, q = tid & 3;
            const float4 v = *reinterpret_cast<const float4*>(a.iop + (c0 + r) * a.Kp + off + k0 + 4 * q);
            sm.op.A[4 * q + 0][r] = v.x; sm.op.A[4 * q + 1][r] = v.y;
            sm.op.A[4 * q + 2][r] = v.z; sm.op.A[4 * q + 3][r] = v.w;
          }
#pragma unroll
          for (int rep = 0; rep < 4; ++rep) {
            const int idx = rep * 256 + tid, r = idx >> 2, q = idx & 3;
            const float4 v = *reinterpret_cast<const float4*>(a.uop + (u0 + r) * a.Kp + off + k0 + 4 * q);
            sm.op.B[4 * q + 0][r] = v.x; sm.op.B[4 * q + 1][r] = v.y;
            sm.op.B[4 * q + 2][r] = v.z; sm.op.B[4 * q + 3][r] = v.w;
          }
          __syncthreads();
#pragma unroll
          for (int kk = 0; kk < KS; kk += 2) {
            const int kr = kk + (lane >> 5), l = lane & 31;
            const float a0 = sm.op.A[kr][l], a1 = sm.op.A[kr][32 + l];
            const float b0 = sm.op.B[kr][w * 64 + l], b1 = sm.op.B[kr][w * 64 + 32 + l];
            if (part == 0) {
              accm[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, accm[0][0], 0, 0, 0);
              accm[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, accm[0][1], 0, 0, 0);
              accm[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, accm[1][0], 0, 0, 0);
              accm[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, accm[1][1], 0, 0, 0);
            } else {
              accv[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, accv[0][0], 0, 0, 0);
              accv[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, accv[0][1], 0, 0, 0);
              accv[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, accv[1][0], 0, 0, 0);
              accv[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, accv[1][1], 0, 0, 0);
            }
          }
        }
      }
      __syncthreads();                  // (the score image overwrites the operand stage)
      // C/D map of the 32x32 f32 MFMA: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
      for (int ib = 0; ib < 2; ++ib)
#pragma unroll
        for (int ub = 0; ub < 2; ++ub)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int it = ib * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), uc = w * 64 + ub * 32 + (lane & 31);
            const float m = (accm[ib][ub][r] + ucm[ub]) + ci_m[it];
            const float v = (accv[ib][ub][r] + ucv[ub]) + ci_v[it];
            sm.S[it][uc] = score_of(STRAT, m, v);
          }
      __syncthreads();
    }
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

// ---------------------------------------------------------------------------------------------------------------------
// k_rank_merge: one workgroup per user.  Each list entry's final rank = its position in its own list + the number of
// entries of the other lists that beat it (binary search: every list is sorted); entries of rank < k are written with
// their moments recomputed from the tables, the rest of the k slots padded.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MERGE_BLOCK) void k_rank_merge(int64_t U, int k, int S, const float* __restrict__ ls,
                                                            const int* __restrict__ lc, const int64_t* __restrict__ users,
                                                            const int64_t* __restrict__ cand, int64_t item_lo, int64_t T,
                                                            int d, bool sp, const float* __restrict__ ent,
                                                            const float* __restrict__ bias, const float* __restrict__ scal,
                                                            int64_t* __restrict__ out_items, float* __restrict__ out_score,
                                                            float* __restrict__ out_m, float* __restrict__ out_v) {
  __shared__ int n_valid;
  const int64_t u = blockIdx.x;
  if (threadIdx.x == 0) n_valid = 0;
  __syncthreads();
  const int64_t uid = users[u];
  const bool uok = uid >= 0 && uid < T;
  for (int e = threadIdx.x; e < S * k; e += MERGE_BLOCK) {
    const int s = e / k, p = e - s * k;
    const float sc = ls[((int64_t)s * U + u) * k + p];
    const int c = lc[((int64_t)s * U + u) * k + p];
    if (c == INT32_MAX) continue;
    atomicAdd(&n_valid, 1);
    int rank = p;
    for (int s2 = 0; s2 < S && rank < k; ++s2) {
      if (s2 == s) continue;
      const float* L2s = ls + ((int64_t)s2 * U + u) * k;
      const int* L2c = lc + ((int64_t)s2 * U + u) * k;
      int lo = 0, hi = k;              // first position whose entry does not beat (sc, c)
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (beats(L2s[mid], L2c[mid], sc, c)) lo = mid + 1;
        else hi = mid;
      }
      rank += lo;
    }
    if (rank >= k) continue;
    const int64_t iid = cand ? cand[c] : item_lo + c;
    float m = __builtin_nanf(""), v = __builtin_nanf("");
    if (uok && iid >= 0 && iid < T)
      pair_moments(ent + uid * 2 * d, ent + iid * 2 * d, bias + uid * 2, bias + iid * 2, scal[1], link_of(scal[2], sp), d,
                   sp, m, v);
    out_items[u * k + rank] = iid;
    out_score[u * k + rank] = sc;
    out_m[u * k + rank] = m;
    out_v[u * k + rank] = v;
  }
  __syncthreads();
  for (int p = min(n_valid, k) + threadIdx.x; p < k; p += MERGE_BLOCK) {
    out_items[u * k + p] = -1;
    out_score[u * k + p] = -INFINITY;
    out_m[u * k + p] = __builtin_nanf("");
    out_v[u * k + p] = __builtin_nanf("");
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

struct Layout {
  int KA, KB, Kp, S, n_tiles;
  int64_t U_pad, C_pad, off_uop, off_iop, off_ucon, off_icon, off_ls, off_lc, bytes;
};

Layout layout_of(int64_t U, int64_t n_cand, int d, int k, int strategy, int n_splits) {
  Layout L;
  L.KA = (strategy == VFM_RANK_TOP || strategy == VFM_RANK_MEAN) ? (int)round_up(d, KS) : 0;
  L.KB = (strategy == VFM_RANK_VARIANCE || strategy == VFM_RANK_MEAN) ? (int)round_up(2 * (int64_t)d, KS) : 0;
  L.Kp = L.KA + L.KB;
  L.U_pad = round_up(U, UT);
  L.C_pad = round_up(n_cand, IT);
  L.n_tiles = (int)(L.C_pad / IT);
  if (n_splits > 0) {
    L.S = n_splits;
  } else {                             // about two workgroups per CU of the 256: split the items when the users do not
    const int64_t n_ut = L.U_pad / UT;
    int64_t S = n_ut > 0 ? (512 + n_ut - 1) / n_ut : 1;
    S = S < 1 ? 1 : S;
    S = S > VFM_RANK_MAX_SPLITS ? VFM_RANK_MAX_SPLITS : S;
    S = S > L.n_tiles ? L.n_tiles : S;
    L.S = (int)(S < 1 ? 1 : S);
  }
  int64_t off = 0;
  auto take = [&](int64_t bytes) { const int64_t o = off; off += round_up(bytes, 256); return o; };
  L.off_uop = take(L.U_pad * L.Kp * 4);
  L.off_iop = take(L.C_pad * L.Kp * 4);
  L.off_ucon = take(L.U_pad * 2 * 4);
  L.off_icon = take(L.C_pad * 2 * 4);
  L.off_ls = take((int64_t)L.S * U * k * 4);
  L.off_lc = take((int64_t)L.S * U * k * 4);
  L.bytes = off;
  return L;
}

int check_common(int64_t T, int32_t d, int32_t flags, int32_t strategy) {
  if (T < 1) return vfm::fail(VFM_E_INVALID, "T < 1");
  if (d < 1 || d > 4096) return vfm::fail(VFM_E_INVALID, "d out of range [1,4096]");
  if (flags & ~VFM_FLAG_LINK_SOFTPLUS) return vfm::fail(VFM_E_INVALID, "flags: only VFM_FLAG_LINK_SOFTPLUS is accepted");
  if (strategy < VFM_RANK_TOP || strategy > VFM_RANK_RANDOM) return vfm::fail(VFM_E_INVALID, "unknown strategy");
  return 0;
}

int launch_status(const char* where) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : vfm::fail_hip(e, where);
}

}  // namespace

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
  if (int rc = check_common(T, d, flags, strategy)) return rc;
  if (F != 2) return vfm::fail(VFM_E_INVALID, "rank_items: two-field models only (F == 2)");
  if (k < 1 || k > VFM_RANK_MAX_K) return vfm::fail(VFM_E_INVALID, "k out of range [1,128]");
  if (U < 0) return vfm::fail(VFM_E_INVALID, "U < 0");
  if (n_cand < 0 || n_cand >= ((int64_t)1 << 31)) return vfm::fail(VFM_E_INVALID, "n_cand out of range [0,2^31)");
  if (n_splits < 0 || n_splits > VFM_RANK_MAX_SPLITS) return vfm::fail(VFM_E_INVALID, "n_splits out of range [0,64]");
  if (!cand && (item_lo < 0 || item_lo + n_cand > T)) return vfm::fail(VFM_E_INVALID, "item range outside [0,T)");
  if (n_excl < 0 || (n_excl > 0 && (!excl_ptr || !excl_items)))
    return vfm::fail(VFM_E_INVALID, "exclusion lists: excl_ptr and excl_items together, n_excl >= 0");
  if (U == 0) return 0;
  if (!users || !entity_params || !bias_params || !scalars || !workspace || !out_items || !out_score || !out_mean ||
      !out_var)
    return vfm::fail(VFM_E_INVALID, "null pointer");
  const Layout L = layout_of(U, n_cand, d, k, strategy, n_splits);
  if (workspace_bytes < L.bytes) return vfm::fail(VFM_E_INVALID, "workspace too small (vfm_rank_workspace_bytes)");
  if (((uintptr_t)workspace) & 255) return vfm::fail(VFM_E_INVALID, "workspace must be 256-byte aligned");

  const hipStream_t st = (hipStream_t)stream;
  const bool sp = (flags & VFM_FLAG_LINK_SOFTPLUS) != 0;
  char* ws = (char*)workspace;
  RankArgs a;
  a.U = U; a.n_cand = n_cand; a.item_lo = item_lo; a.n_excl = excl_ptr ? n_excl : 0;
  a.users = users; a.cand = cand; a.excl_ptr = excl_ptr; a.excl_items = excl_items;
  a.uop = (const float*)(ws + L.off_uop); a.iop = (const float*)(ws + L.off_iop);
  a.ucon = (const float*)(ws + L.off_ucon); a.icon = (const float*)(ws + L.off_icon);
  a.ls = (float*)(ws + L.off_ls); a.lc = (int*)(ws + L.off_lc);
  a.Kp = L.Kp; a.KA = L.KA; a.KB = L.KB; a.k = k; a.n_tiles = L.n_tiles; a.S = L.S; a.seed = seed;
  if (strategy != VFM_RANK_RANDOM) {
    const int64_t nu = L.U_pad * (L.Kp + 2), ni = L.C_pad * (L.Kp + 2);
    hipLaunchKernelGGL(k_rank_prep, dim3((unsigned)((nu + 255) / 256)), dim3(256), 0, st, L.U_pad, U, users, (int64_t)0,
                       T, L.Kp, L.KA, d, false, sp, entity_params, bias_params, scalars, (float*)(ws + L.off_uop),
                       (float*)(ws + L.off_ucon));
    if (ni > 0)
      hipLaunchKernelGGL(k_rank_prep, dim3((unsigned)((ni + 255) / 256)), dim3(256), 0, st, L.C_pad, n_cand, cand,
                         item_lo, T, L.Kp, L.KA, d, true, sp, entity_params, bias_params, scalars,
                         (float*)(ws + L.off_iop), (float*)(ws + L.off_icon));
    if (int rc = launch_status("k_rank_prep")) return rc;
  }
  const dim3 grid((unsigned)(L.U_pad / UT), (unsigned)L.S);
  switch (strategy) {
    case VFM_RANK_TOP: hipLaunchKernelGGL(k_rank<VFM_RANK_TOP>, grid, dim3(256), 0, st, a); break;
    case VFM_RANK_VARIANCE: hipLaunchKernelGGL(k_rank<VFM_RANK_VARIANCE>, grid, dim3(256), 0, st, a); break;
    case VFM_RANK_MEAN: hipLaunchKernelGGL(k_rank<VFM_RANK_MEAN>, grid, dim3(256), 0, st, a); break;
    default: hipLaunchKernelGGL(k_rank<VFM_RANK_RANDOM>, grid, dim3(256), 0, st, a); break;
  }
  if (int rc = launch_status("k_rank")) return rc;
  hipLaunchKernelGGL(k_rank_merge, dim3((unsigned)U), dim3(MERGE_BLOCK), 0, st, U, k, L.S, a.ls, a.lc, users, cand,
                     item_lo, T, d, sp, entity_params, bias_params, scalars, out_items, out_score, out_mean, out_var);
  return launch_status("k_rank_merge");
}

}  // extern "C"

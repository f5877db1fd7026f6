// vfm_rank_tile.hpp -- what the catalog ranking (vfm_rank.hip: k_rank) and the held-out evaluation
// (vfm_rank_eval.hip: k_rank_eval) share: the pair score functions, the operand packing (k_rank_prep) and the 256-user x
// 64-item MFMA score tile.  Both units are compiled with -ffp-contract=off, so a pair's score is one k-ordered fp32 fma
// chain whichever unit, tile, split or grid forms it, and equals the k_moments score of the pair bit for bit.  The pair
// functions pin that mode themselves (#pragma clang fp contract(off)): the elicitation session (vfm_elicit.hip) inlines
// them next to the fold-in's arithmetic, which is defined under contraction `on`.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "vfm_launch.hpp"             // launch_status
#include "vfm_rank.h"

namespace vfm {
int fail(int code, const char* msg);          // (vfm_abi.hip: the thread's vfm_last_error() text)
}  // namespace vfm

namespace {

constexpr int UT = 256;       // users per workgroup (one per thread in the per-user scan)
constexpr int IT = 64;        // candidate items per tile
constexpr int KS = 16;        // K values per LDS stage (operand rows are padded to a multiple of KS with zeros)
constexpr float PI_OVER_8 = 0.39269908169872414f;

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float link_of(float s, bool softplus) {
  if (!softplus) return fabsf(s);
  return s > 0.f ? s + log1pf(expf(-s)) : log1pf(expf(s));
}

__device__ __forceinline__ float score_of(int strat, float m, float v) {
#pragma clang fp contract(off)
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
#pragma clang fp contract(off)
  const int k = kb < d ? kb : kb - d;
  const float m = row[k], s = link_of(row[d + k], sp);
  if (!item) return kb < d ? m * m : s * s;
  return kb < d ? s * s : m * m + s * s;
}

// Closed-form moments of the pair (u, i): the same fp32 chains, in the same k order, as the MFMA accumulation of the tile
__device__ void pair_moments(const float* eu, const float* ei, const float* bu, const float* bi, float m0, float sg0,
                             int d, bool sp, float& mean, float& var) {
#pragma clang fp contract(off)
  float am = 0.f, av = 0.f;
  for (int k = 0; k < d; ++k) am = fmaf(op_mean(eu, k), op_mean(ei, k), am);
  for (int kb = 0; kb < 2 * d; ++kb) av = fmaf(op_var(eu, kb, d, false, sp), op_var(ei, kb, d, true, sp), av);
  const float sgu = link_of(bu[1], sp), sgi = link_of(bi[1], sp);
  mean = (am + (m0 + bu[0])) + bi[0];
  var = (av + (sg0 * sg0 + sgu * sgu)) + sgi * sgi;
}

// The order of a ranking: score descending, then id ascending (ids: candidate positions or entity ids, which agree
// because the candidates are strictly ascending)
template <typename ID>
__device__ __forceinline__ bool beats(float s, ID c, float ts, ID tc) { return s > ts || (s == ts && c < tc); }

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

// The LDS of a tile: the operand stage (k-major, KS values of K) and the score image [item][user] that aliases it
union TileSmem {
  struct {
    float A[KS][IT + 4];
    float B[KS][UT + 4];
  } op;
  float S[IT][UT];
};

// The packed operands of one call (k_rank_prep's output)
struct TileOps {
  const float *uop, *iop, *ucon, *icon;
  int Kp, KA, KB;
};

// The user constants the tile adds to the accumulators of this thread's MFMA columns (mean, variance)
template <int STRAT>
__device__ __forceinline__ void tile_user_consts(const TileOps& o, int64_t u0, int tid, float ucm[2], float ucv[2]) {
  const int lane = tid & 63, w = tid >> 6;
  ucm[0] = ucm[1] = ucv[0] = ucv[1] = 0.f;
  if constexpr (STRAT != VFM_RANK_RANDOM) {
    for (int ub = 0; ub < 2; ++ub) {
      const int64_t uc = u0 + w * 64 + ub * 32 + (lane & 31);
      ucm[ub] = o.ucon[uc * 2];
      ucv[ub] = o.ucon[uc * 2 + 1];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// score_tile: the workgroup's 256 users x the 64 candidates from c0 into sm.S[item][user], on return after a barrier.
// The four waves form the block with v_mfma_f32_32x32x2_f32 (wave w: users 64w .. 64w+63 x all 64 items, 2 x 2 blocks
// of 32 x 32; items on the A / row side, users on the B / column side), operands staged k-major in LDS per KS values of
// K.  Only the accumulators the strategy needs run (not called for VFM_RANK_RANDOM).
// ---------------------------------------------------------------------------------------------------------------------
template <int STRAT>
__device__ __forceinline__ void score_tile(const TileOps& o, TileSmem& sm, float* ci_m, float* ci_v, int64_t u0,
                                           int64_t c0, int tid, const float ucm[2], const float ucv[2]) {
  const int lane = tid & 63, w = tid >> 6;
  f32x16 accm[2][2], accv[2][2];
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2; ++j) { accm[i][j] = (f32x16)(0.f); accv[i][j] = (f32x16)(0.f); }
  if (tid < IT) { ci_m[tid] = o.icon[(c0 + tid) * 2]; ci_v[tid] = o.icon[(c0 + tid) * 2 + 1]; }
#pragma unroll
  for (int part = 0; part < 2; ++part) {
    const int K = part == 0 ? o.KA : o.KB, off = part == 0 ? 0 : o.KA;
    if ((part == 0 && STRAT == VFM_RANK_VARIANCE) || (part == 1 && STRAT == VFM_RANK_TOP)) continue;
    for (int k0 = 0; k0 < K; k0 += KS) {
      __syncthreads();
      {
        const int r = tid >> 2, q = tid & 3;
        const float4 v = *reinterpret_cast<const float4*>(o.iop + (c0 + r) * o.Kp + off + k0 + 4 * q);
        sm.op.A[4 * q + 0][r] = v.x; sm.op.A[4 * q + 1][r] = v.y;
        sm.op.A[4 * q + 2][r] = v.z; sm.op.A[4 * q + 3][r] = v.w;
      }
#pragma unroll
      for (int rep = 0; rep < 4; ++rep) {
        const int idx = rep * 256 + tid, r = idx >> 2, q = idx & 3;
        const float4 v = *reinterpret_cast<const float4*>(o.uop + (u0 + r) * o.Kp + off + k0 + 4 * q);
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
  __syncthreads();                      // (the score image overwrites the operand stage)
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

// ---------------------------------------------------------------------------------------------------------------------
// host side: the packed-operand part of a workspace, the split count, and the call record (RankCall) with the argument
// checks and the launch-record fill that every ranking entry shares
// ---------------------------------------------------------------------------------------------------------------------
inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

struct OpLayout {
  int KA, KB, Kp, S, n_tiles;
  int64_t U_pad, C_pad, off_uop, off_iop, off_ucon, off_icon, end;
};

// The operand blocks from offset 0 (256-byte aligned each) and the split count (n_splits = 0: about two workgroups per
// CU of the 256 -- split the items when the users do not fill the chip)
inline OpLayout op_layout_of(int64_t U, int64_t n_cand, int d, int strategy, int n_splits) {
  OpLayout L;
  L.KA = (strategy == VFM_RANK_TOP || strategy == VFM_RANK_MEAN) ? (int)round_up(d, KS) : 0;
  L.KB = (strategy == VFM_RANK_VARIANCE || strategy == VFM_RANK_MEAN) ? (int)round_up(2 * (int64_t)d, KS) : 0;
  L.Kp = L.KA + L.KB;
  L.U_pad = round_up(U, UT);
  L.C_pad = round_up(n_cand, IT);
  L.n_tiles = (int)(L.C_pad / IT);
  if (n_splits > 0) {
    L.S = n_splits;
  } else {
    const int64_t n_ut = L.U_pad / UT;
    int64_t S = n_ut > 0 ? (512 + n_ut - 1) / n_ut : 1;
    S = S < 1 ? 1 : S;
    S = S > VFM_RANK_MAX_SPLITS ? VFM_RANK_MAX_SPLITS : S;
    S = S > L.n_tiles ? L.n_tiles : S;
    L.S = (int)(S < 1 ? 1 : S);
  }
  L.off_uop = 0;
  L.off_iop = L.off_uop + round_up(L.U_pad * L.Kp * 4, 256);
  L.off_ucon = L.off_iop + round_up(L.C_pad * L.Kp * 4, 256);
  L.off_icon = L.off_ucon + round_up(L.U_pad * 2 * 4, 256);
  L.end = L.off_icon + round_up(L.C_pad * 2 * 4, 256);
  return L;
}

inline int check_common(int64_t T, int32_t d, int32_t flags, int32_t strategy) {
  if (T < 1) return vfm::fail(VFM_E_INVALID, "T < 1");
  if (d < 1 || d > 4096) return vfm::fail(VFM_E_INVALID, "d out of range [1,4096]");
  if (flags & ~VFM_FLAG_LINK_SOFTPLUS) return vfm::fail(VFM_E_INVALID, "flags: only VFM_FLAG_LINK_SOFTPLUS is accepted");
  if (strategy < VFM_RANK_TOP || strategy > VFM_RANK_RANDOM) return vfm::fail(VFM_E_INVALID, "unknown strategy");
  return 0;
}

// One ranking call as its extern "C" entry received it (host only; never a kernel argument).  The six ranking entries
// fill it and hand it on: the checks, the preps and the launch records read it instead of thirty positional arguments.
struct RankCall {
  int64_t Q = 0;                                            // the queries:
  const int64_t* queries = nullptr;                         //   users [Q] (pair forms) or contexts [Q, F] (field forms)
  const int64_t* qkey = nullptr;                            //   field forms: the caller's Philox keys [Q], or NULL
  int32_t field = 0, post_field = -1;                       //   field forms: the ranked column; the supplied column
  bool has_post = false;
  const float* post = nullptr;                              //   [Q, 2d + 2] when has_post
  int64_t n_cand = 0, cand_lo = 0;                          // the candidates: cand [n_cand], or the range from cand_lo
  const int64_t* cand = nullptr;
  const int64_t *excl_ptr = nullptr, *excl_items = nullptr; // the exclusion CSR over the queries
  int64_t n_excl = 0;
  const int64_t *pos_ptr = nullptr, *pos_items = nullptr;   // held-out forms: the positives CSR over the queries
  int64_t n_pos = 0;
  int64_t T = 0;                                            // the tables
  int32_t F = 0, d = 0;
  const float *ent = nullptr, *bias = nullptr, *scal = nullptr;
  void* workspace = nullptr;
  int64_t workspace_bytes = 0;
  int32_t k = 0, strategy = 0, flags = 0, n_splits = 0;     // k: top-k forms
  uint64_t seed = 0;
  int64_t* out_items = nullptr;                             // top-k forms: [Q, k] each
  float *out_score = nullptr, *out_mean = nullptr, *out_var = nullptr;
  int64_t *out_rank = nullptr, *out_rank_neg = nullptr;     // held-out forms: [n_pos] each
  int64_t *out_n_eligible = nullptr, *out_n_neg = nullptr;  //   and [Q] each
  hipStream_t stream = nullptr;

  bool softplus() const { return (flags & VFM_FLAG_LINK_SOFTPLUS) != 0; }
  int64_t n_excl_used() const { return excl_ptr ? n_excl : 0; }
};

// What an entry asks of a call
enum RankAsk { RANK_ASK_TOPK = 0, RANK_ASK_HELDOUT = 1, RANK_ASK_FIELD = 2 };      // (FIELD: or-ed in by the field forms)

// The checks every ranking entry makes after check_common and its own conditions on F and the fields.  Q == 0 passes
// before any pointer is looked at: the caller returns 0 then.
inline int check_rank_call(const RankCall& r, int ask) {
  const bool heldout = (ask & RANK_ASK_HELDOUT) != 0, fieldf = (ask & RANK_ASK_FIELD) != 0;
  if (!heldout && (r.k < 1 || r.k > VFM_RANK_MAX_K)) return vfm::fail(VFM_E_INVALID, "k out of range [1,128]");
  if (r.Q < 0) return vfm::fail(VFM_E_INVALID, fieldf ? "Q < 0" : "U < 0");
  if (r.n_cand < 0 || r.n_cand >= ((int64_t)1 << 31)) return vfm::fail(VFM_E_INVALID, "n_cand out of range [0,2^31)");
  if (heldout && (r.n_pos < 0 || r.n_pos >= ((int64_t)1 << 40)))
    return vfm::fail(VFM_E_INVALID, "n_pos out of range [0,2^40)");
  if (r.n_splits < 0 || r.n_splits > VFM_RANK_MAX_SPLITS) return vfm::fail(VFM_E_INVALID, "n_splits out of range [0,64]");
  if (!r.cand && (r.cand_lo < 0 || r.cand_lo + r.n_cand > r.T))
    return vfm::fail(VFM_E_INVALID, fieldf ? "candidate range outside [0,T)" : "item range outside [0,T)");
  if (r.n_excl < 0 || (r.n_excl > 0 && (!r.excl_ptr || !r.excl_items)))
    return vfm::fail(VFM_E_INVALID, "exclusion lists: excl_ptr and excl_items together, n_excl >= 0");
  if (heldout && r.n_pos > 0 && !r.pos_items) return vfm::fail(VFM_E_INVALID, "null pointer: pos_items");
  if (r.Q == 0) return 0;
  if (!r.queries || !r.ent || !r.bias || !r.scal || !r.workspace) return vfm::fail(VFM_E_INVALID, "null pointer");
  if (heldout ? (!r.pos_ptr || !r.out_n_eligible || !r.out_n_neg || (r.n_pos > 0 && (!r.out_rank || !r.out_rank_neg)))
              : (!r.out_items || !r.out_score || !r.out_mean || !r.out_var))
    return vfm::fail(VFM_E_INVALID, "null pointer");
  if (r.has_post && !r.post) return vfm::fail(VFM_E_INVALID, "null pointer: post");
  return 0;
}

// The workspace of a checked call against the bytes its layout needs (too_small: the message, which names the entry
// point that tells the size)
inline int check_rank_workspace(const RankCall& r, int64_t bytes, const char* too_small) {
  if (r.workspace_bytes < bytes) return vfm::fail(VFM_E_INVALID, too_small);
  if (((uintptr_t)r.workspace) & 255) return vfm::fail(VFM_E_INVALID, "workspace must be 256-byte aligned");
  return 0;
}

// What a scan record (vfm::RankScan) and an evaluation record (vfm::RankEval) name alike, from the call and the operand
// blocks of its workspace (L: OpLayout, or the field form's layout with the same members)
template <class R, class L>
inline void fill_scan(R& a, const RankCall& r, const L& lay, const int64_t* keys) {
  const char* ws = (const char*)r.workspace;
  a.U = r.Q; a.n_cand = r.n_cand; a.item_lo = r.cand_lo; a.n_excl = r.n_excl_used();
  a.keys = keys; a.cand = r.cand; a.excl_ptr = r.excl_ptr; a.excl_items = r.excl_items;
  a.uop = (const float*)(ws + lay.off_uop); a.iop = (const float*)(ws + lay.off_iop);
  a.ucon = (const float*)(ws + lay.off_ucon); a.icon = (const float*)(ws + lay.off_icon);
  a.Kp = lay.Kp; a.KA = lay.KA; a.KB = lay.KB;
  a.n_tiles = lay.n_tiles; a.S = lay.S; a.seed = r.seed;
}

// k_rank_prep over the query users and the candidates into the operand blocks of L (not for VFM_RANK_RANDOM)
inline int launch_rank_prep(const OpLayout& L, const RankCall& r) {
  char* ws = (char*)r.workspace;
  const bool sp = r.softplus();
  const int64_t nu = L.U_pad * (L.Kp + 2), ni = L.C_pad * (L.Kp + 2);
  hipLaunchKernelGGL(k_rank_prep, dim3((unsigned)((nu + 255) / 256)), dim3(256), 0, r.stream, L.U_pad, r.Q, r.queries,
                     (int64_t)0, r.T, L.Kp, L.KA, (int)r.d, false, sp, r.ent, r.bias, r.scal, (float*)(ws + L.off_uop),
                     (float*)(ws + L.off_ucon));
  if (ni > 0)
    hipLaunchKernelGGL(k_rank_prep, dim3((unsigned)((ni + 255) / 256)), dim3(256), 0, r.stream, L.C_pad, r.n_cand, r.cand,
                       r.cand_lo, r.T, L.Kp, L.KA, (int)r.d, true, sp, r.ent, r.bias, r.scal, (float*)(ws + L.off_iop),
                       (float*)(ws + L.off_icon));
  return launch_status("k_rank_prep");
}

}  // namespace

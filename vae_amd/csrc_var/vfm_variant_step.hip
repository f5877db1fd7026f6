// vfm_variant_step.hip -- the fused training step of the ELBO variants (include/vfm_variant_step.h): the backward of
// csrc/vfm_variants.hip / vfm_variants8.hpp with torch.optim.Adam's dense update applied to a table row while its
// gradient is still in registers.  The forward stays vfm_variant_fwd_f32.
//
// Outside csrc/ (build.sources_digest() ties the committed traffic profile to those files).  VarArgs and the variant
// arithmetic live inside vfm_variants.hip and cannot be included, so this unit RESTATES the entity-centric walk and the
// epilogue formulas of k_var_bwd / k_var_bwd8, the span / row guards and k_positions; the fp64 tests of
// tests/test_gpu_variant_step.py are what ties the two copies together.  Included from csrc/: the Philox stream
// (vfm_rng.hpp), SIGMA_MIN / signf / group_index (vfm_common.hpp), the error plumbing (vfm_args.hpp).
//
// One kernel template serves both families:
//   W = 8  d % 8 == 0: a lane group of LPE lanes owns a table row, lane p the blocks p + i LPE (i < CPL) of 8 coordinates
//          -- two float4 loads per table, the 8 normals of one Philox call (the shapes of k_var_bwd8)
//   W = 1  any other d: LPE lanes per row, lane p the coordinates p + i LPE (d = 2, VFMClosedForm's default: 4 lanes)
// Workgroups own CONTIGUOUS entity ranges and walk them one id group at a time; two occurrences of a row's list are in
// flight.  Races: a lane group reads only its own table row, the per-batch-row state / grow (never written here) and
// scalars / priors (written by the launch that FOLLOWS), so the in-place update of (p, m, v) of a row is race free.
// scalars[3] and the priors are read by every workgroup: workgroup 0 forms the scalars' gradient, every workgroup
// writes one partial row per id group of the prior gradients, and k_vstep_small sums those rows in a fixed order (no
// float atomics for any d: the step is reproducible bit for bit) and updates scalars and priors.
// Update form: k_adam's (csrc/vfm_adam.hpp) -- IEEE sqrt and divisions, plain moments, streamed non-temporally.
// gfx950 only, wave = 64.
#include <math.h>
#include <string.h>

#include "vfm_args.hpp"
#include "vfm_variant_step.h"

namespace vfm {
namespace {

#include "vfm_rng.hpp"
#include "vfm_common.hpp"

constexpr int VSTEP_BLOCKS = 2048;     // workgroup cap of k_vstep (rows of the prior-gradient scratch: + G)
constexpr int VSTEP_KT = 8;            // k_vstep_small: elements of the prior vector per workgroup ...
constexpr int VSTEP_CH = 32;           // ... times chunks of the partial-row range, each summed by its own lanes
constexpr int VSTEP_MAX_D = 1024;
constexpr int VSTEP_POS_BLOCKS = 4096;
typedef float v2f __attribute__((ext_vector_type(2)));

struct StepArgs {
  int64_t B, T;
  int32_t F, d, G, lik, eps_mode, n_occ;
  float ll_scale;                      // nb_train / B_global
  RngKey key;
  const float* xv;                     // [B,F] feature values or NULL
  float* entity;
  float* bias;
  const float* inv_occ;
  const float* scalars;
  const double* W;
  const float* priors;                 // [2 | G | G | G*d | G*d] or NULL
  const float* eps_entity;
  const float* eps_bias;
  const float* eps_global;
  const int32_t* occ_ptr;
  const int32_t* occ_rows;
  const int32_t* occ_pos;              // positions r*F + f of the occurrences (with values)
  const float* state;
  const float* grow;
  const double* partials;
  const float* grad_out;
  float* m_entity; float* v_entity; float* m_bias; float* v_bias;
  float* prows;                        // [VSTEP_BLOCKS + G, 2d + 2] partial rows of the prior gradients
  float* gsmall;                       // [8] gradients of scalars[3] and of the global prior (2)
  int32_t* status;                     // vfm_index_t.status: clamped index entries (may be NULL)
  float b1, b2, eps, step_size, bc2_sqrt;
  int64_t group_hi[VFM_MAX_FIELDS];
  double group_n[VFM_MAX_FIELDS];
};

// torch.optim.Adam's single-tensor update, the operation sequence of k_adam
__device__ __forceinline__ void adam1(const StepArgs& a, float& p, float g, float& m, float& v) {
  m = m + (g - m) * (1.0f - a.b1);
  v = v * a.b2 + ((1.0f - a.b2) * g) * g;
  const float denom = __fsqrt_rn(v) / a.bc2_sqrt + a.eps;
  p = p + (-a.step_size * m) / denom;
}

template <int W>
__device__ __forceinline__ void ldw(const float* __restrict__ p, float (&v)[W]) {
  if constexpr (W == 8) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  } else {
    v[0] = *p;
  }
}
template <int W>
__device__ __forceinline__ void stw(float* __restrict__ p, const float (&v)[W]) {
  if constexpr (W == 8) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
  } else {
    *p = v[0];
  }
}
// the moments: read and written once per step and far larger than the caches (as k_adam streams them)
template <int W>
__device__ __forceinline__ void ldw_nt(const float* __restrict__ p, float (&v)[W]) {
  if constexpr (W == 8) {
    const v4f a = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(p));
    const v4f b = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(p + 4));
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  } else {
    v[0] = __builtin_nontemporal_load(p);
  }
}
template <int W>
__device__ __forceinline__ void stw_nt(float* __restrict__ p, const float (&v)[W]) {
  if constexpr (W == 8) {
    const v4f a = {v[0], v[1], v[2], v[3]}, b = {v[4], v[5], v[6], v[7]};
    __builtin_nontemporal_store(a, reinterpret_cast<v4f*>(p));
    __builtin_nontemporal_store(b, reinterpret_cast<v4f*>(p + 4));
  } else {
    __builtin_nontemporal_store(v[0], p);
  }
}

__device__ __forceinline__ float2 step_prior0(const StepArgs& a) {
  return a.priors ? make_float2(a.priors[0], fmaxf(fabsf(a.priors[1]), SIGMA_MIN)) : make_float2(0.f, 1.f);
}

// ---------------------------------------------------------------------------------------
// the table kernel
// ---------------------------------------------------------------------------------------
template <int W, int LPE, int CPL, bool CF, bool HASV, bool PRI>
__global__ __launch_bounds__(BLOCK) void k_vstep(const StepArgs a) {
  constexpr int GPB = BLOCK / LPE;
  constexpr int NS = CF ? 3 : 1;
  constexpr int DP = W * LPE * CPL;                             // coordinates a lane group has room for (>= d)
  __shared__ float sh_acc[PRI ? GPB * 2 * DP : 1];              // [GPB][2 DP] partial prior gradients
  __shared__ float sh_w[PRI ? 2 * GPB : 1];
  __shared__ float sh_cw[VFM_MAX_FIELDS];
  __shared__ int64_t sh_hi[VFM_MAX_FIELDS];
  const int tid = threadIdx.x, lig = tid % LPE, grp = tid / LPE;
  const int d = a.d, NI = d / W;                                // NI: items (W coordinates each) of a row
  if (tid < a.G) { sh_cw[tid] = (float)(a.group_n[tid] / a.W[tid]); sh_hi[tid] = a.group_hi[tid]; }
  __syncthreads();
  const float gout = a.grad_out[0];
  const float alpha = a.scalars[0], m0 = a.scalars[1], s0 = a.scalars[2];
  const float aabs = fabsf(alpha), sg0 = fmaxf(fabsf(s0), SIGMA_MIN);
  const float h = CF ? 0.5f * a.ll_scale * aabs : 0.f;          // dloss/dT_n
  const bool tab = a.eps_mode == EPS_TABLE;
  if (blockIdx.x == 0 && tid == 0) {                            // the three scalars + the global prior (k_var_bwd's formulas)
    const bool ok = a.partials[VFM_P_REDUCED] == 1.0;
    const float nanv = __builtin_nanf("");
    const float sum_g = ok ? (float)a.partials[VFM_P_G] : nanv, sum_a = (float)a.partials[VFM_P_ALPHA];
    const float2 p0 = step_prior0(a);
    const float dm = m0 - p0.x;
    float e0 = 0.f;
    if constexpr (!CF) {
      if (tab) {
        e0 = a.eps_global[0];
      } else {
        float n[8], nb;
        normal8b(a.key, 0xFFFFFFFFu, 0u, n, nb);
        e0 = n[0];
      }
    }
    a.gsmall[0] = (a.lik == VFM_LIK_NORMAL) ? gout * signf(alpha) * a.ll_scale * sum_a : 0.f;
    a.gsmall[1] = gout * (sum_g + dm / (p0.y * p0.y));
    a.gsmall[2] = gout * signf(s0) * (e0 * sum_g + 2.f * h * sg0 * (float)a.B + sg0 / (p0.y * p0.y) - 1.f / sg0);
    if constexpr (PRI) {
      a.gsmall[3] = gout * (-dm / (p0.y * p0.y));
      a.gsmall[4] = gout * signf(a.priors[1]) * (1.f / p0.y - (sg0 * sg0 + dm * dm) / (p0.y * p0.y * p0.y));
    }
  }
  const float* pri_m = PRI ? a.priors + 2 + 2 * a.G : nullptr;
  const float* pri_s = PRI ? pri_m + (size_t)a.G * d : nullptr;
  int nclamp = 0;                                               // index entries clamped (vfm_index_t.status)
  // this workgroup's contiguous entity range, walked one id group at a time (uniform loop)
  int64_t epb = (a.T + gridDim.x - 1) / gridDim.x;
  epb = (epb + GPB - 1) / GPB * GPB;
  int64_t e_lo = (int64_t)blockIdx.x * epb;
  const int64_t e_end = e_lo + epb < a.T ? e_lo + epb : a.T;
  int g = e_lo < a.T ? group_index(sh_hi, a.G, e_lo) : 0;
  while (e_lo < e_end) {
    const int64_t seg_hi = (sh_hi[g] < e_end && g + 1 < a.G) ? sh_hi[g] : e_end;
    float acc_mp[CPL][W], acc_sp[CPL][W], acc_mw = 0.f, acc_sw = 0.f;
#pragma unroll
    for (int i = 0; i < CPL; ++i)
#pragma unroll
      for (int t = 0; t < W; ++t) { acc_mp[i][t] = 0.f; acc_sp[i][t] = 0.f; }
    float pwm = 0.f, pws = 1.f, pws_raw = 1.f;
    if constexpr (PRI) { pwm = a.priors[2 + g]; pws_raw = a.priors[2 + a.G + g]; pws = fmaxf(fabsf(pws_raw), SIGMA_MIN); }
    for (int64_t e = e_lo + grp; e < seg_hi; e += GPB) {
      int beg = a.occ_ptr[e], end = a.occ_ptr[e + 1];
      if (beg < 0 || end < beg || end > a.n_occ) { beg = end = 0; nclamp += (lig == 0); }    // a bad span is not followed
      const size_t ro = (size_t)e * (2 * (size_t)d);
      // the entity's own row (independent of the walk)
      float mu[CPL][W], s[CPL][W];
#pragma unroll
      for (int i = 0; i < CPL; ++i) {
        int j = lig + i * LPE;
        j = j < NI ? j : NI - 1;                                // (lanes past the end re-load the last item)
        ldw<W>(a.entity + ro + W * j, mu[i]);
        ldw<W>(a.entity + ro + d + W * j, s[i]);
      }
      float2 th = *reinterpret_cast<const float2*>(a.bias + 2 * (size_t)e);
      float gb0 = 0.f, gb1 = 0.f;                               // gradient of the bias pair
      // (p, m, v) of item i <- one Adam step with the gradient (gm, gs)
      auto update = [&](int i, const float (&gm)[W], const float (&gs)[W]) {
        const int j = lig + i * LPE;
        if (j >= NI) return;
        const size_t o = ro + (size_t)W * j;
        float m1[W], v1[W], m2[W], v2[W];
        ldw_nt<W>(a.m_entity + o, m1); ldw_nt<W>(a.v_entity + o, v1);
        ldw_nt<W>(a.m_entity + o + d, m2); ldw_nt<W>(a.v_entity + o + d, v2);
#pragma unroll
        for (int t = 0; t < W; ++t) {
          adam1(a, mu[i][t], gm[t], m1[t], v1[t]);
          adam1(a, s[i][t], gs[t], m2[t], v2[t]);
        }
        stw_nt<W>(a.m_entity + o, m1); stw_nt<W>(a.v_entity + o, v1);
        stw_nt<W>(a.m_entity + o + d, m2); stw_nt<W>(a.v_entity + o + d, v2);
        stw<W>(a.entity + o, mu[i]);
        stw<W>(a.entity + o + d, s[i]);
      };
      if (beg == end) {                                         // not in the batch: the zero-gradient step of dense Adam
        float z[W];
#pragma unroll
        for (int t = 0; t < W; ++t) z[t] = 0.f;
#pragma unroll
        for (int i = 0; i < CPL; ++i) update(i, z, z);
      } else {
        const float c = sh_cw[g] * a.inv_occ[e] * (float)(end - beg);          // KL weight of e
        // walk: A1 = sum g_r v S_r, A2 = sum v^2 S2_r, A3 = sum v^2 Q_r; gv = sum g_r v, gv2 = sum g_r v^2, ...
        float A1[CPL][W], A2[CF ? CPL : 1][W], A3[CF ? CPL : 1][W];
#pragma unroll
        for (int i = 0; i < CPL; ++i)
#pragma unroll
          for (int t = 0; t < W; ++t) { A1[i][t] = 0.f; if constexpr (CF) { A2[i][t] = 0.f; A3[i][t] = 0.f; } }
        float gv = 0.f, gv2 = 0.f, vv2 = 0.f, v4 = 0.f;
        auto one = [&](int r, float v, float gr) {
          const float gw = gr * v, w2 = v * v;
          gv += gw; gv2 = fmaf(gw, v, gv2); vv2 += w2; v4 = fmaf(w2, w2, v4);
          const float* st = a.state + (size_t)r * NS * d;
#pragma unroll
          for (int i = 0; i < CPL; ++i) {
            int j = lig + i * LPE;
            j = j < NI ? j : NI - 1;
            float x1[W];
            ldw<W>(st + W * j, x1);
#pragma unroll
            for (int t = 0; t < W; ++t) A1[i][t] = fmaf(gw, x1[t], A1[i][t]);
            if constexpr (CF) {
              float x2[W], x3[W];
              ldw<W>(st + d + W * j, x2);
              ldw<W>(st + 2 * d + W * j, x3);
#pragma unroll
              for (int t = 0; t < W; ++t) { A2[i][t] = fmaf(w2, x2[t], A2[i][t]); A3[i][t] = fmaf(w2, x3[t], A3[i][t]); }
            }
          }
        };
        auto row_of = [&](int o) {                              // a bad row number is not followed
          int r = a.occ_rows[o];
          if ((unsigned)r >= (unsigned)a.B) { r = 0; nclamp += (lig == 0); }
          return r;
        };
        auto value_of = [&](int o) {
          int pos = a.occ_pos[o];
          pos = (unsigned)pos < (unsigned)a.n_occ ? pos : 0;
          return a.xv[pos];
        };
        int o = beg;
        for (; o + 1 < end; o += 2) {                           // two occurrences in flight
          const int ra = row_of(o), rb = row_of(o + 1);
          float va = 1.f, vb = 1.f;
          if constexpr (HASV) { va = value_of(o); vb = value_of(o + 1); }
          const float ga = a.grow[ra], gb = a.grow[rb];
          one(ra, va, ga);
          one(rb, vb, gb);
        }
        if (o < end) {
          const int ra = row_of(o);
          float va = 1.f;
          if constexpr (HASV) va = value_of(o);
          one(ra, va, a.grow[ra]);
        }
        // epilogue (the formulas of k_var_bwd), item by item: gradient, prior-gradient share, Adam
        float nb = 0.f;
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
          const int j = lig + i * LPE;
          const bool valid = j < NI;
          const int jc = valid ? j : 0;
          float ep[W];
#pragma unroll
          for (int t = 0; t < W; ++t) ep[t] = 0.f;
          if constexpr (!CF) {
            if (tab) {
              ldw<W>(a.eps_entity + (size_t)e * d + W * jc, ep);
              if (i == 0) nb = a.eps_bias[e];
            } else {
              float n[8], nbi;
              normal8b(a.key, (uint32_t)e, W == 8 ? (uint32_t)jc : ((uint32_t)jc >> 3), n, nbi);
              if (i == 0) nb = nbi;                             // (item 0 sits in lane 0, i == 0: Philox block 0)
              if constexpr (W == 8) {
#pragma unroll
                for (int t = 0; t < 8; ++t) ep[t] = n[t];
              } else {
                float v = n[0];
#pragma unroll
                for (int t = 1; t < 8; ++t) v = ((jc & 7) == t) ? n[t] : v;
                ep[0] = v;
              }
            }
          }
          float pm[W], ps[W];
          if constexpr (PRI) { ldw<W>(pri_m + (size_t)g * d + W * jc, pm); ldw<W>(pri_s + (size_t)g * d + W * jc, ps); }
          float gm8[W], gs8[W];
#pragma unroll
          for (int t = 0; t < W; ++t) {
            const float m_ = mu[i][t], s_ = s[i][t], sg = fmaxf(fabsf(s_), SIGMA_MIN);
            const float z = CF ? m_ : fmaf(fabsf(s_), ep[t], m_);
            const float prm = PRI ? pm[t] : 0.f, prs = PRI ? fmaxf(fabsf(ps[t]), SIGMA_MIN) : 1.f;
            const float dm = m_ - prm, ip2 = 1.f / (prs * prs);
            float gmu = A1[i][t] - z * gv2, gs_;
            if constexpr (CF) {
              const float b2 = s_ * s_, am = m_ * m_;
              gmu += 2.f * h * m_ * (A2[i][t] - v4 * b2);
              gs_ = 2.f * h * s_ * (A3[i][t] - v4 * (am + b2));
            } else {
              gs_ = signf(s_) * (A1[i][t] - z * gv2) * ep[t];
            }
            gmu += c * dm * ip2;
            gs_ += c * signf(s_) * (sg * ip2 - 1.f / sg);
            gm8[t] = gout * gmu;
            gs8[t] = gout * gs_;
            if constexpr (PRI) {
              if (valid) {
                acc_mp[i][t] += gout * c * (-dm * ip2);
                acc_sp[i][t] += gout * c * signf(ps[t]) * (1.f / prs - (sg * sg + dm * dm) * ip2 / prs);
              }
            }
          }
          update(i, gm8, gs8);
        }
        if (lig == 0) {
          const float sw = fmaxf(fabsf(th.y), SIGMA_MIN);
          const float dm = th.x - pwm, ip2 = 1.f / (pws * pws);
          const float g0 = gv + c * dm * ip2;
          const float g1 = (CF ? 2.f * h * th.y * vv2 : signf(th.y) * gv * nb) + c * signf(th.y) * (sw * ip2 - 1.f / sw);
          gb0 = gout * g0; gb1 = gout * g1;
          if constexpr (PRI) {
            acc_mw += gout * c * (-dm * ip2);
            acc_sw += gout * c * signf(pws_raw) * (1.f / pws - (sw * sw + dm * dm) * ip2 / pws);
          }
        }
      }
      if (lig == 0) {                                           // the bias pair
        v2f mb = __builtin_nontemporal_load(reinterpret_cast<const v2f*>(a.m_bias + 2 * (size_t)e));
        v2f vb = __builtin_nontemporal_load(reinterpret_cast<const v2f*>(a.v_bias + 2 * (size_t)e));
        float mbx = mb.x, mby = mb.y, vbx = vb.x, vby = vb.y;
        adam1(a, th.x, gb0, mbx, vbx);
        adam1(a, th.y, gb1, mby, vby);
        mb.x = mbx; mb.y = mby; vb.x = vbx; vb.y = vby;
        __builtin_nontemporal_store(mb, reinterpret_cast<v2f*>(a.m_bias + 2 * (size_t)e));
        __builtin_nontemporal_store(vb, reinterpret_cast<v2f*>(a.v_bias + 2 * (size_t)e));
        *reinterpret_cast<float2*>(a.bias + 2 * (size_t)e) = th;
      }
    }
    if constexpr (PRI) {           // this workgroup's share of group g's prior gradients -> partial row blockIdx.x + g
      __syncthreads();
#pragma unroll
      for (int i = 0; i < CPL; ++i)
#pragma unroll
        for (int t = 0; t < W; ++t) {
          const int k = W * (lig + i * LPE) + t;
          sh_acc[(size_t)grp * 2 * DP + k] = acc_mp[i][t];
          sh_acc[(size_t)grp * 2 * DP + DP + k] = acc_sp[i][t];
        }
      if (lig == 0) { sh_w[2 * grp] = acc_mw; sh_w[2 * grp + 1] = acc_sw; }
      __syncthreads();
      float* prow = a.prows + ((size_t)blockIdx.x + (size_t)g) * (2 * (size_t)d + 2);
      for (int k = tid; k < 2 * d; k += BLOCK) {
        const int kk = k < d ? k : DP + (k - d);
        float t = 0.f;
        for (int q = 0; q < GPB; ++q) t += sh_acc[(size_t)q * 2 * DP + kk];
        prow[k] = t;
      }
      if (tid < 2) {
        float t = 0.f;
        for (int q = 0; q < GPB; ++q) t += sh_w[2 * q + tid];
        prow[2 * d + tid] = t;
      }
    }
    e_lo = seg_hi;
    ++g;
    if (g >= a.G) g = a.G - 1;
  }
  if (nclamp != 0 && a.status) atomicAdd(a.status, nclamp);
}

// ---------------------------------------------------------------------------------------
// scalars and priors: the launch after the table kernel.  Workgroup (g, y) of the first G columns owns VSTEP_KT
// elements of group g's share of the prior vector: VSTEP_CH chunks of the partial-row range are summed side by side
// (eight rows in flight each), the chunks in order, and the owner of an element applies Adam to it.  The last column's
// workgroup updates the three scalars and the global prior from the gradients workgroup 0 of k_vstep left.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_vstep_small(const StepArgs a, float* __restrict__ scalars, float* __restrict__ priors,
                                                       float* __restrict__ m_sc, float* __restrict__ v_sc,
                                                       float* __restrict__ m_pr, float* __restrict__ v_pr, int64_t epb,
                                                       int nblk) {
  __shared__ float sh[VSTEP_CH][VSTEP_KT];
  if (blockIdx.x == gridDim.x - 1) {
    const int t = threadIdx.x;
    if (blockIdx.y != 0) return;
    if (t < 3) {
      float p = scalars[t], m = m_sc[t], v = v_sc[t];
      adam1(a, p, a.gsmall[t], m, v);
      scalars[t] = p; m_sc[t] = m; v_sc[t] = v;
    } else if (t < 5 && priors) {
      float p = priors[t - 3], m = m_pr[t - 3], v = v_pr[t - 3];
      adam1(a, p, a.gsmall[t], m, v);
      priors[t - 3] = p; m_pr[t - 3] = m; v_pr[t - 3] = v;
    }
    return;
  }
  const int g = blockIdx.x, G = a.G, d = a.d;
  const int kk = threadIdx.x % VSTEP_KT, c = threadIdx.x / VSTEP_KT;
  const int k = blockIdx.y * VSTEP_KT + kk;
  const size_t len = 2 * (size_t)d + 2;
  const int64_t lo = g > 0 ? a.group_hi[g - 1] : 0;
  int64_t hi = (g + 1 < G) ? a.group_hi[g] : a.T;
  if (hi > a.T) hi = a.T;
  float part = 0.f;
  if (k < 2 * d + 2 && hi > lo) {
    const int64_t b0 = lo / epb;
    int64_t b1 = (hi - 1) / epb;
    if (b1 > nblk - 1) b1 = nblk - 1;
    const int64_t per = (b1 - b0 + VSTEP_CH) / VSTEP_CH;        // rows per chunk
    int64_t b = b0 + c * per;
    const int64_t be = b + per - 1 < b1 ? b + per - 1 : b1;
    const float* base = a.prows + (size_t)g * len + k;
    float t[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (; b + 7 <= be; b += 8) {
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] += base[(size_t)(b + u) * len];
    }
    for (; b <= be; ++b) t[0] += base[(size_t)b * len];
    part = ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]));
  }
  sh[c][kk] = part;
  __syncthreads();
  if (c == 0 && k < 2 * d + 2) {
    float gsum = 0.f;
#pragma unroll 8
    for (int q = 0; q < VSTEP_CH; ++q) gsum += sh[q][kk];
    size_t idx;
    if (k < d) idx = 2 + 2 * (size_t)G + (size_t)g * d + k;
    else if (k < 2 * d) idx = 2 + 2 * (size_t)G + (size_t)G * d + (size_t)g * d + (k - d);
    else if (k == 2 * d) idx = 2 + (size_t)g;
    else idx = 2 + (size_t)G + g;
    float p = priors[idx], m = m_pr[idx], v = v_pr[idx];
    adam1(a, p, gsum, m, v);
    priors[idx] = p; m_pr[idx] = m; v_pr[idx] = v;
  }
}

// the inverted index stores ROW numbers; with values the walk needs the position r*F + f of every occurrence
// (k_positions of vfm_variants.hip, restated)
__global__ void k_vstep_positions(const int32_t* __restrict__ occ_ptr, const int32_t* __restrict__ occ_rows, const void* x,
                                  int id64, int F, int64_t T, int32_t* __restrict__ occ_pos, int64_t B,
                                  int32_t* __restrict__ status) {
  // entity e's occurrences in row r: the fields f of r with x[r,f] == e, in field order (the index is stable)
  const int n_occ = (int)(B * F);
  int nclamp = 0;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < T; e += (int64_t)gridDim.x * blockDim.x) {
    int beg = occ_ptr[e], end = occ_ptr[e + 1];
    if (beg < 0 || end < beg || end > n_occ) { beg = end = 0; ++nclamp; }
    int last_r = -1, f = 0;
    for (int o = beg; o < end; ++o) {
      int r = occ_rows[o];
      if ((unsigned)r >= (unsigned)B) { r = 0; ++nclamp; }
      if (r != last_r) { last_r = r; f = 0; }
      for (; f < F; ++f) {
        const int64_t id = id64 ? ((const int64_t*)x)[(int64_t)r * F + f] : (int64_t)((const int32_t*)x)[(int64_t)r * F + f];
        if (id == e || (e == 0 && (id < 0 || id >= T))) break;
      }
      occ_pos[o] = r * F + (f < F ? f : F - 1);
      ++f;
    }
  }
  if (nclamp != 0 && status) atomicAdd(status, nclamp);
}

// ---------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------
// lane-group shapes.  W = 8 (d % 8 == 0): those of k_var_bwd8;  W = 1: 4, 16 or 64 lanes, up to 16 coordinates per lane
#define VFM_FOR_VSTEP_SHAPES8(X) X(8, 1, 1) X(8, 2, 1) X(8, 4, 1) X(8, 8, 1) X(8, 16, 1) X(8, 32, 1) X(8, 64, 1) X(8, 64, 2)
#define VFM_FOR_VSTEP_SHAPES1(X) X(1, 4, 1) X(1, 16, 1) X(1, 64, 1) X(1, 64, 2) X(1, 64, 4) X(1, 64, 16)
void vstep_shape(int d, int* w, int* lpe, int* cpl) {
  if ((d & 7) == 0) {
    const int D8 = d >> 3;
    int l = 1;
    while (l < D8 && l < 64) l <<= 1;
    *w = 8; *lpe = l; *cpl = (D8 + l - 1) / l;
  } else {
    const int l = d <= 4 ? 4 : d <= 16 ? 16 : 64;
    const int c = (d + l - 1) / l;
    *w = 1; *lpe = l; *cpl = c <= 2 ? c : c <= 4 ? 4 : 16;
  }
}

size_t vstep_pos_elems(int64_t B, int F) { return ((size_t)B * F + 63) / 64 * 64; }
size_t vstep_prow_elems(int F, int d) { return ((size_t)(VSTEP_BLOCKS + F) * (2 * (size_t)d + 2) + 63) / 64 * 64; }

template <int W, int LPE, int CPL>
void launch_vstep(const StepArgs& a, bool cf, bool hv, bool pri, unsigned nb, hipStream_t st) {
#define VSTEP_GO(CF_, HV_, PR_) hipLaunchKernelGGL((k_vstep<W, LPE, CPL, CF_, HV_, PR_>), dim3(nb), dim3(BLOCK), 0, st, a)
  if (cf) {
    if (hv) { if (pri) VSTEP_GO(true, true, true); else VSTEP_GO(true, true, false); }
    else { if (pri) VSTEP_GO(true, false, true); else VSTEP_GO(true, false, false); }
  } else {
    if (hv) { if (pri) VSTEP_GO(false, true, true); else VSTEP_GO(false, true, false); }
    else { if (pri) VSTEP_GO(false, false, true); else VSTEP_GO(false, false, false); }
  }
#undef VSTEP_GO
}

}  // namespace
}  // namespace vfm

using namespace vfm;

extern "C" {

int64_t vfm_variant_step_workspace_bytes(int64_t B, int32_t F, int32_t d) {
  if (B < 0 || F < 1 || F > VFM_MAX_FIELDS || d < 1 || d > VSTEP_MAX_D || B * (int64_t)F > 0x7FFFFFFFLL) return -1;
  return (int64_t)sizeof(float) * (int64_t)(vstep_pos_elems(B, F) + vstep_prow_elems(F, d) + 64);
}

int vfm_variant_step_f32(const vfm_problem_t* p, int32_t objective, const vfm_index_t* idx, void* workspace, const void* x,
                         const float* values, float* entity_params, float* bias_params, const float* inv_occ,
                         float* scalars, const double* W, float* priors, const float* eps_entity, const float* eps_bias,
                         const float* eps_global, const float* state, const float* grow, const double* partials,
                         const float* grad_out, float* m_entity, float* v_entity, float* m_bias, float* v_bias,
                         float* m_scalars, float* v_scalars, float* m_priors, float* v_priors, float lr, float beta1,
                         float beta2, float eps_adam, int64_t adam_step, void* stream) {
  if (!p) return fail(VFM_E_INVALID, "vfm_variant_step_f32: problem is NULL");
  if (p->struct_size != (uint32_t)sizeof(vfm_problem_t) || p->abi_version != (uint32_t)VFM_ABI_VERSION)
    return fail(VFM_E_INVALID, "vfm_problem_t: struct_size / abi_version differ from this library's (VFM_STRUCT_INIT)");
  if (p->d < 1 || p->d > VSTEP_MAX_D) return fail(VFM_E_INVALID, "vfm_variant_step_f32: d out of range [1,1024]");
  if (p->B < 0 || p->T <= 0 || p->T > 0xFFFFFFFELL || p->F < 1 || p->F > VFM_MAX_FIELDS ||
      (p->id_bits != 32 && p->id_bits != 64) || p->B * (int64_t)p->F > 0x7FFFFFFFLL)
    return fail(VFM_E_INVALID, "vfm_variant_step_f32: bad problem (B, T, F, id_bits)");
  if (objective != VFM_OBJ_SAMPLED && objective != VFM_OBJ_CLOSED_FORM)
    return fail(VFM_E_INVALID, "vfm_variant_step_f32: unknown objective");
  if (p->likelihood != VFM_LIK_NORMAL && p->likelihood != VFM_LIK_BERNOULLI)
    return fail(VFM_E_INVALID, "vfm_variant_step_f32: unknown likelihood");
  if (objective == VFM_OBJ_CLOSED_FORM && p->likelihood != VFM_LIK_NORMAL)
    return fail(VFM_E_UNSUPPORTED, "vfm_variant_step_f32: the closed-form expected log-likelihood is the Normal one");
  if (p->n_samples != 1) return fail(VFM_E_UNSUPPORTED, "vfm_variant_step_f32: one variational sample");
  if (p->flags != 0) return fail(VFM_E_UNSUPPORTED, "vfm_variant_step_f32: no flags (|.| link, single rank, plain moments)");
  if (p->dev_step || p->wrec)
    return fail(VFM_E_UNSUPPORTED, "vfm_variant_step_f32: no device-side step state / packed first-order records");
  if (adam_step < 1) return fail(VFM_E_INVALID, "vfm_variant_step_f32: adam_step < 1");
  if (!(lr >= 0.f) || !(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f) || !(eps_adam >= 0.f))
    return fail(VFM_E_INVALID, "vfm_variant_step_f32: lr, beta1, beta2 or eps_adam out of range");
  if (idx && (idx->struct_size != (uint32_t)sizeof(vfm_index_t) || idx->abi_version != (uint32_t)VFM_ABI_VERSION))
    return fail(VFM_E_INVALID, "vfm_index_t: struct_size / abi_version differ from this library's (VFM_STRUCT_INIT)");
  if (!idx || !idx->occ_ptr || (p->B > 0 && !idx->occ_rows) || !workspace || !x || !entity_params || !bias_params ||
      !inv_occ || !scalars || !W || !partials || !grad_out || (p->B > 0 && (!state || !grow)) || !m_entity || !v_entity ||
      !m_bias || !v_bias || !m_scalars || !v_scalars)
    return fail(VFM_E_INVALID, "vfm_variant_step_f32: NULL pointer");
  if ((priors != nullptr) != (m_priors != nullptr) || (priors != nullptr) != (v_priors != nullptr))
    return fail(VFM_E_INVALID, "vfm_variant_step_f32: NULL pointer (m_priors / v_priors go with priors)");
  const int neps = (eps_entity != nullptr) + (eps_bias != nullptr) + (eps_global != nullptr);
  if (neps != 0 && neps != 3) return fail(VFM_E_INVALID, "vfm_variant_step_f32: give all three eps tables or none");
  if (((uintptr_t)workspace) & 15) return fail(VFM_E_INVALID, "vfm_variant_step_f32: workspace must be 16-byte aligned");

  StepArgs a;
  memset(&a, 0, sizeof(a));
  a.B = p->B; a.T = p->T; a.F = p->F; a.d = p->d; a.G = p->F; a.lik = p->likelihood;
  a.n_occ = (int32_t)(p->B * (int64_t)p->F);
  a.eps_mode = eps_entity ? EPS_TABLE : EPS_PHILOX;
  a.ll_scale = (float)((double)p->nb_train / (double)(p->B_global > 0 ? p->B_global : 1));
  a.key.seed_lo = (uint32_t)p->seed; a.key.seed_hi = (uint32_t)(p->seed >> 32);
  a.key.step_lo = (uint32_t)p->step; a.key.step_hi = (uint32_t)(p->step >> 32);
  a.xv = values; a.entity = entity_params; a.bias = bias_params; a.inv_occ = inv_occ; a.scalars = scalars; a.W = W;
  a.priors = priors; a.eps_entity = eps_entity; a.eps_bias = eps_bias; a.eps_global = eps_global;
  a.occ_ptr = idx->occ_ptr; a.occ_rows = idx->occ_rows; a.status = idx->status;
  a.state = state; a.grow = grow; a.partials = partials; a.grad_out = grad_out;
  a.m_entity = m_entity; a.v_entity = v_entity; a.m_bias = m_bias; a.v_bias = v_bias;
  int32_t* occ_pos = reinterpret_cast<int32_t*>(workspace);
  a.occ_pos = occ_pos;
  a.prows = reinterpret_cast<float*>(workspace) + vstep_pos_elems(p->B, p->F);
  a.gsmall = a.prows + vstep_prow_elems(p->F, p->d);
  for (int g = 0; g < p->F; ++g) { a.group_hi[g] = p->group_hi[g]; a.group_n[g] = p->group_n[g]; }
  // torch.optim.Adam's step constants, as vfm_adam_f32 forms them
  const double bc1 = 1.0 - pow((double)beta1, (double)adam_step), bc2 = 1.0 - pow((double)beta2, (double)adam_step);
  a.b1 = beta1; a.b2 = beta2; a.eps = eps_adam;
  a.step_size = (float)((double)lr / bc1);
  a.bc2_sqrt = (float)sqrt(bc2);

  hipStream_t st = (hipStream_t)stream;
  if (values) {
    int64_t nbp = (p->T + 255) / 256;
    if (nbp > VSTEP_POS_BLOCKS) nbp = VSTEP_POS_BLOCKS;
    hipLaunchKernelGGL(k_vstep_positions, dim3((unsigned)nbp), dim3(256), 0, st, idx->occ_ptr, idx->occ_rows, x,
                       (int)(p->id_bits == 64), (int)p->F, p->T, occ_pos, p->B, idx->status);
  }
  int w, lpe, cpl;
  vstep_shape(p->d, &w, &lpe, &cpl);
  const int GPB = BLOCK / lpe;
  int64_t nb = (p->T + GPB - 1) / GPB;
  if (nb > VSTEP_BLOCKS) nb = VSTEP_BLOCKS;
  const bool cf = objective == VFM_OBJ_CLOSED_FORM, hv = values != nullptr, pri = priors != nullptr;
#define X(W_, L_, C_) if (w == W_ && lpe == L_ && cpl == C_) launch_vstep<W_, L_, C_>(a, cf, hv, pri, (unsigned)nb, st);
  VFM_FOR_VSTEP_SHAPES8(X)
  VFM_FOR_VSTEP_SHAPES1(X)
#undef X
  int64_t epb = (p->T + nb - 1) / nb;
  epb = (epb + GPB - 1) / GPB * GPB;
  const unsigned ky = pri ? (unsigned)((2 * p->d + 2 + VSTEP_KT - 1) / VSTEP_KT) : 1u;
  hipLaunchKernelGGL(k_vstep_small, dim3(pri ? (unsigned)p->F + 1u : 1u, ky), dim3(BLOCK), 0, st, a, scalars, priors,
                     m_scalars, v_scalars, m_priors, v_priors, epb, (int)nb);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail_hip(e, "vfm_variant_step_f32");
}

}  // extern "C"

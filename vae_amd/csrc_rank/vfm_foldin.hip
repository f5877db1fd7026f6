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

#include "vfm_args.hpp"
#include "vfm_foldin.h"

namespace vfm {
namespace {
#include "vfm_rng.hpp"
#include "vfm_common.hpp"

constexpr int FB = 256;                  // threads per block
constexpr int LDS_BYTES = 48 * 1024;     // row stage per block (three blocks per CU)
constexpr float LOG_2PI_HALF = 0.918938533204672742f;

struct FoldArgs {
  int64_t E, R, T;
  int32_t F, d, col, lik, S, n_steps, reset, mode, cap;
  float lr, klw;
  int64_t t0;
  RngKey key;
  const int64_t *ent, *ptr, *x, *row_op;
  const float* y;
  const float* ops;                      // [n_ops, 3, DP]  M | A | C
  const float* opc;                      // [n_ops, 2]      c_mean, c_var
  float *entity, *bias;
  const float* scal;
  float *loss, *grad;
};

__device__ __forceinline__ RngKey key_at(const FoldArgs& a, int64_t step) {
  RngKey k = a.key;
  k.step_lo = (uint32_t)step;
  k.step_hi = (uint32_t)((uint64_t)step >> 32);
  return k;
}

// eps of coordinate kc of entity e: normal8b(k, e, kc / 8).n[kc % 8] with only the pair it needs (same bits, same floats)
__device__ __forceinline__ float eps_coord(const RngKey& k, uint32_t e, int kc) {
  uint32_t o[4];
  philox4x32_10((uint32_t)kc >> 3, e, k.step_lo, k.step_hi, k.seed_lo, k.seed_hi, o);
  const int pr = (kc & 7) >> 1;
  const uint32_t f = pr == 0 ? o[0]
                     : pr == 1 ? __builtin_amdgcn_alignbit(o[1], o[0], 26)
                     : pr == 2 ? __builtin_amdgcn_alignbit(o[2], o[1], 20)
                               : __builtin_amdgcn_alignbit(o[3], o[2], 14);
  float n0, n1;
  box_muller_bits<16, 10>(f, n0, n1);
  return (kc & 1) ? n1 : n0;
}

// eps of entity e's first-order weight (normal8b's nb, p = 0); e = 0xFFFFFFFF: the global bias' (normal8b's n[0])
__device__ __forceinline__ float eps_first(const RngKey& k, uint32_t e) {
  uint32_t o[4];
  philox4x32_10(0u, e, k.step_lo, k.step_hi, k.seed_lo, k.seed_hi, o);
  float n0, n1;
  if (e == 0xFFFFFFFFu) box_muller_bits<16, 10>(o[0], n0, n1);
  else box_muller_bits<16, 8>(o[3] >> 8, n0, n1);
  return n0;
}

template <int LINK>
__device__ __forceinline__ float prior_s() { return LINK == LINK_ABS ? 1.0f : 0.541324854612918f; }   // link(s) = 1

__device__ __forceinline__ double softplus_d(double p) { return fmax(p, 0.0) + log1p(exp(-fabs(p))); }

// ---------------------------------------------------------------------------------------------------------------------
// k_foldin_prep: operand o from the frozen fields of op_x[o] (every column but `col`)
// ---------------------------------------------------------------------------------------------------------------------
template <int LINK>
__global__ __launch_bounds__(FB) void k_foldin_prep(int64_t n_ops, int F, int d, int DP, int col, int64_t T,
                                                    const int64_t* __restrict__ opx, const float* __restrict__ ent,
                                                    const float* __restrict__ bias, const float* __restrict__ scal,
                                                    float* __restrict__ ops, float* __restrict__ opc) {
  const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= n_ops) return;
  const int64_t* xr = opx + o * F;
  bool ok = true;
  for (int f = 0; f < F; ++f) ok = ok && (f == col || (xr[f] >= 0 && xr[f] < T));
  float* out = ops + o * 3 * (int64_t)DP;
  if (!ok) {
    for (int k = 0; k < 3 * DP; ++k) out[k] = __builtin_nanf("");
    opc[o * 2] = opc[o * 2 + 1] = __builtin_nanf("");
    return;
  }
  const double sg0 = link_f<LINK>(scal[2]);
  double cm = scal[1], cv = sg0 * sg0;
  for (int f = 0; f < F; ++f) {
    if (f == col) continue;
    const double sw = link_f<LINK>(bias[xr[f] * 2 + 1]);
    cm += bias[xr[f] * 2];
    cv += sw * sw;
  }
  for (int k = 0; k < DP; ++k) {
    if (k >= d) { out[k] = out[DP + k] = out[2 * DP + k] = 0.f; continue; }
    double sm = 0., smm = 0., ss = 0., sss = 0.;
    for (int f = 0; f < F; ++f) {
      if (f == col) continue;
      const float* row = ent + xr[f] * 2 * (int64_t)d;
      const double m = row[k], s = link_f<LINK>(row[d + k]), s2 = s * s;
      sm += m; smm += m * m; ss += s2; sss += s2 * s2;
    }
    double lin = 0., cov = 0.;
    for (int f = 0; f < F; ++f) {
      if (f == col) continue;
      const float* row = ent + xr[f] * 2 * (int64_t)d;
      const double m = row[k], s = link_f<LINK>(row[d + k]), oth = sm - m;
      lin += s * s * oth * oth;
      cov += s * s * oth;
    }
    cm += 0.5 * (sm * sm - smm);
    cv += 0.5 * (ss * ss - sss) + lin;
    out[k] = (float)sm;
    out[DP + k] = (float)ss;
    out[2 * DP + k] = (float)(2.0 * cov);
  }
  opc[o * 2] = (float)cm;
  opc[o * 2 + 1] = (float)cv;
}

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
    for (int64_t i = 0; i < n; ++i) {
      const int64_t o = a.row_op[r0 + i];
      const float* op = a.ops + o * 3 * DP;
#pragma unroll
      for (int j = 0; j < CPL; ++j) {
        const float M = op[j * W + l], A = op[DP + j * W + l], C = op[2 * DP + j * W + l];
        SA[j] += A;
        SB[j] += fmaf(M, M, A);
        SC[j] += C;
        if (i < a.cap) Ms[i * DP + j * W + l] = M;
      }
      Scv += a.opc[o * 2 + 1];
      if (i < a.cap && l == 0) Cy[i] = a.opc[o * 2] - a.y[r0 + i];
    }
    __syncthreads();                     // (the stage is read across lanes of the group below; the only barrier)
  }

  // ---- Adam state
  float am[CPL], av[CPL], bm[CPL], bv[CPL];
#pragma unroll
  for (int j = 0; j < CPL; ++j) am[j] = av[j] = bm[j] = bv[j] = 0.f;
  float amw = 0.f, avw = 0.f, bmw = 0.f, bvw = 0.f;

  for (int it = 0; it <= a.n_steps; ++it) {
    const bool last = it == a.n_steps;
    float sg[CPL], gm[CPL], gs[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) { sg[j] = link_f<LINK>(sp[j]); gm[j] = gs[j] = 0.f; }
    const float sgw = link_f<LINK>(spw);
    float gmw = 0.f, gsw = 0.f;
    double lsum = 0.0;                    // sum of the rows' expected nll (last pass only)

    if constexpr (!SAMPLED) {
      // E pred_r - y_r = (c_mean,r - y_r) + mu_w + mu . M_r; four rows' reductions in flight at a time
      float racc = 0.f, rsq = 0.f;
      for (int64_t i = 0; i < n; i += 4) {
        float Mv[4][CPL], cy[4], dot[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int64_t ii = i + u;
          const bool rv = ii < n;
          if (rv && ii < a.cap) {
#pragma unroll
            for (int j = 0; j < CPL; ++j) Mv[u][j] = Ms[ii * DP + j * W + l];
            cy[u] = Cy[ii];
          } else if (rv) {
            const int64_t o = a.row_op[r0 + ii];
#pragma unroll
            for (int j = 0; j < CPL; ++j) Mv[u][j] = a.ops[o * 3 * DP + j * W + l];
            cy[u] = a.opc[o * 2] - a.y[r0 + ii];
          } else {
#pragma unroll
            for (int j = 0; j < CPL; ++j) Mv[u][j] = 0.f;
            cy[u] = 0.f;
          }
          float p = 0.f;
#pragma unroll
          for (int j = 0; j < CPL; ++j) p = fmaf(mu[j], Mv[u][j], p);
          dot[u] = p;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) dot[u] = group_sum<W>(dot[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float res = i + u < n ? (cy[u] + muw) + dot[u] : 0.f;
#pragma unroll
          for (int j = 0; j < CPL; ++j) gm[j] = fmaf(res, Mv[u][j], gm[j]);
          racc += res;
          rsq = fmaf(res, res, rsq);
        }
      }
      // d/dmu: prec (sum_r res_r M_r + mu SA + SC / 2); d/dsigma: prec sigma SB; (w) prec sum_r res_r, prec n sigma_w
#pragma unroll
      for (int j = 0; j < CPL; ++j) {
        gm[j] = prec * (gm[j] + fmaf(mu[j], SA[j], 0.5f * SC[j]));
        gs[j] = prec * sg[j] * SB[j];
      }
      gmw = prec * racc;
      gsw = prec * (float)n * sgw;
      if (last) {
        float vq = 0.f;                   // sum_k (mu^2 SA + sigma^2 SB + mu SC)
#pragma unroll
        for (int j = 0; j < CPL; ++j) vq += fmaf(mu[j] * mu[j], SA[j], fmaf(sg[j] * sg[j], SB[j], mu[j] * SC[j]));
        vq = group_sum<W>(vq);
        const double sumv = (double)Scv + (double)n * sgw * sgw + vq;
        lsum = 0.5 * prec * ((double)rsq + sumv) +
               (double)n * ((double)LOG_2PI_HALF - 0.5 * log((double)prec));
      }
    } else {
      const int64_t tkey = a.t0 + it;
      const float invS = 1.0f / (float)a.S;
      int nq = 0;
      for (int f = 0; f < a.F; ++f) nq += f != a.col;
      for (int s = 0; s < a.S; ++s) {
        const RngKey key = key_at(a, tkey * a.S + s);
        const float w0 = fmaf(sg0, eps_first(key, 0xFFFFFFFFu), m0);
        float ee[CPL], z[CPL], acc[CPL];
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
          ee[j] = vk[j] ? eps_coord(key, (uint32_t)e, j * W + l) : 0.f;
          z[j] = fmaf(sg[j], ee[j], mu[j]);
          acc[j] = 0.f;
        }
        const float ew = eps_first(key, (uint32_t)e);
        const float we = fmaf(sgw, ew, muw);
        float gsum = 0.f;
        for (int64_t i = 0; i < n; ++i) {
          const int64_t r = r0 + i;
          float Sq[CPL], Qq[CPL];
#pragma unroll
          for (int j = 0; j < CPL; ++j) Sq[j] = Qq[j] = 0.f;
          float wsum = 0.f;
          bool bad = false;
          for (int f = 0; f < a.F; ++f) {
            if (f == a.col) continue;
            int64_t q = a.x[r * a.F + f];
            if (q < 0 || q >= a.T) { bad = true; q = 0; }
            const float* row = a.entity + q * 2 * d;
#pragma unroll
            for (int j = 0; j < CPL; ++j) {
              if (!vk[j]) continue;
              const int kc = j * W + l;
              const float zq = fmaf(link_f<LINK>(row[d + kc]), eps_coord(key, (uint32_t)q, kc), row[kc]);
              Sq[j] += zq;
              Qq[j] = fmaf(zq, zq, Qq[j]);
            }
            wsum += fmaf(link_f<LINK>(a.bias[q * 2 + 1]), eps_first(key, (uint32_t)q), a.bias[q * 2]);
          }
          float part = 0.f;
#pragma unroll
          for (int j = 0; j < CPL; ++j) {
            part = fmaf(z[j], Sq[j], part);
            if (nq >= 2) part += 0.5f * fmaf(Sq[j], Sq[j], -Qq[j]);
          }
          float pred = ((w0 + we) + wsum) + group_sum<W>(part);
          if (bad) pred = __builtin_nanf("");
          const float yr = a.y[r];
          float gp;
          if (a.lik == VFM_LIK_NORMAL) {
            gp = prec * (pred - yr);
            if (last) {
              const double df = (double)yr - (double)pred;
              lsum += 0.5 * prec * df * df + ((double)LOG_2PI_HALF - 0.5 * log((double)prec));
            }
          } else {
            gp = 1.0f / (1.0f + __expf(-pred)) - yr;
            if (last) lsum += softplus_d(pred) - (double)yr * (double)pred;
          }
#pragma unroll
          for (int j = 0; j < CPL; ++j) acc[j] = fmaf(gp, Sq[j], acc[j]);
          gsum += gp;
        }
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
          gm[j] = fmaf(acc[j], invS, gm[j]);
          gs[j] = fmaf(acc[j] * ee[j], invS, gs[j]);
        }
        gmw = fmaf(gsum, invS, gmw);
        gsw = fmaf(gsum * ew, invS, gsw);
      }
      lsum /= (double)a.S;
    }

    // ---- KL to N(0, 1): d/dmu = mu, d/dsigma = sigma - 1/sigma; chain sigma = link(s)
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      gm[j] = fmaf(a.klw, mu[j], gm[j]);
      gs[j] = fmaf(a.klw, sg[j] - inv_sigma(sg[j]), gs[j]) * dlink_f<LINK>(sp[j]);
    }
    gmw = fmaf(a.klw, muw, gmw);
    gsw = fmaf(a.klw, sgw - inv_sigma(sgw), gsw) * dlink_f<LINK>(spw);

    if (last) {
      float kl = 0.f;
#pragma unroll
      for (int j = 0; j < CPL; ++j)
        if (vk[j]) kl += kl_std_normal(mu[j], sg[j]);
      kl = group_sum<W>(kl) + kl_std_normal(muw, sgw);
      if (live && l == 0) a.loss[g] = eok ? (float)(lsum + (double)a.klw * (double)kl) : __builtin_nanf("");
      if (live && a.mode == VFM_FOLDIN_OBJECTIVE && a.grad) {
        float* go = a.grad + g * (2 * (int64_t)d + 2);
#pragma unroll
        for (int j = 0; j < CPL; ++j)
          if (vk[j]) { go[j * W + l] = gm[j]; go[d + j * W + l] = gs[j]; }
        if (l == 0) { go[2 * d] = gmw; go[2 * d + 1] = gsw; }
      }
      break;
    }

    // ---- Adam (torch.optim.Adam, single-tensor: lerp / mul + addcmul / sqrt / div / add eps / addcdiv)
    const int t = it + 1;
    const double bc1 = 1.0 - pow(0.9, (double)t), bc2 = 1.0 - pow(0.999, (double)t);
    const float step_size = (float)((double)a.lr / bc1), bc2s = (float)sqrt(bc2);
    auto upd = [&](float& p, float& m, float& v, float gr) {
      m = m + (gr - m) * 0.1f;
      v = v * 0.999f + (0.001f * gr) * gr;
      const float den = __fsqrt_rn(v) / bc2s + 1e-8f;
      p = p + (-step_size * m) / den;
    };
#pragma unroll
    for (int j = 0; j < CPL; ++j)
      if (vk[j]) { upd(mu[j], am[j], av[j], gm[j]); upd(sp[j], bm[j], bv[j], gs[j]); }
    upd(muw, amw, avw, gmw);
    upd(spw, bmw, bvw, gsw);
  }

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
struct FShape {
  int W, CPL;
};

FShape shape_of(int d) {
  const int W = d <= 8 ? 8 : d <= 16 ? 16 : d <= 32 ? 32 : 64;
  const int c = (d + W - 1) / W;
  return {W, c <= 1 ? 1 : c <= 2 ? 2 : c <= 4 ? 4 : 8};
}

int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

int64_t ops_off_opc(int64_t n_ops, int d) {
  const FShape s = shape_of(d);
  return round_up(n_ops * 3 * (int64_t)(s.W * s.CPL) * 4, 256);
}

template <int W, int CPL, int LINK, bool SAMPLED>
void launch(const FoldArgs& a, hipStream_t st) {
  constexpr int GPB = FB / W;
  const size_t shm = SAMPLED ? 0 : (size_t)GPB * a.cap * (W * CPL + 1) * 4;
  hipLaunchKernelGGL((k_foldin<W, CPL, LINK, SAMPLED>), dim3((unsigned)((a.E + GPB - 1) / GPB)), dim3(FB), shm, st, a);
}

template <int LINK, bool SAMPLED>
void launch_shape(const FShape& s, const FoldArgs& a, hipStream_t st) {
  switch (s.W * 16 + s.CPL) {
    case 8 * 16 + 1: launch<8, 1, LINK, SAMPLED>(a, st); break;
    case 16 * 16 + 1: launch<16, 1, LINK, SAMPLED>(a, st); break;
    case 32 * 16 + 1: launch<32, 1, LINK, SAMPLED>(a, st); break;
    case 64 * 16 + 1: launch<64, 1, LINK, SAMPLED>(a, st); break;
    case 64 * 16 + 2: launch<64, 2, LINK, SAMPLED>(a, st); break;
    case 64 * 16 + 4: launch<64, 4, LINK, SAMPLED>(a, st); break;
    default: launch<64, 8, LINK, SAMPLED>(a, st); break;
  }
}

int launch_status(const char* where) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail_hip(e, where);
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
  const int DP = s.W * s.CPL;
  vfm::FoldArgs a;
  a.E = p->E; a.R = p->R; a.T = p->T;
  a.F = p->F; a.d = p->d; a.col = p->col; a.lik = p->likelihood; a.S = cf ? 1 : p->n_samples;
  a.n_steps = p->n_steps; a.reset = p->reset ? 1 : 0; a.mode = p->mode;
  a.lr = p->lr; a.klw = p->kl_weight; a.t0 = p->t0;
  a.key.seed_lo = (uint32_t)p->seed; a.key.seed_hi = (uint32_t)(p->seed >> 32);
  a.key.step_lo = a.key.step_hi = 0; a.key.chunk_off = 0;
  a.ent = p->entities; a.ptr = p->row_ptr; a.x = p->x; a.row_op = p->row_op; a.y = p->y;
  a.entity = p->entity_params; a.bias = p->bias_params; a.scal = p->scalars;
  a.loss = p->out_loss; a.grad = p->out_grad;
  a.ops = nullptr; a.opc = nullptr; a.cap = 0;
  if (cf) {
    char* w = (char*)p->workspace;
    float* ops = (float*)w;
    float* opc = (float*)(w + vfm::ops_off_opc(n_ops, p->d));
    a.ops = ops; a.opc = opc;
    const int cap = vfm::LDS_BYTES / 4 / (vfm::FB / s.W) / (DP + 1);
    a.cap = p->lds_rows < 0 ? cap : (p->lds_rows < cap ? p->lds_rows : cap);
    if (n_ops > 0) {
      const unsigned nb = (unsigned)((n_ops + vfm::FB - 1) / vfm::FB);
      if (sp)
        hipLaunchKernelGGL(vfm::k_foldin_prep<vfm::LINK_SOFTPLUS>, dim3(nb), dim3(vfm::FB), 0, st, n_ops, p->F, p->d, DP,
                           p->col, p->T, p->op_x, p->entity_params, p->bias_params, p->scalars, ops, opc);
      else
        hipLaunchKernelGGL(vfm::k_foldin_prep<vfm::LINK_ABS>, dim3(nb), dim3(vfm::FB), 0, st, n_ops, p->F, p->d, DP,
                           p->col, p->T, p->op_x, p->entity_params, p->bias_params, p->scalars, ops, opc);
      if (int rc = vfm::launch_status("k_foldin_prep")) return rc;
    }
    if (sp) vfm::launch_shape<vfm::LINK_SOFTPLUS, false>(s, a, st);
    else vfm::launch_shape<vfm::LINK_ABS, false>(s, a, st);
  } else {
    if (sp) vfm::launch_shape<vfm::LINK_SOFTPLUS, true>(s, a, st);
    else vfm::launch_shape<vfm::LINK_ABS, true>(s, a, st);
  }
  return vfm::launch_status("k_foldin");
}

}  // extern "C"

// vfm_foldin_body.hpp -- the per-entity body of the fold-in, shared by k_foldin (vfm_foldin.hip), the exact fold-in
// (vfm_foldin_solve.hip) and the elicitation sessions (vfm_elicit.hip, vfm_elicit_field.hip): the operand prep, the row
// sums and LDS stage of the closed form, the Adam loop, and the host side every such unit needs (the lane-group shape
// and its dispatch, the FoldArgs fill, the prep launch, the LDS budget).
// Included inside `namespace vfm { namespace {` of a unit, after vfm_rng.hpp and vfm_common.hpp.  The host side uses
// std::integral_constant and launch_status: the unit includes <type_traits> and vfm_launch.hpp at file scope first
// (an #include here would land inside the namespace).
//
// The body is parameterised over where the entity's rows come from (a Rows object: op(i), y(i), partner(i, f) of row i
// in fold order).  The row sums are sequential in row order, so fold_stage_rows over [0, n) and over [0, m) then [m, n)
// form the same chains.  Rounding: the gradient and Adam expressions are DEFINED under fp contraction `on` (a * b + c
// fuses inside one source expression only); the pragma at the top of each body pins that whichever flag the including
// unit is compiled with -- the mode is fixed by the front end, inlining does not change it.
#pragma once

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

// the rows of k_foldin: entity g's slice [r0, r0 + n) of the sorted row list
struct ListRows {
  const FoldArgs& a;
  int64_t r0;
  __device__ __forceinline__ int64_t op(int64_t i) const { return a.row_op[r0 + i]; }
  __device__ __forceinline__ float y(int64_t i) const { return a.y[r0 + i]; }
  __device__ __forceinline__ int64_t partner(int64_t i, int f) const { return a.x[(r0 + i) * a.F + f]; }
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
#pragma clang fp contract(on)
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
// closed form: rows [i0, i1) of the entity added to the row-independent sums; rows below a.cap staged in LDS
// (Ms [cap, DP]: M_r; Cy [cap]: c_mean,r - y_r).  The caller puts a barrier between this and fold_run.
// ---------------------------------------------------------------------------------------------------------------------
template <int W, int CPL, class Rows>
__device__ __forceinline__ void fold_stage_rows(const FoldArgs& a, const Rows& rows, int64_t i0, int64_t i1, int l,
                                                float* Ms, float* Cy, float (&SA)[CPL], float (&SB)[CPL],
                                                float (&SC)[CPL], float& Scv) {
#pragma clang fp contract(on)
  constexpr int DP = W * CPL;
  for (int64_t i = i0; i < i1; ++i) {
    const int64_t o = rows.op(i);
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
    if (i < a.cap && l == 0) Cy[i] = a.opc[o * 2] - rows.y(i);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// fold_run: a.n_steps Adam updates of theta_e (registers, fresh moments) over the entity's n rows, then one more pass
// at the final parameters whose loss and gradient go to fin(loss, gm, gs, gmw, gsw).  Lane l of the group owns
// coordinates j W + l.  t0: the draw key of the first iteration (sampled objective).
// ---------------------------------------------------------------------------------------------------------------------
template <int W, int CPL, int LINK, bool SAMPLED, class Rows, class Fin>
__device__ __forceinline__ void fold_run(const FoldArgs& a, const Rows& rows, int64_t n, int64_t e, int64_t t0, int l,
                                         const float* Ms, const float* Cy, float prec, float m0, float sg0,
                                         float (&mu)[CPL], float (&sp)[CPL], const bool (&vk)[CPL], float& muw,
                                         float& spw, const float (&SA)[CPL], const float (&SB)[CPL],
                                         const float (&SC)[CPL], float Scv, Fin&& fin) {
#pragma clang fp contract(on)
  constexpr int DP = W * CPL;
  const int d = a.d;
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
            const int64_t o = rows.op(ii);
#pragma unroll
            for (int j = 0; j < CPL; ++j) Mv[u][j] = a.ops[o * 3 * DP + j * W + l];
            cy[u] = a.opc[o * 2] - rows.y(ii);
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
      const int64_t tkey = t0 + it;
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
          float Sq[CPL], Qq[CPL];
#pragma unroll
          for (int j = 0; j < CPL; ++j) Sq[j] = Qq[j] = 0.f;
          float wsum = 0.f;
          bool bad = false;
          for (int f = 0; f < a.F; ++f) {
            if (f == a.col) continue;
            int64_t q = rows.partner(i, f);
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
          const float yr = rows.y(i);
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
      fin((float)(lsum + (double)a.klw * (double)kl), gm, gs, gmw, gsw);
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
}

// ---------------------------------------------------------------------------------------------------------------------
// host side: the lane-group shape for an embedding size and its dispatch, the operand block of a workspace, the
// FoldArgs fill, the prep launch, the LDS budget
// ---------------------------------------------------------------------------------------------------------------------
struct FShape {
  int W, CPL;
};

inline FShape shape_of(int d) {
  const int W = d <= 8 ? 8 : d <= 16 ? 16 : d <= 32 ? 32 : 64;
  const int c = (d + W - 1) / W;
  return {W, c <= 1 ? 1 : c <= 2 ? 2 : c <= 4 ? 4 : 8};
}

template <int N>
using IntC = std::integral_constant<int, N>;

// fn(IntC<W>, IntC<CPL>) for the shape s: the one place that lists the shapes kernels are instantiated for
template <class Fn>
void for_shape(const FShape& s, Fn&& fn) {
  switch (s.W * 16 + s.CPL) {
    case 8 * 16 + 1: fn(IntC<8>{}, IntC<1>{}); break;
    case 16 * 16 + 1: fn(IntC<16>{}, IntC<1>{}); break;
    case 32 * 16 + 1: fn(IntC<32>{}, IntC<1>{}); break;
    case 64 * 16 + 1: fn(IntC<64>{}, IntC<1>{}); break;
    case 64 * 16 + 2: fn(IntC<64>{}, IntC<2>{}); break;
    case 64 * 16 + 4: fn(IntC<64>{}, IntC<4>{}); break;
    default: fn(IntC<64>{}, IntC<8>{}); break;
  }
}

// fn(IntC<LINK>) for the link function of the flags
template <class Fn>
void for_link(bool softplus, Fn&& fn) {
  if (softplus) fn(IntC<LINK_SOFTPLUS>{});
  else fn(IntC<LINK_ABS>{});
}

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

inline int64_t ops_off_opc(int64_t n_ops, int d) {
  const FShape s = shape_of(d);
  return round_up(n_ops * 3 * (int64_t)(s.W * s.CPL) * 4, 256);
}

// The options and tables every entry point passes; the rest is zero / NULL (R and the row list, the operands, cap, the
// outputs) for the caller to set.
inline FoldArgs fill_fold_args(int64_t E, int64_t T, int F, int d, int col, int lik, int S, int n_steps, int reset,
                               int mode, float lr, float klw, int64_t t0, uint64_t seed, float* entity, float* bias,
                               const float* scal) {
  FoldArgs a = {};
  a.E = E; a.T = T;
  a.F = F; a.d = d; a.col = col; a.lik = lik; a.S = S;
  a.n_steps = n_steps; a.reset = reset; a.mode = mode;
  a.lr = lr; a.klw = klw; a.t0 = t0;
  a.key.seed_lo = (uint32_t)seed; a.key.seed_hi = (uint32_t)(seed >> 32);
  a.entity = entity; a.bias = bias; a.scal = scal;
  return a;
}

// k_foldin_prep over the n_ops rows of op_x into a's operand tables (nothing to launch for n_ops = 0)
inline int launch_foldin_prep(bool sp, const FoldArgs& a, int64_t n_ops, const int64_t* op_x, float* ops, float* opc,
                              hipStream_t st) {
  if (n_ops <= 0) return 0;
  const FShape s = shape_of(a.d);
  for_link(sp, [&](auto link) {
    hipLaunchKernelGGL(k_foldin_prep<decltype(link)::value>, dim3((unsigned)((n_ops + FB - 1) / FB)), dim3(FB), 0, st,
                       n_ops, a.F, a.d, s.W * s.CPL, a.col, a.T, op_x, a.entity, a.bias, a.scal, ops, opc);
  });
  return launch_status("k_foldin_prep");
}

// rows per entity staged in LDS: what a block's LDS_BYTES leave each group after theta_floats of its own, capped by the
// caller's lds_rows (-1: no cap)
inline int lds_cap(const FShape& s, int theta_floats, int lds_rows) {
  const int c = (LDS_BYTES / 4 / (FB / s.W) - theta_floats) / (s.W * s.CPL + 1);
  const int cap = c < 0 ? 0 : c;
  return lds_rows < 0 || lds_rows > cap ? cap : lds_rows;
}

// vfm_foldin_bound_body.hpp -- the per-entity body of the bound fold-in (include/vfm_bound.h), shared by k_foldin_bound
// (vfm_foldin_bound.hip) and the bound elicitation session (k_elicit_bound of vfm_elicit_bound.hip): the fp64 c_var
// pass, the start from fp32 parameters, the n_iters rounds of the Jaakkola-Jordan bound's two block minimisers (phases
// X, A, B, C of vfm_foldin_bound.hip's head comment), the rounding (put_params) and B_e at the rounded parameters
// (bound_loss).  Included inside `namespace vfm { namespace {` of a unit, after vfm_foldin_solve_body.hpp.
//
// Like solve_body the body is parameterised over where the entity's rows come from (a Rows object: op(i), y(i) of row i
// in fold order) and takes the base of the entity's row weights as an argument.  Every sum is fp64 in a fixed order
// that depends on the entity's rows and d alone, under fp contraction `on` (pinned by the pragma of each body), so the
// bits are the same wherever the body is instantiated and wherever the triangle lives.
#pragma once

// LDS of a block in doubles: the exact fold-in's and sigma_w^2, sigma_k^2 [d] behind the triangle
__host__ __device__ inline int64_t bound_lds_doubles(int d, int cap_dim) { return lds_doubles(d, cap_dim) + d + 1; }

// c_var of operand o in fp64: k_foldin_prep's sum, not rounded to fp32, the links of the fp32 table values in fp64
template <int LINK>
__global__ __launch_bounds__(FB) void k_foldin_bound_prep(int64_t n_ops, int F, int d, int col, int64_t T,
                                                          const int64_t* __restrict__ opx, const float* __restrict__ ent,
                                                          const float* __restrict__ bias, const float* __restrict__ scal,
                                                          double* __restrict__ cvo) {
#pragma clang fp contract(on)
  const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= n_ops) return;
  const int64_t* xr = opx + o * F;
  bool ok = true;
  for (int f = 0; f < F; ++f) ok = ok && (f == col || (xr[f] >= 0 && xr[f] < T));
  if (!ok) {
    cvo[o] = __builtin_nan("");
    return;
  }
  const double sg0 = link_d<LINK>(scal[2]);
  double cv = sg0 * sg0;
  for (int f = 0; f < F; ++f) {
    if (f == col) continue;
    const double sw = link_d<LINK>(bias[xr[f] * 2 + 1]);
    cv += sw * sw;
  }
  for (int k = 0; k < d; ++k) {
    double sm = 0., ss = 0., sss = 0.;
    for (int f = 0; f < F; ++f) {
      if (f == col) continue;
      const float* row = ent + xr[f] * 2 * (int64_t)d;
      const double m = row[k], sg = link_d<LINK>(row[d + k]), s2 = sg * sg;
      sm += m; ss += s2; sss += s2 * s2;
    }
    double lin = 0.;
    for (int f = 0; f < F; ++f) {
      if (f == col) continue;
      const float* row = ent + xr[f] * 2 * (int64_t)d;
      const double m = row[k], sg = link_d<LINK>(row[d + k]), oth = sm - m;
      lin += sg * sg * oth * oth;
    }
    cv += 0.5 * (ss * ss - sss) + lin;
  }
  cvo[o] = cv;
}

// k_foldin_bound_prep over the n_ops rows of op_x (n_ops > 0) into cv64
inline int launch_bound_prep(bool sp, const FoldArgs& a, int64_t n_ops, const int64_t* op_x, double* cv64, hipStream_t st) {
  const unsigned nb = (unsigned)((n_ops + FB - 1) / FB);
  for_link(sp, [&](auto link) {
    hipLaunchKernelGGL(k_foldin_bound_prep<decltype(link)::value>, dim3(nb), dim3(FB), 0, st, n_ops, a.F, a.d, a.col, a.T,
                       op_x, a.entity, a.bias, a.scal, cv64);
  });
  return launch_status("k_foldin_bound_prep");
}

// what the bound fold-in's workspaces (vfm_foldin_bound.hip, vfm_foldin_bound_split.hip) hold behind the operand block:
// c_var [n_ops], the row weights [R], then the unit's own
inline int64_t off_cv64(int64_t n_ops, int d) { return off_slabs(n_ops, d); }
inline int64_t off_wrow(int64_t n_ops, int d) { return off_cv64(n_ops, d) + round_up(n_ops * 8, 256); }
inline int64_t off_bound_own(int64_t R, int64_t n_ops, int d) { return off_wrow(n_ops, d) + round_up(R * 8, 256); }

// fill_solve_args for the two bound entries, with cv64 and wrow
template <class S, class P>
void fill_bound_args(S& s, const P* p, int mode) {
  fill_solve_args(s, p, VFM_LIK_BERNOULLI, p->n_iters, p->reset != 0, mode);
  char* w = (char*)p->workspace;
  s.cv64 = (double*)(w + off_cv64(p->n_ops, p->d));
  s.wrow = (double*)(w + off_wrow(p->n_ops, p->d));
}

// phase E: B_e at the fp32 parameters pf = [mu_w, mu [d] | s_w, s [d]] (LDS), by wave 0; its 64 / W lane groups all
// hold this entity, lane l of a group owns coordinates j W + l.  PRIOR (include/vfm_bound_prior.h): the KL is to the field's
// prior pr = m [d + 1] | lam [d + 1] (LDS, stage_prior), evaluated as solve_body's phase E evaluates it
template <int W, int CPL, int LINK, bool PRIOR = false, class Rows>
__device__ __forceinline__ void bound_loss(const FoldArgs& a, const Rows& rows, int64_t n, const float* pf, int lane,
                                           float* loss, const double* pr = nullptr) {
#pragma clang fp contract(on)
  constexpr int DP = W * CPL;
  const int d = a.d, d1 = d + 1, l = lane % W;
  float mu[CPL], sg[CPL];
  bool vk[CPL];
#pragma unroll
  for (int j = 0; j < CPL; ++j) {
    const int kc = j * W + l;
    vk[j] = kc < d;
    mu[j] = vk[j] ? pf[1 + kc] : 0.f;
    sg[j] = link_f<LINK>(vk[j] ? pf[d1 + 1 + kc] : prior_s<LINK>());
  }
  const float muw = pf[0], sgw = link_f<LINK>(pf[d1]);
  double lsum = 0.0;
  for (int64_t i = 0; i < n; ++i) {
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
    x2 = x2 < 0.f ? 0.f : x2;            // (a NaN stays a NaN)
    const float xi = sqrtf(x2);
    const float t = -(rows.y(i) - 0.5f) * Ef + 0.5f * xi + log1pf(expf(-xi));
    lsum += (double)t;
  }
  float klq = 0.f;
#pragma unroll
  for (int j = 0; j < CPL; ++j) {
    if constexpr (PRIOR) {
      if (vk[j]) klq += kl_prior_normal(mu[j], sg[j], (float)pr[1 + j * W + l], sqrtf((float)pr[d1 + 1 + j * W + l]));
    } else {
      if (vk[j]) klq += kl_std_normal(mu[j], sg[j]);
    }
  }
  if constexpr (PRIOR) klq = group_sum<W>(klq) + kl_prior_normal(muw, sgw, (float)pr[0], sqrtf((float)pr[d1]));
  else klq = group_sum<W>(klq) + kl_std_normal(muw, sgw);
  if (lane == 0) *loss = (float)(lsum + (double)a.klw * (double)klq);
}

// ---------------------------------------------------------------------------------------------------------------------
// bound_body: a.n_steps rounds of the bound's two block minimisers for one entity over its n rows, by the whole workgroup
// (FB threads, every thread calls it: it holds barriers).  a: the options (n_steps: the rounds) and the fp32 operands of
// the loss pass (a.cap = 0: nothing staged); ops64 [n_ops, 3, d] = M | A | C, cm64 and cv64 [n_ops] = c_mean and c_var,
// unrounded; wrow: this entity's row weights, fold row i at wrow[i] (written and read by this workgroup alone); sm: the
// block's LDS (bound_lds_doubles); Hm: the packed triangle of solve_dim(n, d), in LDS or in the workgroup's slab; sg2:
// the d + 1 doubles of scales behind the LDS triangle.
// The start: xi^(0) is taken at the fp32 parameters pf = (float*)(sm + 7 (d + 1)) = [mu_w, mu [d] | s_w, s [d]], which
// the caller has written and published by a barrier, read through the link in fp64; prior_start: at mu = 0, sigma = 1
// instead (pf is not read).  The iterate stays in fp64 for all rounds; put_params rounds it once into pf; after the
// barrier that publishes pf every thread calls store(pf); then wave 0 evaluates B_e at pf into *loss.  The caller puts a
// barrier before pf or any other LDS of the block is written again.
// PRIOR (include/vfm_bound_prior.h): the entity's prior is N(m_c, 1 / lam_c) per coordinate, pr = m [d + 1] | lam [d + 1] in
// LDS (stage_prior): D_c = kl lam_c + sum_r w_r A_r, b_c += kl lam_c m_c, sigma_c^2 = kl / (kl lam_c + sum_r w_r (A_r +
// M_r^2)), prior_start is mu = m, sigma^2 = 1 / lam, and the KL of B_e is to that prior.  At m = 0, lam = 1 every
// expression rounds as with PRIOR off.
// ---------------------------------------------------------------------------------------------------------------------
template <int W, int CPL, int LINK, bool PRIOR = false, class Rows, class Store>
__device__ __forceinline__ void bound_body(const FoldArgs& a, const double* ops64, const double* cm64, const double* cv64,
                                           double* wrow, const Rows& rows, int64_t n, bool prior_start, double* sm,
                                           double* Hm, double* sg2, float* loss, Store&& store,
                                           const double* pr = nullptr) {
#pragma clang fp contract(on)
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int d = a.d, d1 = d + 1;
  double* Dd = sm;                       // D                                  [d + 1]  (0: the first-order weight)
  double* Di = Dd + d1;                  // 1 / D
  double* bv = Di + d1;                  // primal: b; dual: D^-1 b
  double* yv = bv + d1;                  // the right-hand side, then L^-1 of it; between two rounds: theta
  double* dv = yv + d1;                  // 1 / L_jj
  double* xv = dv + d1;                  // the solution of the system
  double* SBd = xv + d1;                 // sum_r w_r, sum_r w_r (A_rk + M_rk^2)
  float* pf = (float*)(SBd + d1);        // the fp32 parameters: mu_w, mu [d] | s_w, s [d]
  double* th = yv;
  const double kl = a.klw;
  const int64_t os = 3 * (int64_t)d;     // stride of an fp64 operand
  const bool dual = n <= d;
  const int m = solve_dim(n, d);

  // ---- the start: xi^(0) is taken at the fp32 parameters, or at the prior
  for (int c = tid; c < d1; c += FB) {
    double t0 = 0., v0 = 1.;
    if constexpr (PRIOR) {
      t0 = pr[c];
      v0 = 1.0 / pr[d1 + c];
    }
    if (!prior_start) {
      const double sg = link_d<LINK>(pf[d1 + c]);
      t0 = pf[c];
      v0 = sg * sg;
    }
    th[c] = t0;
    sg2[c] = v0;
  }
  __syncthreads();

  for (int it = 0; it < a.n_steps; ++it) {
    // ---- X: the rows' weights at the current iterate
    for (int64_t i = wv; i < n; i += FB / 64) {
      const int64_t o = rows.op(i);
      const double* op = ops64 + o * os;
      double pe = 0., pv = 0.;
      for (int k = lane; k < d; k += 64) {
        const double M = op[k], A = op[d + k], C = op[2 * d + k], mu = th[k + 1];
        pe += mu * M;
        pv += mu * mu * A + sg2[k + 1] * (A + M * M) + mu * C;
      }
      pe = wave_sum_d(pe);
      pv = wave_sum_d(pv);
      const double Ef = cm64[o] + th[0] + pe;
      const double Vf = cv64[o] + sg2[0] + pv;
      double x2 = Ef * Ef + Vf;
      x2 = x2 < 0. ? 0. : x2;            // (a NaN stays a NaN)
      const double xi = sqrt(x2);
      const double w = xi < 1e-3 ? 0.25 - x2 / 48.0 : tanh(0.5 * xi) / (2.0 * xi);
      if (lane == 0) wrow[i] = w;
    }
    __syncthreads();

    // ---- A: the weighted row sums of each coordinate
    for (int c = tid; c < d1; c += FB) {
      double SA = 0., SB = 0., SC = 0., bM = 0.;
      if (c == 0) {
        for (int64_t i = 0; i < n; ++i) {
          const double w = wrow[i];
          SB += w;
          bM += ((double)rows.y(i) - 0.5) - w * cm64[rows.op(i)];
        }
      } else {
        for (int64_t i = 0; i < n; ++i) {
          const int64_t o = rows.op(i);
          const double* op = ops64 + o * os + (c - 1);
          const double M = op[0], A = op[d], C = op[2 * d], w = wrow[i];
          const double t = ((double)rows.y(i) - 0.5) - w * cm64[o];
          SA += w * A;
          SB += w * (A + M * M);
          SC += w * C;
          bM += t * M;
        }
      }
      double D, b;
      if constexpr (PRIOR) {
        const double kll = kl * pr[d1 + c], b0 = bM - 0.5 * SC;
        D = kll + SA;
        b = b0 + kll * pr[c];
      } else {
        D = kl + SA;
        b = bM - 0.5 * SC;
      }
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
        const double* Mi = ops64 + rows.op(i) * os;
        const double* Mj = ops64 + rows.op(j) * os;
        double acc = 0.;
        for (int k = lane; k < d; k += 64) acc += Mi[k] * Mj[k] * Di[k + 1];
        acc = wave_sum_d(acc);
        if (lane == 0) Hm[p] = acc + Di[0] + (i == j ? 1.0 / wrow[i] : 0.0);
      }
      for (int i = wv; i < m; i += FB / 64) {
        const double* Mi = ops64 + rows.op(i) * os;
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
          for (int64_t r = 0; r < n; ++r) acc += wrow[r];
        } else if (j == 0) {
          for (int64_t r = 0; r < n; ++r) acc += wrow[r] * ops64[rows.op(r) * os + (i - 1)];
        } else {
          for (int64_t r = 0; r < n; ++r) {
            const double* op = ops64 + rows.op(r) * os;
            acc += wrow[r] * op[i - 1] * op[j - 1];
          }
        }
        Hm[p] = acc + (i == j ? Dd[i] : 0.0);
      }
      for (int c = tid; c < d1; c += FB) yv[c] = bv[c];
    }
    __syncthreads();

    // ---- C: the factorisation and the two substitutions
    chol_solve(Hm, yv, dv, xv, m);

    // ---- the iterate, in fp64: the means and the scales' closed forms
    for (int c = tid; c < d1; c += FB) {
      double t;
      if (dual) {
        double acc = 0.;
        if (c == 0) {
          for (int i = 0; i < m; ++i) acc += xv[i];
        } else {
          for (int i = 0; i < m; ++i) acc += ops64[rows.op(i) * os + (c - 1)] * xv[i];
        }
        t = bv[c] - Di[c] * acc;
      } else {
        t = xv[c];
      }
      th[c] = t;
      if constexpr (PRIOR) {
        const double kll = kl * pr[d1 + c];
        sg2[c] = kl / (kll + SBd[c]);
      } else {
        sg2[c] = kl / (kl + SBd[c]);
      }
    }
    __syncthreads();
  }

  // ---- D: rounded to fp32 once
  for (int c = tid; c < d1; c += FB) {
    if constexpr (PRIOR) put_params<LINK, true>(pf, d1, c, th[c], kl, 1.0, SBd[c], kl * pr[d1 + c]);
    else put_params<LINK>(pf, d1, c, th[c], kl, 1.0, SBd[c]);
  }
  __syncthreads();
  store(pf);

  // ---- E: B_e at the fp32 parameters
  if (wv == 0) bound_loss<W, CPL, LINK, PRIOR>(a, rows, n, pf, lane, loss, pr);
}

// vfm_implicit_body.hpp -- the per-entity body of the implicit-feedback solve (include/vfm_implicit.h), shared by
// k_implicit_solve (vfm_implicit.hip) and the implicit elicitation sessions (vfm_elicit_implicit.hip: ImplicitFold, the
// fold of a round of exact_session): the sums of an entity's observed rows (coord_sums, list_elem: a thread per
// coordinate and a thread per triangle element, rows in order), and implicit_body -- phases A-E of vfm_implicit.hip's
// head comment: H = kl I + prec (w0 base + dw share), chol_solve and put_params of vfm_foldin_solve_body.hpp, and L_e off
// the factor.  Included inside `namespace vfm { namespace {` of a unit, after vfm_foldin_solve_body.hpp.
//
// The tables are read through any struct with the members d, entity, bias and scal (ImpArgs, FoldArgs); the operands of a
// partner j are read from the fp32 tables where they are used (F = 2: M = mu_j, A = link(s_j)^2 in fp64, C = 0,
// c_mean = m_0 + mu_w,j, c_var = link(s_0)^2 + link(s_w,j)^2).  Every sum is fp64 in a fixed order under fp contraction
// `on`, so the bits are the same wherever the body is instantiated and wherever the triangle lives.
#pragma once

// c_mean and c_var of partner j
template <int LINK, class Tab>
__device__ __forceinline__ void partner_consts(const Tab& s, int64_t j, double& cm, double& cv) {
  const double s0 = link_d<LINK>(s.scal[2]), sw = link_d<LINK>(s.bias[j * 2 + 1]);
  cm = (double)s.scal[1] + (double)s.bias[j * 2];
  cv = s0 * s0 + sw * sw;
}

// t and q of an observed row of target y under the one weight w1: what it adds to sum t u and to tt' above the
// unobserved pair the base counted in its place
__device__ __forceinline__ double obs_t(double w0, double w1, double y, double cm) { return w1 * y - (w1 - w0) * cm; }
__device__ __forceinline__ double obs_q(double w0, double w1, double y, double cm, double cv) {
  const double res = y - cm;
  return w1 * res * res - w0 * cm * cm + (w1 - w0) * cv;
}

// coordinate c's sums over n rows in order: SA, SB, bM = sum t u_c and, for c = 0, tt = sum q; false when a row is bad.
// WROW: SA = sum g A, SB = sum g (A + M^2) and, for c = 0, SB = sum g over every row (bad or not, as the row count is).
// Rows: id(r) the partner of row r (-1: outside the base's range), t(r, cm), q(r, cm, cv) and, WROW, g(r)
template <int LINK, bool WROW = false, class Tab, class Rows>
__device__ __forceinline__ bool coord_sums(const Tab& s, const Rows& rows, int64_t n, int c, double& SA, double& SB,
                                           double& bM, double& tt) {
#pragma clang fp contract(on)
  const int d = s.d;
  bool ok = true;
  SA = SB = bM = tt = 0.;
  if (c == 0) {
    for (int64_t r = 0; r < n; ++r) {
      if constexpr (WROW) SB += rows.g(r);
      const int64_t j = rows.id(r);
      if (j < 0) { ok = false; continue; }
      double cm, cv;
      partner_consts<LINK>(s, j, cm, cv);
      bM += rows.t(r, cm);
      tt += rows.q(r, cm, cv);
    }
    if constexpr (!WROW) SB = (double)n;
  } else {
    for (int64_t r = 0; r < n; ++r) {
      const int64_t j = rows.id(r);
      if (j < 0) { ok = false; continue; }
      const float* row = s.entity + j * 2 * (int64_t)d;
      const double M = row[c - 1], sg = link_d<LINK>(row[d + c - 1]), A = sg * sg;
      const double cm = (double)s.scal[1] + (double)s.bias[j * 2];
      if constexpr (WROW) {
        const double g = rows.g(r);
        SA += g * A;
        SB += g * (A + M * M);
      } else {
        SA += A;
        SB += A + M * M;
      }
      bM += rows.t(r, cm) * M;
    }
  }
  return ok;
}

// element (i, j), j <= i, of the triangle of sum u u^T (WROW: sum g u u^T) over n rows in order; NaN when a row is bad
// (row 0 of the triangle, a count, stays)
template <bool WROW, class Tab, class Rows>
__device__ __forceinline__ double list_elem(const Tab& s, const Rows& rows, int64_t n, int i, int j) {
#pragma clang fp contract(on)
  const int d = s.d;
  double acc = 0.;
  if (i == 0) {
    if constexpr (WROW) {
      for (int64_t r = 0; r < n; ++r) acc += rows.g(r);
    } else {
      acc = (double)n;
    }
  } else {
    bool bad = false;
    for (int64_t r = 0; r < n; ++r) {
      const int64_t k = rows.id(r);
      if (k < 0) { bad = true; continue; }
      const float* M = s.entity + k * 2 * (int64_t)d;
      if constexpr (WROW) {
        const double gM = rows.g(r) * (double)M[i - 1];
        acc += j == 0 ? gM : gM * (double)M[j - 1];
      } else {
        acc += j == 0 ? (double)M[i - 1] : (double)M[i - 1] * (double)M[j - 1];
      }
    }
    if (bad) acc = __builtin_nan("");
  }
  return acc;
}

// the share of an entity whose observed rows are a list, accumulated where it is used: implicit_body's source of the
// row-list form (k_implicit_solve's own source adds the chunk form's slabs in front of the same two calls)
template <int LINK, bool WROW, class Tab, class Rows>
struct ListShare {
  const Tab& s;
  const Rows& rows;
  int64_t n;
  __device__ __forceinline__ void coord(int c, double& SA, double& SB, double& bM, double& tt) const {
    if (!coord_sums<LINK, WROW>(s, rows, n, c, SA, SB, bM, tt)) {
      SA = bM = tt = __builtin_nan("");
      if (c > 0) SB = __builtin_nan("");
    }
  }
  __device__ __forceinline__ double elem(int64_t, int i, int j) const { return list_elem<WROW>(s, rows, n, i, j); }
};

// ---------------------------------------------------------------------------------------------------------------------
// implicit_body: the optimum of one entity over every pair, by the whole workgroup (FB threads, every thread calls it:
// it holds barriers).  sh: the entity's share of the observed rows -- coord(c, SA, SB, bM, tt) the sums of coordinate c
// (NaN where a row is bad; SB[0], a count, stays) and elem(p, i, j) element p = (i, j) of the triangle; B: the partner
// field's base block; sm: the block's LDS behind the prior (solve_body's layout: lds_doubles); Hm: the packed triangle of
// d + 1, in LDS or in the workgroup's slab.  solve_body's contract: the fp32 parameters land in pf = (float*)(sm + 7 (d + 1))
// = [mu_w, mu [d] | s_w, s [d]]; after the barrier that publishes them every thread calls store(pf); then L_e at them goes
// to *loss by thread 0.  No barrier at the end: the caller puts one before pf or any other LDS of the block is written
// again -- the body's own 8 bytes of static LDS (tts, the entity's tt', one slot per kernel whatever the number of call
// sites) included: thread 0 reads it in its loss sum, so a second call in the same kernel needs that barrier too.
// WROW: the share is weighted already (w0 base + share in place of w0 base + dw share).  PRIOR
// (include/vfm_implicit_prior.h): pr = m [d + 1] | lam [d + 1] in LDS (stage_prior).
// ---------------------------------------------------------------------------------------------------------------------
template <int LINK, bool PRIOR, bool WROW, class Share, class Store>
__device__ __forceinline__ void implicit_body(const Share& sh, int d, const double* B, double kl, double w0, double dw,
                                              double prec, double* sm, double* Hm, float* loss, Store&& store,
                                              const double* pr = nullptr) {
#pragma clang fp contract(on)
  __shared__ double tts;                 // tt' of the entity
  const int tid = threadIdx.x;
  const int d1 = d + 1;
  double* Dd = sm;                       // solve_body's layout: D | loss terms | b | right-hand side | 1 / L_jj | solution | SB' | fp32
  double* lt = Dd + d1;
  double* bs = lt + d1;
  double* yv = bs + d1;
  double* dv = yv + d1;
  double* xv = dv + d1;
  double* SBd = xv + d1;
  float* pf = (float*)(SBd + d1);
  const int64_t nt = tri(d1);

  // ---- A: the sums of each coordinate, D, b and SB'
  for (int c = tid; c < d1; c += FB) {
    double SA = 0., SB = 0., bM = 0., tt = 0.;
    sh.coord(c, SA, SB, bM, tt);
    const double b = prec * (w0 * B[nt + 2 * d1 + c] + bM);
    if constexpr (WROW) {              // (the share is weighted already: w0 base + share)
      if constexpr (PRIOR) {
        const double kll = kl * pr[d1 + c];
        Dd[c] = kll + prec * (w0 * B[nt + c] + SA);
        yv[c] = b + kll * pr[c];
      } else {
        Dd[c] = kl + prec * (w0 * B[nt + c] + SA);
        yv[c] = b;
      }
    } else if constexpr (PRIOR) {
      const double kll = kl * pr[d1 + c];
      Dd[c] = kll + prec * (w0 * B[nt + c] + dw * SA);
      yv[c] = b + kll * pr[c];
    } else {
      Dd[c] = kl + prec * (w0 * B[nt + c] + dw * SA);
      yv[c] = b;
    }
    bs[c] = b;                         // (b of the data: the loss takes the prior's part through its KL)
    if constexpr (WROW) SBd[c] = w0 * B[nt + d1 + c] + SB;
    else SBd[c] = w0 * B[nt + d1 + c] + dw * SB;
    if (c == 0) tts = w0 * B[nt + 3 * d1] + tt;
  }
  __syncthreads();

  // ---- B: the system
  for (int64_t p = tid; p < nt; p += FB) {
    int i, j;
    tri_decode(p, i, j);
    const double acc = sh.elem(p, i, j);
    if constexpr (WROW) Hm[p] = prec * (w0 * B[p] + acc) + (i == j ? Dd[i] : 0.0);
    else Hm[p] = prec * (w0 * B[p] + dw * acc) + (i == j ? Dd[i] : 0.0);
  }
  __syncthreads();

  // ---- C, D: the factorisation, the substitutions and the rounding of the exact fold-in
  chol_solve(Hm, yv, dv, xv, d1);
  for (int c = tid; c < d1; c += FB) {
    if constexpr (PRIOR) put_params<LINK, true>(pf, d1, c, xv[c], kl, prec, SBd[c], kl * pr[d1 + c]);
    else put_params<LINK>(pf, d1, c, xv[c], kl, prec, SBd[c]);
  }
  __syncthreads();
  store(pf);

  // ---- E: L_e at the written parameters from the system; column c of L^T theta, the diagonal of L is 1 / dv
  for (int c = tid; c < d1; c += FB) {
    const double th = pf[c], sg = link_d<LINK>(pf[d1 + c]);
    double l = th / dv[c];
    for (int i = c + 1; i < d1; ++i) l += Hm[tri(i) + c] * (double)pf[i];
    if constexpr (PRIOR) {
      // KL(N(th, sg^2) || N(m, 1 / lam)) = KL(N(sqrt(lam) (th - m), lam sg^2) || N(0, 1)), as kl_prior_normal takes it
      const double kll = kl * pr[d1 + c], sl = sqrt(pr[d1 + c]);
      const double tm = sl * (th - pr[c]), ts = sl * sg;
      const double klq = 0.5 * (ts * ts + tm * tm - 1.0) - log(ts);
      lt[c] = (l * l - kll * th * th) - 2.0 * th * bs[c] + prec * sg * sg * SBd[c] + 2.0 * kl * klq;
    } else {
      const double klq = 0.5 * (sg * sg + th * th - 1.0) - log(sg);
      lt[c] = (l * l - kl * th * th) - 2.0 * th * bs[c] + prec * sg * sg * SBd[c] + 2.0 * kl * klq;
    }
  }
  __syncthreads();
  if (tid == 0) {
    double sum = prec * tts;
    for (int c = 0; c < d1; ++c) sum += lt[c];
    *loss = (float)(0.5 * sum + SBd[0] * ((double)LOG_2PI_HALF - 0.5 * log(prec)));
  }
}

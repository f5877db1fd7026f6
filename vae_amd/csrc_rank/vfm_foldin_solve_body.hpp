// vfm_foldin_solve_body.hpp -- the per-entity body of the exact fold-in, shared by k_foldin_solve
// (vfm_foldin_solve.hip), the exact elicitation sessions (exact_session of vfm_elicit_exact_body.hpp: k_elicit_solve and
// k_elicit_design) and, for its phases C and D, the split solve (vfm_foldin_split.hip): the fp64 operand pass, the solve
// of one entity's closed-form optimum by a workgroup (phases A-E of vfm_foldin_solve.hip's head comment) and the host
// helpers of the workspace the units lay out alike -- the operand block and the placement of the slabs (SolveSlabs,
// place_slabs, slabs_bytes).  Included inside `namespace vfm { namespace {` of a unit, after vfm_foldin_body.hpp.
//
// The body is parameterised over where the entity's rows come from (a Rows object: op(i), y(i) of row i in fold
// order), as fold_run is.  Every sum is fp64 in a fixed order that depends on the entity's rows alone, under fp
// contraction `on` (the pragma at the top of each body pins it whichever flag the including unit is compiled with), so
// the bits are the same wherever the body is instantiated and wherever the triangle lives.
#pragma once

__host__ __device__ inline int64_t tri(int64_t m) { return m * (m + 1) / 2; }

// (i, j), j <= i, of packed index p = i (i + 1) / 2 + j
__device__ __forceinline__ void tri_decode(int64_t p, int& i, int& j) {
  int r = (int)((sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
  while (tri(r + 1) <= p) ++r;
  while (tri(r) > p) --r;
  i = r;
  j = (int)(p - tri(r));
}

// all-reduce over the wave, a fixed butterfly: every lane ends with the same bits
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// LDS of a block in doubles: seven vectors of d + 1, the fp32 parameters (2 (d + 1) floats), the triangle
__host__ __device__ inline int64_t lds_doubles(int d, int cap_dim) { return 8 * (int64_t)(d + 1) + tri(cap_dim); }
// ... of a block that solves under a field prior (include/vfm_prior.h): the prior's mean | precision [2, d + 1] in front
__host__ __device__ inline int64_t lds_doubles_prior(int d, int cap_dim) { return 2 * (int64_t)(d + 1) + lds_doubles(d, cap_dim); }

template <int LINK>
__device__ __forceinline__ double link_d(float s) { return LINK == LINK_ABS ? fabs((double)s) : softplus_d((double)s); }

// k_foldin_prep's operand o in fp64: the same sums, not rounded to fp32, the links of the fp32 table values in fp64
template <int LINK>
__global__ __launch_bounds__(FB) void k_foldin_solve_prep(int64_t n_ops, int F, int d, int col, int64_t T,
                                                          const int64_t* __restrict__ opx, const float* __restrict__ ent,
                                                          const float* __restrict__ bias, const float* __restrict__ scal,
                                                          double* __restrict__ ops, double* __restrict__ cmo) {
#pragma clang fp contract(on)
  const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= n_ops) return;
  const int64_t* xr = opx + o * F;
  bool ok = true;
  for (int f = 0; f < F; ++f) ok = ok && (f == col || (xr[f] >= 0 && xr[f] < T));
  double* out = ops + o * 3 * (int64_t)d;
  if (!ok) {
    for (int k = 0; k < 3 * d; ++k) out[k] = __builtin_nan("");
    cmo[o] = __builtin_nan("");
    return;
  }
  double cm = scal[1];
  for (int f = 0; f < F; ++f)
    if (f != col) cm += bias[xr[f] * 2];
  for (int k = 0; k < d; ++k) {
    double sm = 0., smm = 0., ss = 0.;
    for (int f = 0; f < F; ++f) {
      if (f == col) continue;
      const float* row = ent + xr[f] * 2 * (int64_t)d;
      const double m = row[k], sg = link_d<LINK>(row[d + k]);
      sm += m; smm += m * m; ss += sg * sg;
    }
    double cov = 0.;
    for (int f = 0; f < F; ++f) {
      if (f == col) continue;
      const float* row = ent + xr[f] * 2 * (int64_t)d;
      const double m = row[k], sg = link_d<LINK>(row[d + k]);
      cov += sg * sg * (sm - m);
    }
    cm += 0.5 * (sm * sm - smm);
    out[k] = sm;
    out[d + k] = ss;
    out[2 * d + k] = 2.0 * cov;
  }
  cmo[o] = cm;
}

// the size of the system of an entity with n rows: the dual n x n while n <= d, else the primal (d + 1) x (d + 1)
__device__ __forceinline__ int solve_dim(int64_t n, int d) { return n <= d ? (int)n : d + 1; }

// phase C of solve_body, by the whole workgroup (it holds barriers): L L^T = the packed system Hm [m] (row i of L:
// thread i mod FB; row m: the right-hand side yv), one barrier per column, so the forward substitution is part of the
// factorisation; then L^T x = yv from the last column back.  dv: 1 / L_jj; xv: the solution.
__device__ __forceinline__ void chol_solve(double* Hm, double* yv, double* dv, double* xv, int m) {
#pragma clang fp contract(on)
  const int tid = threadIdx.x;
  for (int j = 0; j < m; ++j) {
    const double* Lj = Hm + tri(j);
    int i = j + 1 + (tid - (j + 1) % FB + FB) % FB;        // the first row below j that this thread owns
    if (i <= m) {
      double sjj = Lj[j];
      for (int k = 0; k < j; ++k) sjj -= Lj[k] * Lj[k];
      const double rinv = 1.0 / sqrt(sjj);
      if (i == j + 1) dv[j] = rinv;
      for (; i <= m; i += FB) {
        double* Li = i < m ? Hm + tri(i) : yv;
        double sij = Li[j];
        for (int k = 0; k < j; ++k) sij -= Li[k] * Lj[k];
        Li[j] = sij * rinv;
      }
    }
    __syncthreads();
  }
  // L^T x = yv, from the last column back
  for (int j = m - 1; j >= 0; --j) {
    const double xj = yv[j] * dv[j];
    const double* Lj = Hm + tri(j);
    for (int i = tid; i < j; i += FB) yv[i] -= Lj[i] * xj;
    if (tid == 0) xv[j] = xj;
    __syncthreads();
  }
}

// the field prior of a workgroup (PRIOR instantiations): prior [2, d + 1] fp32 = mean | precision into pr in fp64, by the
// whole workgroup; the caller puts the barrier
__device__ __forceinline__ void stage_prior(const float* __restrict__ prior, double* pr, int d1) {
  for (int c = threadIdx.x; c < 2 * d1; c += FB) pr[c] = (double)prior[c];
}

// the scale parameter of the prior's own sigma = lam^-1/2, to fp32: what a session's `reset` starts a respondent at under
// a prior (vfm_elicit_exact_body.hpp).  At lam = 1 the bits of prior_s<LINK>().
template <int LINK>
__device__ __forceinline__ float prior_row_s(double lam) {
  const double sg = sqrt(1.0 / lam);
  return (float)(LINK == LINK_ABS ? sg : log(expm1(sg)));
}

// KL(N(mu, sg^2) || N(m, 1 / lam)) = kl_std_normal(sqrt(lam) (mu - m), sqrt(lam) sg); at m = 0, lam = 1 its bits
__device__ __forceinline__ float kl_prior_normal(float mu, float sg, float m, float sl) {
  return kl_std_normal(sl * (mu - m), sl * sg);
}

// phase D's rounding: coordinate c's mean th and its scale from the closed form sigma^2 = kl / (kl + prec SB), to fp32
// (PRIOR: kl / (kll + prec SB), kll = kl lam_c)
template <int LINK, bool PRIOR = false>
__device__ __forceinline__ void put_params(float* pf, int d1, int c, double th, double kl, double prec, double SB,
                                           double kll = 0.) {
#pragma clang fp contract(on)
  double den;
  if constexpr (PRIOR) den = kll + prec * SB;
  else den = kl + prec * SB;
  const double sg = sqrt(kl / den);
  pf[c] = (float)th;
  pf[d1 + c] = (float)(LINK == LINK_ABS ? sg : log(expm1(sg)));
}

// ---------------------------------------------------------------------------------------------------------------------
// solve_body: the closed-form optimum of one entity over its n rows, by the whole workgroup (FB threads, every thread
// calls it: it holds barriers).  a: the options and the fp32 operands of the loss pass (a.cap = 0: nothing staged);
// ops64 [n_ops, 3, d] = M | A | C and cm64 [n_ops] = c_mean, unrounded; sm: the block's LDS (lds_doubles); Hm: the
// packed triangle of solve_dim(n, d), in LDS or in the workgroup's slab.  The fp32 parameters land in LDS, pf =
// (float*)(sm + 7 (d + 1)): [mu_w, mu [d] | s_w, s [d]]; after the barrier that publishes them every thread calls
// store() (the fold-in writes the table row there, a session its out_theta); then wave 0 evaluates L_e at them into
// *loss.  The caller puts a barrier before pf or any other LDS of the block is written again.
// PRIOR (include/vfm_prior.h): the entity's prior is N(m_c, 1 / lam_c) per coordinate, pr = m [d + 1] | lam [d + 1] in
// LDS (stage_prior): D_c = kl lam_c + prec SA_c, b_c += kl lam_c m_c, sigma_c^2 = kl / (kl lam_c + prec SB_c), and the
// KL of the loss is to that prior.  At m = 0, lam = 1 every expression rounds as with PRIOR off.
// ---------------------------------------------------------------------------------------------------------------------
template <int W, int CPL, int LINK, bool PRIOR = false, class Rows, class Store>
__device__ __forceinline__ void solve_body(const FoldArgs& a, const double* ops64, const double* cm64, const Rows& rows,
                                           int64_t n, double* sm, double* Hm, float precf, double prec, float* loss,
                                           Store&& store, const double* pr = nullptr) {
#pragma clang fp contract(on)
  constexpr int DP = W * CPL;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int d = a.d, d1 = d + 1;
  double* Dd = sm;                       // D                                  [d + 1]  (0: the first-order weight)
  double* Di = Dd + d1;                  // 1 / D
  double* bv = Di + d1;                  // primal: b; dual: D^-1 b
  double* yv = bv + d1;                  // the right-hand side, then L^-1 of it
  double* dv = yv + d1;                  // 1 / L_jj
  double* xv = dv + d1;                  // the solution of the system
  double* SBd = xv + d1;                 // n, sum_r (A_rk + M_rk^2)
  float* pf = (float*)(SBd + d1);        // the fp32 parameters written: mu_w, mu [d] | s_w, s [d]
  const double kl = a.klw;
  const int64_t os = 3 * (int64_t)d;     // stride of an fp64 operand
  const bool dual = n <= d;
  const int m = dual ? (int)n : d1;

  // ---- A: the row sums of each coordinate
  for (int c = tid; c < d1; c += FB) {
    double SA = 0., SB = 0., SC = 0., bM = 0.;
    if (c == 0) {
      for (int64_t i = 0; i < n; ++i) bM += (double)rows.y(i) - cm64[rows.op(i)];
      SB = (double)n;
    } else {
      for (int64_t i = 0; i < n; ++i) {
        const int64_t o = rows.op(i);
        const double* op = ops64 + o * os + (c - 1);
        const double M = op[0], A = op[d], C = op[2 * d];
        const double t = (double)rows.y(i) - cm64[o];
        SA += A;
        SB += A + M * M;
        SC += C;
        bM += t * M;
      }
    }
    double D, b;
    if constexpr (PRIOR) {
      const double kll = kl * pr[d1 + c], b0 = prec * (bM - 0.5 * SC);
      D = kll + prec * SA;
      b = b0 + kll * pr[c];
    } else {
      D = kl + prec * SA;
      b = prec * (bM - 0.5 * SC);
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
      if (lane == 0) Hm[p] = acc + Di[0] + (i == j ? 1.0 / prec : 0.0);
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
        acc = (double)n;
      } else if (j == 0) {
        for (int64_t r = 0; r < n; ++r) acc += ops64[rows.op(r) * os + (i - 1)];
      } else {
        for (int64_t r = 0; r < n; ++r) {
          const double* op = ops64 + rows.op(r) * os;
          acc += op[i - 1] * op[j - 1];
        }
      }
      Hm[p] = prec * acc + (i == j ? Dd[i] : 0.0);
    }
    for (int c = tid; c < d1; c += FB) yv[c] = bv[c];
  }
  __syncthreads();

  // ---- C: the factorisation and the two substitutions
  chol_solve(Hm, yv, dv, xv, m);

  // ---- D: the means and the scales, rounded to fp32
  for (int c = tid; c < d1; c += FB) {
    double th;
    if (dual) {
      double acc = 0.;
      if (c == 0) {
        for (int i = 0; i < m; ++i) acc += xv[i];
      } else {
        for (int i = 0; i < m; ++i) acc += ops64[rows.op(i) * os + (c - 1)] * xv[i];
      }
      th = bv[c] - Di[c] * acc;
    } else {
      th = xv[c];
    }
    if constexpr (PRIOR) put_params<LINK, true>(pf, d1, c, th, kl, prec, SBd[c], kl * pr[d1 + c]);
    else put_params<LINK>(pf, d1, c, th, kl, prec, SBd[c]);
  }
  __syncthreads();
  store(pf);

  // ---- E: L_e at the written parameters (wave 0; its 64 / W lane groups all hold this entity).  The last pass of
  // fold_run's closed form, expression for expression: fp32 chains in row order, lane l of a group owns j W + l
  if (wv == 0) {
    const int l = lane % W;
    float mu[CPL], sg[CPL], SA[CPL], SB[CPL], SC[CPL];
    bool vk[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      const int kc = j * W + l;
      vk[j] = kc < d;
      mu[j] = vk[j] ? pf[1 + kc] : 0.f;
      sg[j] = link_f<LINK>(vk[j] ? pf[d1 + 1 + kc] : prior_s<LINK>());
      SA[j] = SB[j] = SC[j] = 0.f;
    }
    const float muw = pf[0], sgw = link_f<LINK>(pf[d1]);
    float Scv = 0.f, rsq = 0.f;
    fold_stage_rows<W, CPL>(a, rows, 0, n, l, nullptr, nullptr, SA, SB, SC, Scv);     // (a.cap = 0: nothing staged)
    for (int64_t i = 0; i < n; ++i) {
      const int64_t o = rows.op(i);
      float p = 0.f;
#pragma unroll
      for (int j = 0; j < CPL; ++j) p = fmaf(mu[j], a.ops[o * 3 * DP + j * W + l], p);
      const float res = ((a.opc[o * 2] - rows.y(i)) + muw) + group_sum<W>(p);
      rsq = fmaf(res, res, rsq);
    }
    float vq = 0.f, klq = 0.f;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      vq += fmaf(mu[j] * mu[j], SA[j], fmaf(sg[j] * sg[j], SB[j], mu[j] * SC[j]));
      if constexpr (PRIOR) {
        if (vk[j]) klq += kl_prior_normal(mu[j], sg[j], (float)pr[1 + j * W + l], sqrtf((float)pr[d1 + 1 + j * W + l]));
      } else {
        if (vk[j]) klq += kl_std_normal(mu[j], sg[j]);
      }
    }
    vq = group_sum<W>(vq);
    if constexpr (PRIOR) klq = group_sum<W>(klq) + kl_prior_normal(muw, sgw, (float)pr[0], sqrtf((float)pr[d1]));
    else klq = group_sum<W>(klq) + kl_std_normal(muw, sgw);
    const double sumv = (double)Scv + (double)n * sgw * sgw + vq;
    const double lsum = 0.5 * precf * ((double)rsq + sumv) + (double)n * ((double)LOG_2PI_HALF - 0.5 * log((double)precf));
    if (lane == 0) *loss = (float)(lsum + (double)a.klw * (double)klq);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side: the LDS rule of the triangle, the slabs, the operand block both units put in their workspace
// [fp32 operands | their constants | fp64 operands | fp64 c_mean | slabs], the two operand passes, and what the four
// solve entry points do alike: the checks, the FoldArgs fill, the launch with dynamic LDS, the split units' placement
// ---------------------------------------------------------------------------------------------------------------------
inline int cap_dim_of(int d, int lds_dim) {
  const int fit = d + 1 < VFM_FOLDIN_SOLVE_LDS_DIM ? d + 1 : VFM_FOLDIN_SOLVE_LDS_DIM;
  return lds_dim < 0 || lds_dim > fit ? fit : lds_dim;
}

inline int64_t slab_bytes(int d) { return round_up(tri(d + 1) * 8, 256); }

// where the systems too large for LDS go: a slab per workgroup of the solving kernel
struct SolveSlabs {
  double* slab;                          // [gridDim.x, slab_elems] or NULL when every system stays in LDS
  int64_t slab_elems;
  int32_t cap_dim;                       // systems up to this size live in LDS
};

// the slabs' bytes in a workspace that solves n entities
inline int64_t slabs_bytes(int64_t n, int d, int lds_dim) {
  if (d + 1 <= cap_dim_of(d, lds_dim)) return 0;
  return (n < VFM_FOLDIN_SOLVE_SLABS ? n : VFM_FOLDIN_SOLVE_SLABS) * slab_bytes(d);
}

// sl for n entities with the slabs at `base`; returns the grid of the solving kernel: n, capped at the slabs when they
// are needed, else at gcap
inline unsigned place_slabs(int d, int lds_dim, int64_t n, char* base, int64_t gcap, SolveSlabs& sl) {
  sl.cap_dim = cap_dim_of(d, lds_dim);
  const bool slabs = d + 1 > sl.cap_dim;
  sl.slab = slabs ? (double*)base : nullptr;
  sl.slab_elems = slab_bytes(d) / 8;
  const int64_t gmax = slabs ? VFM_FOLDIN_SOLVE_SLABS : gcap;
  return (unsigned)(n < gmax ? n : gmax);
}

inline int64_t off_ops64(int64_t n_ops, int d) { return ops_off_opc(n_ops, d) + round_up(n_ops * 2 * 4, 256); }
inline int64_t off_cm64(int64_t n_ops, int d) { return off_ops64(n_ops, d) + round_up(n_ops * 3 * d * 8, 256); }
inline int64_t off_slabs(int64_t n_ops, int d) { return off_cm64(n_ops, d) + round_up(n_ops * 8, 256); }

// k_foldin_prep and k_foldin_solve_prep over the n_ops rows of op_x (n_ops > 0) into the operand block at w
inline int launch_solve_preps(bool sp, const FoldArgs& a, int64_t n_ops, const int64_t* op_x, char* w, hipStream_t st) {
  float* ops = (float*)w;
  float* opc = (float*)(w + ops_off_opc(n_ops, a.d));
  double* ops64 = (double*)(w + off_ops64(n_ops, a.d));
  double* cm64 = (double*)(w + off_cm64(n_ops, a.d));
  if (int rc = launch_foldin_prep(sp, a, n_ops, op_x, ops, opc, st)) return rc;
  const unsigned nb = (unsigned)((n_ops + FB - 1) / FB);
  for_link(sp, [&](auto link) {
    hipLaunchKernelGGL(k_foldin_solve_prep<decltype(link)::value>, dim3(nb), dim3(FB), 0, st, n_ops, a.F, a.d, a.col, a.T,
                       op_x, a.entity, a.bias, a.scal, ops64, cm64);
  });
  return launch_status("k_foldin_solve_prep");
}

// ---- what the four solve entry points (vfm_foldin_solve.hip, vfm_foldin_split.hip, vfm_foldin_bound.hip,
// vfm_foldin_bound_split.hip) do alike; P: the entry's C struct, S: its kernel-argument struct

// The checks of *p, p not NULL: the scalars, then own() -- the entry's own checks, a message or NULL -- and, for
// E > 0, the pointers (list: row_ptr or chunk_ptr; chunks: false only when a chunk table with rows is missing) and the
// workspace against ws, the value of the size function named ws_fn.  0 with E == 0: nothing to do.
template <class P, class Own>
int check_solve(const P* p, const void* list, bool chunks, int64_t ws, const char* ws_fn, Own own) {
  if (p->T < 1) return fail(VFM_E_INVALID, "T < 1");
  if (p->d < 1 || p->d > VFM_FOLDIN_MAX_D) return fail(VFM_E_INVALID, "d out of range [1,512]");
  if (p->F < 1 || p->F > VFM_MAX_FIELDS) return fail(VFM_E_INVALID, "F out of range [1,64]");
  if (p->col < 0 || p->col >= p->F) return fail(VFM_E_INVALID, "col out of range [0,F)");
  if (p->E < 0 || p->R < 0) return fail(VFM_E_INVALID, "E < 0 or R < 0");
  if (p->n_ops < 0 || (p->R > 0 && p->n_ops < 1)) return fail(VFM_E_INVALID, "n_ops out of range");
  if (p->flags & ~VFM_FLAG_LINK_SOFTPLUS) return fail(VFM_E_INVALID, "flags: only VFM_FLAG_LINK_SOFTPLUS is accepted");
  if (p->lds_dim < -1) return fail(VFM_E_INVALID, "lds_dim: -1 or >= 0");
  if (!(p->kl_weight > 0.f) || !(p->kl_weight <= 3.0e38f))
    return fail(VFM_E_INVALID, "kl_weight must be > 0 and finite (the prior is what makes the system positive definite)");
  if (const char* msg = own()) return fail(VFM_E_INVALID, msg);
  if (p->E == 0) return 0;
  if (!p->entities || !list || !p->entity_params || !p->bias_params || !p->scalars || !p->out_loss || !chunks ||
      (p->R > 0 && (!p->y || !p->op_x || !p->row_op)))
    return fail(VFM_E_INVALID, "null pointer");
  char msg[96];
  if (ws < 0) {
    snprintf(msg, sizeof(msg), "sizes out of range (%s)", ws_fn);
    return fail(VFM_E_INVALID, msg);
  }
  if (p->workspace_bytes < ws || (ws > 0 && !p->workspace)) {
    snprintf(msg, sizeof(msg), "workspace too small (%s)", ws_fn);
    return fail(VFM_E_INVALID, msg);
  }
  if (ws > 0 && (((uintptr_t)p->workspace) & 255)) return fail(VFM_E_INVALID, "workspace must be 256-byte aligned");
  return 0;
}

// s.f for a solve of p's rows (a.ptr stays NULL: the entries with a row list set it) and the operand block at the head
// of p's workspace
template <class S, class P>
void fill_solve_args(S& s, const P* p, int lik, int n_iters, int reset, int mode) {
  FoldArgs& a = s.f;
  a = fill_fold_args(p->E, p->T, p->F, p->d, p->col, lik, 1, n_iters, reset, mode, 0.f, p->kl_weight, 0, 0,
                     p->entity_params, p->bias_params, p->scalars);
  a.R = p->R; a.ent = p->entities; a.row_op = p->row_op; a.y = p->y;
  a.loss = p->out_loss;
  char* w = (char*)p->workspace;
  a.ops = (float*)w;
  a.opc = (float*)(w + ops_off_opc(p->n_ops, p->d));
  s.ops64 = (double*)(w + off_ops64(p->n_ops, p->d));
  s.cm64 = (double*)(w + off_cm64(p->n_ops, p->d));
}

// a kernel of FB threads with shm bytes of dynamic LDS (more than 64 KiB: state the size first; a runtime that needs no
// opt-in ignores it)
template <class K, class... S>
void launch_lds(K k, unsigned grid, size_t shm, hipStream_t st, const S&... s) {
  (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
  (void)hipGetLastError();
  hipLaunchKernelGGL(k, dim3(grid), dim3(FB), shm, st, s...);
}

// ---- the two split units: a slab of part_doubles(d) per chunk [triangle tri(d + 1) | SA [d + 1] | SB [d + 1] |
// sum t u [d + 1] | SC [d]], a loss partial per chunk, then the solve slabs
inline int64_t part_doubles(int d) { return tri(d + 1) + 4 * (int64_t)d + 3; }
inline int64_t part_bytes(int64_t n_chunks, int d) { return round_up(n_chunks * part_doubles(d) * 8, 256); }
inline int64_t lpart_bytes(int64_t n_chunks) { return round_up(n_chunks * 8, 256); }

struct SplitGrids {
  unsigned c, e;                         // a workgroup per chunk, per entity
};

// p's chunk table and, from `base` on, part, lpart and the solve slabs into s
template <class S, class P>
SplitGrids place_split(S& s, const P* p, char* base) {
  s.chunk_ptr = p->chunk_ptr; s.chunks = p->chunks;
  s.n_ops = p->n_ops; s.n_chunks = p->n_chunks;
  s.part_elems = part_doubles(p->d);
  s.part = (double*)base;
  base += part_bytes(p->n_chunks, p->d);
  s.lpart = (double*)base;
  const int64_t gcap = (int64_t)1 << 20;
  const unsigned grid_e = place_slabs(p->d, p->lds_dim, p->E, base + lpart_bytes(p->n_chunks), gcap, s.sl);
  return {(unsigned)(p->n_chunks < gcap ? p->n_chunks : gcap), grid_e};
}

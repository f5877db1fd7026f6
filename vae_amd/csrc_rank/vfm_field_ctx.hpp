// vfm_field_ctx.hpp -- the context / candidate arithmetic of the field form (include/vfm_rank.h), shared by the
// field-form ranking (vfm_rank_field.hip) and the field-form elicitation session (vfm_elicit_field.hip): the fp64
// context operands of a coordinate, their fp32 roundings, the context's constants, the candidate's operands and the two
// fp32 chains of a (context, candidate) pair.  One definition, so a field-form score is the same bits wherever it is
// formed.  Every function pins fp contraction off itself (#pragma clang fp contract(off)): the ranking units are
// compiled with -ffp-contract=off anyway, the session unit with `on` for the fold-in's body.
//
// A context column's parameters come from a row-source: TableRows (the table rows of the column's id) or PostRows (the
// same for every column but one, whose parameters are a supplied posterior row [mu | s | mu_w | s_w]: the *_post_f32
// entry points of vfm_rank.h).  The arithmetic does not know which: the same sums, in the same column order.
#pragma once

#include "vfm_rank_tile.hpp"         // link_of, op_mean

namespace {

// Coordinate k of a context (the columns f != field of xr), in fp64, sums in column order.  With S the sum of the
// context embeddings and P their pair term:  M = E S,  A = Var S,  C = 2 Cov(S, P) = 2 sum_q sigma_q^2 (M - mu_q),
// ep = E P = ((sum mu)^2 - sum mu^2) / 2,  vp = Var P = sum_{q<r} sigma_q^2 sigma_r^2 + sum_q sigma_q^2 (M - mu_q)^2
// (the context-only part of the variance of vfm_rank.h), the sums over q expanded so that one pass over the rows serves.
struct CtxCoord {
  double M, A, C, ep, vp;
};

// Row-sources: where column f of a context (entity id `id`) keeps its [mu | s] and [mu_w, s_w].  at(r): the source of
// query r of a call.
struct TableRows {
  const float* __restrict__ ent;
  const float* __restrict__ bias;
  __device__ __forceinline__ TableRows at(int64_t) const { return *this; }
  __device__ __forceinline__ const float* ent_row(int, int64_t id, int d) const { return ent + id * 2 * d; }
  __device__ __forceinline__ const float* bias_row(int, int64_t id, int) const { return bias + id * 2; }
};

// Column post_field from the query's row of post [., 2d + 2] = [mu | s | mu_w | s_w] (raw stored values: the link is
// applied as for a table row); the table rows of that column's id are never read
struct PostRows {
  const float* __restrict__ ent;
  const float* __restrict__ bias;
  const float* __restrict__ post;
  int post_field, d;
  __device__ __forceinline__ PostRows at(int64_t r) const {
    return PostRows{ent, bias, post + r * (2 * (int64_t)d + 2), post_field, d};
  }
  __device__ __forceinline__ const float* ent_row(int f, int64_t id, int dd) const {
    return f == post_field ? post : ent + id * 2 * dd;
  }
  __device__ __forceinline__ const float* bias_row(int f, int64_t id, int dd) const {
    return f == post_field ? post + 2 * dd : bias + id * 2;
  }
};

template <typename ID, typename SRC>
__device__ __forceinline__ CtxCoord ctx_coord_of(const ID* xr, int F, int field, int k, int d, bool sp, const SRC& src) {
#pragma clang fp contract(off)
  double s1 = 0., smm = 0., ss = 0., sss = 0., ssm = 0., ssmm = 0.;
  for (int f = 0; f < F; ++f) {
    if (f == field) continue;
    const float* row = src.ent_row(f, (int64_t)xr[f], d);
    const double m = row[k], s = link_of(row[d + k], sp), s2 = s * s;
    s1 += m; smm += m * m; ss += s2; sss += s2 * s2; ssm += s2 * m; ssmm += s2 * (m * m);
  }
  CtxCoord c;
  c.M = s1;
  c.A = ss;
  c.C = 2. * (s1 * ss - ssm);
  c.ep = 0.5 * (s1 * s1 - smm);
  c.vp = 0.5 * (ss * ss - sss) + ((s1 * s1) * ss - 2. * s1 * ssm + ssmm);
  return c;
}

template <typename ID>
__device__ __forceinline__ CtxCoord ctx_coord(const ID* xr, int F, int field, int k, int d, bool sp,
                                              const float* __restrict__ ent) {
  return ctx_coord_of(xr, F, field, k, d, sp, TableRows{ent, nullptr});
}

// The stored (fp32, rounded once) query operands of a coordinate: mean part [M], variance part [A | A + M^2 | C]
__device__ __forceinline__ float ctx_op_var(const CtxCoord& c, int part) {
#pragma clang fp contract(off)
  return part == 0 ? (float)c.A : part == 1 ? (float)(c.A + c.M * c.M) : (float)c.C;
}

// The context's constants before the coordinates are added: (m0 + sum_q mu_w,q, sigma0^2 + sum_q sigma_w,q^2)
template <typename ID, typename SRC>
__device__ __forceinline__ void ctx_consts_of(const ID* xr, int F, int field, int d, bool sp, const SRC& src,
                                              const float* __restrict__ scal, double& cm, double& cv) {
#pragma clang fp contract(off)
  const double sg0 = (double)link_of(scal[2], sp);
  cm = (double)scal[1];
  cv = sg0 * sg0;
  for (int f = 0; f < F; ++f) {
    if (f == field) continue;
    const float* b = src.bias_row(f, (int64_t)xr[f], d);
    const double sw = (double)link_of(b[1], sp);
    cm += (double)b[0];
    cv += sw * sw;
  }
}

template <typename ID>
__device__ __forceinline__ void ctx_consts(const ID* xr, int F, int field, bool sp, const float* __restrict__ bias,
                                           const float* __restrict__ scal, double& cm, double& cv) {
  ctx_consts_of(xr, F, field, 0, sp, TableRows{nullptr, bias}, scal, cm, cv);
}

template <typename ID>
__device__ __forceinline__ bool ctx_valid(const ID* xr, int F, int field, int64_t T) {
  bool ok = true;
  for (int f = 0; f < F; ++f) ok = ok && (f == field || ((int64_t)xr[f] >= 0 && (int64_t)xr[f] < T));
  return ok;
}

// The candidate's operands: mean part [mu], variance part [mu^2 | sigma^2 | mu]
__device__ __forceinline__ float cand_op_var(const float* row, int kb, int d, bool sp) {
#pragma clang fp contract(off)
  if (kb < d) return row[kb] * row[kb];
  if (kb < 2 * d) {
    const float s = link_of(row[kb], sp);        // (row[d + (kb - d)])
    return s * s;
  }
  return row[kb - 2 * d];
}

// A candidate's operands read from its table rows (ec [2d] = [mu | s], bc [2] = [mu_w, s_w])
struct TableCand {
  const float *ec, *bc;
  int d;
  bool sp;
  __device__ float mean_op(int k) const { return op_mean(ec, k); }
  __device__ float var_op(int part, int k) const { return cand_op_var(ec, part * d + k, d, sp); }   // (kb = part d + k)
  __device__ float mu_w() const { return bc[0]; }
  __device__ float var_w() const {
#pragma clang fp contract(off)
    const float sw = link_of(bc[1], sp);
    return sw * sw;
  }
};

// ---------------------------------------------------------------------------------------------------------------------
// field_chain_moments: the moments of (context, candidate) from the query's operands q (q.mean_op(k), q.var_op(part, k))
// and the candidate's c (c.mean_op(k), c.var_op(part, k), c.mu_w(), c.var_w()); part 0 .. 2 of the variance operands
// as listed above.  The same fp32 chains, in the same k order (the variance chain: part by part), as the MFMA
// accumulation of the tile, and the tile's epilogue (accumulator + query constant) + candidate constant.
// ---------------------------------------------------------------------------------------------------------------------
template <typename QOP, typename COP>
__device__ __forceinline__ void field_chain_moments(const QOP& q, const COP& c, float c_mean, float c_var, int d,
                                                    float& mean, float& var) {
#pragma clang fp contract(off)
  float am = 0.f, av = 0.f;
  for (int k = 0; k < d; ++k) am = fmaf(c.mean_op(k), q.mean_op(k), am);
#pragma unroll
  for (int part = 0; part < 3; ++part)
    for (int k = 0; k < d; ++k) av = fmaf(c.var_op(part, k), q.var_op(part, k), av);
  mean = (am + c_mean) + c.mu_w();
  var = (av + c_var) + c.var_w();
}

// the candidate from its table rows (the ranking's merge, positives and k_field_moments)
template <typename QOP>
__device__ void field_pair_moments(const QOP& q, const float* ec, const float* bc, float c_mean, float c_var, int d,
                                   bool sp, float& mean, float& var) {
  field_chain_moments(q, TableCand{ec, bc, d, sp}, c_mean, c_var, d, mean, var);
}

}  // namespace

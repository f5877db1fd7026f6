// vfm_design_score.hpp -- the target-aware question score (include/vfm_design.h) on the device: the two walks that form
// a respondent's scale sums S and target weights W, and the score of one candidate row.  Used by k_design_score (every
// pool row's score, one round) and DesignScore (the score k_elicit_design gives the session loop of
// vfm_elicit_exact_body.hpp, whose order of the choice it shares with k_elicit_solve), both in vfm_elicit_design.hip,
// so a score exists once.  Included inside `namespace vfm { namespace {` of a unit, after vfm_foldin_solve_body.hpp.
//
// With the partners frozen the scales of a respondent's optimum do not depend on the answers:
//   sigma_k^2 = v_k(S_k) = kl / (kl + prec S_k),  S_k = sum_{r in R} (A_rk + M_rk^2);  sigma_w^2 = v_w(n) = kl / (kl + prec n)
// so the posterior a question q would leave behind is known before it is asked, and with it the drop of the mean over
// the target contexts J of the part of Var pred_j that the respondent's scales carry:
//   score(q) = (v_w(n) - v_w(n + 1)) + sum_k W_k (v_k(S_k) - v_k(S_k + a_qk)),  W_k = (1 / |J|) sum_{j in J} a_jk,
//   a_rk = A_rk + M_rk^2.
// Everything is fp64 over the unrounded operands of k_foldin_solve_prep (ops64 [n_ops, 3, d] = M | A | C) and rounded
// to fp32 once.  Orders: S in row order, W in the target list's order, the score from the bias term on in k order.
// Contraction: S is phase A of solve_body -- the same statement under the same pragma (`on`), so the same bits; W, v
// and the score are under `off`.
//
// PRIOR (include/vfm_elicit_prior.h): under the respondents' field prior N(m_c, 1 / lam_c) the optimum's scales are
//   sigma_k^2 = kl / (kl lam_k + prec S_k),  sigma_w^2 = kl / (kl lam_0 + prec n)
// so v takes kll = kl lam_c as the denominator's constant; kll is formed in a statement of its own (as put_params' caller
// and k_bsplit_solve form it), so at lam = 1 it is kl and v rounds as with PRIOR off.  lam [d + 1] (0: the weight) is the
// second half of the prior staged in LDS (stage_prior); m is never read: the score still depends on no answer.
#pragma once

// v(S) = kl / (kl + prec S): the squared scale of the optimum of a coordinate whose rows sum to S  (PRIOR: kl / (kll +
// prec S))
template <bool PRIOR = false>
__device__ __forceinline__ double design_v(double kl, double prec, double S, double kll = 0.) {
#pragma clang fp contract(off)
  if constexpr (PRIOR) return kl / (kll + prec * S);
  else return kl / (kl + prec * S);
}

// vS [d] of S [d], by the thread that wrote S[k] (the walk's own distribution); lam: as design_score's
template <bool PRIOR = false>
__device__ __forceinline__ void design_put_v(double kl, double prec, const double* S, int d, double* vS,
                                             const double* lam = nullptr) {
#pragma clang fp contract(off)
  for (int k = threadIdx.x; k < d; k += FB) {
    double kll = 0.;
    if constexpr (PRIOR) kll = kl * lam[1 + k];
    vS[k] = design_v<PRIOR>(kl, prec, S[k], kll);
  }
}

// S [d]: thread t forms the coordinates t, t + FB, .. over the n rows of `rows` (op(i): the operand of row i) in row
// order.  An operand outside [0, n_ops) makes the respondent's sums NaN.  No barrier: the caller publishes S.
template <class Rows>
__device__ __forceinline__ void design_walk_S(const double* ops64, int64_t n_ops, int d, const Rows& rows, int64_t n,
                                              double* S) {
#pragma clang fp contract(on)
  const int64_t os = 3 * (int64_t)d;
  for (int k = threadIdx.x; k < d; k += FB) {
    double SB = 0.;
    for (int64_t i = 0; i < n; ++i) {
      const int64_t o = rows.op(i);
      if (o < 0 || o >= n_ops) { SB += __builtin_nan(""); continue; }
      const double* op = ops64 + o * os + k;
      const double M = op[0], A = op[d];
      SB += A + M * M;                   // (phase A of solve_body, to the letter)
    }
    S[k] = SB;
  }
}

// W [d]: the mean of a_jk over the nt target operands, in the list's order; an empty list gives 0, a target operand
// outside [0, n_ops) or of an invalid context (a NaN row of ops64) gives NaN.  No barrier.
__device__ __forceinline__ void design_walk_W(const double* ops64, int64_t n_ops, int d, const int64_t* tgt_op, int64_t nt,
                                              double* W) {
#pragma clang fp contract(off)
  const int64_t os = 3 * (int64_t)d;
  const double inv = nt > 0 ? 1.0 / (double)nt : 0.0;
  for (int k = threadIdx.x; k < d; k += FB) {
    double s = 0.;
    for (int64_t j = 0; j < nt; ++j) {
      const int64_t o = tgt_op[j];
      if (o < 0 || o >= n_ops) { s += __builtin_nan(""); continue; }
      const double* op = ops64 + o * os + k;
      const double M = op[0], A = op[d];
      const double a = A + M * M;
      s += a;
    }
    W[k] = nt > 0 ? inv * s : 0.0;
  }
}

// the score of the candidate whose operand row is opq = ops64 + o * 3 d, for a respondent with n fold rows, sums S,
// weights W and vS[k] = design_v(kl, prec, S[k]) (design_put_v); PRIOR: lam [d + 1], the prior's precisions
template <bool PRIOR = false>
__device__ __forceinline__ float design_score(const double* S, const double* W, const double* vS, double n,
                                              const double* opq, int d, double kl, double prec,
                                              const double* lam = nullptr) {
#pragma clang fp contract(off)
  double kll = 0.;
  if constexpr (PRIOR) kll = kl * lam[0];
  double acc = design_v<PRIOR>(kl, prec, n, kll) - design_v<PRIOR>(kl, prec, n + 1.0, kll);
  for (int k = 0; k < d; ++k) {
    const double M = opq[k], A = opq[d + k];
    const double a = A + M * M;
    if constexpr (PRIOR) kll = kl * lam[1 + k];
    const double drop = vS[k] - design_v<PRIOR>(kl, prec, S[k] + a, kll);
    acc += W[k] * drop;
  }
  return (float)acc;
}

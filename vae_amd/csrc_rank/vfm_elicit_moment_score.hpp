// vfm_elicit_moment_score.hpp -- MomentScore, the score policy of exact_session (vfm_elicit_exact_body.hpp) that scores a
// pool row whole by its predictive moments at theta_e (field_chain_moments / score_of / philox_uniform:
// vfm_elicit_field.hip's scores, bit for bit).  Used by k_elicit_solve (vfm_elicit_solve.hip) and k_elicit_bound
// (vfm_elicit_bound.hip).  Included inside `namespace vfm { namespace {` of a unit, after vfm_elicit_exact_body.hpp.
#pragma once

// the questions scored by the predictive moments under the respondent's posterior (or at random)
struct MomentScore {
  using Args = ElicitSolveArgs;
  static constexpr bool THETA_OPS_EVERY_ROUND = true, ROUND_END_BARRIER = false;
  __host__ __device__ static int64_t lds_doubles(int) { return 0; }

  const ElicitFieldArgs& a;
  __device__ __forceinline__ MomentScore(const Args& s, double*, double*, double, const double*) : a(s.e) {}
  __device__ __forceinline__ void begin_respondent(int64_t) const {}
  __device__ __forceinline__ void begin_round(int, const FieldSessionRows&, int64_t) const {}

  template <int DP>
  __device__ __forceinline__ float pool_row(int q, int64_t p0, int64_t p, bool, bool eok, int64_t e, int64_t,
                                            const float* uth) const {
    const int64_t o = a.pool_op[p0 + p];
    float mean = __builtin_nanf(""), var = __builtin_nanf(""), sc = __builtin_nanf("");
    if (pool_row_ok(a, p0 + p, o, eok)) {
      if (a.strat != VFM_RANK_RANDOM || a.out_mean) pool_row_moments<DP>(a, o, uth, mean, var);
      sc = a.strat == VFM_RANK_RANDOM ? philox_uniform(a.seed + (uint64_t)q, a.pool_x[(p0 + p) * a.f.F + a.key_col], e)
                                      : score_of(a.strat, mean, var);
    }
    put_moments(a, q, p0, p, mean, var);
    return sc;
  }
};

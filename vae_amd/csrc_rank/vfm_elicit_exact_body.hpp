// vfm_elicit_exact_body.hpp -- the exact elicitation session, once: ask, solve the respondent's closed-form optimum,
// ask again -- every round of every respondent in one launch.  Used by k_elicit_solve (vfm_elicit_solve.hip: the
// questions scored by the predictive moments), k_elicit_design (vfm_elicit_design.hip: the target-aware score) and
// k_elicit_bound (vfm_elicit_bound.hip: a 'class' model, the fold of a round exchanged for the bound's rounds); each
// of the kernels is exact_session instantiated with its score and its fold.  Also the host path both entry points share: the
// workspace, the kernel arguments, the operand passes, the launch and the checks the two word alike.  Included inside
// `namespace vfm { namespace {` of a unit, after vfm_foldin_solve_body.hpp, vfm_elicit_host.hpp and
// vfm_elicit_field_score.hpp.
//
// exact_session<Score, W, CPL, LINK>: k_foldin_solve's layout -- one workgroup of FB threads per respondent in a
//   grid-stride loop (capped at VFM_FOLDIN_SOLVE_SLABS blocks when slabs are needed), over <W, CPL, LINK> because the
//   loss pass of the solve needs the fold-in's lane groups.  theta_e lives in LDS (pf of solve_body) over all rounds.
//   Per round: the candidate operands of theta_e [mu | mu^2 | sigma^2 | mu_w, sigma_w^2] are refreshed in LDS (when the
//   score or out_mean reads them); thread t scores the pool rows t, t + FB, .. whole; the best (score descending,
//   position ascending) is reduced by a wave butterfly, then across the waves through LDS -- a total order, so the tree
//   does not matter; thread 0 records out_row, out_score and the asked flag; after a barrier solve_body runs on the
//   history followed by the rows asked so far, from the rows themselves (1 / D changes with every appended row, so
//   nothing of the system is carried over).  The table row is written once at the end, and only with `write`.  No
//   atomics.
//
// Score, a compile-time policy (everything it decides is an `if constexpr` or inlined; no runtime flag separates the
// two forms):
//   Args                       the kernel's arguments: ElicitSolveArgs or a struct derived from it
//   lds_doubles(d)             doubles of LDS of its own, between the triangle and the waves' winners
//   THETA_OPS_EVERY_ROUND      are the candidate operands read by the score (else only by out_mean / out_var)?
//   ROUND_END_BARRIER          does begin_round write LDS that solve_body reads (its contract: a barrier first)?
//   Score(s, sm, own, prec, pr)   sm: the block's LDS (behind the prior); own: its lds_doubles; pr: the staged prior or NULL
//   begin_respondent(g)        before the barrier that publishes theta_e
//   begin_round(q, rows, n)    before the barrier that publishes the round's operands; n: fold rows so far
//   pool_row(q, p0, p, was, eok, e, n, uth)   the score of pool row p0 + p (NaN: no candidate); writes out_mean / out_var
//
// LDS of a block: k_foldin_solve's (64 (d + 1) bytes of vectors and the packed triangle of min(d + 1, 135, lds_dim)),
// the score's own doubles, the reduction's words and 3 DP + 2 floats of candidate operands; larger systems go to the
// workgroup's slab.  Everything a respondent reads from LDS or its slab is written for that respondent first.
//
// Evidence that the shared text is the two former kernels.  Code (tools/isa_summary.py, profiles/exact_session_isa_parent.txt
// before, profiles/exact_session_isa.txt after): in all 28 instances VGPRs, scratch (0), LDS, waves per SIMD and the
// s_barrier count (10 moment / 11 design) are unchanged, as are the counts of every load, store and LDS class; the
// instruction counts move by -2 % .. +1.5 % (design <64, 2, softplus>: +4.8 %) with the order the scheduler leaves the
// same operations in.  One spelling mattered: put_moments sums its index as q P + p0 + p; as q P + (p0 + p) every
// instance took 4 more VGPRs and ten lost a wave per SIMD.  Time on an MI355X (tools/elicit_design_bench.py,
// 10,000 respondents x 100 rows, d = 128, 20 rounds, medians of 5; the former kernels' build and this one in one visit,
// the two lines of 2026-10-20 in profiles/elicit_design_bench.jsonl): design 47.117 -> 47.175 ms (+0.12 %; the former
// build's own spread 0.39 %), variance 52.269 -> 52.355 ms (+0.16 %; spread 0.27 %).  Two more unrecorded pairs gave
// +0.19 % / +0.23 % (spreads 0.27 % / 0.19 %) and, with this build run first on a cold device, +1.07 % / +0.24 % (its
// own spread 3.5 % / 1.8 %): a difference of about 0.2 % is not excluded.  session_kernel_ms of
// tools/elicit_field_exact_bench.py: 48.520 before (the day before), 48.546 after.
#pragma once

struct ElicitSolveArgs {
  ElicitFieldArgs e;                     // (e.f.cap = 0; e.f.ops / e.f.opc: the fp32 operands of the loss)
  const double* ops64;                   // [n_ops, 3, d]  M | A | C, unrounded
  const double* cm64;                    // [n_ops]        c_mean
  SolveSlabs sl;                         // the slabs and the LDS rule of the triangle
};

constexpr int NW = FB / WAVE;            // waves of a block

// bytes of a block's LDS past k_foldin_solve's and the score's own: the waves' winners (position, score) and the
// candidate operands
__host__ __device__ inline int64_t session_tail_bytes(int DP) { return NW * 8 + NW * 4 + (3 * (int64_t)DP + 2) * 4; }

// does (os, op) come before (bs, bp) in the order (score descending, position ascending)?  op < 0: no candidate
__device__ __forceinline__ bool better(float os, long long op, float bs, long long bp) {
  return op >= 0 && (bp < 0 || os > bs || (os == bs && op < bp));
}

// slice g of a CSR pointer array over N rows, clamped into [0, N]: first row and count
__device__ __forceinline__ void clamped_range(const int64_t* ptr, int64_t g, int64_t N, int64_t& x0, int64_t& n) {
  x0 = min(max(ptr[g], (int64_t)0), N);
  n = min(max(ptr[g + 1], x0), N) - x0;
}

// respondent g's pool and history slices (no history pointer: no history)
struct RespondentRanges {
  int64_t p0, np, h0, nh;
};
__device__ __forceinline__ RespondentRanges respondent_ranges(const ElicitFieldArgs& a, int64_t g) {
  RespondentRanges r = {0, 0, 0, 0};
  clamped_range(a.pool_ptr, g, a.P, r.p0, r.np);
  if (a.hist_ptr) clamped_range(a.hist_ptr, g, a.H, r.h0, r.nh);
  return r;
}

// is pool row `row` (operand o) a question that can be put: a live respondent, an operand of the table, a valid context?
__device__ __forceinline__ bool pool_row_ok(const ElicitFieldArgs& a, int64_t row, int64_t o, bool eok) {
  return eok && o >= 0 && o < a.n_ops && ctx_valid(a.pool_x + row * a.f.F, a.f.F, a.f.col, a.f.T);
}

// the predictive moments of pool row `row` (operand o) at the candidate operands uth
template <int DP>
__device__ __forceinline__ void pool_row_moments(const ElicitFieldArgs& a, int64_t o, const float* uth, float& mean,
                                                 float& var) {
  const int d = a.f.d;
  field_chain_moments(CtxRowOp{a.sop + o * 4 * (int64_t)d, d}, ThetaCand{uth, DP}, a.soc[o * 2], a.soc[o * 2 + 1], d, mean,
                      var);
}

// out_mean / out_var of pool row p0 + p in round q, when asked for.  (The index is summed in this order on purpose: the
// block-uniform part first keeps it out of the vector registers.)
__device__ __forceinline__ void put_moments(const ElicitFieldArgs& a, int q, int64_t p0, int64_t p, float mean, float var) {
  if (!a.out_mean) return;
  a.out_mean[(int64_t)q * a.P + p0 + p] = mean;
  a.out_var[(int64_t)q * a.P + p0 + p] = var;
}

// The fold of a round, the second compile-time policy of the session: the closed-form optimum of a 'reg' model
// (solve_body), the present one; BoundFold of vfm_elicit_bound.hip runs the Jaakkola-Jordan rounds of a 'class' model
// (bound_body of vfm_foldin_bound_body.hpp) in its place.
//   lds_doubles(d)             doubles of LDS of its own, between the triangle and the score's
//   run<W, CPL, LINK, PRIOR>(s, f, rows, n, g, sm, Hm, own, precf, prec, loss, store, pr)   the fold of respondent g over
//                              its n rows from theta_e in pf; solve_body's contract: pf rewritten, store(pf) by every
//                              thread after the barrier that publishes it, the loss by wave 0, no barrier at the end;
//                              pr: the staged prior of a PRIOR session (else NULL)
//   ALL_PAIRS                  does the fold run over every (respondent, partner) pair of a two-field model (ImplicitFold of
//                              vfm_elicit_implicit.hip)?  Then its system is always the primal (d + 1) x (d + 1) one, and
//                              pool_ok(s, row) says whether pool row `row` names a partner the fold's base block covers
struct SolveFold {
  static constexpr bool ALL_PAIRS = false;
  __host__ __device__ static int64_t lds_doubles(int) { return 0; }
  template <int W, int CPL, int LINK, bool PRIOR, class Args, class Rows, class Store>
  __device__ __forceinline__ static void run(const Args& s, const FoldArgs& f, const Rows& rows, int64_t n, int64_t,
                                             double* sm, double* Hm, double*, float precf, double prec, float* loss,
                                             Store&& store, const double* pr) {
    solve_body<W, CPL, LINK, PRIOR>(f, s.ops64, s.cm64, rows, n, sm, Hm, precf, prec, loss, store, pr);
  }
};

// PRIOR (include/vfm_elicit_prior.h): `prior` [2, d + 1] fp32 = mean | precision of the respondents' field is staged once
// per workgroup, in fp64, in LDS in front of everything else (lds_doubles_prior's rule: k_foldin_solve's), so sm -- and
// with it every LDS pointer of the session -- starts 2 (d + 1) doubles later; the fold of a round runs under it, the
// score is constructed with it, and `reset` starts a respondent at mu = m, sigma = lam^-1/2 (prior_row_s).  Without
// PRIOR nothing of this is compiled: sm is the block's LDS itself and the instance is the parent's.
template <class Score, int W, int CPL, int LINK, class Fold = SolveFold, bool PRIOR = false, class Args>
__device__ __forceinline__ void exact_session(const Args& s, const float* prior = nullptr) {
  extern __shared__ double sm_all[];
  double* sm = sm_all + (PRIOR ? 2 * (s.e.f.d + 1) : 0);
  const double* pr = PRIOR ? sm_all : nullptr;
  constexpr int DP = W * CPL;
  constexpr bool SP = LINK == LINK_SOFTPLUS;
  const ElicitFieldArgs& a = s.e;
  const FoldArgs& f = a.f;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int d = f.d, d1 = d + 1, Q = a.Q;
  float* pf = (float*)(sm + 7 * d1);     // theta_e: mu_w, mu [d] | s_w, s [d]  (solve_body's)
  double* Hl = sm + 8 * d1;
  double* fown = Hl + tri(s.sl.cap_dim);                    // the fold's own doubles
  double* own = fown + Fold::lds_doubles(d);                // the score's own doubles
  long long* rpos = (long long*)(own + Score::lds_doubles(d));  // [NW] the waves' winners
  float* rsc = (float*)(rpos + NW);                         // [NW]
  float* uth = rsc + NW;                                    // [3 DP + 2] the candidate operands of theta_e
  double* Hg = s.sl.slab ? s.sl.slab + (int64_t)blockIdx.x * s.sl.slab_elems : nullptr;
  const float precf = link_f<LINK>(f.scal[0]);
  const double prec = link_d<LINK>(f.scal[0]);
  Score score(s, sm, own, prec, pr);
  if constexpr (PRIOR) {
    stage_prior(prior, sm_all, d1);
    __syncthreads();
  }

  for (int64_t g = blockIdx.x; g < a.U; g += gridDim.x) {
    const RespondentRanges r = respondent_ranges(a, g);
    const int64_t p0 = r.p0, np = r.np;
    const int64_t e = a.ents[g];
    const bool eok = e >= 0 && e < f.T;                     // (block-uniform)
    const FieldSessionRows rows{a, r.h0, r.nh, a.out_row + g * Q};

    // ---- theta_e: the table row, or the prior
    for (int c = tid; c < d1; c += FB) {
      float m = 0.f, sp = prior_s<LINK>();
      if (eok && !f.reset) {
        m = c == 0 ? f.bias[e * 2] : f.entity[e * 2 * d + (c - 1)];
        sp = c == 0 ? f.bias[e * 2 + 1] : f.entity[e * 2 * d + d + (c - 1)];
      } else if constexpr (PRIOR) {
        m = (float)pr[c];
        sp = prior_row_s<LINK>(pr[d1 + c]);
      }
      pf[c] = m;
      pf[d1 + c] = sp;
    }
    score.begin_respondent(g);
    for (int64_t p = tid; p < np; p += FB) a.asked[p0 + p] = 0;
    int64_t n = r.nh;
    __syncthreads();

    const auto put_theta = [&](int q) {                     // theta_e after round q, by every thread
      if (!a.out_theta) return;
      float* to = a.out_theta + (g * Q + q) * (2 * (int64_t)d + 2);
      for (int k = tid; k < d; k += FB) { to[k] = pf[1 + k]; to[d + k] = pf[d1 + 1 + k]; }
      if (tid == 0) { to[2 * d] = pf[0]; to[2 * d + 1] = pf[d1]; }
    };

    for (int q = 0; q <= Q; ++q) {
      if (Score::THETA_OPS_EVERY_ROUND || a.out_mean) {
        for (int k = tid; k < d; k += FB) {
          float m2, s2;
          theta_cand_ops(pf[1 + k], pf[d1 + 1 + k], SP, m2, s2);
          uth[k] = pf[1 + k]; uth[DP + k] = m2; uth[2 * DP + k] = s2;
        }
        if (tid == 0) {
          float m2, s2;
          theta_cand_ops(pf[0], pf[d1], SP, m2, s2);
          uth[3 * DP] = pf[0]; uth[3 * DP + 1] = s2;
        }
      }
      score.begin_round(q, rows, n);
      __syncthreads();                   // (the round's operands and the asked flags are read across the block)
      if (q == Q && !a.out_mean) break;

      // ---- score: thread t takes the pool rows t, t + FB, ..; its best by (score, position)
      float bs = 0.f;
      long long bp = -1;
      for (int64_t p = tid; p < np; p += FB) {
        const bool was = a.asked[p0 + p] != 0;
        if (was && !a.out_mean) continue;
        float sc = score.template pool_row<DP>(q, p0, p, was, eok, e, n, uth);
        if constexpr (Fold::ALL_PAIRS) {   // (a partner outside the base's range is never a candidate)
          if (!Fold::pool_ok(s, p0 + p)) sc = __builtin_nanf("");
        }
        if (!was && sc == sc && (bp < 0 || sc > bs)) { bs = sc; bp = p; }
      }
      if (q == Q) break;

      // ---- choose: a butterfly over the wave, then the waves' winners in wave order; a total order
#pragma unroll
      for (int off = WAVE / 2; off >= 1; off >>= 1) {
        const float os = __shfl_xor(bs, off, WAVE);
        const long long op = __shfl_xor(bp, off, WAVE);
        if (better(os, op, bs, bp)) { bs = os; bp = op; }
      }
      if (lane == 0) { rsc[wv] = bs; rpos[wv] = bp; }
      __syncthreads();
      bs = rsc[0]; bp = rpos[0];
#pragma unroll
      for (int w = 1; w < NW; ++w)
        if (better(rsc[w], rpos[w], bs, bp)) { bs = rsc[w]; bp = rpos[w]; }
      const bool act = eok && bp >= 0;   // (block-uniform)
      if (tid == 0) {
        a.out_row[g * Q + q] = act ? p0 + bp : -1;
        a.out_score[g * Q + q] = act ? bs : __builtin_nanf("");
        if (act) a.asked[p0 + bp] = 1;
        else a.out_loss[g * Q + q] = __builtin_nanf("");
      }
      __syncthreads();                   // (out_row: the asked row is fold row n from here on)

      // ---- fold in: the optimum over the history and the rows asked so far, from the rows themselves
      if (act) {
        ++n;
        int m;
        if constexpr (Fold::ALL_PAIRS) m = d1;              // (the base has full rank: always the primal system)
        else m = solve_dim(n, d);
        Fold::template run<W, CPL, LINK, PRIOR>(s, f, rows, n, g, sm, m <= s.sl.cap_dim ? Hl : Hg, fown, precf, prec,
                                                a.out_loss + g * Q + q, [&](const float*) { put_theta(q); }, pr);
      } else {
        put_theta(q);
      }
      if constexpr (Score::ROUND_END_BARRIER) __syncthreads();  // (solve_body's contract: begin_round writes its LDS again)
    }

    if (eok && a.write) {
      for (int k = tid; k < d; k += FB) {
        f.entity[e * 2 * d + k] = pf[1 + k];
        f.entity[e * 2 * d + d + k] = pf[d1 + 1 + k];
      }
      if (tid == 0) { f.bias[e * 2] = pf[0]; f.bias[e * 2 + 1] = pf[d1]; }
    }
    __syncthreads();                     // (pf and the score's own LDS are rewritten by the next respondent)
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side: what vfm_elicit_solve_f32 and vfm_design_elicit_f32 (and, but for the launch, vfm_design_scores_f32) share.
// P: vfm_elicit_solve_t or vfm_design_t, which name everything shared alike.
// workspace: [asked flags | the moments' operands | their constants | the fold-in's operand block and slabs]
// ---------------------------------------------------------------------------------------------------------------------
inline int64_t off_fold(int64_t P, int64_t n_ops, int d) { return flags_bytes(P) + sop_bytes(n_ops, d) + soc_bytes(n_ops); }

inline int64_t exact_session_workspace_bytes(int64_t U, int64_t P, int64_t n_ops, int32_t d, int32_t lds_dim) {
  if (U < 0 || P < 0 || n_ops < 0 || d < 1 || d > VFM_FOLDIN_MAX_D || lds_dim < -1) return VFM_E_INVALID;
  return off_fold(P, n_ops, d) + off_slabs(n_ops, d) + slabs_bytes(U, d, lds_dim);
}

// F and the respondents' column; the entry point's own columns follow
template <class P>
int check_exact_field(const P* p) {
  if (p->F < 2 || p->F > VFM_MAX_FIELDS) return fail(VFM_E_INVALID, "F out of range [2,64]");
  if (p->field < 0 || p->field >= p->F) return fail(VFM_E_INVALID, "field out of range [0,F)");
  return 0;
}

// d, the sizes (own_ok: the entry point's own sizes are all >= 0) and the rounds of a session
template <class P>
int check_exact_sizes(const P* p, bool own_ok, const char* sizes_msg, bool session) {
  if (p->d < 1 || p->d > VFM_FOLDIN_MAX_D) return fail(VFM_E_INVALID, "d out of range [1,512]");
  if (p->U < 0 || p->P < 0 || p->H < 0 || !own_ok) return fail(VFM_E_INVALID, sizes_msg);
  if (session && (p->n_rounds < 0 || p->n_rounds > VFM_ELICIT_MAX_ROUNDS))
    return fail(VFM_E_INVALID, "n_rounds out of range [0,4096]");
  return 0;
}

// the operand table (n_rows: the rows that name an operand), the options and a session's moments
template <class P>
int check_exact_options(const P* p, int64_t n_rows, const char* kl_msg, bool session) {
  if (p->n_ops < 0 || (n_rows > 0 && p->n_ops < 1)) return fail(VFM_E_INVALID, "n_ops out of range");
  if (p->flags & ~VFM_FLAG_LINK_SOFTPLUS) return fail(VFM_E_INVALID, "flags: only VFM_FLAG_LINK_SOFTPLUS is accepted");
  if (p->lds_dim < -1) return fail(VFM_E_INVALID, "lds_dim: -1 or >= 0");
  if (!(p->kl_weight > 0.f) || !(p->kl_weight <= 3.0e38f)) return fail(VFM_E_INVALID, kl_msg);
  if (session && (p->out_mean == nullptr) != (p->out_var == nullptr))
    return fail(VFM_E_INVALID, "out_mean and out_var: both or neither");
  return 0;
}

// the operands' pointers (need_op_x: does anything name an operand?) and the workspace
template <class P>
int check_exact_operands(const P* p, bool need_op_x, const char* small_msg) {
  if ((need_op_x && !p->op_x) || (p->P > 0 && !p->pool_op) || (p->H > 0 && !p->hist_op))
    return fail(VFM_E_INVALID, "op_x, pool_op and hist_op needed");
  return check_session_workspace(p, exact_session_workspace_bytes(p->U, p->P, p->n_ops, p->d, p->lds_dim), small_msg);
}

// The workspace carved up and the kernel arguments both forms name alike, from p.  A: ElicitSolveArgs or a struct
// derived from it; session: rounds, `reset`, `write` and the session's outputs count (else one round, nothing written);
// seed: of the random strategy.  operand_block false (the implicit session, whose fold reads the tables): the fold-in's
// operand block is absent -- its four pointers stay NULL -- and the slabs follow the score's constants directly.
// Returns the grid of the session kernel; the unit adds its score's own fields.
template <class A, class P>
unsigned exact_session_args(const P* p, bool session, uint64_t seed, A& s, bool operand_block = true) {
  const int64_t n_ops = p->n_ops;
  char* w = (char*)p->workspace + flags_bytes(p->P);
  float* sop = (float*)w;
  w += sop_bytes(n_ops, p->d);
  float* soc = (float*)w;
  w += soc_bytes(n_ops);                 // (w: the fold-in's operand block)
  s = {};
  ElicitFieldArgs& a = s.e;
  a.f = fill_fold_args(p->U, p->T, p->F, p->d, p->field, VFM_LIK_NORMAL, 1, 0, session && p->reset ? 1 : 0, VFM_FOLDIN_FIT,
                       0.f, p->kl_weight, 0, seed, p->entity_params, p->bias_params, p->scalars);
  a.U = p->U; a.P = p->P; a.H = p->H; a.n_ops = n_ops;
  a.Q = session ? p->n_rounds : 0; a.write = session && p->write ? 1 : 0;
  a.seed = seed;
  a.ents = p->entities; a.pool_ptr = p->pool_ptr; a.pool_x = p->pool_x; a.pool_y = p->pool_y;
  a.hist_ptr = p->H > 0 ? p->hist_ptr : nullptr; a.hist_x = p->hist_x; a.hist_y = p->hist_y;
  a.pool_op = p->pool_op; a.hist_op = p->hist_op;
  a.sop = sop; a.soc = soc;
  if (session) {
    a.out_row = p->out_row; a.out_score = p->out_score; a.out_loss = p->out_loss; a.out_theta = p->out_theta;
    a.out_mean = p->out_mean; a.out_var = p->out_var;
  }
  a.asked = (uint8_t*)p->workspace;
  if (!operand_block) return place_slabs(p->d, p->lds_dim, p->U, w, (int64_t)1 << 20, s.sl);
  a.f.ops = (const float*)w;
  a.f.opc = (const float*)(w + ops_off_opc(n_ops, p->d));
  s.ops64 = (const double*)(w + off_ops64(n_ops, p->d));
  s.cm64 = (const double*)(w + off_cm64(n_ops, p->d));
  return place_slabs(p->d, p->lds_dim, p->U, w + off_slabs(n_ops, p->d), (int64_t)1 << 20, s.sl);
}

// the operand passes, once, whatever the number of rounds: k_elicit_ctx_prep (the moments' operands), k_foldin_prep (the
// fold-in's fp32 operands, for the loss) and k_foldin_solve_prep (its fp64 operands)
template <class P>
int launch_exact_session_preps(const P* p, bool sp, const ElicitSolveArgs& s, hipStream_t st) {
  if (p->n_ops <= 0) return 0;
  const unsigned nb = (unsigned)((p->n_ops + NW - 1) / NW);
  hipLaunchKernelGGL(k_elicit_ctx_prep, dim3(nb), dim3(FB), 0, st, p->n_ops, p->op_x, (int)p->F, (int)p->field, p->T,
                     (int)p->d, sp, p->entity_params, p->bias_params, p->scalars, (float*)s.e.sop, (float*)s.e.soc);
  if (int rc = launch_status("k_elicit_ctx_prep")) return rc;
  return launch_solve_preps(sp, s.e.f, p->n_ops, p->op_x, (char*)s.e.f.ops, st);
}

// One launch of the session kernel.  kernel_of(IntC<W>, IntC<CPL>, IntC<LINK>): the unit's instance; extra: what the
// kernel takes behind s (the PRIOR instances: the prior, with prior_doubles = 2 (d + 1) more doubles of LDS in front).
template <class Score, class Fold = SolveFold, class Args, class KernelOf, class... Extra>
void launch_exact_session(bool sp, const Args& s, unsigned grid, hipStream_t st, KernelOf&& kernel_of,
                          int64_t prior_doubles = 0, const Extra&... extra) {
  const int d = s.e.f.d;
  for_link(sp, [&](auto link) {
    for_shape(shape_of(d), [&](auto w, auto c) {
      constexpr int DP = decltype(w)::value * decltype(c)::value;
      const size_t shm =
          (size_t)(prior_doubles + lds_doubles(d, s.sl.cap_dim) + Fold::lds_doubles(d) + Score::lds_doubles(d)) * 8 +
          (size_t)session_tail_bytes(DP);
      launch_lds(kernel_of(w, c, link), grid, shm, st, s, extra...);
    });
  });
}

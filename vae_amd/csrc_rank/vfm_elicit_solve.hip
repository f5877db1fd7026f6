// vfm_elicit_solve.hip -- the exact field-form elicitation session (include/vfm_elicit.h: vfm_elicit_solve_f32): ask,
// solve the respondent's closed-form optimum, ask again -- every round of every respondent in one launch.
//
// Operand passes, once, whatever the number of rounds: k_elicit_ctx_prep (the score's operands,
// vfm_elicit_field_score.hpp), k_foldin_prep (the fold-in's fp32 operands, for the loss) and k_foldin_solve_prep (its
// fp64 operands, vfm_foldin_solve_body.hpp).
// k_elicit_solve: k_foldin_solve's layout -- one workgroup of FB threads per respondent in a grid-stride loop (capped at
//   VFM_FOLDIN_SOLVE_SLABS blocks when slabs are needed), instantiated over <W, CPL, LINK> because the loss pass of the
//   solve needs the fold-in's lane groups.  theta_e lives in LDS (pf of solve_body) over all rounds.  Per round: the
//   candidate operands of theta_e [mu | mu^2 | sigma^2 | mu_w, sigma_w^2] are refreshed in LDS; thread t scores the
//   pool rows t, t + FB, .. whole (field_chain_moments / score_of / philox_uniform: vfm_elicit_field.hip's scores, bit
//   for bit); the best (score descending, position ascending) is reduced by a wave butterfly, then across the waves
//   through LDS -- a total order, so the tree does not matter; thread 0 records out_row, out_score and the asked flag;
//   after a barrier solve_body runs on the history followed by the rows asked so far, from the rows themselves (1 / D
//   changes with every appended row, so nothing of the system is carried over).  The table row is written once at the
//   end, and only with `write`.  No atomics.
//
// LDS of a block: k_foldin_solve's (64 (d + 1) bytes of vectors and the packed triangle of min(d + 1, 135, lds_dim))
// plus the reduction's words and 3 DP + 2 floats of candidate operands; larger systems go to the workgroup's slab.
// Everything a respondent reads from LDS or its slab is written for that respondent first.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "vfm_args.hpp"
#include "vfm_elicit.h"
#include "vfm_launch.hpp"            // launch_status
#include "vfm_rank_tile.hpp"         // score_of, philox_uniform, link_of
#include "vfm_field_ctx.hpp"         // ctx_valid, field_chain_moments

namespace vfm {
namespace {
#include "vfm_rng.hpp"
#include "vfm_common.hpp"
#include "vfm_foldin_body.hpp"       // FoldArgs, k_foldin_prep, fold_stage_rows, the host side
#include "vfm_foldin_solve_body.hpp" // solve_body, k_foldin_solve_prep, the operand block and the slabs
#include "vfm_elicit_host.hpp"       // the checks the session entry points share
#include "vfm_elicit_field_score.hpp" // k_elicit_ctx_prep, ElicitFieldArgs, FieldSessionRows, the score's operand views

struct ElicitSolveArgs {
  ElicitFieldArgs e;                     // (e.f.cap = 0; e.f.ops / e.f.opc: the fp32 operands of the loss)
  const double* ops64;                   // [n_ops, 3, d]  M | A | C, unrounded
  const double* cm64;                    // [n_ops]        c_mean
  double* slab;                          // [gridDim.x, slab_elems] or NULL when every system stays in LDS
  int64_t slab_elems;
  int32_t cap_dim;                       // systems up to this size live in LDS
};

constexpr int NW = FB / WAVE;            // waves of a block

// bytes of a block's LDS past k_foldin_solve's: the waves' winners (position, score) and the candidate operands
__host__ __device__ inline int64_t session_tail_bytes(int DP) { return NW * 8 + NW * 4 + (3 * (int64_t)DP + 2) * 4; }

// does (os, op) come before (bs, bp) in the order (score descending, position ascending)?  op < 0: no candidate
__device__ __forceinline__ bool better(float os, long long op, float bs, long long bp) {
  return op >= 0 && (bp < 0 || os > bs || (os == bs && op < bp));
}

template <int W, int CPL, int LINK>
__global__ __launch_bounds__(FB) void k_elicit_solve(const ElicitSolveArgs s) {
  extern __shared__ double sm[];
  constexpr int DP = W * CPL;
  constexpr bool SP = LINK == LINK_SOFTPLUS;
  const ElicitFieldArgs& a = s.e;
  const FoldArgs& f = a.f;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int d = f.d, d1 = d + 1, Q = a.Q, F = f.F;
  float* pf = (float*)(sm + 7 * d1);     // theta_e: mu_w, mu [d] | s_w, s [d]  (solve_body's)
  double* Hl = sm + 8 * d1;
  long long* rpos = (long long*)(Hl + tri(s.cap_dim));      // [NW] the waves' winners
  float* rsc = (float*)(rpos + NW);                         // [NW]
  float* uth = rsc + NW;                                    // [3 DP + 2] the candidate operands of theta_e
  double* Hg = s.slab ? s.slab + (int64_t)blockIdx.x * s.slab_elems : nullptr;
  const float precf = link_f<LINK>(f.scal[0]);
  const double prec = link_d<LINK>(f.scal[0]);

  for (int64_t g = blockIdx.x; g < a.U; g += gridDim.x) {
    const int64_t p0 = min(max(a.pool_ptr[g], (int64_t)0), a.P);
    const int64_t np = min(max(a.pool_ptr[g + 1], p0), a.P) - p0;
    int64_t h0 = 0, nh = 0;
    if (a.hist_ptr) {
      h0 = min(max(a.hist_ptr[g], (int64_t)0), a.H);
      nh = min(max(a.hist_ptr[g + 1], h0), a.H) - h0;
    }
    const int64_t e = a.ents[g];
    const bool eok = e >= 0 && e < f.T;                     // (block-uniform)
    const FieldSessionRows rows{a, h0, nh, a.out_row + g * Q};

    // ---- theta_e: the table row, or the prior
    for (int c = tid; c < d1; c += FB) {
      float m = 0.f, sp = prior_s<LINK>();
      if (eok && !f.reset) {
        m = c == 0 ? f.bias[e * 2] : f.entity[e * 2 * d + (c - 1)];
        sp = c == 0 ? f.bias[e * 2 + 1] : f.entity[e * 2 * d + d + (c - 1)];
      }
      pf[c] = m;
      pf[d1 + c] = sp;
    }
    for (int64_t p = tid; p < np; p += FB) a.asked[p0 + p] = 0;
    int64_t n = nh;
    __syncthreads();

    const auto put_theta = [&](int q) {                     // theta_e after round q, by every thread
      if (!a.out_theta) return;
      float* to = a.out_theta + (g * Q + q) * (2 * (int64_t)d + 2);
      for (int k = tid; k < d; k += FB) { to[k] = pf[1 + k]; to[d + k] = pf[d1 + 1 + k]; }
      if (tid == 0) { to[2 * d] = pf[0]; to[2 * d + 1] = pf[d1]; }
    };

    for (int q = 0; q <= Q; ++q) {
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
      __syncthreads();                   // (uth and the asked flags are read across the block)
      if (q == Q && !a.out_mean) break;

      // ---- score: thread t takes the pool rows t, t + FB, ..; its best by (score, position)
      float bs = 0.f;
      long long bp = -1;
      for (int64_t p = tid; p < np; p += FB) {
        const bool was = a.asked[p0 + p] != 0;
        if (was && !a.out_mean) continue;
        const int64_t* xr = a.pool_x + (p0 + p) * F;
        const int64_t o = a.pool_op[p0 + p];
        float mean = __builtin_nanf(""), var = __builtin_nanf(""), sc = __builtin_nanf("");
        if (eok && o >= 0 && o < a.n_ops && ctx_valid(xr, F, f.col, f.T)) {
          if (a.strat != VFM_RANK_RANDOM || a.out_mean)
            field_chain_moments(CtxRowOp{a.sop + o * 4 * (int64_t)d, d}, ThetaCand{uth, DP}, a.soc[o * 2], a.soc[o * 2 + 1],
                                d, mean, var);
          sc = a.strat == VFM_RANK_RANDOM ? philox_uniform(a.seed + (uint64_t)q, xr[a.key_col], e)
                                          : score_of(a.strat, mean, var);
        }
        if (a.out_mean) {
          a.out_mean[(int64_t)q * a.P + p0 + p] = mean;
          a.out_var[(int64_t)q * a.P + p0 + p] = var;
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
        const int m = solve_dim(n, d);
        solve_body<W, CPL, LINK>(f, s.ops64, s.cm64, rows, n, sm, m <= s.cap_dim ? Hl : Hg, precf, prec,
                                 a.out_loss + g * Q + q, [&](const float*) { put_theta(q); });
      } else {
        put_theta(q);
      }
    }

    if (eok && a.write) {
      for (int k = tid; k < d; k += FB) {
        f.entity[e * 2 * d + k] = pf[1 + k];
        f.entity[e * 2 * d + d + k] = pf[d1 + 1 + k];
      }
      if (tid == 0) { f.bias[e * 2] = pf[0]; f.bias[e * 2 + 1] = pf[d1]; }
    }
    __syncthreads();                     // (pf is rewritten by the next respondent)
  }
}

void launch(const FShape& sh, bool sp, const ElicitSolveArgs& s, unsigned grid, hipStream_t st) {
  for_link(sp, [&](auto link) {
    for_shape(sh, [&](auto w, auto c) {
      constexpr int DP = decltype(w)::value * decltype(c)::value;
      const size_t shm = (size_t)lds_doubles(s.e.f.d, s.cap_dim) * 8 + (size_t)session_tail_bytes(DP);
      const auto k = k_elicit_solve<decltype(w)::value, decltype(c)::value, decltype(link)::value>;
      // (more than 64 KiB of dynamic LDS: state the size; a runtime that needs no opt-in ignores it)
      (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
      (void)hipGetLastError();
      hipLaunchKernelGGL(k, dim3(grid), dim3(FB), shm, st, s);
    });
  });
}

// workspace: [asked flags | score operands | their constants | the fold-in's operand block and slabs]
inline int64_t off_fold(int64_t P, int64_t n_ops, int d) { return flags_bytes(P) + sop_bytes(n_ops, d) + soc_bytes(n_ops); }

}  // namespace
}  // namespace vfm

extern "C" {

int64_t vfm_elicit_solve_workspace_bytes(int64_t U, int64_t P, int64_t n_ops, int32_t d, int32_t lds_dim) {
  if (U < 0 || P < 0 || n_ops < 0 || d < 1 || d > VFM_FOLDIN_MAX_D || lds_dim < -1) return VFM_E_INVALID;
  int64_t b = vfm::off_fold(P, n_ops, d) + vfm::off_slabs(n_ops, d);
  if (d + 1 > vfm::cap_dim_of(d, lds_dim))
    b += (U < VFM_FOLDIN_SOLVE_SLABS ? U : VFM_FOLDIN_SOLVE_SLABS) * vfm::slab_bytes(d);
  return b;
}

int vfm_elicit_solve_f32(const vfm_elicit_solve_t* p, void* stream) {
  using namespace vfm;
  if (int rc = check_session_struct(
          p, "vfm_elicit_solve_f32: NULL argument struct",
          "vfm_elicit_solve_t: struct_size / abi_version differ from this library's (VFM_STRUCT_INIT)"))
    return rc;
  if (p->F < 2 || p->F > VFM_MAX_FIELDS) return fail(VFM_E_INVALID, "F out of range [2,64]");
  if (p->field < 0 || p->field >= p->F) return fail(VFM_E_INVALID, "field out of range [0,F)");
  if (p->key_col < 0 || p->key_col >= p->F || p->key_col == p->field)
    return fail(VFM_E_INVALID, "key_col must be a context column: in [0,F) and not field");
  if (p->d < 1 || p->d > VFM_FOLDIN_MAX_D) return fail(VFM_E_INVALID, "d out of range [1,512]");
  if (p->U < 0 || p->P < 0 || p->H < 0) return fail(VFM_E_INVALID, "U < 0, P < 0 or H < 0");
  if (p->n_rounds < 0 || p->n_rounds > VFM_ELICIT_MAX_ROUNDS) return fail(VFM_E_INVALID, "n_rounds out of range [0,4096]");
  if (p->strategy < VFM_RANK_TOP || p->strategy > VFM_RANK_RANDOM) return fail(VFM_E_INVALID, "unknown strategy");
  if (p->n_ops < 0 || (p->P + p->H > 0 && p->n_ops < 1)) return fail(VFM_E_INVALID, "n_ops out of range");
  if (p->flags & ~VFM_FLAG_LINK_SOFTPLUS) return fail(VFM_E_INVALID, "flags: only VFM_FLAG_LINK_SOFTPLUS is accepted");
  if (p->lds_dim < -1) return fail(VFM_E_INVALID, "lds_dim: -1 or >= 0");
  if (!(p->kl_weight > 0.f) || !(p->kl_weight <= 3.0e38f))
    return fail(VFM_E_INVALID, "kl_weight must be > 0 and finite (the prior is what makes the system positive definite)");
  if ((p->out_mean == nullptr) != (p->out_var == nullptr))
    return fail(VFM_E_INVALID, "out_mean and out_var: both or neither");
  if (p->U == 0) return 0;
  if (!p->entities || (p->P > 0 && !p->pool_x) || (p->H > 0 && !p->hist_x) || session_pointers_missing(p))
    return fail(VFM_E_INVALID, "null pointer");
  if ((p->P + p->H > 0 && !p->op_x) || (p->P > 0 && !p->pool_op) || (p->H > 0 && !p->hist_op))
    return fail(VFM_E_INVALID, "op_x, pool_op and hist_op needed");
  const int64_t n_ops = p->n_ops;
  if (int rc = check_session_workspace(p, vfm_elicit_solve_workspace_bytes(p->U, p->P, n_ops, p->d, p->lds_dim),
                                       "workspace too small (vfm_elicit_solve_workspace_bytes)"))
    return rc;

  const hipStream_t st = (hipStream_t)stream;
  const bool sp = (p->flags & VFM_FLAG_LINK_SOFTPLUS) != 0;
  const FShape sh = shape_of(p->d);
  char* w = (char*)p->workspace + flags_bytes(p->P);
  float* sop = (float*)w;
  w += sop_bytes(n_ops, p->d);
  float* soc = (float*)w;
  w += soc_bytes(n_ops);                 // (w: the fold-in's operand block)

  ElicitSolveArgs s = {};
  ElicitFieldArgs& a = s.e;
  a.f = fill_fold_args(p->U, p->T, p->F, p->d, p->field, VFM_LIK_NORMAL, 1, 0, p->reset ? 1 : 0, VFM_FOLDIN_FIT, 0.f,
                       p->kl_weight, 0, p->seed, p->entity_params, p->bias_params, p->scalars);
  a.U = p->U; a.P = p->P; a.H = p->H; a.n_ops = n_ops;
  a.Q = p->n_rounds; a.strat = p->strategy; a.write = p->write ? 1 : 0; a.key_col = p->key_col;
  a.seed = p->seed;
  a.ents = p->entities; a.pool_ptr = p->pool_ptr; a.pool_x = p->pool_x; a.pool_y = p->pool_y;
  a.hist_ptr = p->H > 0 ? p->hist_ptr : nullptr; a.hist_x = p->hist_x; a.hist_y = p->hist_y;
  a.pool_op = p->pool_op; a.hist_op = p->hist_op;
  a.sop = sop; a.soc = soc;
  a.out_row = p->out_row; a.out_score = p->out_score; a.out_loss = p->out_loss; a.out_theta = p->out_theta;
  a.out_mean = p->out_mean; a.out_var = p->out_var;
  a.asked = (uint8_t*)p->workspace;
  a.f.ops = (const float*)w;
  a.f.opc = (const float*)(w + ops_off_opc(n_ops, p->d));
  s.ops64 = (const double*)(w + off_ops64(n_ops, p->d));
  s.cm64 = (const double*)(w + off_cm64(n_ops, p->d));
  s.cap_dim = cap_dim_of(p->d, p->lds_dim);
  const bool slabs = p->d + 1 > s.cap_dim;
  s.slab = slabs ? (double*)(w + off_slabs(n_ops, p->d)) : nullptr;
  s.slab_elems = slab_bytes(p->d) / 8;
  const int64_t gmax = slabs ? VFM_FOLDIN_SOLVE_SLABS : ((int64_t)1 << 20);
  const unsigned grid = (unsigned)(p->U < gmax ? p->U : gmax);

  if (n_ops > 0) {
    const unsigned nb = (unsigned)((n_ops + NW - 1) / NW);
    hipLaunchKernelGGL(k_elicit_ctx_prep, dim3(nb), dim3(FB), 0, st, n_ops, p->op_x, (int)p->F, (int)p->field, p->T,
                       (int)p->d, sp, p->entity_params, p->bias_params, p->scalars, sop, soc);
    if (int rc = launch_status("k_elicit_ctx_prep")) return rc;
    if (int rc = launch_solve_preps(sp, a.f, n_ops, p->op_x, w, st)) return rc;
  }
  launch(sh, sp, s, grid, st);
  return launch_status("k_elicit_solve");
}

}  // extern "C"

// vfm_rank_eval.hip -- held-out ranking evaluation (include/vfm_rank.h: vfm_rank_heldout_f32): the exact position of
// every held-out positive in its user's full catalog ranking, in the order of vfm_rank_items_f32.
//   k_eval_pos_score -> k_eval_pos_sort:  each user's positives, scored and sorted best first
//   k_rank_prep -> k_rank_eval:           the score tiles of k_rank, scanned into per-(split, user) histograms
//   k_rank_eval_merge:                    splits summed, prefix sums -> rank, rank_neg; n_eligible, n_neg
// The sort, the scan and the merge are instantiated here only; the field form (vfm_rank_field.hip) scores its positives
// and packs its operands itself and launches the three through vfm::launch_rank_eval (vfm_rank_eval.hpp).
//
// Compiled with -ffp-contract=off (as vfm_rank.hip): the positives' scores (pair_moments) and the tile scores (MFMA) are
// the same k-ordered fp32 fma chains, so a candidate compares with a positive exactly as rank_items orders them.
// Everything past the scores is integer counting: the results do not depend on the split count, the grid or the stream.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "vfm_rank.h"
#include "vfm_rank_tile.hpp"        // pair scores, operand packing (k_rank_prep), the MFMA score tile
#include "vfm_rank_eval.hpp"        // the launch other operand forms share, the eval tail, segment_of, pos_row_of

namespace {

constexpr int MERGE_WAVE = 64;      // k_rank_eval_merge: one wave per user

// ---------------------------------------------------------------------------------------------------------------------
// k_eval_pos_score: one thread per positive p: its user (the row of pos_ptr holding p) and the strategy's score of the
// pair, as k_moments forms it (NaN for an id outside [0, T)).
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(POS_BLOCK) void k_eval_pos_score(int64_t U, int64_t n_pos, const int64_t* __restrict__ users,
                                                              const int64_t* __restrict__ pos_ptr,
                                                              const int64_t* __restrict__ pos_items, int64_t T, int d,
                                                              bool sp, int strat, uint64_t seed,
                                                              const float* __restrict__ ent,
                                                              const float* __restrict__ bias,
                                                              const float* __restrict__ scal, float* __restrict__ raw,
                                                              int64_t* __restrict__ pusr) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pos) return;
  int64_t row;
  const int64_t lo = pos_row_of(pos_ptr, U, n_pos, p, row);
  pusr[p] = row;
  const int64_t uid = users[lo], iid = pos_items[p];
  float sc = __builtin_nanf("");
  if (uid >= 0 && uid < T && iid >= 0 && iid < T) {
    if (strat == VFM_RANK_RANDOM) {
      sc = philox_uniform(seed, uid, iid);
    } else {
      float m, v;
      pair_moments(ent + uid * 2 * d, ent + iid * 2 * d, bias + uid * 2, bias + iid * 2, scal[1], link_of(scal[2], sp), d,
                   sp, m, v);
      sc = score_of(strat, m, v);
    }
  }
  raw[p] = sc;
}

// ---------------------------------------------------------------------------------------------------------------------
// k_eval_pos_sort: one thread per positive p: its position r in its user's positives sorted best first (the ranking
// order; equal (score, id) pairs by index) by counting the ones ahead of it, O(n_u) per positive.  Writes the sorted
// (score, id) at lo + r and p's slot lo + r (-1 for a positive outside its row's segment).
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(POS_BLOCK) void k_eval_pos_sort(int64_t n_pos, const int64_t* __restrict__ pos_ptr,
                                                             const int64_t* __restrict__ pos_items,
                                                             const float* __restrict__ raw,
                                                             const int64_t* __restrict__ pusr, float* __restrict__ pscore,
                                                             int64_t* __restrict__ pid, int64_t* __restrict__ slot) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pos) return;
  const int64_t u = pusr[p];
  if (u < 0) { slot[p] = -1; return; }
  int64_t lo, hi;
  segment_of(pos_ptr, u, n_pos, lo, hi);
  const float s = raw[p];
  const int64_t id = pos_items[p];
  int64_t r = 0;
  for (int64_t q = lo; q < hi; ++q) {
    const float sq = raw[q];
    const int64_t iq = pos_items[q];
    r += beats(sq, iq, s, id) || (sq == s && iq == id && q < p);
  }
  slot[p] = lo + r;
  pscore[lo + r] = s;
  pid[lo + r] = id;
}

struct EvalArgs {
  int64_t U, n_cand, item_lo, n_excl, n_pos;
  const int64_t *users, *cand, *excl_ptr, *excl_items, *pos_ptr, *pos_items;
  const float* pscore;                     // [n_pos] each user's positives, best first
  const int64_t* pid;
  int *hist_all, *hist_neg;                // [S, n_pos]: per (split, user) over the user's segment
  int *cnt_el, *cnt_pos;                   // [S, U]
  TileOps ops;
  int n_tiles, S;
  uint64_t seed;
};

// ---------------------------------------------------------------------------------------------------------------------
// k_rank_eval: the grid and score tiles of k_rank (workgroup = 256 users x an item split).  Each thread walks its user's
// column in item order: the exclusion cursor; a cursor over the user's positive ids (ascending) that marks a candidate
// as a positive; a register compare against the user's last positive (a candidate that does not beat it moves no rank);
// else f = the first positive in the sorted list the candidate beats (register compare against the first, then a binary
// search), counted in hist_all[f] and, for a negative, hist_neg[f].  Each histogram belongs to one thread: no atomics.
// ---------------------------------------------------------------------------------------------------------------------
template <int STRAT>
__global__ __launch_bounds__(256, 2) void k_rank_eval(EvalArgs a) {
  __shared__ TileSmem sm;
  __shared__ float ci_m[IT], ci_v[IT];
  const int tid = threadIdx.x;
  const int64_t u0 = (int64_t)blockIdx.x * UT, u = u0 + tid;
  const int s = blockIdx.y;
  const bool uvalid = u < a.U;
  const int t_lo = (int)((int64_t)s * a.n_tiles / a.S), t_hi = (int)((int64_t)(s + 1) * a.n_tiles / a.S);
  int64_t cx = 0, cx_end = 0, ex = INT64_MAX, uid = 0;
  int64_t pc = 0, pc_end = 0, pnext = INT64_MAX, plo = 0;
  int np = 0;
  float hi_s = 0.f, lo_s = 0.f;
  int64_t hi_id = 0, lo_id = 0;
  int *ha = nullptr, *hn = nullptr;
  if (uvalid) {
    if (a.excl_ptr) {
      cx = min(max(a.excl_ptr[u], (int64_t)0), a.n_excl);
      cx_end = min(max(a.excl_ptr[u + 1], cx), a.n_excl);
      ex = cx < cx_end ? a.excl_items[cx] : INT64_MAX;
    }
    segment_of(a.pos_ptr, u, a.n_pos, pc, pc_end);
    plo = pc;
    np = (int)min(pc_end - pc, (int64_t)INT32_MAX);
    pnext = pc < pc_end ? a.pos_items[pc] : INT64_MAX;
    ha = a.hist_all + (int64_t)s * a.n_pos + plo;
    hn = a.hist_neg + (int64_t)s * a.n_pos + plo;
    for (int j = 0; j < np; ++j) { ha[j] = 0; hn[j] = 0; }
    if (np > 0) {
      hi_s = a.pscore[plo]; hi_id = a.pid[plo];
      lo_s = a.pscore[plo + np - 1]; lo_id = a.pid[plo + np - 1];
    }
    uid = a.users[u];
  }
  int n_el = 0, n_ps = 0;
  float ucm[2], ucv[2];
  tile_user_consts<STRAT>(a.ops, u0, tid, ucm, ucv);
  for (int t = t_lo; t < t_hi; ++t) {
    const int64_t c0 = (int64_t)t * IT;
    if constexpr (STRAT != VFM_RANK_RANDOM) score_tile<STRAT>(a.ops, sm, ci_m, ci_v, u0, c0, tid, ucm, ucv);
    if (uvalid) {
      const int jn = (int)min((int64_t)IT, a.n_cand - c0);
      for (int j = 0; j < jn; ++j) {
        const int c = (int)(c0 + j);
        const int64_t id = a.cand ? a.cand[c] : a.item_lo + c;
        while (ex < id) {
          ++cx;
          ex = cx < cx_end ? a.excl_items[cx] : INT64_MAX;
        }
        if (ex == id) continue;
        while (pnext < id) {
          ++pc;
          pnext = pc < pc_end ? a.pos_items[pc] : INT64_MAX;
        }
        const bool is_pos = pnext == id;
        ++n_el;
        n_ps += is_pos;
        if (np == 0) continue;
        float sc;
        if constexpr (STRAT == VFM_RANK_RANDOM) sc = philox_uniform(a.seed, uid, id);
        else sc = sm.S[j][tid];
        if (!beats(sc, id, lo_s, lo_id)) continue;
        int f = 0;
        if (!beats(sc, id, hi_s, hi_id)) {      // then 1 <= f <= np - 1
          int lo = 1, hi = np - 1;
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (beats(sc, id, a.pscore[plo + mid], a.pid[plo + mid])) hi = mid;
            else lo = mid + 1;
          }
          f = lo;
        }
        ha[f] += 1;
        if (!is_pos) hn[f] += 1;
      }
    }
  }
  if (uvalid) {
    a.cnt_el[(int64_t)s * a.U + u] = n_el;
    a.cnt_pos[(int64_t)s * a.U + u] = n_ps;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// k_rank_eval_merge: one wave per user.  Sums the splits' histograms and prefix-sums them over the sorted positives
// (into split 0's rows), then gives each positive the count at its slot: rank = #{eligible c beating it},
// rank_neg = #{eligible negatives beating it}.  n_eligible and n_neg from the splits' counters.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MERGE_WAVE) void k_rank_eval_merge(int64_t U, int S, int64_t n_pos,
                                                                const int64_t* __restrict__ pos_ptr, int* hist_all,
                                                                int* hist_neg, const int* __restrict__ cnt_el,
                                                                const int* __restrict__ cnt_pos,
                                                                const int64_t* __restrict__ slot,
                                                                int64_t* __restrict__ out_rank,
                                                                int64_t* __restrict__ out_rank_neg,
                                                                int64_t* __restrict__ out_n_eligible,
                                                                int64_t* __restrict__ out_n_neg) {
  const int64_t u = blockIdx.x;
  const int lane = threadIdx.x;
  int64_t lo, hi;
  segment_of(pos_ptr, u, n_pos, lo, hi);
  int carry_a = 0, carry_n = 0;
  for (int64_t base = lo; base < hi; base += MERGE_WAVE) {
    const int64_t j = base + lane;
    int ta = 0, tn = 0;
    if (j < hi)
      for (int sp = 0; sp < S; ++sp) {
        ta += hist_all[(int64_t)sp * n_pos + j];
        tn += hist_neg[(int64_t)sp * n_pos + j];
      }
#pragma unroll
    for (int off = 1; off < MERGE_WAVE; off <<= 1) {      // inclusive scan over the wave
      const int ya = __shfl_up(ta, off), yn = __shfl_up(tn, off);
      if (lane >= off) { ta += ya; tn += yn; }
    }
    ta += carry_a;
    tn += carry_n;
    if (j < hi) { hist_all[j] = ta; hist_neg[j] = tn; }
    carry_a = __shfl(ta, MERGE_WAVE - 1);
    carry_n = __shfl(tn, MERGE_WAVE - 1);
  }
  __syncthreads();
  for (int64_t p = lo + lane; p < hi; p += MERGE_WAVE) {
    const int64_t sl = slot[p];
    const bool ok = sl >= lo && sl < hi;
    out_rank[p] = ok ? hist_all[sl] : -1;
    out_rank_neg[p] = ok ? hist_neg[sl] : -1;
  }
  if (lane == 0) {
    int64_t el = 0, ps = 0;
    for (int sp = 0; sp < S; ++sp) {
      el += cnt_el[(int64_t)sp * U + u];
      ps += cnt_pos[(int64_t)sp * U + u];
    }
    out_n_eligible[u] = el;
    out_n_neg[u] = el - ps;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
struct EvalLayout : OpLayout, EvalTail {};

EvalLayout eval_layout_of(int64_t U, int64_t n_cand, int64_t n_pos, int d, int strategy, int n_splits) {
  EvalLayout L;
  static_cast<OpLayout&>(L) = op_layout_of(U, n_cand, d, strategy, n_splits);
  static_cast<EvalTail&>(L) = eval_tail_of(L.end, L.S, U, n_pos);
  return L;
}

}  // namespace

int vfm::launch_rank_eval(const RankEval& r, int strategy, unsigned n_query_tiles, hipStream_t st) {
  if (r.n_pos > 0) {
    const unsigned nb = (unsigned)((r.n_pos + POS_BLOCK - 1) / POS_BLOCK);
    hipLaunchKernelGGL(k_eval_pos_sort, dim3(nb), dim3(POS_BLOCK), 0, st, r.n_pos, r.pos_ptr, r.pos_items, r.raw, r.pusr,
                       r.pscore, r.pid, r.slot);
    if (int rc = launch_status("k_eval_pos_sort")) return rc;
  }
  EvalArgs a;
  a.U = r.U; a.n_cand = r.n_cand; a.item_lo = r.item_lo; a.n_excl = r.n_excl; a.n_pos = r.n_pos;
  a.users = r.keys; a.cand = r.cand; a.excl_ptr = r.excl_ptr; a.excl_items = r.excl_items;
  a.pos_ptr = r.pos_ptr; a.pos_items = r.pos_items;
  a.pscore = r.pscore; a.pid = r.pid;
  a.hist_all = r.hist_all; a.hist_neg = r.hist_neg;
  a.cnt_el = r.cnt_el; a.cnt_pos = r.cnt_pos;
  a.ops = TileOps{r.uop, r.iop, r.ucon, r.icon, r.Kp, r.KA, r.KB};
  a.n_tiles = r.n_tiles; a.S = r.S; a.seed = r.seed;
  const dim3 grid(n_query_tiles, (unsigned)r.S);
  switch (strategy) {
    case VFM_RANK_TOP: hipLaunchKernelGGL(k_rank_eval<VFM_RANK_TOP>, grid, dim3(256), 0, st, a); break;
    case VFM_RANK_VARIANCE: hipLaunchKernelGGL(k_rank_eval<VFM_RANK_VARIANCE>, grid, dim3(256), 0, st, a); break;
    case VFM_RANK_MEAN: hipLaunchKernelGGL(k_rank_eval<VFM_RANK_MEAN>, grid, dim3(256), 0, st, a); break;
    default: hipLaunchKernelGGL(k_rank_eval<VFM_RANK_RANDOM>, grid, dim3(256), 0, st, a); break;
  }
  if (int rc = launch_status("k_rank_eval")) return rc;
  hipLaunchKernelGGL(k_rank_eval_merge, dim3((unsigned)r.U), dim3(MERGE_WAVE), 0, st, r.U, r.S, r.n_pos, r.pos_ptr,
                     r.hist_all, r.hist_neg, r.cnt_el, r.cnt_pos, r.slot, r.out_rank, r.out_rank_neg, r.out_n_eligible,
                     r.out_n_neg);
  return launch_status("k_rank_eval_merge");
}

extern "C" {

int64_t vfm_rank_eval_workspace_bytes(int64_t U, int64_t n_cand, int64_t n_pos, int32_t d, int32_t strategy,
                                      int32_t n_splits) {
  if (!eval_sizes_ok(U, n_cand, n_pos) || d < 1 || d > 4096 || strategy < VFM_RANK_TOP || strategy > VFM_RANK_RANDOM ||
      n_splits < 0 || n_splits > VFM_RANK_MAX_SPLITS)
    return VFM_E_INVALID;
  return eval_layout_of(U, n_cand, n_pos, d, strategy, n_splits).bytes;
}

int vfm_rank_heldout_f32(int64_t U, const int64_t* users, int64_t n_cand, const int64_t* cand, int64_t item_lo,
                         int64_t T, int32_t F, int32_t d, int32_t strategy, int32_t flags, uint64_t seed,
                         int32_t n_splits, const int64_t* excl_ptr, const int64_t* excl_items, int64_t n_excl,
                         const int64_t* pos_ptr, const int64_t* pos_items, int64_t n_pos,
                         const float* entity_params, const float* bias_params, const float* scalars, void* workspace,
                         int64_t workspace_bytes, int64_t* out_rank, int64_t* out_rank_neg, int64_t* out_n_eligible,
                         int64_t* out_n_neg, void* stream) {
  RankCall r;
  r.Q = U; r.queries = users;
  r.n_cand = n_cand; r.cand = cand; r.cand_lo = item_lo;
  r.excl_ptr = excl_ptr; r.excl_items = excl_items; r.n_excl = n_excl;
  r.pos_ptr = pos_ptr; r.pos_items = pos_items; r.n_pos = n_pos;
  r.T = T; r.F = F; r.d = d; r.ent = entity_params; r.bias = bias_params; r.scal = scalars;
  r.workspace = workspace; r.workspace_bytes = workspace_bytes;
  r.strategy = strategy; r.flags = flags; r.n_splits = n_splits; r.seed = seed;
  r.out_rank = out_rank; r.out_rank_neg = out_rank_neg; r.out_n_eligible = out_n_eligible; r.out_n_neg = out_n_neg;
  r.stream = (hipStream_t)stream;
  if (int rc = check_common(T, d, flags, strategy)) return rc;
  if (F != 2) return vfm::fail(VFM_E_INVALID, "rank_heldout: two-field models only (F == 2)");
  if (int rc = check_rank_call(r, RANK_ASK_HELDOUT)) return rc;
  if (U == 0) return 0;
  const EvalLayout L = eval_layout_of(U, n_cand, n_pos, d, strategy, n_splits);
  if (int rc = check_rank_workspace(r, L.bytes, "workspace too small (vfm_rank_eval_workspace_bytes)")) return rc;

  char* ws = (char*)workspace;
  if (n_pos > 0) {
    const unsigned nb = (unsigned)((n_pos + POS_BLOCK - 1) / POS_BLOCK);
    hipLaunchKernelGGL(k_eval_pos_score, dim3(nb), dim3(POS_BLOCK), 0, r.stream, U, n_pos, users, pos_ptr, pos_items, T,
                       d, r.softplus(), strategy, seed, entity_params, bias_params, scalars, (float*)(ws + L.off_raw),
                       (int64_t*)(ws + L.off_pusr));
    if (int rc = launch_status("k_eval_pos_score")) return rc;
  }
  if (strategy != VFM_RANK_RANDOM)
    if (int rc = launch_rank_prep(L, r)) return rc;
  return eval_after_scores(r, L, users);
}

}  // extern "C"

// vfm_rank_eval.hpp -- what the two-field held-out evaluation (vfm_rank_eval.hip) and its field form
// (vfm_rank_field.hip: vfm_rank_heldout_field_f32) share past the positives' raw scores: one launch sequence
//   k_eval_pos_sort -> k_rank_eval<strategy> -> k_rank_eval_merge
// (all three instantiated in vfm_rank_eval.hip only), the eval tail of the workspace behind the operand blocks, and the
// row search of the per-positive kernels.  Like the ranking scan (vfm_rank_scan.hpp), k_rank_eval reads nothing but
// packed operands (TileOps), the candidate ids, the two CSRs and one int64 key per query (the Philox key of
// VFM_RANK_RANDOM), so it serves any operand form whose score is
//   (query operand . candidate operand + query constant) + candidate constant   per part (mean, variance).
#pragma once

#include "vfm_rank_tile.hpp"

namespace vfm {

// One evaluation past the positives' scores, in plain fields (an external-linkage mirror of EvalArgs of
// vfm_rank_eval.hip plus the buffers of the sort and the merge)
struct RankEval {
  int64_t U, n_cand, item_lo, n_excl, n_pos;
  const int64_t *keys, *cand, *excl_ptr, *excl_items;      // keys [U]: the query's Philox key (two fields: the user id)
  const int64_t *pos_ptr, *pos_items;                      // the positives CSR over the queries
  const float *uop, *iop, *ucon, *icon;                     // packed operands [U_pad | C_pad, Kp], constants [.., 2]
  int Kp, KA, KB;
  const float* raw;                                         // [n_pos] the positives' scores (the caller's kernel wrote them)
  const int64_t* pusr;                                      // [n_pos] the positives' query rows (-1: outside its segment)
  float* pscore;                                            // [n_pos] the eval tail: each query's positives, best first
  int64_t *pid, *slot;                                      // [n_pos]
  int *hist_all, *hist_neg;                                 // [S, n_pos]
  int *cnt_el, *cnt_pos;                                    // [S, U]
  int n_tiles, S;
  uint64_t seed;
  int64_t *out_rank, *out_rank_neg, *out_n_eligible, *out_n_neg;
};

// k_eval_pos_sort (n_pos > 0), k_rank_eval<strategy> over grid (n_query_tiles, S), k_rank_eval_merge, on `st`
// (vfm_rank_eval.hip)
int launch_rank_eval(const RankEval& a, int strategy, unsigned n_query_tiles, hipStream_t st);

}  // namespace vfm

namespace {

constexpr int POS_BLOCK = 256;      // per-positive kernels

// The clamped CSR segment [lo, hi) of row u (a malformed ptr array gives wrong counts, never an access out of range)
__device__ __forceinline__ void segment_of(const int64_t* ptr, int64_t u, int64_t n, int64_t& lo, int64_t& hi) {
  lo = min(max(ptr[u], (int64_t)0), n);
  hi = min(max(ptr[u + 1], lo), n);
}

// The row of pos_ptr [U+1] holding positive p (the last row whose offset is <= p), and in `pusr` that row, or -1 when p
// lies outside the row's clamped segment
__device__ __forceinline__ int64_t pos_row_of(const int64_t* __restrict__ pos_ptr, int64_t U, int64_t n_pos, int64_t p,
                                              int64_t& pusr) {
  int64_t lo = 0, hi = U - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (pos_ptr[mid] <= p) lo = mid;
    else hi = mid - 1;
  }
  int64_t s0, s1;
  segment_of(pos_ptr, lo, n_pos, s0, s1);
  pusr = (p >= s0 && p < s1) ? lo : -1;
  return lo;
}

// The eval tail of a workspace, behind the operand blocks: O(S (U + n_pos))
struct EvalTail {
  int64_t off_pscore, off_pid, off_raw, off_pusr, off_slot, off_ha, off_hn, off_cel, off_cpos, bytes;
};

inline EvalTail eval_tail_of(int64_t ops_end, int S, int64_t U, int64_t n_pos) {
  EvalTail L;
  int64_t off = ops_end;
  auto take = [&](int64_t bytes) { const int64_t o = off; off += round_up(bytes, 256); return o; };
  L.off_pscore = take(n_pos * 4);
  L.off_pid = take(n_pos * 8);
  L.off_raw = take(n_pos * 4);
  L.off_pusr = take(n_pos * 8);
  L.off_slot = take(n_pos * 8);
  L.off_ha = take((int64_t)S * n_pos * 4);
  L.off_hn = take((int64_t)S * n_pos * 4);
  L.off_cel = take((int64_t)S * U * 4);
  L.off_cpos = take((int64_t)S * U * 4);
  L.bytes = off;
  return L;
}

// The evaluation of a checked call once the positives' raw scores and query rows stand in the eval tail of its workspace:
// the launch record from the call and its layout L (operand blocks and EvalTail), then vfm::launch_rank_eval.  keys [Q]:
// the queries' Philox keys.
template <class L>
inline int eval_after_scores(const RankCall& r, const L& lay, const int64_t* keys) {
  char* ws = (char*)r.workspace;
  vfm::RankEval a;
  fill_scan(a, r, lay, keys);
  a.n_pos = r.n_pos; a.pos_ptr = r.pos_ptr; a.pos_items = r.pos_items;
  a.raw = (const float*)(ws + lay.off_raw); a.pusr = (const int64_t*)(ws + lay.off_pusr);
  a.pscore = (float*)(ws + lay.off_pscore); a.pid = (int64_t*)(ws + lay.off_pid); a.slot = (int64_t*)(ws + lay.off_slot);
  a.hist_all = (int*)(ws + lay.off_ha); a.hist_neg = (int*)(ws + lay.off_hn);
  a.cnt_el = (int*)(ws + lay.off_cel); a.cnt_pos = (int*)(ws + lay.off_cpos);
  a.out_rank = r.out_rank; a.out_rank_neg = r.out_rank_neg; a.out_n_eligible = r.out_n_eligible; a.out_n_neg = r.out_n_neg;
  return vfm::launch_rank_eval(a, r.strategy, (unsigned)(lay.U_pad / UT), r.stream);
}

inline bool eval_sizes_ok(int64_t U, int64_t n_cand, int64_t n_pos) {
  return U >= 0 && n_cand >= 0 && n_cand < ((int64_t)1 << 31) && n_pos >= 0 && n_pos < ((int64_t)1 << 40);
}

}  // namespace

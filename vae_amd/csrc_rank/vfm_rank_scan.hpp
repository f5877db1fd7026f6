// vfm_rank_scan.hpp -- what the two-field ranking (vfm_rank.hip) and the field-form ranking (vfm_rank_field.hip) share
// past the score tile: the launch of the per-query scan (k_rank, instantiated in vfm_rank.hip only), the merge of the
// split lists (k_rank_merge, parametrised by the function that recomputes a winner's moments) and the workspace of the
// lists.  The scan reads nothing but packed operands (TileOps), the candidate ids, the exclusion lists and one int64 key
// per query (the Philox key of VFM_RANK_RANDOM), so it serves any operand form whose score is
//   (query operand . candidate operand + query constant) + candidate constant   per part (mean, variance).
#pragma once

#include "vfm_rank_tile.hpp"

namespace vfm {

// One scan launch, in plain fields (an external-linkage mirror of RankArgs of vfm_rank.hip)
struct RankScan {
  int64_t U, n_cand, item_lo, n_excl;
  const int64_t *keys, *cand, *excl_ptr, *excl_items;      // keys [U]: the query's Philox key (two fields: the user id)
  const float *uop, *iop, *ucon, *icon;                     // packed operands [U_pad | C_pad, Kp], constants [.., 2]
  int Kp, KA, KB;
  float* ls;                                                // [S, U, k] the split lists: scores
  int* lc;                                                  //           and candidate positions
  int k, n_tiles, S;
  uint64_t seed;
};

// k_rank<strategy> over grid (n_query_tiles, S) on `st` (vfm_rank.hip)
int launch_rank_scan(const RankScan& a, int strategy, unsigned n_query_tiles, hipStream_t st);

}  // namespace vfm

namespace {

constexpr int MERGE_BLOCK = 256;

// ---------------------------------------------------------------------------------------------------------------------
// k_rank_merge: one workgroup per query.  Each list entry's final rank = its position in its own list + the number of
// entries of the other lists that beat it (binary search: every list is sorted); entries of rank < k are written with
// their moments recomputed by pm(query, candidate id, mean, var), the rest of the k slots padded.
// ---------------------------------------------------------------------------------------------------------------------
template <typename PM>
__global__ __launch_bounds__(MERGE_BLOCK) void k_rank_merge(int64_t U, int k, int S, const float* __restrict__ ls,
                                                            const int* __restrict__ lc, const int64_t* __restrict__ cand,
                                                            int64_t item_lo, PM pm, int64_t* __restrict__ out_items,
                                                            float* __restrict__ out_score, float* __restrict__ out_m,
                                                            float* __restrict__ out_v) {
  __shared__ int n_valid;
  const int64_t u = blockIdx.x;
  if (threadIdx.x == 0) n_valid = 0;
  __syncthreads();
  for (int e = threadIdx.x; e < S * k; e += MERGE_BLOCK) {
    const int s = e / k, p = e - s * k;
    const float sc = ls[((int64_t)s * U + u) * k + p];
    const int c = lc[((int64_t)s * U + u) * k + p];
    if (c == INT32_MAX) continue;
    atomicAdd(&n_valid, 1);
    int rank = p;
    for (int s2 = 0; s2 < S && rank < k; ++s2) {
      if (s2 == s) continue;
      const float* L2s = ls + ((int64_t)s2 * U + u) * k;
      const int* L2c = lc + ((int64_t)s2 * U + u) * k;
      int lo = 0, hi = k;              // first position whose entry does not beat (sc, c)
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (beats(L2s[mid], L2c[mid], sc, c)) lo = mid + 1;
        else hi = mid;
      }
      rank += lo;
    }
    if (rank >= k) continue;
    const int64_t iid = cand ? cand[c] : item_lo + c;
    float m = __builtin_nanf(""), v = __builtin_nanf("");
    pm(u, iid, m, v);
    out_items[u * k + rank] = iid;
    out_score[u * k + rank] = sc;
    out_m[u * k + rank] = m;
    out_v[u * k + rank] = v;
  }
  __syncthreads();
  for (int p = min(n_valid, k) + threadIdx.x; p < k; p += MERGE_BLOCK) {
    out_items[u * k + p] = -1;
    out_score[u * k + p] = -INFINITY;
    out_m[u * k + p] = __builtin_nanf("");
    out_v[u * k + p] = __builtin_nanf("");
  }
}

// The split lists behind the operand blocks of a workspace
struct ListLayout {
  int64_t off_ls, off_lc, bytes;
};

inline ListLayout list_layout_of(int64_t ops_end, int S, int64_t U, int k) {
  ListLayout L;
  L.off_ls = ops_end;
  L.off_lc = L.off_ls + round_up((int64_t)S * U * k * 4, 256);
  L.bytes = L.off_lc + round_up((int64_t)S * U * k * 4, 256);
  return L;
}

// The scan of a checked call over the operand blocks of its workspace, then the merge of the split lists into the call's
// outputs.  L: the workspace's layout (operand blocks and ListLayout); keys [Q]: the queries' Philox keys; pm: the
// winners' moments (k_rank_merge).
template <class L, class PM>
inline int scan_and_merge(const RankCall& r, const L& lay, const int64_t* keys, const PM& pm) {
  char* ws = (char*)r.workspace;
  vfm::RankScan a;
  fill_scan(a, r, lay, keys);
  a.ls = (float*)(ws + lay.off_ls); a.lc = (int*)(ws + lay.off_lc);
  a.k = r.k;
  if (int rc = vfm::launch_rank_scan(a, r.strategy, (unsigned)(lay.U_pad / UT), r.stream)) return rc;
  hipLaunchKernelGGL(k_rank_merge<PM>, dim3((unsigned)r.Q), dim3(MERGE_BLOCK), 0, r.stream, r.Q, (int)r.k, lay.S, a.ls,
                     a.lc, r.cand, r.cand_lo, pm, r.out_items, r.out_score, r.out_mean, r.out_var);
  return launch_status("k_rank_merge");
}

}  // namespace

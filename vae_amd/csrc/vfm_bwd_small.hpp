// vfm_bwd_small.hpp -- k_bwd_small: the fused backward + dense Adam for SMALL TABLES, one wave per table row.
// Included inside `namespace vfm { namespace {` of vfm_bwd.hip (the fused-Adam part).
#pragma once

// Why.  With a small table under a large batch (BASELINE configs[1], the ML-100K shape: 2,625 entities under 80,000 rows,
// vfm-torch.py:31-57,77 -- ONE batch per epoch) every entity sits in ~60 rows.  k_bwd gives a table row to one lane group:
// 2,625 lane groups = 330 waves on a chip of 1,024 SIMDs, each walking its list serially; the long lists therefore go
// through k_heavy first (work items of `heavy_list` occurrences, one lane group each) and the step is three dependent
// launches of under-filled grids: 31 us of backward for 4.6 MB of traffic (profiles/r04_cfg2_pmc_summary.txt).
// Here ONE launch does all of it: a WAVE owns a table row; its 64 / LPE lane groups reduce the row's work items side by
// side (item j of the list = occurrences [beg + j L, beg + (j+1) L): exactly the cut vfm_build_index writes into
// heavy_items, recomputed here from the list itself), the item records meet in LDS, and the wave's first lane group adds
// them up, finishes the gradient and applies Adam.  2,625 waves, no pre-reduction kernel, no scratch table.
//
// BITWISE the trajectory of k_heavy + k_heavy_sum + k_bwd<ADAM = 1> on the same index: every sum is formed in the order
// those kernels use --
//   an item:          A = fma(g_r, sumz_r, A) over its occurrences in list order, gs += g_r              (k_heavy)
//   a heavy entity:   P_g = items g, g + GPB, g + 2 GPB ... added in that order, GPB = 256 / LPE (k_heavy_sum's lane
//                     groups), then P_0 + P_1 + ... in order; with at most VFM_HEAVY_DIRECT items k_bwd adds the items in
//                     order itself -- here: VFM_HEAVY_DIRECT partial sums of one item each (0 + x = x)
//   a short list:     k_bwd's own walk: A = fma(g1, s1, fma(g0, s0, A)) two occurrences at a time, gs += g0 + g1
// -- and the scalars, the short walk and the epilogue (eps regeneration, KL part, link, Adam, stores) are k_bwd's own
// functions (vfm_bwd.hpp; the unit is compiled with -ffp-contract=on: fusion follows the source expression, so the same
// function gives the same bits in both kernels).  What is written out here is this kernel's alone: the per-item partial
// sums in LDS.  tests/test_gpu_model.py runs both paths side by side (VFM_BWD_SMALL=0 forces the three-launch path).
// Serves: STAGE_FULL, fused dense Adam (scaled or plain moments), Philox eps, one sample, every row, d % 4 == 0, d <= 256.
template <int LPE, int LINK>
__global__ __launch_bounds__(BLOCK) void k_bwd_small(const KArgs a, const BwdArgs b, const AdamArgs ad_in, int L, int THR) {
  constexpr int VEC = 4;
  constexpr int LGW = 64 / LPE;                      // lane groups of a wave
  constexpr int GPBH = BLOCK / LPE;                  // lane groups of a k_heavy_sum workgroup: the partial sums P_g
  constexpr int WPB = BLOCK / 64;                    // waves (= table rows) per workgroup
  constexpr int U = 8;                               // occurrences of a work item in flight
  AdamArgs ad = ad_in;
  RngKey key = a.key, next_key = b.next_key;
  int32_t la_step = 0, la_k = 0;
  load_dev_step(a, key, ad, la_step, la_k, next_key, blockIdx.x == 0 && threadIdx.x == 0);
  __shared__ float sh_cs[VFM_MAX_FIELDS];
  __shared__ int64_t sh_hi[VFM_MAX_FIELDS];
  __shared__ double sh_fin[7][BLOCK / 64];
  constexpr int NPMAX = GPBH > VFM_HEAVY_DIRECT ? GPBH : VFM_HEAVY_DIRECT;
  __shared__ __attribute__((aligned(16))) float sh_P[WPB][NPMAX][4 * LPE + 4];     // per wave: P_g = (A[0 .. 4 LPE) | gs, -, -, -)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lig = lane % LPE, lg = lane / LPE;
  const int d = a.d;
  const int C = (d + VEC - 1) / VEC;
  const int ligc = lig < C ? lig : C - 1;            // lanes past the last chunk re-load the last one (their sums are never used)
  if (tid < a.G) {
    sh_cs[tid] = (float)(a.group_n[tid] / a.W[tid]);
    sh_hi[tid] = a.group_hi[tid];
  }
  __syncthreads();
  const float gout = 1.0f;

  // ---- loss + the three scalars: workgroup 0, as in k_bwd
  scalars_and_loss<EPS_PHILOX, 1, STAGE_FULL, LINK, false>(a, b, ad, key, gout, true, true, sh_fin);

  // ---- the table rows: one wave each
  IndexGuard ig(a, b);
  float(*P)[4 * LPE + 4] = sh_P[wave];
  for (int64_t e = (int64_t)blockIdx.x * WPB + wave; e < a.T; e += (int64_t)gridDim.x * WPB) {
    const int2 pq = ig.span_ok(make_int2(b.occ_ptr[e], b.occ_ptr[e + 1]));
    const int beg = pq.x, end = pq.y;
    const bool touched = beg != end;
    const float cntf = (float)(end - beg);
    // the row's own parameters and moments: issued before the list is walked (first lane group of the wave)
    RowRegs<VEC, 1> own;
    load_own_row<LPE, 1, VEC, EPS_PHILOX, 1>(a, ad, e, d, C, lig, lg == 0, touched, touched, own);

    Chunk<VEC> A1[1];
    Chunk<VEC>& A = A1[0];
#pragma unroll
    for (int t = 0; t < VEC; ++t) A.v[t] = 0.f;
    float gs = 0.f;
    const int cnt = end - beg;
    if (cnt > THR) {
      // heavy: the items of the list, L occurrences each, in list order.  Lane group lg forms the partial sums P_g of
      // g = lg, lg + LGW, ... (g < GPBH): items g, g + GPBH, ... -- each item a sequential fma chain as k_heavy forms it
      const int n_items = (cnt + L - 1) / L;
      // partial sums: k_heavy_sum's lane groups (items g, g + GPBH, ...) -- or, with at most VFM_HEAVY_DIRECT items, one per
      // item, which is k_bwd's own in-order sum of the item records (with 64 lanes per entity GPBH is 4: fewer than that)
      const int NP = n_items <= VFM_HEAVY_DIRECT ? VFM_HEAVY_DIRECT : GPBH;
      for (int g = lg; g < NP; g += LGW) {
        Chunk<VEC> Pg;
#pragma unroll
        for (int t = 0; t < VEC; ++t) Pg.v[t] = 0.f;
        float Pgs = 0.f;
        for (int it = g; it < n_items; it += NP) {
          const int ib = beg + it * L, ie = (ib + L < end) ? ib + L : end;
          Chunk<VEC> Ai;
#pragma unroll
          for (int t = 0; t < VEC; ++t) Ai.v[t] = 0.f;
          float gi = 0.f;
          // U occurrences in flight: every load of a batch is issued before the first fma needs one; the sums themselves
          // are formed one occurrence at a time in list order, as k_heavy forms them.  The row ids of the NEXT batch are
          // fetched under the current one.
          int rn[U];
#pragma unroll
          for (int u = 0; u < U; ++u) rn[u] = b.occ_rows[ib + u < ie ? ib + u : ie - 1];
          for (int o = ib; o < ie; o += U) {
            int r[U];
            float g[U];
            Chunk<VEC> sv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) r[u] = ig.row_ok(rn[u], o + u < ie);
#pragma unroll
            for (int u = 0; u < U; ++u) {
              g[u] = b.grow[r[u]];
              sv[u] = ld_chunk<VEC>(b.sumz + (size_t)r[u] * d + (size_t)ligc * VEC);      // (no load under a branch)
            }
#pragma unroll
            for (int u = 0; u < U; ++u) rn[u] = b.occ_rows[o + U + u < ie ? o + U + u : ie - 1];
#pragma unroll
            for (int u = 0; u < U; ++u) {
              if (o + u < ie) {
                gi += g[u];
#pragma unroll
                for (int t = 0; t < VEC; ++t) Ai.v[t] = fmaf(g[u], sv[u].v[t], Ai.v[t]);
              }
            }
          }
          Pgs += gi;
#pragma unroll
          for (int t = 0; t < VEC; ++t) Pg.v[t] += Ai.v[t];
        }
        *reinterpret_cast<float4*>(&P[g][4 * lig]) = make_float4(Pg.v[0], Pg.v[1], Pg.v[2], Pg.v[3]);
        if (lig == 0) P[g][4 * LPE] = Pgs;
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");      // (one wave: its LDS writes are ordered before the reads below)
      __builtin_amdgcn_wave_barrier();
      if (lg == 0) {                                 // P_0 + P_1 + ... in order
        for (int g = 0; g < NP; ++g) {
          const float4 t4 = *reinterpret_cast<const float4*>(&P[g][4 * lig]);
          A.v[0] += t4.x; A.v[1] += t4.y; A.v[2] += t4.z; A.v[3] += t4.w;
          gs += P[g][4 * LPE];
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");      // (... and the reads before the next row's writes)
      __builtin_amdgcn_wave_barrier();
    } else if (lg == 0) {
      walk_pairs<LPE, 1, VEC, false>(b, b.sumz, beg, end, d, C, 0, lig, ig, A1, gs);      // a short list: k_bwd's own walk
    }
    if (lg != 0) continue;                           // (the row's epilogue, k_bwd's: the wave's first lane group)

    const float c = touched ? kl_weight(sh_cs, sh_hi, a.G, e, own.io, cntf) : 0.f;
    float nb_eps = 0.f;
    if (lig < C) {
      Chunk<VEC> gm, gv;
      if (touched) {
        Chunk<VEC> epc;
        chunk_eps<VEC, EPS_PHILOX>(key, e, lig, own.ep[0], epc, nb_eps);
        chunk_grad<VEC, LINK, false>(own.mu[0], own.s[0], epc, A, gs, c, gout, gm, gv);
      } else {
#pragma unroll
        for (int t = 0; t < VEC; ++t) { gm.v[t] = 0.f; gv.v[t] = 0.f; }
      }
      Chunk<VEC> pm, ps;
      adam_row_step<VEC, false>(own.mu[0].v, own.s[0].v, own.mm[0].v, own.ms[0].v, own.vm[0].v, own.vs[0].v, gm.v, gv.v, 0, 0, nullptr, touched,
                                ad, pm.v, ps.v);
      store_row_chunk<VEC>(a, ad, e, d, lig, touched, pm, ps, own.mm[0], own.ms[0], own.vm[0], own.vs[0]);
    }
    if (lig == 0) {
      float g0 = 0.f, g1 = 0.f;
      if (touched) first_order_grad<LINK>(own.th, gs, nb_eps, c, gout, g0, g1);
      const float2 pn = adam_pair_step<false>(own.th, own.mb, own.vb, g0, g1, 0, 0, nullptr, touched, ad);
      store_first_order(a, ad, e, touched, pn, own.mb, own.vb);
    }
  }
  ig.report(b.status);
}

// vfm_bwd.hpp -- k_bwd: entity-centric gradients / fused Adam / multi-rank stages.
// Included inside `namespace vfm { namespace {` of vfm_bwd.hip (one object per link function).
#pragma once

// ---------------------------------------------------------------------------------------
// backward (entity-centric, dense gradient rows, no atomics) -- optionally with the dense Adam
// update fused in (ADAM = 1): the gradient row never leaves registers.
//
// A lane group owns one TABLE row e: it sums grow[r] * sumz[r,:] over the batch rows that contain
// e (inverted index occ_ptr / occ_rows), adds the KL part, and either stores the dense gradient
// row (zeros when e is not in the batch: the reference's nn.Embedding gradients are dense) or
// applies torch.optim.Adam's update to (p, m, v) of that row in place.  Only e's own parameters
// are read, so the in-place update is race free.  All loads that do not depend on the index
// chain (own row, Adam moments, next entity's offsets) are issued before walking it.
// ---------------------------------------------------------------------------------------
//
// Variational samples S > 1 (STAGE_FULL only): sumz holds one [B,d] block per sample and grow[r] the
// sum over samples of dloss/dpred[s,r]; with A^s = sum_r grow_r sumz^s_r and gs = sum_r grow_r,
//   dloss/dmu_e = 1/S sum_s (A^s - z^s gs),   dloss/ds_e = link'(s_e) 1/S sum_s eps^s (A^s - z^s gs)
// (+ the KL part, which does not depend on the sample): the list of e is walked once per sample.
// Scaled moments (VFM_FLAG_SCALED_MOMENTS): with ms = m / b1^k and vs = v / b2^k stored instead of m and
// v (k = steps since the last period boundary), the decay of a row WITHOUT gradient is implicit -- its ms
// and vs do not change, so they are read but not written back: 16 instead of 24 bytes per parameter for
// the rows a batch does not touch.  Same dense-Adam mathematics (every row still moves every step):
//   ms += (1-b1) g / b1^k,  vs += (1-b2) g^2 / b2^k,  m = ms b1^k,  v = vs b2^k,  p -= lr_t m / (sqrt(v)/.. + eps)
// At the end of a period of VFM_MOMENT_PERIOD steps the true m, v are written for every row (k restarts),
// which bounds 1 / b1^k (0.9^-128 = 7e5).
// The scaled form in its two halves (adam_update below runs them back to back): the moments take the gradient, then the
// parameter moves given r = sqrt(stored second moment).  The look-ahead instances call the halves themselves: a replayed
// row without gradient already holds that root (its second moment does not change), so it is taken once, not twice.
__device__ __forceinline__ void adam_accum(float g, float& m, float& v, const AdamArgs& ad) {
  m = fmaf(ad.c1, g, m);
  v = fmaf(ad.c2 * g, g, v);
}
__device__ __forceinline__ float adam_apply(float p, float& m, float& v, float r, const AdamArgs& ad) {
  const float denom = fmaf(r, ad.q2, ad.eps);
  const float pn = fmaf(-ad.a1 * m, __builtin_amdgcn_rcpf(denom), p);
  if (ad.store_true) { m = m * ad.s1; v = v * ad.s2; }
  return pn;
}

__device__ __forceinline__ float adam_update(float p, float g, float& m, float& v, const AdamArgs& ad) {
  if (ad.scaled) {                     // uniform
    // (this form is not bitwise torch's anyway: hardware sqrt / rcp, 1 ulp each, instead of the IEEE
    // sqrt and the two IEEE divisions of the plain form below -- ~10 instead of ~45 VALU instructions
    // per coordinate, which the kernel would otherwise not hide behind its memory traffic)
    // p -= step_size m_t / (sqrt(v_t) / sqrt(bc2) + eps) with m_t = ms b1^k, v_t = vs b2^k, the per-step factors folded
    // into two scalars (a1, q2): sqrt is taken of the STORED second moment, so a row without gradient needs it once
    // however many steps are replayed (k_adam_catchup runs exactly these operations)
    adam_accum(g, m, v, ad);
    return adam_apply(p, m, v, __builtin_amdgcn_sqrtf(v), ad);
  }
  m = m + (g - m) * (1.0f - ad.b1);
  v = v * ad.b2 + ((1.0f - ad.b2) * g) * g;
  const float denom = __fsqrt_rn(v) / ad.bc2_sqrt + ad.eps;
  return p + (-ad.step_size * m) / denom;
}

__device__ __forceinline__ int heavy_slot_of(const int32_t* ids, int n, int e) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ids[mid] < e) lo = mid + 1; else hi = mid;
  }
  return (n > 0 && ids[lo] == e) ? lo : -1;
}

// one replayed zero-gradient step of the scaled-moment form, given r = sqrt(stored second moment) and the step's
// (a1, q2): exactly adam_update's scaled branch with g = 0 (k_adam_catchup, vfm_adam.hpp, runs the same operations)
__device__ __forceinline__ float replay_one(float p, float m, float r, float2 c, float eps) {
  return fmaf(-c.x * m, __builtin_amdgcn_rcpf(fmaf(r, c.y, eps)), p);
}
// ---------------------------------------------------------------------------------------
// The phases of a row's update.  k_bwd's loop body below is a sequence of them, and k_bwd_small (vfm_bwd_small.hpp) calls
// the same functions: its step is specified as bitwise the three-launch one, and under -ffp-contract=on equal source
// expressions give equal bits.  Every arithmetic expression of the update lives here, once.
// ---------------------------------------------------------------------------------------

// the i-th chunk of lane `lig` of a lane group of LPE lanes
template <int LPE>
__device__ __forceinline__ int chunk_of(int lig, int i) { return lig + i * LPE; }

// Index guard.  A corrupted index is clamped, never followed: list offsets to [0, n_occ], row numbers to [0, B), listed
// entities to [0, T); every clamp that fires is counted for b.status (vfm_index_t.status), the caller's next look.
struct IndexGuard {
  int n_occ, Bm1;
  int64_t T;
  int nclamp;
  __device__ __forceinline__ IndexGuard(const KArgs& a, const BwdArgs& b)
      : n_occ(b.n_occ), Bm1(a.B > 0 ? (int)a.B - 1 : 0), T(a.T), nclamp(0) {}
  __device__ __forceinline__ int64_t ent_ok(int64_t v) {
    const bool ok = v >= 0 && v < T;
    nclamp += ok ? 0 : 1;
    return ok ? v : 0;
  }
  __device__ __forceinline__ int2 span_ok(int2 v) {
    const bool ok = v.x >= 0 && v.y >= v.x && v.y <= n_occ;
    nclamp += ok ? 0 : 1;
    return ok ? v : make_int2(0, 0);
  }
  // (live = false: a padding slot of a batch of loads, clamped without being counted)
  __device__ __forceinline__ int row_ok(int v, bool live = true) {
    const bool ok = (unsigned)v <= (unsigned)Bm1;
    nclamp += (ok || !live) ? 0 : 1;
    return ok ? v : 0;
  }
  __device__ __forceinline__ void report(int32_t* status) const {
    if (nclamp != 0 && status) atomicAdd(status, nclamp);       // (integer: the total does not depend on the order)
  }
};

// Scalars and loss: the duties of workgroup 0.  `duty`: this launch forms the loss and moves the scalars; `last`: it is
// the last chunk of a chunked run.
__device__ __forceinline__ void adam_scalar(int i, float g, const KArgs& a, const AdamArgs& ad) {
  float* sc = const_cast<float*>(a.scalars);
  float m = ad.m_scal[i], v = ad.v_scal[i];
  sc[i] = adam_update(sc[i], g, m, v, ad);
  ad.m_scal[i] = m; ad.v_scal[i] = v;
}

template <int EPS, int ADAM, int STAGE, int LINK, bool MULTI>
__device__ __forceinline__ void scalars_and_loss(const KArgs& a, const BwdArgs& b, const AdamArgs& ad, const RngKey& key, float gout,
                                                 bool duty, bool last, double (*sh_fin)[BLOCK / 64]) {
  const int tid = threadIdx.x;
  double fin[6] = {0, 0, 0, 0, 0, 0};
  const bool fold = STAGE == STAGE_FULL && b.loss != nullptr && duty;   // uniform: fold vfm_elbo_finalize_f32 in
  if (blockIdx.x == 0 && fold)
    reduce_slots_and_loss(b.partials, a.scalars, a.ll_scale_d, a.flags, b.loss, sh_fin, fin);
  if (STAGE == STAGE_ACC && blockIdx.x == 0 && tid == 0 && a.e_lo == 0) {
    // (a caller that skipped vfm_elbo_finalize_f32 gets NaN, not stale sums)
    const bool reduced = b.partials[VFM_P_REDUCED] == 1.0;
    b.sums[0] = reduced ? (float)b.partials[VFM_P_G] : __builtin_nanf("");   // this rank's row sums, to be summed over ranks
    b.sums[1] = reduced ? (float)b.partials[VFM_P_ALPHA] : __builtin_nanf("");
  }
  if (STAGE != STAGE_ACC && blockIdx.x == 0 && tid == 0 && last && duty) {
    const float alpha = a.scalars[0], m0 = a.scalars[1], s0 = a.scalars[2];
    // (no fold and the forward's slots never reduced -- vfm_elbo_finalize_f32 skipped --: NaN, not stale sums)
    const bool stale = STAGE == STAGE_FULL && !fold && b.partials[VFM_P_REDUCED] != 1.0;
    const float sum_g = stale ? __builtin_nanf("")
                              : (STAGE == STAGE_APPLY) ? b.sums[0] : (float)(fold ? fin[VFM_P_G] : b.partials[VFM_P_G]);
    const float sum_a = (STAGE == STAGE_APPLY) ? b.sums[1]
                                               : (float)(fold ? fin[VFM_P_ALPHA] : b.partials[VFM_P_ALPHA]);
    float e0 = 0.f;
    if constexpr (EPS == EPS_TABLE) e0 = a.eps_global[0];
    if constexpr (EPS == EPS_PHILOX) {
      float n[8], nb;
      normal8b(key, 0xFFFFFFFFu, 0u, n, nb);
      e0 = n[0];
    }
    const float as0 = link_f<LINK>(s0);
    const float prior = (a.flags & VFM_FLAG_NO_PRIOR_TERMS) ? 0.f : 1.f;
    const float ga = (a.lik == VFM_LIK_NORMAL)
                         ? gout * dlink_f<LINK>(alpha) * a.ll_scale * sum_a : 0.f;
    const float gm = gout * (sum_g + prior * m0);
    // S > 1: every sample has its own eps0 -- the forward accumulated sum_s eps0^s sum_r g_sr
    const float ge0 = MULTI ? (float)(fold ? fin[VFM_P_GE0] : b.partials[VFM_P_GE0]) : e0 * sum_g;
    const float gs = gout * dlink_f<LINK>(s0) * (ge0 + prior * (as0 - inv_sigma(as0)));
    if constexpr (ADAM) {
      // alpha has no gradient under the Bernoulli likelihood (reference: grad None, Adam skips it)
      if (a.lik == VFM_LIK_NORMAL) adam_scalar(0, ga, a, ad);
      adam_scalar(1, gm, a, ad);
      adam_scalar(2, gs, a, ad);
    } else {
      b.g_scalars[0] = ga; b.g_scalars[1] = gm; b.g_scalars[2] = gs;
    }
  }
}

// Row cursor: the entity of position `at` (of the row list, or of the table scan) and its occ_ptr pair, fetched one
// iteration before the row is visited.  STAGE_APPLY reads no lists: its pair stays (0, 0).
template <int STAGE>
__device__ __forceinline__ void fetch_row(const BwdArgs& b, bool listed, int64_t at, int64_t li_end, IndexGuard& ig,
                                          int64_t& e_cur, int2& pq) {
  if (at >= li_end) return;
  e_cur = listed ? ig.ent_ok(b.row_ids[at]) : at;
  if constexpr (STAGE != STAGE_APPLY) pq = ig.span_ok(make_int2(b.occ_ptr[e_cur], b.occ_ptr[e_cur + 1]));
}

// Own-row loads: what does not depend on the index chain -- parameters, moments, table eps, the first-order pair and
// 1 / occurrences.  `active`: this lane group holds the row (k_bwd_small: the wave's first one).
template <int VEC, int CPL>
struct RowRegs {
  Chunk<VEC> mu[CPL], s[CPL], ep[CPL], mm[CPL], ms[CPL], vm[CPL], vs[CPL];
  float2 th = make_float2(0.f, 1.f), mb = make_float2(0.f, 0.f), vb = make_float2(0.f, 0.f);
  float io = 0.f, epw = 0.f;
};

template <int LPE, int CPL, int VEC, int EPS, int ADAM>
__device__ __forceinline__ void load_own_row(const KArgs& a, const AdamArgs& ad, int64_t e, int d, int C, int lig, bool active,
                                             bool touched, bool want_io, RowRegs<VEC, CPL>& r) {
  const float* prow = a.entity + (size_t)e * (2 * (size_t)d);
#pragma unroll
  for (int i = 0; i < CPL; ++i) {
    const int j = chunk_of<LPE>(lig, i);
    if (active && j < C) {
      r.mu[i] = ld_chunk<VEC>(prow + (size_t)j * VEC);
      r.s[i] = ld_chunk<VEC>(prow + d + (size_t)j * VEC);
      if constexpr (ADAM) {
        const size_t o = (size_t)e * (2 * (size_t)d) + (size_t)j * VEC;
        r.mm[i] = ld_chunk_nt<VEC>(ad.m_entity + o); r.ms[i] = ld_chunk_nt<VEC>(ad.m_entity + o + d);
        r.vm[i] = ld_chunk_nt<VEC>(ad.v_entity + o); r.vs[i] = ld_chunk_nt<VEC>(ad.v_entity + o + d);
      }
      if constexpr (EPS == EPS_TABLE)
        if (touched) r.ep[i] = ld_chunk<VEC>(a.eps_entity + (size_t)e * d + (size_t)j * VEC);
    }
  }
  if (active && lig == 0) {
    r.th = *reinterpret_cast<const float2*>(a.bias + 2 * (size_t)e);
    if constexpr (ADAM) {
      r.mb = *reinterpret_cast<const float2*>(ad.m_bias + 2 * (size_t)e);
      r.vb = *reinterpret_cast<const float2*>(ad.v_bias + 2 * (size_t)e);
    }
  }
  if (active && want_io) {
    r.io = a.inv_occ[e];
    if constexpr (EPS == EPS_TABLE) r.epw = a.eps_bias[e];
  }
}

// List walk, heavy part: a list pre-reduced by k_heavy -- read the record(s) instead of walking
template <int LPE, int CPL, int VEC>
__device__ __forceinline__ void read_heavy(const BwdArgs& b, const float* __restrict__ hacc, int hslot, int64_t xs, int C, int lig,
                                           IndexGuard& ig, Chunk<VEC> (&A)[CPL], float& gs) {
  const float* rec = hacc + (size_t)hslot * xs;
  int4 hd = *reinterpret_cast<const int4*>(rec);      // (sum grow, count, first item, last item + 1)
  if (hd.z < 0 || hd.w < hd.z || hd.w > b.heavy_stride - b.n_heavy) { hd.z = hd.w = 0; ++ig.nclamp; }
  if (hd.w - hd.z <= VFM_HEAVY_DIRECT) {      // few work items: add their records here, in item order
    for (int it = hd.z; it < hd.w; ++it) {
      const float* ir = hacc + ((size_t)b.n_heavy + (size_t)it) * xs;
      gs += ir[0];
#pragma unroll
      for (int i = 0; i < CPL; ++i) {
        const int j = chunk_of<LPE>(lig, i);
        if (j < C) {
          const Chunk<VEC> t4 = ld_chunk<VEC>(ir + 4 + (size_t)j * VEC);
#pragma unroll
          for (int t = 0; t < VEC; ++t) A[i].v[t] += t4.v[t];
        }
      }
    }
  } else {                                    // k_heavy_sum added them into the entity's record
    gs = __int_as_float(hd.x);
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      const int j = chunk_of<LPE>(lig, i);
      if (j < C) A[i] = ld_chunk<VEC>(rec + 4 + (size_t)j * VEC);
    }
  }
}

// List walk, the walk itself: A += sum_r g_r * sumz_r, gs += sum_r g_r over occurrences [o, end), two in flight.
// PIPE: the sample of the OTHER entity of the row (this step's records) stands in for the sumz row.
template <bool PIPE>
__device__ __forceinline__ const float* walk_source(const BwdArgs& b, const float* __restrict__ sz, int oo, int r, int d, int64_t xs,
                                                    IndexGuard& ig) {
  if constexpr (PIPE) return b.zrec + (size_t)ig.ent_ok(b.occ_other[oo]) * xs + 4;
  return sz + (size_t)r * d;
}

template <int LPE, int CPL, int VEC, bool PIPE>
__device__ __forceinline__ void walk_pairs(const BwdArgs& b, const float* __restrict__ sz, int o, int end, int d, int C, int64_t xs,
                                           int lig, IndexGuard& ig, Chunk<VEC> (&A)[CPL], float& gs) {
  for (; o + 1 < end; o += 2) {      // two occurrences in flight
    const int r0 = ig.row_ok(b.occ_rows[o]), r1 = ig.row_ok(b.occ_rows[o + 1]);
    const float g0 = b.grow[r0], g1 = b.grow[r1];
    const float* p0 = walk_source<PIPE>(b, sz, o, r0, d, xs, ig);
    const float* p1 = walk_source<PIPE>(b, sz, o + 1, r1, d, xs, ig);
    gs += g0 + g1;
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      const int j = chunk_of<LPE>(lig, i);
      if (j < C) {
        const Chunk<VEC> s0v = ld_chunk<VEC>(p0 + (size_t)j * VEC);
        const Chunk<VEC> s1v = ld_chunk<VEC>(p1 + (size_t)j * VEC);
#pragma unroll
        for (int t = 0; t < VEC; ++t) A[i].v[t] = fmaf(g1, s1v.v[t], fmaf(g0, s0v.v[t], A[i].v[t]));
      }
    }
  }
  if (o < end) {
    const int r0 = ig.row_ok(b.occ_rows[o]);
    const float g0 = b.grow[r0];
    const float* p0 = walk_source<PIPE>(b, sz, o, r0, d, xs, ig);
    gs += g0;
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      const int j = chunk_of<LPE>(lig, i);
      if (j < C) {
        const Chunk<VEC> s0v = ld_chunk<VEC>(p0 + (size_t)j * VEC);
#pragma unroll
        for (int t = 0; t < VEC; ++t) A[i].v[t] = fmaf(g0, s0v.v[t], A[i].v[t]);
      }
    }
  }
}

// the whole list of one sample (sz / hacc: the sample's blocks)
template <int LPE, int CPL, int VEC, bool PIPE>
__device__ __forceinline__ void walk_list(const BwdArgs& b, const float* __restrict__ sz, const float* __restrict__ hacc, int hslot,
                                          int beg, int end, int d, int C, int64_t xs, int lig, IndexGuard& ig, Chunk<VEC> (&A)[CPL],
                                          float& gs) {
#pragma unroll
  for (int i = 0; i < CPL; ++i)
#pragma unroll
    for (int t = 0; t < VEC; ++t) A[i].v[t] = 0.f;
  gs = 0.f;
  if (hslot >= 0) read_heavy<LPE, CPL, VEC>(b, hacc, hslot, xs, C, lig, ig, A, gs);
  else walk_pairs<LPE, CPL, VEC, PIPE>(b, sz, beg, end, d, C, xs, lig, ig, A, gs);
}

// weight of the row's KL part
__device__ __forceinline__ float kl_weight(const float* sh_cs, const int64_t* sh_hi, int G, int64_t e, float io, float cntf) {
  return sh_cs[group_index(sh_hi, G, e)] * io * cntf;
}

// eps of chunk j of entity e: the table's (`tab`, loaded by the caller), zero, or regenerated (nb: the first-order eps)
template <int VEC, int EPS>
__device__ __forceinline__ void chunk_eps(const RngKey& key, int64_t e, int j, const Chunk<VEC>& tab, Chunk<VEC>& epc, float& nb) {
  nb = 0.f;
  if constexpr (EPS == EPS_TABLE) {
    epc = tab;
  } else if constexpr (EPS == EPS_ZERO) {
#pragma unroll
    for (int t = 0; t < VEC; ++t) epc.v[t] = 0.f;
  } else {
    eps_of_chunk<VEC>(key, (uint32_t)e, j, epc.v, nb);
  }
}

// Chunk gradient, one sample: (mu, s, eps, A, gs, c, gout) -> (gm, gv)
template <int VEC, int LINK, bool PIPE>
__device__ __forceinline__ void chunk_grad(const Chunk<VEC>& mu, const Chunk<VEC>& s, const Chunk<VEC>& epc, const Chunk<VEC>& A,
                                           float gs, float c, float gout, Chunk<VEC>& gm, Chunk<VEC>& gv) {
#pragma unroll
  for (int t = 0; t < VEC; ++t) {
    const float sg = link_f<LINK>(s.v[t]);
    const float z = fmaf(sg, epc.v[t], mu.v[t]);
    // sum_r g_r (sumz_rk - z_ek); PIPE: A already sums the other entity's z alone
    const float gz = PIPE ? A.v[t] : A.v[t] - z * gs;
    gm.v[t] = gout * (gz + c * mu.v[t]);
    gv.v[t] = gout * dlink_f<LINK>(s.v[t]) * (gz * epc.v[t] + c * (sg - inv_sigma(sg)));
  }
}

// Chunk gradient, S > 1: one sample's share of g1s = sum_s (A^s - z^s gs), g2s = sum_s eps^s (A^s - z^s gs) ...
template <int VEC, int LINK>
__device__ __forceinline__ void chunk_grad_sample(const Chunk<VEC>& mu, const Chunk<VEC>& s, const Chunk<VEC>& epc,
                                                  const Chunk<VEC>& A, float gs, Chunk<VEC>& g1s, Chunk<VEC>& g2s) {
#pragma unroll
  for (int t = 0; t < VEC; ++t) {
    const float z = fmaf(link_f<LINK>(s.v[t]), epc.v[t], mu.v[t]);
    const float gz = A.v[t] - z * gs;
    g1s.v[t] += gz;
    g2s.v[t] = fmaf(gz, epc.v[t], g2s.v[t]);
  }
}
// ... and the gradient from the sample means
template <int VEC, int LINK>
__device__ __forceinline__ void chunk_grad_multi(const Chunk<VEC>& mu, const Chunk<VEC>& s, const Chunk<VEC>& g1s,
                                                 const Chunk<VEC>& g2s, float c, float gout, Chunk<VEC>& gm, Chunk<VEC>& gv) {
#pragma unroll
  for (int t = 0; t < VEC; ++t) {
    const float sg = link_f<LINK>(s.v[t]);
    gm.v[t] = gout * (g1s.v[t] + c * mu.v[t]);
    gv.v[t] = gout * dlink_f<LINK>(s.v[t]) * (g2s.v[t] + c * (sg - inv_sigma(sg)));
  }
}

// S > 1 (uniform): the list is walked once per sample (A, gs hold the first sample's walk on entry, the last one's on
// return); g1s, g2s = the means over the samples, nb_eps = mean_s eps_w^s
template <int LPE, int CPL, int VEC, int EPS, int LINK>
__device__ __forceinline__ void sample_means(const KArgs& a, const BwdArgs& b, const RngKey& key, int64_t e, int hslot, int beg,
                                             int end, int d, int C, int64_t xs, int lig, IndexGuard& ig,
                                             const RowRegs<VEC, CPL>& r, Chunk<VEC> (&A)[CPL], float& gs, Chunk<VEC> (&g1s)[CPL],
                                             Chunk<VEC> (&g2s)[CPL], float& nb_eps) {
#pragma unroll
  for (int i = 0; i < CPL; ++i)
#pragma unroll
    for (int t = 0; t < VEC; ++t) { g1s[i].v[t] = 0.f; g2s[i].v[t] = 0.f; }
  for (int sm = 0; sm < a.S; ++sm) {
    if (sm > 0)
      walk_list<LPE, CPL, VEC, false>(b, b.sumz + (size_t)sm * (size_t)a.B * d,
                                      b.heavy_acc + (size_t)sm * (size_t)b.heavy_stride * xs, hslot, beg, end, d, C, xs, lig, ig, A, gs);
    const RngKey ks = key_of_sample(key, sm);
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      const int j = chunk_of<LPE>(lig, i);
      if (j < C) {
        Chunk<VEC> tab, epc;
        float nb;
        if constexpr (EPS == EPS_TABLE)
          tab = ld_chunk<VEC>(a.eps_entity + ((size_t)sm * (size_t)a.T + (size_t)e) * d + (size_t)j * VEC);
        chunk_eps<VEC, EPS>(ks, e, j, tab, epc, nb);
        if (EPS == EPS_PHILOX && i == 0) nb_eps += nb;
        chunk_grad_sample<VEC, LINK>(r.mu[i], r.s[i], epc, A[i], gs, g1s[i], g2s[i]);
      }
    }
    if constexpr (EPS == EPS_TABLE) nb_eps += a.eps_bias[(size_t)sm * (size_t)a.T + (size_t)e];
  }
  nb_eps *= a.inv_S;
#pragma unroll
  for (int i = 0; i < CPL; ++i)
#pragma unroll
    for (int t = 0; t < VEC; ++t) { g1s[i].v[t] *= a.inv_S; g2s[i].v[t] *= a.inv_S; }
}

// First-order gradient: (th, gs, nb_eps, c, gout) -> (g0, g1)
template <int LINK>
__device__ __forceinline__ void first_order_grad(float2 th, float gs, float nb_eps, float c, float gout, float& g0, float& g1) {
  const float sg = link_f<LINK>(th.y);
  g0 = gout * (gs + c * th.x);
  g1 = gout * dlink_f<LINK>(th.y) * (gs * nb_eps + c * (sg - inv_sigma(sg)));
}

// Adam step of 2 N parameters (a chunk's mu | s, or the first-order pair): p -> q, moments in place.
// LA (always the scaled form): the row first replays the la_gap zero-gradient steps it skipped ((a1, q2) of the period's
// steps in `tab`), then takes adam_update in its halves -- a replayed row without gradient keeps its second moments
// (fma(c2 0, 0, v) = v), so the roots taken for the replay are handed over to this step's update.
template <int N, bool LA>
__device__ __forceinline__ void adam_row_step(float (&p0)[N], float (&p1)[N], float (&m0)[N], float (&m1)[N], float (&v0)[N],
                                              float (&v1)[N], const float (&g0)[N], const float (&g1)[N], int la_gap, int la_k,
                                              const float2* tab, bool touched, const AdamArgs& ad, float (&q0)[N], float (&q1)[N]) {
  if constexpr (LA) {
    float r0[N], r1[N];          // sqrt of the stored second moments
    if (la_gap > 0) {            // (uniform over the lane group) bring the row up to the step before this one
#pragma unroll
      for (int t = 0; t < N; ++t) { r0[t] = __builtin_amdgcn_sqrtf(v0[t]); r1[t] = __builtin_amdgcn_sqrtf(v1[t]); }
      for (int k = la_k - la_gap; k < la_k; ++k) {
        const float2 c = tab[k];
#pragma unroll
        for (int t = 0; t < N; ++t) {
          p0[t] = replay_one(p0[t], m0[t], r0[t], c, ad.eps);
          p1[t] = replay_one(p1[t], m1[t], r1[t], c, ad.eps);
        }
      }
    }
#pragma unroll
    for (int t = 0; t < N; ++t) {
      adam_accum(g0[t], m0[t], v0[t], ad);
      adam_accum(g1[t], m1[t], v1[t], ad);
    }
    if (!(la_gap > 0 && !touched)) {
#pragma unroll
      for (int t = 0; t < N; ++t) { r0[t] = __builtin_amdgcn_sqrtf(v0[t]); r1[t] = __builtin_amdgcn_sqrtf(v1[t]); }
    }
#pragma unroll
    for (int t = 0; t < N; ++t) {
      q0[t] = adam_apply(p0[t], m0[t], v0[t], r0[t], ad);
      q1[t] = adam_apply(p1[t], m1[t], v1[t], r1[t], ad);
    }
  } else {
#pragma unroll
    for (int t = 0; t < N; ++t) {
      q0[t] = adam_update(p0[t], g0[t], m0[t], v0[t], ad);
      q1[t] = adam_update(p1[t], g1[t], m1[t], v1[t], ad);
    }
  }
}

// the same for the first-order pair (mu_w, s_w)
template <bool LA>
__device__ __forceinline__ float2 adam_pair_step(float2 th, float2& mb, float2& vb, float g0, float g1, int la_gap, int la_k,
                                                 const float2* tab, bool touched, const AdamArgs& ad) {
  float p0[1] = {th.x}, p1[1] = {th.y}, m0[1] = {mb.x}, m1[1] = {mb.y}, v0[1] = {vb.x}, v1[1] = {vb.y};
  const float ga[1] = {g0}, gb[1] = {g1};
  float q0[1], q1[1];
  adam_row_step<1, LA>(p0, p1, m0, m1, v0, v1, ga, gb, la_gap, la_k, tab, touched, ad, q0, q1);
  mb = make_float2(m0[0], m1[0]);
  vb = make_float2(v0[0], v1[0]);
  return make_float2(q0[0], q1[0]);
}

// Moment write-back rule (scaled form: rows without gradient keep ms, vs -- their decay is implicit) ...
__device__ __forceinline__ bool moments_written(const AdamArgs& ad, bool touched) {
  return !ad.scaled || touched || ad.store_true;
}
// ... and the stores of an updated chunk / first-order pair
template <int VEC>
__device__ __forceinline__ void store_row_chunk(const KArgs& a, const AdamArgs& ad, int64_t e, int d, int j, bool touched,
                                                const Chunk<VEC>& pm, const Chunk<VEC>& ps, const Chunk<VEC>& mm,
                                                const Chunk<VEC>& ms, const Chunk<VEC>& vm, const Chunk<VEC>& vs) {
  float* prow = const_cast<float*>(a.entity) + (size_t)e * (2 * (size_t)d);
  const size_t o2 = (size_t)e * (2 * (size_t)d) + (size_t)j * VEC;
  st_chunk<VEC>(prow + (size_t)j * VEC, pm);
  st_chunk<VEC>(prow + d + (size_t)j * VEC, ps);
  if (moments_written(ad, touched)) {
    st_chunk_nt<VEC>(ad.m_entity + o2, mm); st_chunk_nt<VEC>(ad.m_entity + o2 + d, ms);
    st_chunk_nt<VEC>(ad.v_entity + o2, vm); st_chunk_nt<VEC>(ad.v_entity + o2 + d, vs);
  }
}
__device__ __forceinline__ void store_first_order(const KArgs& a, const AdamArgs& ad, int64_t e, bool touched, float2 pn, float2 mb,
                                                  float2 vb) {
  *reinterpret_cast<float2*>(const_cast<float*>(a.bias) + 2 * (size_t)e) = pn;
  if (a.wrec) *reinterpret_cast<float2*>(a.wrec + 4 * (size_t)e) = pn;      // packed first-order record: (mu_w, s_w | 1/occ, 0)
  if (moments_written(ad, touched)) {
    *reinterpret_cast<float2*>(ad.m_bias + 2 * (size_t)e) = mb;
    *reinterpret_cast<float2*>(ad.v_bias + 2 * (size_t)e) = vb;
  }
}

// Next-step record of PIPE: the updated row is in registers -- sample it for the next step right here.  A chunk ...
template <int VEC, int LINK>
__device__ __forceinline__ void next_record_chunk(const BwdArgs& b, const RngKey& next_key, int64_t e, int j, int64_t xs,
                                                  const Chunk<VEC>& pm, const Chunk<VEC>& ps, bool first, float& nb_next,
                                                  float& kl_next) {
  Chunk<VEC> ep2, zn;
  float nb2;
  eps_of_chunk<VEC>(next_key, (uint32_t)e, j, ep2.v, nb2);
  if (first) nb_next = nb2;
#pragma unroll
  for (int t = 0; t < VEC; ++t) {
    const float sg2 = link_f<LINK>(ps.v[t]);
    zn.v[t] = fmaf(sg2, ep2.v[t], pm.v[t]);
    kl_next += kl_std_normal(pm.v[t], sg2);
  }
  st_chunk<VEC>(b.zrec_next + (size_t)e * xs + 4 + (size_t)j * VEC, zn);
}
// ... the sampled first-order weight ...
template <int LINK>
__device__ __forceinline__ void next_record_weight(float2 pn, float nb_next, float& w_next, float& kl_next) {
  const float sgw2 = link_f<LINK>(pn.y);
  w_next = fmaf(sgw2, nb_next, pn.x);
  kl_next += kl_std_normal(pn.x, sgw2);
}
// ... and (uniform over the lane group) the header of the record: (w, weighted KL, 0, 0)
template <int LPE>
__device__ __forceinline__ void next_record_header(const BwdArgs& b, int64_t e, int64_t xs, int lig, float w_next, float kl_next,
                                                   float cs_next, float io) {
  kl_next = group_sum<LPE>(kl_next);
  if (lig == 0)
    *reinterpret_cast<float4*>(b.zrec_next + (size_t)e * xs) = make_float4(w_next, kl_next * (cs_next * io), 0.f, 0.f);
}

// STAGE_ACC: store the statistics (dense: zeros for rows not in this shard); STAGE_APPLY: read the summed ones
template <int LPE, int CPL, int VEC>
__device__ __forceinline__ void store_statistics(float* rec, int C, int lig, const Chunk<VEC> (&A)[CPL], float gs, float cntf) {
#pragma unroll
  for (int i = 0; i < CPL; ++i) {
    const int j = chunk_of<LPE>(lig, i);
    if (j < C) st_chunk<VEC>(rec + 4 + (size_t)j * VEC, A[i]);
  }
  if (lig == 0) *reinterpret_cast<float4*>(rec) = make_float4(gs, cntf, 0.f, 0.f);
}
template <int LPE, int CPL, int VEC>
__device__ __forceinline__ void load_statistics(const float* rec, int C, int lig, Chunk<VEC> (&A)[CPL]) {
#pragma unroll
  for (int i = 0; i < CPL; ++i) {
    const int j = chunk_of<LPE>(lig, i);
    if (j < C) A[i] = ld_chunk<VEC>(rec + 4 + (size_t)j * VEC);
  }
}
// gradient form, entity not in the batch: the dense zero row
template <int LPE, int CPL, int VEC>
__device__ __forceinline__ void store_zero_row(float* grow_e, float* g_bias_e, int d, int C, int lig) {
  Chunk<VEC> zc;
#pragma unroll
  for (int t = 0; t < VEC; ++t) zc.v[t] = 0.f;
#pragma unroll
  for (int i = 0; i < CPL; ++i) {
    const int j = chunk_of<LPE>(lig, i);
    if (j < C) {
      st_chunk_nt<VEC>(grow_e + (size_t)j * VEC, zc);
      st_chunk_nt<VEC>(grow_e + d + (size_t)j * VEC, zc);
    }
  }
  if (lig == 0) *reinterpret_cast<float2*>(g_bias_e) = make_float2(0.f, 0.f);
}

// ---------------------------------------------------------------------------------------
// k_bwd.  Template parameters: the lane-group shape (LPE lanes per row, CPL chunks of VEC coordinates per lane), the eps
// source, ADAM 0 gradients / 1 dense Adam fused / 2 row-sparse Adam fused, the multi-rank STAGE, the link, and the forms
// of the fused single-sample dense step: MULTI (S > 1), PIPE (software-pipelined), LA (look-ahead lazy Adam).
// ---------------------------------------------------------------------------------------
template <int LPE, int CPL, int VEC, int EPS, int ADAM, int STAGE, int LINK, bool MULTI, bool PIPE = false, bool LA = false>
__global__ __launch_bounds__(BLOCK, (PIPE && CPL == 1) ? 4 : 1) void k_bwd(const KArgs a, const BwdArgs b, const AdamArgs ad_in) {
  constexpr int GPB = BLOCK / LPE;
  static_assert(!PIPE || (ADAM == 1 && STAGE == STAGE_FULL && !MULTI), "the pipelined step is the fused single-sample one");
  static_assert(!LA || (ADAM == 1 && STAGE == STAGE_FULL && !MULTI), "look-ahead lazy Adam is a form of the fused dense step");
  // step-dependent values: from the kernel arguments, or (replayable step, a.dev) from device memory
  AdamArgs ad = ad_in;
  RngKey key = a.key, next_key = b.next_key;
  int32_t la_step = b.la_step, la_k = b.la_k;
  if constexpr (ADAM == 1 && STAGE == STAGE_FULL)
    load_dev_step(a, key, ad, la_step, la_k, next_key,
                  blockIdx.x == 0 && threadIdx.x == 0 && a.row_filter != 3 && a.e_hi == a.T);
  __shared__ float sh_cs[VFM_MAX_FIELDS];
  __shared__ float sh_cs_next[PIPE ? VFM_MAX_FIELDS : 1];
  __shared__ int64_t sh_hi[VFM_MAX_FIELDS];
  __shared__ double sh_fin[7][BLOCK / 64];
  __shared__ float2 sh_tab[LA ? VFM_MOMENT_PERIOD + 1 : 1];      // LA: (a1, q2) of the period's earlier steps, for replays
  const int tid = threadIdx.x;
  const int lig = tid % LPE;
  const int d = a.d;
  const int C = (d + VEC - 1) / VEC;
  if (STAGE != STAGE_ACC && tid < a.G) {
    sh_cs[tid] = (float)(a.group_n[tid] / a.W[tid]);
    sh_hi[tid] = a.group_hi[tid];
    if constexpr (PIPE) sh_cs_next[tid] = b.zrec_next ? (float)(a.group_n[tid] / b.next_W[tid]) : 0.f;
  }
  if constexpr (LA) {
    for (int k = tid; k < la_k; k += BLOCK) sh_tab[k] = b.step_tab[k];
  }
  __syncthreads();
  if constexpr (LA) {
    if (blockIdx.x == 0 && tid == 0) b.step_tab[la_k] = make_float2(ad.a1, ad.q2);     // for later replays of this step
  }
  const float gout = (ADAM || STAGE == STAGE_ACC) ? 1.0f : b.grad_out[0];

  // a.row_filter (fused Adam, STAGE_FULL): 0 = every row; 2 = only the rows of the batch (+ the scalars and the loss);
  // 3 / 4 (the long-list pre-reduction overlapped with this kernel, vfm_abi.hip): 4 = every row but the heavy
  // entities (+ the scalars and the loss), 3 = the heavy entities only, listed
  scalars_and_loss<EPS, ADAM, STAGE, LINK, MULTI>(a, b, ad, key, gout, a.row_filter != 3, a.e_hi == a.T, sh_fin);

  const int64_t stride = (int64_t)gridDim.x * GPB;
  const int64_t xs = 4 + (((int64_t)d + 3) & ~(int64_t)3);          // floats per exchange record
  // fused Adam with a row list (the lazy exact-Adam step): li runs over the list (the batch's entities), not over
  // the table.  The SAME instance serves the dense step, so the two agree bit for bit on the rows they share
  // (different template instances are compiled with different fma contractions).
  // (the multi-rank stages take a list too -- vfm_elbo_bwd_acc_rows_f32 / vfm_elbo_apply_adam_rows_f32: the rows some
  // rank's shard contains; their records sit in the DENSE statistics table at the entity's own index, or, with
  // b.rec_by_slot, in a COMPACT buffer at the row's position in the list)
  const bool listed = b.row_ids != nullptr && (STAGE == STAGE_FULL ? ADAM != 0 : true);
  IndexGuard ig(a, b);
  const int64_t li_end = listed ? b.n_rows : a.e_hi;
  int64_t li = (listed ? 0 : a.e_lo) + (int64_t)blockIdx.x * GPB + tid / LPE;
  int64_t e_cur = li;
  int2 pq = make_int2(0, 0);
  fetch_row<STAGE>(b, listed, li, li_end, ig, e_cur, pq);
  for (; li < li_end; li += stride) {
    const int64_t e = listed ? e_cur : li;
    const int64_t rec = (listed && !b.rec_by_slot) ? e : li;      // where this row's statistics record sits (multi-rank stages)
    const int beg = pq.x, end = pq.y;
    float2 gc = make_float2(0.f, 0.f);                             // STAGE_APPLY: (sum of grow, occurrences) over ALL ranks
    if constexpr (STAGE == STAGE_APPLY) gc = *reinterpret_cast<const float2*>(b.acc + (size_t)rec * xs);
    fetch_row<STAGE>(b, listed, li + stride, li_end, ig, e_cur, pq);      // next entity's offsets, early
    bool in_next = false;          // PIPE: e is in the next batch -> its next-step record is written below
    if constexpr (PIPE) {
      if (b.zrec_next) in_next = b.next_occ_ptr[e + 1] != b.next_occ_ptr[e];
    }
    const bool touched = (STAGE == STAGE_APPLY) ? gc.y > 0.f : beg != end;
    const float cntf = (STAGE == STAGE_APPLY) ? gc.y : (float)(end - beg);
    int la_gap = 0;                        // LA: skipped zero-gradient steps this row applies before this step's update
    if constexpr (LA) {
      if (!touched && !(b.next_occ_ptr[e + 1] != b.next_occ_ptr[e])) continue;      // in neither batch: the row waits
      la_gap = (la_step - 1) - b.last_step[e];
    }
    if (ADAM == 2 && !touched) continue;   // opt-in row-sparse Adam: rows not in the batch stay as they are
    if (ADAM == 1 && STAGE == STAGE_FULL && a.row_filter == 2 && !touched) continue;

    RowRegs<VEC, CPL> r;
    if (STAGE != STAGE_ACC && (ADAM || touched))
      load_own_row<LPE, CPL, VEC, EPS, ADAM>(a, ad, e, d, C, lig, true, touched, touched || (PIPE && in_next), r);

    // walk the inverted index: A = sum_r g_r * sumz_r, gs = sum_r g_r
    int hslot = -1;
    if (STAGE != STAGE_APPLY && b.n_heavy > 0 && end - beg > VFM_HEAVY_MIN)
      hslot = heavy_slot_of(b.heavy_ids, b.n_heavy, (int)e);
    if (ADAM == 1 && STAGE == STAGE_FULL && a.row_filter == 4 && hslot >= 0) continue;   // (the heavy-only launch takes it)
    Chunk<VEC> A[CPL];
    float gs;
    walk_list<LPE, CPL, VEC, PIPE>(b, b.sumz, b.heavy_acc, hslot, beg, end, d, C, xs, lig, ig, A, gs);

    if constexpr (STAGE == STAGE_ACC) {
      store_statistics<LPE, CPL, VEC>(b.acc + (size_t)rec * xs, C, lig, A, gs, cntf);
      continue;
    }
    if constexpr (STAGE == STAGE_APPLY) {
      gs = gc.x;
      if (touched) load_statistics<LPE, CPL, VEC>(b.acc + (size_t)rec * xs, C, lig, A);
    }
    float* grow_e = ADAM ? nullptr : b.g_entity + (size_t)e * (2 * (size_t)d);
    if (!touched && !ADAM) {
      store_zero_row<LPE, CPL, VEC>(grow_e, b.g_bias + 2 * (size_t)e, d, C, lig);
      continue;
    }

    const float c = touched ? kl_weight(sh_cs, sh_hi, a.G, e, r.io, cntf) : 0.f;
    float nb_eps = 0.f;
    float nb_next = 0.f, kl_next = 0.f, w_next = 0.f;      // PIPE: the next step's first-order eps / KL / sampled weight
    // (MULTI is a template parameter so that the S = 1 instances carry none of this: registers, occupancy)
    constexpr bool multi = MULTI && STAGE == STAGE_FULL;
    Chunk<VEC> g1s[CPL], g2s[CPL];
    if (multi && touched)
      sample_means<LPE, CPL, VEC, EPS, LINK>(a, b, key, e, hslot, beg, end, d, C, xs, lig, ig, r, A, gs, g1s, g2s, nb_eps);
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      const int j = chunk_of<LPE>(lig, i);
      if (j < C) {
        Chunk<VEC> gm, gv;
        if (touched && multi) {
          chunk_grad_multi<VEC, LINK>(r.mu[i], r.s[i], g1s[i], g2s[i], c, gout, gm, gv);
        } else if (touched) {
          Chunk<VEC> epc;
          float nb;
          chunk_eps<VEC, EPS>(key, e, j, r.ep[i], epc, nb);
          if (EPS == EPS_PHILOX && i == 0) nb_eps = nb;
          chunk_grad<VEC, LINK, PIPE>(r.mu[i], r.s[i], epc, A[i], gs, c, gout, gm, gv);
        } else {
#pragma unroll
          for (int t = 0; t < VEC; ++t) { gm.v[t] = 0.f; gv.v[t] = 0.f; }
        }
        if constexpr (ADAM) {
          Chunk<VEC> pm, ps;
          adam_row_step<VEC, LA>(r.mu[i].v, r.s[i].v, r.mm[i].v, r.ms[i].v, r.vm[i].v, r.vs[i].v, gm.v, gv.v, la_gap, la_k, sh_tab,
                                 touched, ad, pm.v, ps.v);
          store_row_chunk<VEC>(a, ad, e, d, j, touched, pm, ps, r.mm[i], r.ms[i], r.vm[i], r.vs[i]);
          if constexpr (PIPE) {
            if (in_next) next_record_chunk<VEC, LINK>(b, next_key, e, j, xs, pm, ps, i == 0, nb_next, kl_next);
          }
        } else {
          st_chunk_nt<VEC>(grow_e + (size_t)j * VEC, gm);
          st_chunk_nt<VEC>(grow_e + d + (size_t)j * VEC, gv);
        }
      }
    }
    if (lig == 0) {
      float g0 = 0.f, g1 = 0.f;
      if (touched) {
        if constexpr (EPS == EPS_TABLE)
          if (!multi) nb_eps = r.epw;
        first_order_grad<LINK>(r.th, gs, nb_eps, c, gout, g0, g1);
      }
      if constexpr (LA) b.last_step[e] = la_step;
      if constexpr (ADAM) {
        const float2 pn = adam_pair_step<LA>(r.th, r.mb, r.vb, g0, g1, la_gap, la_k, sh_tab, touched, ad);
        store_first_order(a, ad, e, touched, pn, r.mb, r.vb);
        if constexpr (PIPE) {
          if (in_next) next_record_weight<LINK>(pn, nb_next, w_next, kl_next);
        }
      } else {
        *reinterpret_cast<float2*>(b.g_bias + 2 * (size_t)e) = make_float2(g0, g1);
      }
    }
    if constexpr (PIPE) {
      if (in_next) next_record_header<LPE>(b, e, xs, lig, w_next, kl_next, sh_cs_next[group_index(sh_hi, a.G, e)], r.io);
    }
  }
  ig.report(b.status);
}

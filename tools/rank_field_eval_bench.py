"""Held-out ranking evaluation in the field form (VFM.rank_heldout_field, include/vfm_rank.h:
vfm_rank_heldout_field_f32) at the ML-20M shape against its yardsticks.

A three-field model: 138,493 users x 26,744 items x 4 formats, d = 128; 8,192 (user, format) contexts, every context
with an exclusion list of ML-20M's size (about 116, geometric, at least 16) and held-out positives drawn geometric with
mean ~14, none of them excluded.  One JSON line per strategy, appended to profiles/rank_field_eval_bench.jsonl with
--record.  Times are HIP-event medians over `--reps` calls after `--warmup`, with the fastest and slowest call beside
them (`*_min`, `*_max`):
  ms            the op alone (workspace and CSRs made once, outside the loop)
  call_ms       the public VFM.rank_heldout_field (grouping, CSR building and the eligibility check included)
  split         kernel time of one call by name, from a torch.profiler trace: prep (k_field_ctx_prep +
                k_field_cand_prep), pos_score (k_field_pos_score), eval (k_rank_eval), other (sort, merge); in
                microseconds; null (with the reason on stderr) if the profiler is missing or records no device time
  torch_ms      the torch fp32 composition in the same process: query operands, addmm, masking, a per-row sort,
                searchsorted of every positive, the positives' own order for rank_neg
  agree         the fraction of positives whose composition rank equals the kernel's (torch mm does not round like the
                k-ordered chain, so this is below 1 where scores nearly tie)
  heldout2_ms   vfm_rank_heldout_f32 on a two-field model of the same queries, catalog, d, exclusions and positives."""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, warmup, reps):
    """(median, fastest, slowest) ms of fn over reps calls after warmup, by HIP events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def kernel_split(fn):
    groups = {"prep": ("k_field_ctx_prep", "k_field_cand_prep"), "pos_score": ("k_field_pos_score",),
              "eval": ("k_rank_eval<", "k_rank_evalILi")}
    try:
        from torch.profiler import ProfilerActivity, profile
    except ImportError as e:                           # (only a missing profiler gives null; a failing call raises)
        print(f"no kernel trace: {e}", file=sys.stderr)
        return None
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    out = {"prep": 0.0, "pos_score": 0.0, "eval": 0.0, "other": 0.0}
    for e in prof.key_averages():
        t = float(getattr(e, "device_time_total", 0.0) or getattr(e, "cuda_time_total", 0.0))
        name = next((g for g, keys in groups.items() if any(k in e.key for k in keys)), "other")
        out[name] += t
    if sum(out.values()) <= 0:
        print("no kernel trace: the profiler recorded no device time", file=sys.stderr)
        return None
    return {k: round(v, 1) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=8192)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--strategies", default="top,variance")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--record", action="store_true", help="append to profiles/rank_field_eval_bench.jsonl")
    args = ap.parse_args()
    from vae_amd import _lib, rank
    from vae_amd.model import VFM
    N, M, Fm, d, field = 138_493, 26_744, 4, args.d, 1
    sizes = [N, M, Fm]
    dev = torch.device("cuda")
    torch.manual_seed(0)
    m = VFM(field_sizes=sizes, embedding_size=d, output="class", device=dev)
    with torch.no_grad():
        m._flat.mul_(0.3)
    T, lo = m.T, N
    g = torch.Generator(device=dev).manual_seed(1)
    users = torch.randperm(N, device=dev, generator=g)[:args.queries].sort().values       # one format per user: the
    ctx = torch.stack([users, torch.zeros_like(users),                                    # two-field run has the same
                       N + M + torch.randint(0, Fm, (users.numel(),), device=dev, generator=g)], 1)      # queries
    Q = ctx.shape[0]
    lens = (torch.rand(Q, device=dev, generator=g).log() * (-(116 - 16))).long() + 16     # mean ~116
    ex = torch.repeat_interleave(ctx, lens, 0)
    ex[:, field] = lo + torch.randint(0, M, (ex.shape[0],), device=dev, generator=g)
    npos = (torch.rand(Q, device=dev, generator=g).log() * (-13.5)).long() + 1            # mean ~14
    pos = torch.repeat_interleave(ctx, npos, 0)
    pos[:, field] = lo + torch.randint(0, M, (pos.shape[0],), device=dev, generator=g)
    cols = [0, 2]
    ptr, ex_items = rank.field_exclusion_csr(ctx, ex, field, cols, T)
    qi = torch.repeat_interleave(torch.arange(Q, device=dev), npos)
    keep = ~rank._ineligible(pos[:, field], qi, None, ptr, ex_items, Q, T)                # none of them excluded
    pos = pos[keep]
    # the positives CSR over the FIXED queries (a context whose every draw was excluded keeps an empty segment)
    pptr, pitems = rank.exclusion_csr(torch.arange(Q, device=dev), torch.stack([qi[keep], pos[:, field]], 1), T)
    n_pos = pitems.numel()
    ent, bia, scal = m._views(m._flat)
    o = _lib.ops()
    qkey = ctx[:, 0].contiguous()
    i64 = dict(dtype=torch.int64, device=dev)
    outs = [torch.empty(n_pos, **i64), torch.empty(n_pos, **i64), torch.empty(Q, **i64), torch.empty(Q, **i64)]
    outs2 = [torch.empty_like(t) for t in outs]
    counts = pptr[1:] - pptr[:-1]
    pmax = int(counts.max())
    pq = torch.repeat_interleave(torch.arange(Q, device=dev), counts)
    pslot = torch.arange(n_pos, device=dev) - pptr[:-1][pq]
    mask_rows = torch.repeat_interleave(torch.arange(Q, device=dev), ptr[1:] - ptr[:-1])
    mask_cols = ex_items - lo
    # the two-field yardstick: the same users, items, exclusions and positives; tables of the same size
    m2 = VFM(N, M, d, output="class", device=dev)
    with torch.no_grad():
        m2._flat.mul_(0.3)
    e2, b2, s2f = m2._views(m2._flat)
    for strategy in args.strategies.split(","):
        code = rank.STRATEGIES[strategy]
        ws = torch.empty(o.rank_eval_field_workspace_bytes(Q, M, n_pos, 3, d, code, 0), dtype=torch.uint8, device=dev)

        def run():
            o.rank_heldout_field(ctx, field, qkey, None, M, lo, ptr, ex_items, pptr, pitems, ent, bia, scal, ws, *outs,
                                 code, 0, 7, 0)
        ms, ms_min, ms_max = timed(run, args.warmup, args.reps)
        cms, cms_min, cms_max = timed(lambda: m.rank_heldout_field(pos, field, exclude=ex, strategy=strategy, seed=7),
                                      1, max(3, args.reps // 2))
        rec = {"strategy": strategy, "queries": Q, "catalog": M, "F": 3, "d": d, "excluded": int(ex_items.numel()),
               "positives": n_pos, "max_positives": pmax, "ms": round(ms, 4), "ms_min": round(ms_min, 4),
               "ms_max": round(ms_max, 4), "call_ms": round(cms, 4), "call_ms_min": round(cms_min, 4),
               "call_ms_max": round(cms_max, 4), "reps": args.reps, "workspace_mb": round(ws.numel() / 2 ** 20, 1),
               "split_us": kernel_split(run)}
        if not args.no_torch and strategy != "random":
            mu, s2 = ent[:, :d], ent[:, d:].abs() ** 2
            mu_c, s2_c = mu[lo:lo + M], s2[lo:lo + M]

            def comp():
                e, b = ent[ctx[:, cols]], bia[ctx[:, cols]]                     # [Q, F-1, 2d]: the gather is part of it
                mq, sq = e[..., :d], e[..., d:].abs() ** 2
                Mq, Aq = mq.sum(1), sq.sum(1)
                if strategy in ("top", "mean"):
                    cm = scal[1] + b[..., 0].sum(1) + 0.5 * (Mq ** 2 - (mq ** 2).sum(1)).sum(1)
                    Sm = torch.addmm(cm[:, None] + bia[lo:lo + M, 0][None, :], Mq, mu_c.T)
                if strategy in ("variance", "mean"):
                    dm = Mq[:, None, :] - mq
                    cv = (scal[2] ** 2 + (b[..., 1] ** 2).sum(1)
                          + (0.5 * (Aq ** 2 - (sq ** 2).sum(1)) + (sq * dm ** 2).sum(1)).sum(1))
                    A3 = torch.cat([Aq, Aq + Mq ** 2, 2 * (sq * dm).sum(1)], 1)
                    B3 = torch.cat([mu_c ** 2, s2_c, mu_c], 1)
                    Sv = torch.addmm(cv[:, None] + (bia[lo:lo + M, 1] ** 2)[None, :], A3, B3.T)
                S = Sm if strategy == "top" else Sv if strategy == "variance" else \
                    -Sm.abs() / torch.sqrt(1 + math.pi / 8 * Sv)
                S[mask_rows, mask_cols] = -float("inf")
                ps = S[pq, pitems - lo]                                      # the positives' scores
                desc = torch.sort(S, dim=1, descending=True).values
                q = torch.full((Q, pmax), float("inf"), device=dev)
                q[pq, pslot] = -ps
                r = torch.searchsorted(-desc, q)                             # #{c : S_c > s_i}
                r_pos = r[pq, pslot]
                rr = torch.full((Q, pmax), torch.iinfo(torch.int64).max, **i64)
                rr[pq, pslot] = r_pos
                within = torch.sort(rr, dim=1).indices.argsort(1)            # each positive's place among its query's
                return r_pos, r_pos - within[pq, pslot]
            tms, tms_min, tms_max = timed(comp, args.warmup, args.reps)
            r_pos, r_neg = comp()
            run()
            torch.cuda.synchronize()
            rec.update({"torch_ms": round(tms, 4), "torch_ms_min": round(tms_min, 4), "torch_ms_max": round(tms_max, 4),
                        "speedup_vs_torch": round(tms / ms, 2),
                        "agree": round(float((r_pos == outs[0]).double().mean()), 5),
                        "agree_neg": round(float((r_neg == outs[1]).double().mean()), 5)})
        ws2 = torch.empty(o.rank_eval_workspace_bytes(Q, M, n_pos, d, code, 0), dtype=torch.uint8, device=dev)

        def run2():
            o.rank_heldout(users, None, M, N, ptr, ex_items, pptr, pitems, e2, b2, s2f, ws2, *outs2, 2, code, 0, 7, 0)
        hms, hms_min, hms_max = timed(run2, args.warmup, args.reps)
        rec.update({"heldout2_ms": round(hms, 4), "heldout2_ms_min": round(hms_min, 4),
                    "heldout2_ms_max": round(hms_max, 4), "vs_heldout2": round(ms / hms, 2)})
        del ws, ws2
        print(json.dumps(rec), flush=True)
        if args.record:
            with open(os.path.join(ROOT, "profiles", "rank_field_eval_bench.jsonl"), "a") as f:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

"""Ranking under supplied posteriors (VFM.rank_field_posterior / rank_heldout_field_posterior, include/vfm_rank.h:
vfm_rank_field_post_f32, vfm_rank_heldout_field_post_f32) at the ML-20M shape of tools/rank_field_eval_bench.py, against
what they replace and against the plain table form, in the same run.

A three-field model: 138,493 users x 26,744 items x 4 formats, d = 128; 8,192 (user, format) contexts with distinct
users, every context with an exclusion list of ML-20M's size and held-out positives (mean ~14), none of them excluded;
one posterior row per query for the user column.  Per op (rank: top 10; heldout) three forms on the same queries:
  post      the posterior form: theta rows read by the prep kernel
  table     the table form on the model as it is (no posterior: the floor the posterior form should sit on)
  replace   what the posterior form replaces: clone the users' parameter rows, scatter theta into them, run the table
            form, restore the rows
The rounds are interleaved (post, table, replace, post, ...) after `--warmup` rounds; times are HIP-event medians over
`--reps` rounds with the fastest and slowest beside them.  The ops are timed alone (workspace and CSRs made once).  The
posterior form and the replace form return the same bits (checked once per op).  One JSON line per op, appended to
profiles/rank_posterior_bench.jsonl with --record."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def interleaved(fns, warmup, reps):
    """{name: (median, fastest, slowest) ms} of the callables, one of each per round, by HIP events."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[name].append(a.elapsed_time(b))
    out = {}
    for name, v in ts.items():
        v.sort()
        out[name] = (v[len(v) // 2], v[0], v[-1])
    return out


@torch.no_grad()
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=8192)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--strategy", default="top")
    ap.add_argument("--record", action="store_true", help="append to profiles/rank_posterior_bench.jsonl")
    args = ap.parse_args()
    from vae_amd import _lib, rank
    from vae_amd.model import VFM
    N, M, Fm, d, field, post_field, k = 138_493, 26_744, 4, args.d, 1, 0, args.k
    dev = torch.device("cuda")
    torch.manual_seed(0)
    m = VFM(field_sizes=[N, M, Fm], embedding_size=d, output="class", device=dev)
    with torch.no_grad():
        m._flat.mul_(0.3)
    T, lo = m.T, N
    g = torch.Generator(device=dev).manual_seed(1)
    users = torch.randperm(N, device=dev, generator=g)[:args.queries].sort().values
    ctx = torch.stack([users, torch.zeros_like(users),
                       N + M + torch.randint(0, Fm, (users.numel(),), device=dev, generator=g)], 1).contiguous()
    Q = ctx.shape[0]
    lens = (torch.rand(Q, device=dev, generator=g).log() * (-(116 - 16))).long() + 16     # mean ~116
    ex = torch.repeat_interleave(ctx, lens, 0)
    ex[:, field] = lo + torch.randint(0, M, (ex.shape[0],), device=dev, generator=g)
    ptr, ex_items = rank.field_exclusion_csr(ctx, ex, field, [0, 2], T)
    npos = (torch.rand(Q, device=dev, generator=g).log() * (-13.5)).long() + 1            # mean ~14
    qi = torch.repeat_interleave(torch.arange(Q, device=dev), npos)
    pid = lo + torch.randint(0, M, (qi.numel(),), device=dev, generator=g)
    keep = ~rank._ineligible(pid, qi, None, ptr, ex_items, Q, T)                          # none of them excluded
    pptr, pitems = rank.query_csr(qi[keep], pid[keep], Q, T)
    n_pos = pitems.numel()
    ent, bia, scal = m._views(m._flat)
    theta = (torch.randn(Q, 2 * d + 2, device=dev, generator=g) * 0.3).contiguous()
    o = _lib.ops()
    code = rank.STRATEGIES[args.strategy]
    qkey = ctx[:, 0].contiguous()
    f32, i64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int64, device=dev)

    def replaced(run):
        """clone the users' rows, scatter theta, run the table form, restore"""
        def fn():
            e0, b0 = ent[users].clone(), bia[users].clone()
            ent[users] = theta[:, :2 * d]
            bia[users] = theta[:, 2 * d:]
            run()
            ent[users] = e0
            bia[users] = b0
        return fn

    recs = []
    # ---- top k
    ws = torch.empty(o.rank_field_workspace_bytes(Q, M, 3, d, k, code, 0), dtype=torch.uint8, device=dev)
    outs = {n: [torch.empty(Q, k, **i64)] + [torch.empty(Q, k, **f32) for _ in range(3)] for n in ("post", "table", "replace")}
    table = lambda name: (lambda: o.rank_field(ctx, field, qkey, None, M, lo, ptr, ex_items, ent, bia, scal, ws,
                                               *outs[name], k, code, 0, 7, 0))
    fns = {"post": lambda: o.rank_field_post(ctx, field, theta, post_field, qkey, None, M, lo, ptr, ex_items, ent, bia,
                                             scal, ws, *outs["post"], k, code, 0, 7, 0),
           "table": table("table"), "replace": replaced(table("replace"))}
    t = interleaved(fns, args.warmup, args.reps)
    torch.cuda.synchronize()
    same = all(torch.equal(a.view(torch.int32) if a.dtype.is_floating_point else a,
                           b.view(torch.int32) if b.dtype.is_floating_point else b)
               for a, b in zip(outs["post"], outs["replace"]))
    recs.append(("rank_field", t, same, ws.numel()))
    del ws
    # ---- held-out ranks
    ws = torch.empty(o.rank_eval_field_workspace_bytes(Q, M, n_pos, 3, d, code, 0), dtype=torch.uint8, device=dev)
    houts = {n: [torch.empty(n_pos, **i64), torch.empty(n_pos, **i64), torch.empty(Q, **i64), torch.empty(Q, **i64)]
             for n in ("post", "table", "replace")}
    htable = lambda name: (lambda: o.rank_heldout_field(ctx, field, qkey, None, M, lo, ptr, ex_items, pptr, pitems, ent,
                                                        bia, scal, ws, *houts[name], code, 0, 7, 0))
    fns = {"post": lambda: o.rank_heldout_field_post(ctx, field, theta, post_field, qkey, None, M, lo, ptr, ex_items,
                                                     pptr, pitems, ent, bia, scal, ws, *houts["post"], code, 0, 7, 0),
           "table": htable("table"), "replace": replaced(htable("replace"))}
    t = interleaved(fns, args.warmup, args.reps)
    torch.cuda.synchronize()
    same = all(torch.equal(a, b) for a, b in zip(houts["post"], houts["replace"]))
    recs.append(("rank_heldout_field", t, same, ws.numel()))
    for op, t, same, wsb in recs:
        rec = {"op": op, "strategy": args.strategy, "queries": Q, "catalog": M, "F": 3, "d": d, "k": k,
               "excluded": int(ex_items.numel()), "positives": n_pos, "reps": args.reps,
               "workspace_mb": round(wsb / 2 ** 20, 1), "bitwise_equal_to_replace": bool(same)}
        for name, (med, lo_, hi_) in t.items():
            rec.update({f"{name}_ms": round(med, 4), f"{name}_ms_min": round(lo_, 4), f"{name}_ms_max": round(hi_, 4)})
        rec["post_vs_table"] = round(t["post"][0] / t["table"][0], 3)
        rec["post_vs_replace"] = round(t["post"][0] / t["replace"][0], 3)
        print(json.dumps(rec), flush=True)
        if args.record:
            with open(os.path.join(ROOT, "profiles", "rank_posterior_bench.jsonl"), "a") as f:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

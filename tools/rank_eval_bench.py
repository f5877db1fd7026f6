"""Held-out ranking evaluation (include/vfm_rank.h: vfm_rank_heldout_f32) at the ML-20M shape against the torch fp32
composition.

One JSON line per strategy: 8,192 users, all 26,744 items, d = 128, every user with an exclusion list of ML-20M's size
(about 116 train ratings per user, drawn geometric, at least 16) and held-out positives drawn geometric with mean ~14
(the first user: 1,100 draws, over 1,000 distinct), none of them excluded.  Times are HIP-event medians over `--reps` calls after `--warmup`:
`ms` the op alone (workspace and CSRs made once, outside the loop), `call_ms` the public VFM.rank_heldout (CSR building
and the eligibility check included), `torch_ms` the composition: addmm + bias terms + masking + a per-row sort +
searchsorted of every positive + the positives' own order for rank_neg.  `agree` is the fraction of positives whose
composition rank equals the kernel's (the composition's scores round differently: torch mm is not the k-ordered
chain).  Then one all-user pass (138,493 users, `top`), the kernel only: the composition's [U, M] score matrix alone
would be 14.8 GB."""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, warmup, reps):
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
    return ts[len(ts) // 2], ts[0]


def workload(users, N, M, g, heavy=1100):
    """(exclusion rows, positive rows) of the query users: geometric lists, positives outside the exclusions."""
    dev = users.device
    U = users.numel()
    T = N + M
    lens = (torch.rand(U, device=dev, generator=g).log() * (-(116 - 16))).long() + 16        # mean ~116
    ex_u = torch.repeat_interleave(users, lens)
    ex = torch.stack([ex_u, N + torch.randint(0, M, (ex_u.numel(),), device=dev, generator=g)], 1)
    npos = (torch.rand(U, device=dev, generator=g).log() * (-13.5)).long() + 1                # mean ~14
    npos[0] = heavy
    pu = torch.repeat_interleave(users, npos)
    pos = torch.stack([pu, N + torch.randint(0, M, (pu.numel(),), device=dev, generator=g)], 1)
    ek = torch.unique(ex[:, 0] * T + ex[:, 1])
    pk = torch.unique(pos[:, 0] * T + pos[:, 1])
    j = torch.searchsorted(ek, pk).clamp_(max=ek.numel() - 1)
    pk = pk[ek[j] != pk]
    return ex, torch.stack([pk // T, pk % T], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=8192)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--strategies", default="top,variance")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-all-users", action="store_true")
    args = ap.parse_args()
    from vae_amd import _lib, rank
    from vae_amd.model import VFM
    N, M, d, U = 138_493, 26_744, args.d, args.users
    dev = torch.device("cuda")
    torch.manual_seed(0)
    m = VFM(N, M, d, output="class", device=dev)
    with torch.no_grad():
        m._flat.mul_(0.3)
    g = torch.Generator(device=dev).manual_seed(1)
    users = torch.randperm(N, device=dev, generator=g)[:U].sort().values
    ex, pos = workload(users, N, M, g)
    ent, bia, scal = m._views(m._flat)
    o = _lib.ops()
    ptr, ex_items = rank.exclusion_csr(users, ex, m.T)
    pptr, pitems = rank.exclusion_csr(users, pos, m.T)
    n_pos = pitems.numel()
    i64 = dict(dtype=torch.int64, device=dev)
    outs = [torch.empty(n_pos, **i64), torch.empty(n_pos, **i64), torch.empty(U, **i64), torch.empty(U, **i64)]
    counts = pptr[1:] - pptr[:-1]
    pmax = int(counts.max())
    puser = torch.repeat_interleave(torch.arange(U, device=dev), counts)
    pslot = torch.arange(n_pos, device=dev) - pptr[:-1][puser]
    mask_rows = torch.repeat_interleave(torch.arange(U, device=dev), ptr[1:] - ptr[:-1])
    mask_cols = ex_items - N
    for strategy in args.strategies.split(","):
        code = rank.STRATEGIES[strategy]
        ws = torch.empty(o.rank_eval_workspace_bytes(U, M, n_pos, d, code, 0), dtype=torch.uint8, device=dev)

        def run():
            o.rank_heldout(users, None, M, N, ptr, ex_items, pptr, pitems, ent, bia, scal, ws, *outs, 2, code, 0, 7, 0)
        ms, ms_min = timed(run, args.warmup, args.reps)
        cms, _ = timed(lambda: m.rank_heldout(pos, exclude=ex, strategy=strategy, seed=7), 1, max(3, args.reps // 2))
        K = {"top": d, "variance": 2 * d, "mean": 3 * d, "random": 0}[strategy]
        rec = {"strategy": strategy, "users": U, "items": M, "d": d, "excluded": int(ex_items.numel()),
               "positives": n_pos, "max_positives": pmax, "ms": round(ms, 4), "ms_min": round(ms_min, 4),
               "call_ms": round(cms, 4), "workspace_mb": round(ws.numel() / 2 ** 20, 1),
               "tflops": None if not K else round(2.0 * U * M * K / (ms * 1e-3) / 1e12, 2)}
        if not args.no_torch and strategy != "random":
            mu, sg = ent[:, :d], ent[:, d:].abs()
            mu_u, mu_i, sg_u, sg_i = mu[users], mu[N:], sg[users], sg[N:]
            cu, ci = (scal[1] + bia[users, 0])[:, None], bia[N:, 0][None, :]
            vu, vi = (scal[2].abs() ** 2 + bia[users, 1] ** 2)[:, None], (bia[N:, 1] ** 2)[None, :]
            A2, B2 = torch.cat([mu_u ** 2, sg_u ** 2], 1), torch.cat([sg_i ** 2, mu_i ** 2 + sg_i ** 2], 1)

            def comp():
                if strategy in ("top", "mean"):
                    Sm = torch.addmm(cu + ci, mu_u, mu_i.T)
                if strategy in ("variance", "mean"):
                    Sv = torch.addmm(vu + vi, A2, B2.T)
                S = Sm if strategy == "top" else Sv if strategy == "variance" else \
                    -Sm.abs() / torch.sqrt(1 + math.pi / 8 * Sv)
                S[mask_rows, mask_cols] = -float("inf")
                ps = S[puser, pitems - N]                                   # the positives' scores
                desc = torch.sort(S, dim=1, descending=True).values
                q = torch.full((U, pmax), float("inf"), device=dev)
                q[puser, pslot] = -ps
                r = torch.searchsorted(-desc, q)                             # #{c : S_c > s_i}
                r_pos = r[puser, pslot]
                rr = torch.full((U, pmax), torch.iinfo(torch.int64).max, **i64)
                rr[puser, pslot] = r_pos
                within = torch.sort(rr, dim=1).indices.argsort(1)            # each positive's place among its user's
                return r_pos, r_pos - within[puser, pslot]
            tms, tms_min = timed(comp, args.warmup, args.reps)
            r_pos, r_neg = comp()
            run()
            torch.cuda.synchronize()
            rec.update({"torch_ms": round(tms, 4), "torch_ms_min": round(tms_min, 4), "speedup": round(tms / ms, 2),
                        "agree": round(float((r_pos == outs[0]).double().mean()), 5),
                        "agree_neg": round(float((r_neg == outs[1]).double().mean()), 5)})
        print(json.dumps(rec), flush=True)
    if not args.no_all_users:
        del ws
        Ua = N
        ua = torch.arange(Ua, device=dev)
        ex, pos = workload(ua, N, M, g)
        ptr, ex_items = rank.exclusion_csr(ua, ex, m.T)
        pptr, pitems = rank.exclusion_csr(ua, pos, m.T)
        n_pos = pitems.numel()
        outs = [torch.empty(n_pos, **i64), torch.empty(n_pos, **i64), torch.empty(Ua, **i64), torch.empty(Ua, **i64)]
        ws = torch.empty(o.rank_eval_workspace_bytes(Ua, M, n_pos, d, 0, 0), dtype=torch.uint8, device=dev)

        def run_all():
            o.rank_heldout(ua, None, M, N, ptr, ex_items, pptr, pitems, ent, bia, scal, ws, *outs, 2, 0, 0, 7, 0)
        ms, ms_min = timed(run_all, 1, 3)
        metrics, _ = rank.ranking_metrics(outs[0], outs[1], pptr, outs[3], ks=(10,))
        print(json.dumps({"strategy": "top", "users": Ua, "items": M, "d": d, "excluded": int(ex_items.numel()),
                          "positives": n_pos, "ms": round(ms, 4), "ms_min": round(ms_min, 4),
                          "workspace_mb": round(ws.numel() / 2 ** 20, 1),
                          "tflops": round(2.0 * Ua * M * d / (ms * 1e-3) / 1e12, 2),
                          "auc": round(metrics["auc"], 4)}), flush=True)


if __name__ == "__main__":
    main()

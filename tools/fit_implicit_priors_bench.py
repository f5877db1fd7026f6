"""Hierarchical implicit sweeps (include/vfm_implicit_prior.h; VFM.fit_implicit(priors=, learn_priors=True)): what a field
prior costs in a sweep, and what learning it buys on planted clicks whose two fields live at different scales.

One JSON line per measurement (also appended to profiles/fit_implicit_priors_bench.jsonl with --write):
  sweep    the shape of tools/fit_implicit_bench.py (138,493 x 26,744, d = 128, --rows distinct observed pairs, Zipf
           items): one fit_implicit sweep (both fields' plans, built once outside the timed span) under priors= against
           the same sweep with priors=None, interleaved round by round in one process, HIP-event medians (and minima) over
           --reps-sweep rounds after --warmup-sweep; every call starts from the same parameters (restored inside the timed
           span).  The priors=None leg runs twice per round, so its own spread is in the line beside the ratio.  The prior
           adds 2 (d + 1) loads per workgroup and a few FMAs per coordinate: a ratio, no threshold.
  planted  clicks planted from user factors of std 0.3 and item factors of std 1.0: J_imp per sweep, the learnt
           precisions and held-out recall / NDCG@10 of fit_implicit with the fixed N(0, 1) prior, with learn_priors=True,
           and at each kl_weight of a small grid (the best of which is what a grid search would have found).  Values only."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from fit_exact_bench import D, M, N, _model  # noqa: E402
from foldin_exact_bench import interleaved, stats  # noqa: E402


def sweep(args, dev):
    from vae_amd import sweep as sw
    from vae_amd.data import synthetic_triples
    m = _model(dev)
    X, _ = synthetic_triples((N, M), args.rows, seed=2, device=dev, zipf=args.zipf)
    key = torch.unique(X[:, 0] * (N + M) + X[:, 1])                       # distinct pairs
    X = torch.stack([key // (N + M), key % (N + M)], 1)
    y = torch.ones(X.shape[0], device=dev)
    start = m._flat.clone()
    x, yy, w0, w1 = sw.check_implicit_args(m, X, y, args.w0, 1.0, 1.0)
    plans = [sw.ImplicitPlan(m, x, yy, f) for f in range(2)]
    pr = sw.GroupPriors(2, D, dev)
    g = torch.Generator().manual_seed(5)
    pr.load_state_dict({"mean": (torch.rand(2, D + 1, generator=g) - 0.5) * 0.2,
                        "prec": torch.exp((torch.rand(2, D + 1, generator=g) - 0.5) * 2.0)})
    rows = [pr.row(f) for f in range(2)]

    def run(priors):
        def fn():
            m._flat.copy_(start)
            for f, p in enumerate(plans):
                p.run(m, 1.0, w0, w1, rows[f] if priors else None)
        return fn

    t = interleaved({"priors": run(True), "none": run(False), "none_again": run(False)}, args.warmup_sweep, args.reps_sweep)
    med = lambda v: v[len(v) // 2]
    rec = {"what": "sweep", "pairs": N * M, "observed": int(X.shape[0]), "zipf": args.zipf, "d": D, "w0": w0,
           "warmup": args.warmup_sweep, "reps": args.reps_sweep}
    rec.update({k + "_ms": stats(v) for k, v in t.items()})
    rec["priors_over_none"] = round(med(t["priors"]) / med(t["none"]), 4)
    rec["none_again_over_none"] = round(med(t["none_again"]) / med(t["none"]), 4)
    return rec


def planted_clicks_scaled(n_u, n_i, rank, per_user, seed, std_u=0.3, std_i=1.0):
    """Each user's per_user clicks: the items with the largest planted affinity plus Gumbel noise, the two fields' planted
    factors at different scales.  Distinct pairs."""
    g = torch.Generator().manual_seed(seed)
    U, V = torch.randn(n_u, rank, generator=g) * std_u, torch.randn(n_i, rank, generator=g) * std_i
    noise = -torch.log(-torch.log(torch.rand(n_u, n_i, generator=g)))
    items = torch.topk((U @ V.T) / (std_u * std_i) + noise, per_user, dim=1).indices
    users = torch.arange(n_u).repeat_interleave(per_user)
    return torch.stack([users, n_u + items.reshape(-1)], 1)


def planted(args, dev):
    from vae_amd.model import VFM
    n_u, n_i, d = 2000, 800, 16
    X = planted_clicks_scaled(n_u, n_i, 6, 30, seed=3)
    held = torch.rand(X.shape[0], generator=torch.Generator().manual_seed(4)) < 0.2
    Xtr, Xte = X[~held].to(dev), X[held].to(dev)
    ones = lambda x: torch.ones(x.shape[0], device=dev)

    def metrics(m):
        r = m.evaluate_ranking(Xte, ones(Xte), ks=(10,), exclude=Xtr, threshold=0.5)
        return round(r["recall@10"], 4), round(r["ndcg@10"], 4)

    def fit(**kw):
        torch.manual_seed(0)
        m = VFM(n_u, n_i, embedding_size=d, output="reg", device=dev)
        out = m.fit_implicit(Xtr, n_sweeps=args.sweeps, w0=args.w0, **kw)
        rec = {"J": [round(v, 2) for v in out["objective"]], "recall_ndcg_at_10": metrics(m)}
        if "priors" in out:
            pr = out["priors"].prec.cpu()
            rec["prec_weight"] = [round(float(pr[f, 0]), 4) for f in range(2)]
            rec["prec_factors_min_median_max"] = [[round(float(v), 4) for v in (pr[f, 1:].min(), pr[f, 1:].median(),
                                                                              pr[f, 1:].max())] for f in range(2)]
            rec["clamped"] = out["clamped"]
        return rec

    grid = {str(k): fit(kl_weight=k) for k in (0.1, 0.3, 1.0, 3.0, 10.0)}
    return {"what": "planted", "users": n_u, "items": n_i, "d": d, "std_users": 0.3, "std_items": 1.0,
            "train_rows": int(Xtr.shape[0]), "w0": args.w0, "sweeps": args.sweeps, "fixed_standard_prior": grid["1.0"],
            "learn_priors": fit(learn_priors=True), "kl_weight_grid": grid,
            "best_kl_weight_by_recall": max(grid, key=lambda k: grid[k]["recall_ndcg_at_10"][0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="sweep,planted")
    ap.add_argument("--warmup-sweep", type=int, default=1)
    ap.add_argument("--reps-sweep", type=int, default=3)
    ap.add_argument("--rows", type=int, default=20_000_000)
    ap.add_argument("--zipf", type=float, default=1.0)
    ap.add_argument("--w0", type=float, default=0.05, help="a starting value: nobody has measured a good one")
    ap.add_argument("--sweeps", type=int, default=8)
    ap.add_argument("--write", action="store_true", help="append the lines to profiles/fit_implicit_priors_bench.jsonl")
    ap.add_argument("--note", default=None, help="kept in the line: what was measured, e.g. the commit")
    args = ap.parse_args()
    dev = torch.device("cuda")
    for what in args.what.split(","):
        rec = {"sweep": sweep, "planted": planted}[what](args, dev)
        rec.update({"device": torch.cuda.get_device_name(0), "when": time.strftime("%Y-%m-%dT%H:%M:%S")})
        if args.note:
            rec["note"] = args.note
        print(json.dumps(rec), flush=True)
        if args.write:
            with open(os.path.join(ROOT, "profiles", "fit_implicit_priors_bench.jsonl"), "a") as f:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

"""Hierarchical bound sweeps (include/vfm_bound_prior.h; VFM.fit_bound(priors=, learn_priors=True)): what a field prior
costs and what learning it buys.

One JSON line per measurement (also appended to profiles/fit_bound_priors_bench.jsonl with --write):
  cost_heavy  one sweep of both fields (no bias block) over the heavy shape of tools/fit_bound_bench.py (10,000 users x 20
              rows and one user of 5,000, d = 128, ML-20M table shape), with priors= against priors=None
  cost_sweep  the same over --rows rows at the ML-20M table shape, Zipf items, split_rows="auto"
              The prior adds 2 (d + 1) loads per workgroup and a few FMAs per coordinate and round, so the expectation
              is a ratio within the spread of the parent's own rounds of 1; the ratio is recorded, nothing is asserted.
              The plans are built once, outside the timed span, as fit_bound builds them.
  benefit     planted 'class' data whose factor std is 0.3 for the users and 1.0 for the items: J, held-out AUC and the
              learnt prec per sweep for the fixed N(0, 1) prior, for learn_priors=True, and for each kl_weight of a small
              grid under the fixed prior (values only; J is each run's own objective)
The calls compared are interleaved round by round in one process; times are HIP-event medians (and minima) over --reps
rounds after --warmup; every call starts from the same parameters (restored inside the timed span)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from fit_bound_bench import D, M, N, _auc, _model  # noqa: E402
from fit_priors_bench import _drawn_priors  # noqa: E402
from foldin_exact_bench import interleaved, stats  # noqa: E402


def _cost(m, X, y, what, n_iters, warmup, reps, dev):
    from vae_amd import foldin, sweep as sw
    start = m._flat.clone()
    pr = _drawn_priors(m, dev)
    plans = [sw.SweepPlan(m, *foldin.check_args_bound(m, X, y, f, 1.0, 1), f, "auto", bound=True) for f in range(2)]
    rows = [pr.row(f) for f in range(2)]

    def one(with_prior):
        def fn():
            m._flat.copy_(start)
            for f, p in enumerate(plans):
                p.run_bound(m, 1.0, n_iters, False, rows[f] if with_prior else None)
        return fn

    t = interleaved({"none": one(False), "priors": one(True)}, warmup, reps)
    rec = {"what": what, "rows": int(X.shape[0]), "d": D, "n_iters": n_iters,
           "split_entities": [p.E - p.n_light for p in plans], "warmup": warmup, "reps": reps}
    rec.update({k + "_ms": stats(v) for k, v in t.items()})
    rec["priors_over_none"] = round(t["priors"][len(t["priors"]) // 2] / t["none"][len(t["none"]) // 2], 4)
    rec["none_max_over_min"] = round(max(t["none"]) / min(t["none"]), 4)      # (the parent's own spread, to read the ratio by)
    return rec


def cost_heavy(args, dev):
    m = _model(dev)
    g = torch.Generator(device=dev).manual_seed(1)
    users = torch.randperm(N, device=dev, generator=g)[:10_000]
    n = torch.full((10_000,), 20, device=dev, dtype=torch.int64)
    n[7] = 5000
    u = users.repeat_interleave(n)
    X = torch.stack([u, N + torch.randint(0, M, (u.numel(),), device=dev, generator=g)], 1)
    y = (torch.rand(u.numel(), device=dev, generator=g) < 0.25).float()
    return _cost(m, X, y, "cost_heavy", args.n_iters, args.warmup, args.reps, dev)


def cost_sweep(args, dev):
    from vae_amd.data import synthetic_triples
    m = _model(dev)
    X, y = synthetic_triples((N, M), args.rows, seed=2, output="class", device=dev, zipf=args.zipf)
    rec = _cost(m, X, y, "cost_sweep", args.n_iters, args.warmup_sweep, args.reps_sweep, dev)
    rec["zipf"] = args.zipf
    return rec


def benefit(args, dev):
    from vae_amd import sweep as sw
    from vae_amd.model import VFM
    n_u, n_i, d, k = 2000, 800, 16, 8
    g = torch.Generator().manual_seed(3)
    U, V = torch.randn(n_u, k, generator=g) * 0.3, torch.randn(n_i, k, generator=g) * 1.0
    R = 120_000
    u, i = torch.randint(0, n_u, (R,), generator=g), torch.randint(0, n_i, (R,), generator=g)
    y = (torch.rand(R, generator=g) < torch.sigmoid(-0.5 + 3.0 * (U[u] * V[i]).sum(1))).float()
    X = torch.stack([u, n_u + i], 1)
    tr = torch.rand(R, generator=g) < 0.9
    Xtr, ytr, Xte, yte = X[tr].to(dev), y[tr].to(dev), X[~tr].to(dev), y[~tr].to(dev)

    def run(kl_weight=1.0, learn=False):
        torch.manual_seed(0)
        m = VFM(n_u, n_i, embedding_size=d, output="class", device=dev)
        pr = sw.GroupPriors(2, d, dev) if learn else None
        auc, pc = [], []

        def on_step(s, w):
            if w == "bias":
                auc.append(round(_auc(m.predictive_moments(Xte)[0], yte), 4))
                if learn:
                    pc.append([[round(v, 3) for v in row] for row in pr.prec.tolist()])

        out = m.fit_bound(Xtr, ytr, n_sweeps=args.sweeps, kl_weight=kl_weight, n_iters=args.n_iters, on_step=on_step,
                          priors=pr, learn_priors=learn)
        rec = {"J": [round(v, 2) for v in out["objective"]], "auc": auc}
        if learn:
            rec.update({"prec": pc, "clamped": out["clamped"]})
        return rec

    grid = {str(w): run(kl_weight=w) for w in args.kl_grid}
    best = max(grid, key=lambda w: grid[w]["auc"][-1])
    return {"what": "benefit", "users": n_u, "items": n_i, "d": d, "factor_std": [0.3, 1.0], "train_rows": int(Xtr.shape[0]),
            "sweeps": args.sweeps, "n_iters": args.n_iters, "fixed": run(), "learn_priors": run(learn=True),
            "kl_weight_grid": grid, "best_kl_weight_by_final_auc": float(best)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="cost_heavy,cost_sweep,benefit")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup-sweep", type=int, default=1)
    ap.add_argument("--reps-sweep", type=int, default=3)
    ap.add_argument("--rows", type=int, default=20_000_000)
    ap.add_argument("--zipf", type=float, default=1.0)
    ap.add_argument("--n-iters", type=int, default=2)
    ap.add_argument("--sweeps", type=int, default=8)
    ap.add_argument("--kl-grid", type=float, nargs="+", default=[0.25, 0.5, 1.0, 2.0, 4.0])
    ap.add_argument("--write", action="store_true", help="append the lines to profiles/fit_bound_priors_bench.jsonl")
    ap.add_argument("--note", default=None, help="kept in the line: what was measured, e.g. the commit")
    args = ap.parse_args()
    dev = torch.device("cuda")
    for what in args.what.split(","):
        rec = {"cost_heavy": cost_heavy, "cost_sweep": cost_sweep, "benefit": benefit}[what](args, dev)
        rec.update({"device": torch.cuda.get_device_name(0), "when": time.strftime("%Y-%m-%dT%H:%M:%S")})
        if args.note:
            rec["note"] = args.note
        print(json.dumps(rec), flush=True)
        if args.write:
            with open(os.path.join(ROOT, "profiles", "fit_bound_priors_bench.jsonl"), "a") as f:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

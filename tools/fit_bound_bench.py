"""The split bound rounds (VFM.fold_in_bound(split_rows=...), VFM.fit_bound) measured: tools/fit_exact_bench.py's
counterpart for 'class' models.

One JSON line per measurement (also appended to profiles/fit_bound_bench.jsonl with --write):
  heavy   the heavy shape of tools/foldin_exact_bench.py with labels: 10,000 users x 20 rows and one user of 5,000,
          d = 128, ML-20M table shape; fold_in_bound unsplit against split_rows="auto" (and chunk_rows 256 / 512),
          interleaved round by round in one process
  sweep   one fit_bound sweep (both fields, no bias block) over --rows rows at the ML-20M table shape, Zipf items
          (synthetic_triples(..., zipf=--zipf)), F = 2, d = 128, for n_iters in --n-iters.  The split path only: the
          unsplit bound at the heaviest item (1.86 M rows at 20 M rows) would run for minutes.  The plans are built
          once, outside the timed span, as fit_bound builds them; every timed sweep starts from the same parameters.
  curve   J per sweep of fit_bound at that shape for n_iters in --n-iters (values only: the data the default of
          n_iters can later be chosen from)
  auc     planted 'class' data: J and held-out AUC per sweep of fit_bound for n_iters in --n-iters, beside fit()
          (values only)
Times are HIP-event medians (and minima) over the rounds after the warm-ups.  Run each measurement as a step of its own
under its own time limit, one process each:
  for w in heavy sweep curve auc; do timeout -k 10 500 python tools/fit_bound_bench.py --what $w --write || break; done"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from foldin_exact_bench import interleaved, stats  # noqa: E402

N, M, D = 138_493, 26_744, 128


def _model(dev):
    from vae_amd.model import VFM
    torch.manual_seed(0)
    m = VFM(N, M, embedding_size=D, output="class", device=dev)
    with torch.no_grad():
        m._flat.mul_(0.3)
    return m


def _median(v):
    return v[len(v) // 2]


def heavy(args, dev):
    m = _model(dev)
    g = torch.Generator(device=dev).manual_seed(1)
    users = torch.randperm(N, device=dev, generator=g)[:10_000]
    n = torch.full((10_000,), 20, device=dev, dtype=torch.int64)
    n[7] = 5000
    u = users.repeat_interleave(n)
    X = torch.stack([u, N + torch.randint(0, M, (u.numel(),), device=dev, generator=g)], 1)
    y = (torch.rand(u.numel(), device=dev, generator=g) < 0.25).float()
    start = m._flat.clone()

    def call(**kw):
        def fn():
            m._flat.copy_(start)
            return m.fold_in_bound(X, y, **kw)
        return fn

    fns = {"unsplit": call(), "split": call(split_rows="auto")}
    fns.update({f"split_chunk{c}": call(split_rows="auto", chunk_rows=c) for c in (256, 512)})
    t = interleaved(fns, args.warmup, args.reps)
    rec = {"what": "heavy", "entities": 10_000, "rows": int(X.shape[0]), "d": D, "n_iters": 8, "split_rows": 4 * (D + 1),
           "warmup": args.warmup, "reps": args.reps}
    rec.update({k + "_ms": stats(v) for k, v in t.items()})
    rec["unsplit_over_split"] = round(_median(t["unsplit"]) / _median(t["split"]), 3)
    return rec


def _sweep_setup(args, dev):
    from vae_amd import foldin, sweep as sw
    from vae_amd.data import synthetic_triples
    m = _model(dev)
    X, y = synthetic_triples((N, M), args.rows, seed=2, output="class", device=dev, zipf=args.zipf)
    plans = [sw.SweepPlan(m, *foldin.check_args_bound(m, X, y, f, 1.0, 1), f, "auto", bound=True) for f in range(2)]
    return m, X, y, plans


def sweep(args, dev):
    m, X, y, plans = _sweep_setup(args, dev)
    start = m._flat.clone()

    def one(n_iters):
        def fn():
            m._flat.copy_(start)
            for p in plans:
                p.run_bound(m, 1.0, n_iters, False)
        return fn

    t = interleaved({f"n_iters{k}": one(k) for k in args.n_iters}, args.warmup_sweep, args.reps_sweep)
    rec = {"what": "sweep", "rows": int(X.shape[0]), "zipf": args.zipf, "d": D, "path": "split only",
           "heaviest_user_item": [int(p.counts.max()) for p in plans],
           "split_entities": [p.E - p.n_light for p in plans], "groups": [len(p.groups) for p in plans],
           "chunks": [sum(g[3].shape[0] for g in p.groups) for p in plans],
           "warmup": args.warmup_sweep, "reps": args.reps_sweep}
    rec.update({k + "_ms": stats(v) for k, v in t.items()})
    return rec


def curve(args, dev):
    from vae_amd import sweep as sw
    m, X, y, plans = _sweep_setup(args, dev)
    start = m._flat.clone()
    seen = torch.unique(X)
    rec = {"what": "curve", "rows": int(X.shape[0]), "zipf": args.zipf, "d": D, "sweeps": args.sweeps_curve,
           "update_bias": True}
    for k in args.n_iters:
        m._flat.copy_(start)
        J = [float(sw.bound_objective_terms(m, X, y, seen, 1.0))]
        for _ in range(args.sweeps_curve):
            for p in plans:
                p.run_bound(m, 1.0, k, False)
            sw.update_bias_bound(m, X, y, 1.0)
            J.append(float(sw.bound_objective_terms(m, X, y, seen, 1.0)))
        rec[f"J_n_iters{k}"] = [round(v, 1) for v in J]
    return rec


def _auc(score, label):
    """Area under the ROC curve by the rank-sum formula (ties by average rank are not needed for continuous scores)."""
    order = torch.argsort(score)
    rank = torch.empty_like(order, dtype=torch.float64)
    rank[order] = torch.arange(1, score.numel() + 1, dtype=torch.float64, device=score.device)
    pos = label > 0.5
    n1, n0 = int(pos.sum()), int((~pos).sum())
    return float((rank[pos].sum() - n1 * (n1 + 1) / 2) / (n1 * n0))


def auc(args, dev):
    """Planted data: labels drawn from the logit of a drawn rank-8 model; 90 % train, 10 % held out."""
    from vae_amd.model import VFM
    n_u, n_i, d = 2000, 800, 16
    g = torch.Generator().manual_seed(3)
    U, V = torch.randn(n_u, 8, generator=g) * 0.8, torch.randn(n_i, 8, generator=g) * 0.8
    R = 120_000
    u, i = torch.randint(0, n_u, (R,), generator=g), torch.randint(0, n_i, (R,), generator=g)
    logit = -0.5 + (U[u] * V[i]).sum(1)
    y = (torch.rand(R, generator=g) < torch.sigmoid(logit)).float()
    X = torch.stack([u, n_u + i], 1)
    tr = torch.rand(R, generator=g) < 0.9
    Xtr, ytr, Xte, yte = X[tr].to(dev), y[tr].to(dev), X[~tr].to(dev), y[~tr].to(dev)
    rec = {"what": "auc", "users": n_u, "items": n_i, "d": d, "train_rows": int(Xtr.shape[0]),
           "heldout_rows": int(Xte.shape[0]), "sweeps": args.sweeps,
           "auc_of_the_planted_logit": round(_auc(logit[~tr].to(dev), yte), 4)}

    def held(m):
        return _auc(m.predictive_moments(Xte)[0], yte)

    for k in args.n_iters:
        torch.manual_seed(0)
        m = VFM(n_u, n_i, embedding_size=d, output="class", device=dev)
        a = []
        out = m.fit_bound(Xtr, ytr, n_sweeps=args.sweeps, n_iters=k,
                          on_step=lambda s, w: a.append(held(m)) if w == "bias" else None)
        rec[f"fit_bound_n_iters{k}"] = {"J": [round(v, 2) for v in out["objective"]], "auc": [round(v, 4) for v in a],
                                        "ms": [round(v, 3) for v in out["ms"]]}
    torch.manual_seed(0)
    m = VFM(n_u, n_i, embedding_size=d, output="class", device=dev)
    ja, aa = [], []
    for _ in range(args.sweeps):
        m.fit(Xtr, ytr, n_epochs=5, batch_size=20_000, verbose=False)
        ja.append(m.bound_objective(Xtr, ytr))
        aa.append(held(m))
    rec["fit_every_5_epochs"] = {"J": [round(v, 2) for v in ja], "auc": [round(v, 4) for v in aa]}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="heavy,sweep,curve,auc")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup-sweep", type=int, default=1)
    ap.add_argument("--reps-sweep", type=int, default=3)
    ap.add_argument("--rows", type=int, default=20_000_000)
    ap.add_argument("--zipf", type=float, default=1.0)
    ap.add_argument("--n-iters", type=lambda s: [int(v) for v in s.split(",")], default=[1, 2, 8])
    ap.add_argument("--sweeps", type=int, default=8)
    ap.add_argument("--sweeps-curve", type=int, default=3)
    ap.add_argument("--write", action="store_true", help="append the lines to profiles/fit_bound_bench.jsonl")
    ap.add_argument("--note", default=None, help="kept in the line: what was measured, e.g. the commit")
    args = ap.parse_args()
    dev = torch.device("cuda")
    for what in args.what.split(","):
        rec = {"heavy": heavy, "sweep": sweep, "curve": curve, "auc": auc}[what](args, dev)
        rec.update({"device": torch.cuda.get_device_name(0), "when": time.strftime("%Y-%m-%dT%H:%M:%S")})
        if args.note:
            rec["note"] = args.note
        print(json.dumps(rec), flush=True)
        if args.write:
            with open(os.path.join(ROOT, "profiles", "fit_bound_bench.jsonl"), "a") as f:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

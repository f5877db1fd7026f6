"""The split exact solve (VFM.fold_in_exact(split_rows=...), VFM.fit_exact) against the unsplit call of the same run.

One JSON line per measurement (also appended to profiles/fit_exact_bench.jsonl with --write):
  heavy   the heavy shape of tools/foldin_exact_bench.py: 10,000 users x 20 ratings and one user of 5,000, d = 128,
          ML-20M table shape; fold_in_exact unsplit against split_rows="auto"
  sweep   one sweep (both fields, no scalars) over --rows rows at the ML-20M table shape, Zipf items
          (synthetic_triples(..., zipf=--zipf)), F = 2, d = 128: unsplit against split with chunk_rows 512 / 2048 / 8192.
          The plans are built once, outside the timed span, as fit_exact builds them.
  curve   J and held-out RMSE per sweep of fit_exact against fit() on the same planted data (values only)
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

from foldin_exact_bench import interleaved, stats  # noqa: E402

N, M, D = 138_493, 26_744, 128


def _model(dev):
    from vae_amd.model import VFM
    torch.manual_seed(0)
    m = VFM(N, M, embedding_size=D, output="reg", device=dev)
    with torch.no_grad():
        m._flat.mul_(0.3)
    return m


def heavy(args, dev):
    m = _model(dev)
    g = torch.Generator(device=dev).manual_seed(1)
    users = torch.randperm(N, device=dev, generator=g)[:10_000]
    n = torch.full((10_000,), 20, device=dev, dtype=torch.int64)
    n[7] = 5000
    u = users.repeat_interleave(n)
    X = torch.stack([u, N + torch.randint(0, M, (u.numel(),), device=dev, generator=g)], 1)
    y = torch.randint(1, 6, (u.numel(),), device=dev, generator=g).float()
    start = m._flat.clone()

    def call(**kw):
        def fn():
            m._flat.copy_(start)
            return m.fold_in_exact(X, y, **kw)
        return fn

    fns = {"unsplit": call(), "split": call(split_rows="auto")}
    fns.update({f"split_chunk{c}": call(split_rows="auto", chunk_rows=c) for c in (256, 512)})
    t = interleaved(fns, args.warmup, args.reps)
    rec = {"what": "heavy", "entities": 10_000, "rows": int(X.shape[0]), "d": D, "split_rows": 4 * (D + 1)}
    rec.update({k + "_ms": stats(v) for k, v in t.items()})
    rec["unsplit_over_split"] = round(t["unsplit"][len(t["unsplit"]) // 2] / t["split"][len(t["split"]) // 2], 3)
    return rec


def sweep(args, dev):
    from vae_amd import foldin, sweep as sw
    from vae_amd.data import synthetic_triples
    m = _model(dev)
    X, y = synthetic_triples((N, M), args.rows, seed=2, device=dev, zipf=args.zipf)
    start = m._flat.clone()
    forms = {"unsplit": dict(split_rows=None), "split": dict(split_rows="auto")}
    forms.update({f"split_chunk{c}": dict(split_rows="auto", chunk_rows=c) for c in (512, 8192)})
    plans = {}
    for k, kw in forms.items():
        plans[k] = [sw.SweepPlan(m, *foldin.check_args_exact(m, X, y, f, 1.0), f, **kw) for f in range(2)]
    heaviest = [int(p.counts.max()) for p in plans["unsplit"]]

    def one(k):
        def fn():
            m._flat.copy_(start)
            for p in plans[k]:
                p.run(m, 1.0)
        return fn

    t = interleaved({k: one(k) for k in forms}, args.warmup_sweep, args.reps_sweep)
    rec = {"what": "sweep", "rows": int(X.shape[0]), "zipf": args.zipf, "d": D, "heaviest_user_item": heaviest,
           "split_entities": [p.E - p.n_light for p in plans["split"]],
           "chunks": [sum(g[3].shape[0] for g in p.groups) for p in plans["split"]], "reps": args.reps_sweep}
    rec.update({k + "_ms": stats(v) for k, v in t.items()})
    rec["unsplit_over_split"] = round(t["unsplit"][len(t["unsplit"]) // 2] / t["split"][len(t["split"]) // 2], 3)
    return rec


def curve(args, dev):
    """Planted data: ratings from a drawn rank-8 model plus noise; 90 % train, 10 % held out."""
    from vae_amd.model import VFM
    n_u, n_i, d = 2000, 800, 16
    g = torch.Generator().manual_seed(3)
    U, V = torch.randn(n_u, 8, generator=g) * 0.6, torch.randn(n_i, 8, generator=g) * 0.6
    R = 120_000
    u, i = torch.randint(0, n_u, (R,), generator=g), torch.randint(0, n_i, (R,), generator=g)
    y = 3.0 + (U[u] * V[i]).sum(1) + 0.3 * torch.randn(R, generator=g)
    X = torch.stack([u, n_u + i], 1)
    tr = torch.rand(R, generator=g) < 0.9
    Xtr, ytr, Xte, yte = X[tr].to(dev), y[tr].to(dev), X[~tr].to(dev), y[~tr].to(dev)

    def rmse(m):
        return float(((m.predictive_moments(Xte)[0] - yte) ** 2).mean().sqrt())

    torch.manual_seed(0)
    m = VFM(n_u, n_i, embedding_size=d, output="reg", device=dev)
    rm = []
    out = m.fit_exact(Xtr, ytr, n_sweeps=args.sweeps, on_step=lambda s, w: rm.append(rmse(m)) if w == "scalars" else None)
    torch.manual_seed(0)
    a = VFM(n_u, n_i, embedding_size=d, output="reg", device=dev)
    ja, ra = [], []
    for _ in range(args.sweeps):
        a.fit(Xtr, ytr, n_epochs=5, batch_size=20_000, verbose=False)
        ja.append(a.exact_objective(Xtr, ytr))
        ra.append(rmse(a))
    return {"what": "curve", "users": n_u, "items": n_i, "d": d, "train_rows": int(Xtr.shape[0]),
            "fit_exact_J": [round(v, 2) for v in out["objective"]], "fit_exact_rmse": [round(v, 4) for v in rm],
            "fit_exact_ms": [round(v, 3) for v in out["ms"]],
            "fit_J_every_5_epochs": [round(v, 2) for v in ja], "fit_rmse_every_5_epochs": [round(v, 4) for v in ra]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="heavy,sweep,curve")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup-sweep", type=int, default=1)
    ap.add_argument("--reps-sweep", type=int, default=3)
    ap.add_argument("--rows", type=int, default=20_000_000)
    ap.add_argument("--zipf", type=float, default=1.0)
    ap.add_argument("--sweeps", type=int, default=8)
    ap.add_argument("--write", action="store_true", help="append the lines to profiles/fit_exact_bench.jsonl")
    ap.add_argument("--note", default=None, help="kept in the line: what was measured, e.g. the commit")
    args = ap.parse_args()
    dev = torch.device("cuda")
    for what in args.what.split(","):
        rec = {"heavy": heavy, "sweep": sweep, "curve": curve}[what](args, dev)
        if what != "curve":
            rec.update({"warmup": args.warmup if what == "heavy" else args.warmup_sweep,
                        "reps": args.reps if what == "heavy" else args.reps_sweep})
        rec.update({"device": torch.cuda.get_device_name(0), "when": time.strftime("%Y-%m-%dT%H:%M:%S")})
        if args.note:
            rec["note"] = args.note
        print(json.dumps(rec), flush=True)
        if args.write:
            with open(os.path.join(ROOT, "profiles", "fit_exact_bench.jsonl"), "a") as f:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

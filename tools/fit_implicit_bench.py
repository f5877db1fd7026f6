"""One fit_implicit sweep (both fields, every (user, item) pair) against one fit_exact sweep over the observed rows alone.

One JSON line per measurement (also appended to profiles/fit_implicit_bench.jsonl with --write):
  sweep   the ML-20M shape of tools/fit_exact_bench.py: 138,493 x 26,744, d = 128, --rows distinct observed pairs, Zipf
          items.  The plans are built once, outside the timed span.  The yardstick, fit_exact's sweep, sees the observed
          rows only and does strictly less work: the ratio is recorded, no threshold is claimed.
  curve   J_imp per sweep and held-out recall / NDCG@10 of fit_implicit beside fit_exact on the same planted clicks
          (values only)
The two calls are interleaved round by round in one process; times are HIP-event medians (and minima) over --reps-sweep
rounds after --warmup-sweep; every call starts from the same parameters (restored inside the timed span)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "examples"))

from fit_exact_bench import D, M, N, _model  # noqa: E402
from foldin_exact_bench import interleaved, stats  # noqa: E402


def sweep(args, dev):
    from vae_amd import foldin, sweep as sw
    from vae_amd.data import synthetic_triples
    m = _model(dev)
    X, _ = synthetic_triples((N, M), args.rows, seed=2, device=dev, zipf=args.zipf)
    key = torch.unique(X[:, 0] * (N + M) + X[:, 1])                       # distinct pairs
    X = torch.stack([key // (N + M), key % (N + M)], 1)
    y = torch.ones(X.shape[0], device=dev)
    start = m._flat.clone()
    x, yy, w0, w1 = sw.check_implicit_args(m, X, y, args.w0, 1.0, 1.0)
    imp = [sw.ImplicitPlan(m, x, yy, f) for f in range(2)]
    exa = [sw.SweepPlan(m, *foldin.check_args_exact(m, X, y, f, 1.0), f, split_rows="auto") for f in range(2)]

    def run(plans, *a):
        def fn():
            m._flat.copy_(start)
            for p in plans:
                p.run(m, 1.0, *a)
        return fn

    t = interleaved({"implicit": run(imp, w0, w1), "exact_observed_only": run(exa)}, args.warmup_sweep, args.reps_sweep)
    rec = {"what": "sweep", "pairs": N * M, "observed": int(X.shape[0]), "zipf": args.zipf, "d": D, "w0": w0,
           "chunks": [sum(g[3].shape[0] for g in p.obs.groups) for p in imp],
           "entities_without_rows": [int(p.empty.numel()) for p in imp],
           "warmup": args.warmup_sweep, "reps": args.reps_sweep}
    rec.update({k + "_ms": stats(v) for k, v in t.items()})
    med = lambda v: v[len(v) // 2]
    rec["implicit_over_exact"] = round(med(t["implicit"]) / med(t["exact_observed_only"]), 3)
    return rec


def curve(args, dev):
    from fit_implicit_synthetic import planted_clicks
    from vae_amd.model import VFM
    n_u, n_i, d = 2000, 800, 16
    X = planted_clicks(n_u, n_i, 6, 30, seed=3)
    held = torch.rand(X.shape[0], generator=torch.Generator().manual_seed(4)) < 0.2
    Xtr, Xte = X[~held].to(dev), X[held].to(dev)
    ones = lambda x: torch.ones(x.shape[0], device=dev)

    def metrics(m):
        r = m.evaluate_ranking(Xte, ones(Xte), ks=(10,), exclude=Xtr, threshold=0.5)
        return round(r["recall@10"], 4), round(r["ndcg@10"], 4)

    torch.manual_seed(0)
    m = VFM(n_u, n_i, embedding_size=d, output="reg", device=dev)
    rm = []
    out = m.fit_implicit(Xtr, n_sweeps=args.sweeps, w0=args.w0,
                         on_step=lambda s, w: rm.append(metrics(m)) if w == "scalars" else None)
    torch.manual_seed(0)
    e = VFM(n_u, n_i, embedding_size=d, output="reg", device=dev)
    re_ = []
    e.fit_exact(Xtr, ones(Xtr), n_sweeps=args.sweeps, on_step=lambda s, w: re_.append(metrics(e)) if w == "scalars" else None)
    return {"what": "curve", "users": n_u, "items": n_i, "d": d, "train_rows": int(Xtr.shape[0]), "w0": args.w0,
            "fit_implicit_J": [round(v, 2) for v in out["objective"]], "fit_implicit_ms": [round(v, 3) for v in out["ms"]],
            "fit_implicit_recall_ndcg_at_10": rm, "fit_exact_recall_ndcg_at_10": re_}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="sweep,curve")
    ap.add_argument("--warmup-sweep", type=int, default=1)
    ap.add_argument("--reps-sweep", type=int, default=3)
    ap.add_argument("--rows", type=int, default=20_000_000)
    ap.add_argument("--zipf", type=float, default=1.0)
    ap.add_argument("--w0", type=float, default=0.05, help="a starting value: nobody has measured a good one")
    ap.add_argument("--sweeps", type=int, default=8)
    ap.add_argument("--write", action="store_true", help="append the lines to profiles/fit_implicit_bench.jsonl")
    ap.add_argument("--note", default=None, help="kept in the line: what was measured, e.g. the commit")
    args = ap.parse_args()
    dev = torch.device("cuda")
    for what in args.what.split(","):
        rec = {"sweep": sweep, "curve": curve}[what](args, dev)
        rec.update({"device": torch.cuda.get_device_name(0), "when": time.strftime("%Y-%m-%dT%H:%M:%S")})
        if args.note:
            rec["note"] = args.note
        print(json.dumps(rec), flush=True)
        if args.write:
            with open(os.path.join(ROOT, "profiles", "fit_implicit_bench.jsonl"), "a") as f:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

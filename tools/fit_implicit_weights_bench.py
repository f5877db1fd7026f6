"""Weighted implicit sweeps (include/vfm_implicit_weights.h; VFM.fit_implicit(weights=)): what a weight per observed pair
costs in a sweep, and what planted play counts buy over the binarised call.

One JSON line per measurement (also appended to profiles/fit_implicit_weights_bench.jsonl with --write):
  sweep    the shape of tools/fit_implicit_bench.py (138,493 x 26,744, d = 128, --rows distinct observed pairs, Zipf
           items): one fit_implicit sweep (both fields' plans, built once outside the timed span) with weights= against
           the same sweep with weights=None, interleaved round by round in one process, HIP-event medians (and minima) over
           --reps-sweep rounds after --warmup-sweep; every call starts from the same parameters (restored inside the timed
           span).  The weights=None leg runs twice per round, so its own spread is in the line beside the ratio.  Per row
           of a 4 x 4 tile the weights add 4 multiplies and one fp32 load to 16 FMAs and 8 loads: a ratio, no threshold.
  planted  clicks with planted play counts that grow with the planted preference
           (examples/fit_implicit_synthetic.planted_counts): J_imp per sweep and held-out recall / NDCG@10 of fit_implicit
           with weights=hkv_weights(counts, w0, alpha) for a few alpha and with log_eps, against the binarised call (all
           ones, w1 = 1).  Values only; the J_imp of different weights are different objectives."""
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
    from vae_amd import sweep as sw
    from vae_amd.data import synthetic_triples
    m = _model(dev)
    X, _ = synthetic_triples((N, M), args.rows, seed=2, device=dev, zipf=args.zipf)
    key = torch.unique(X[:, 0] * (N + M) + X[:, 1])                       # distinct pairs
    X = torch.stack([key // (N + M), key % (N + M)], 1)
    y = torch.ones(X.shape[0], device=dev)
    g = torch.Generator().manual_seed(5)
    counts = 1.0 + torch.poisson(torch.full((X.shape[0],), 2.0), generator=g)
    wts = sw.hkv_weights(counts, args.w0, 1.0 / args.w0).to(dev)
    start = m._flat.clone()
    x, yy, w0, w1 = sw.check_implicit_args(m, X, y, args.w0, 1.0, 1.0, weights=wts)
    plain = [sw.ImplicitPlan(m, x, yy, f) for f in range(2)]
    weighted = [sw.ImplicitPlan(m, x, yy, f, weights=wts) for f in range(2)]

    def run(plans, w):
        def fn():
            m._flat.copy_(start)
            for p in plans:
                p.run(m, 1.0, w0, w1, None, w)
        return fn

    t = interleaved({"weights": run(weighted, wts), "none": run(plain, None), "none_again": run(plain, None)},
                    args.warmup_sweep, args.reps_sweep)
    med = lambda v: v[len(v) // 2]
    rec = {"what": "sweep", "pairs": N * M, "observed": int(X.shape[0]), "zipf": args.zipf, "d": D, "w0": w0,
           "weights_min_max": [round(float(wts.min()), 4), round(float(wts.max()), 4)],
           "warmup": args.warmup_sweep, "reps": args.reps_sweep}
    rec.update({k + "_ms": stats(v) for k, v in t.items()})
    rec["weights_over_none"] = round(med(t["weights"]) / med(t["none"]), 4)
    rec["none_again_over_none"] = round(med(t["none_again"]) / med(t["none"]), 4)
    return rec


def planted(args, dev):
    from fit_implicit_synthetic import planted_counts
    from vae_amd import sweep as sw
    from vae_amd.model import VFM
    n_u, n_i, d = 2000, 800, 16
    X, counts = planted_counts(n_u, n_i, 6, 30, seed=3)
    held = torch.rand(X.shape[0], generator=torch.Generator().manual_seed(4)) < 0.2
    Xtr, Xte, ctr = X[~held].to(dev), X[held].to(dev), counts[~held]
    ones = lambda x: torch.ones(x.shape[0], device=dev)

    def metrics(m):
        r = m.evaluate_ranking(Xte, ones(Xte), ks=(10,), exclude=Xtr, threshold=0.5)
        return round(r["recall@10"], 4), round(r["ndcg@10"], 4)

    def fit(weights=None):
        torch.manual_seed(0)
        m = VFM(n_u, n_i, embedding_size=d, output="reg", device=dev)
        t0 = time.perf_counter()
        out = m.fit_implicit(Xtr, n_sweeps=args.sweeps, w0=args.w0, weights=None if weights is None else weights.to(dev))
        torch.cuda.synchronize()
        rec = {"J": [round(v, 2) for v in out["objective"]], "recall_ndcg_at_10": metrics(m),
               "ms_per_sweep": round(1e3 * (time.perf_counter() - t0) / max(out["sweeps"], 1), 2)}
        if weights is not None:
            rec["weights_min_max"] = [round(float(weights.min()), 4), round(float(weights.max()), 4)]
        return rec

    unit = 1.0 / args.w0                                                   # w0 (1 + unit c) = w0 + c
    rec = {"what": "planted", "users": n_u, "items": n_i, "d": d, "train_rows": int(Xtr.shape[0]), "w0": args.w0,
           "sweeps": args.sweeps, "counts_min_mean_max": [float(ctr.min()), round(float(ctr.mean()), 3), float(ctr.max())],
           "binarised": fit()}
    for name, alpha in (("alpha_0.25_over_w0", 0.25 * unit), ("alpha_1_over_w0", unit), ("alpha_4_over_w0", 4.0 * unit)):
        rec[name] = fit(sw.hkv_weights(ctr, args.w0, alpha))
    rec["alpha_1_over_w0_log_eps_1"] = fit(sw.hkv_weights(ctr, args.w0, unit, log_eps=1.0))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="sweep,planted")
    ap.add_argument("--warmup-sweep", type=int, default=1)
    ap.add_argument("--reps-sweep", type=int, default=3)
    ap.add_argument("--rows", type=int, default=20_000_000)
    ap.add_argument("--zipf", type=float, default=1.0)
    ap.add_argument("--w0", type=float, default=0.05, help="a starting value: nobody has measured a good one")
    ap.add_argument("--sweeps", type=int, default=8)
    ap.add_argument("--write", action="store_true", help="append the lines to profiles/fit_implicit_weights_bench.jsonl")
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
            with open(os.path.join(ROOT, "profiles", "fit_implicit_weights_bench.jsonl"), "a") as f:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

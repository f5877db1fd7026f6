"""Target-aware elicitation (include/vfm_design.h, `VFM.elicit_field_design`) beside the exact session it is built on,
in one process:
  (a) `elicit_field_design`: the design score, targets = each respondent's held-out contexts;
  (b) `elicit_field_exact(strategy="variance")`: the same session with the reference's heuristic.

One shape, one JSON line (appended to profiles/elicit_design_bench.jsonl with --record): tools/elicit_field_exact_bench.py's
-- 10,000 respondents x 100-row pools, F = 3 (user, item, format: ML-20M's user and item counts and 4 formats), d = 128,
'reg', 20 rounds, cold start, planted answers (the model's own mean prediction plus N(0, 0.5^2) noise).  Times: the two
calls interleaved (a, b, a, b, ..), HIP-event medians over `--reps` rounds after `--warmup`, the whole public call each;
both leave the model as they found it.  Quality: `elicitation_ranking_curve_field(exact=True)` of random / variance /
design on the first `--curve-respondents` respondents, whose held-out rows (`--test-rows` each, planted the same way;
relevant: the top quarter of the planted answers) are also the design targets; values only, no threshold."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--respondents", type=int, default=10_000)
    ap.add_argument("--pool", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--test-rows", type=int, default=20)
    ap.add_argument("--curve-respondents", type=int, default=300)
    ap.add_argument("--record", action="store_true", help="append the line to profiles/elicit_design_bench.jsonl")
    ap.add_argument("--note", default=None, help="kept in the line: what was measured, e.g. the commit")
    args = ap.parse_args()
    from vae_amd.model import VFM
    dev = torch.device("cuda")
    torch.manual_seed(0)
    N, M, K = 138_493, 26_744, 4
    m = VFM(field_sizes=[N, M, K], embedding_size=128, output="reg", device=dev)
    with torch.no_grad():
        m._flat.mul_(0.3)
    g = torch.Generator(device=dev).manual_seed(1)
    field = 0

    def rows(users, per):
        R = users.numel() * per
        return torch.stack([users.repeat_interleave(per), N + torch.randint(0, M, (R,), device=dev, generator=g),
                            N + M + torch.randint(0, K, (R,), device=dev, generator=g)], 1)

    def planted(x):
        truth, _, _ = m.field_moments(x, field)
        return truth + 0.5 * torch.randn(x.shape[0], device=dev, generator=g)

    users = torch.sort(torch.randperm(N, device=dev, generator=g)[:args.respondents]).values
    pool = rows(users, args.pool)
    y_pool = planted(pool)
    X_test = rows(users, args.test_rows)
    y_test = planted(X_test)
    start = m._flat.clone()

    def design():
        m.elicit_field_design(pool, y_pool, args.rounds, field, targets=X_test, reset=True)

    def variance():
        m.elicit_field_exact(pool, y_pool, args.rounds, field, "variance", reset=True)

    calls = (("design", design), ("variance", variance))
    ts = {k: [] for k, _ in calls}
    for rep in range(args.warmup + args.reps):              # interleaved: a, b, a, b, ..
        for k, fn in calls:
            t = once(fn)
            if rep >= args.warmup:
                ts[k].append(t)
    med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}

    nc = min(args.curve_respondents, args.respondents)
    keep = users[:nc]
    pm, tm = torch.isin(pool[:, field], keep), torch.isin(X_test[:, field], keep)
    thr = float(torch.quantile(y_test[tm], 0.75))
    curves = m.elicitation_ranking_curve_field(pool[pm], y_pool[pm], args.rounds, field, X_test[tm], y_test[tm], 1,
                                               ks=(10,), strategies=("random", "variance", "design"), exact=True,
                                               threshold=thr, ineligible="drop", reset=True, targets=X_test[tm])
    assert torch.equal(m._flat, start)
    rec = {"shape": "ml20m_formats", "respondents": args.respondents, "pool_rows": pool.shape[0], "F": 3, "field": field,
           "d": m.d, "rounds": args.rounds, "warmup": args.warmup, "reps": args.reps,
           "design_session_ms": round(med["design"], 3), "variance_session_ms": round(med["variance"], 3),
           "design_over_variance": round(med["design"] / med["variance"], 3),
           "design_ms_all": [round(t, 3) for t in ts["design"]], "variance_ms_all": [round(t, 3) for t in ts["variance"]],
           "curve_respondents": nc, "test_rows": args.test_rows, "relevance_threshold": round(thr, 4),
           "n_queries": curves["n_queries"],
           **{f"ndcg10_{s}": [round(v, 5) for v in curves[s]["ndcg@10"]] for s in ("random", "variance", "design")},
           "device": torch.cuda.get_device_name(0), "when": time.strftime("%Y-%m-%dT%H:%M:%S")}
    if args.note:
        rec["note"] = args.note
    print(json.dumps(rec), flush=True)
    if args.record:
        with open(os.path.join(ROOT, "profiles", "elicit_design_bench.jsonl"), "a") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

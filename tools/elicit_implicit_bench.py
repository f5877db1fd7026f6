"""The implicit field-form session (include/vfm_elicit_implicit.h: vfm_elicit_implicit_f32, `VFM.elicit_field_implicit`)
against the loop it replaces, in one process:
  (a) `elicit_field_implicit`: one base block of the item field, then every round of every respondent in one launch;
  (b) the composed loop on the public API: per round `select_next_questions_field(n=1)` on the rows still unasked, then
      `fold_in_implicit(rows so far, entities=respondents)` -- a base assembly and a solve launch per round, the
      `torch.isin` / `torch.cat` glue included;
  (c) `elicit_field_exact` on the same pool, for scale: its dual systems (n <= d rows) are far smaller than the primal
      (d + 1) x (d + 1) system (a) factors per round per respondent, so (a) may well be the slower call.  A ratio, no
      threshold.

One shape, one JSON line (appended to profiles/elicit_implicit_bench.jsonl with --record): the other session benches' --
10,000 respondents x 100-row pools of distinct items, two fields with ML-20M's user and item counts, d = 128, 'reg', 20
rounds, click answers.  Times: the calls interleaved (a, b, c, a, b, c, ..), HIP-event medians over `--reps` rounds after
`--warmup`, the whole public call each; every call leaves the model as it found it (the loop restores it inside its timed
span).  The same line carries the recall / NDCG@10 curve of `elicitation_ranking_curve_field(implicit=True)` beside
`exact=True` on tools/fit_implicit_bench.py's planted clicks: a model fitted by fit_implicit on the other users, the
respondents cold-started by the recipe of elicit_field_implicit's docstring (implicit) and by reset=True (exact); values
only."""
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


def composed_loop(m, pool, y_pool, rounds, strategy, w0):
    """The host-glued loop: the pool shrinks, the answered rows grow."""
    Xa, ya = pool[:0], y_pool[:0]
    for r in range(rounds):
        if pool.shape[0] == 0:
            break
        ents, rows = m.select_next_questions_field(pool, 0, n=1, strategy=strategy, seed=r)
        asked = rows[rows >= 0]
        keep = torch.ones(pool.shape[0], dtype=torch.bool, device=pool.device)
        keep[asked] = False
        Xa, ya = torch.cat([Xa, pool[asked]]), torch.cat([ya, y_pool[asked]])
        who = torch.isin(Xa[:, 0], ents)
        m.fold_in_implicit(Xa[who], ya[who], 0, w0=w0, entities=ents)
        pool, y_pool = pool[keep], y_pool[keep]


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def timing(args, dev):
    from vae_amd.model import VFM
    torch.manual_seed(0)
    N, M = 138_493, 26_744
    m = VFM(N, M, embedding_size=128, output="reg", device=dev)
    with torch.no_grad():
        m._flat.mul_(0.3)
    g = torch.Generator(device=dev).manual_seed(1)
    U, P = args.respondents, args.pool
    assert P * 251 < M                                       # (the stride below keeps a respondent's items distinct)
    users = torch.randperm(N, device=dev, generator=g)[:U]
    first = torch.randint(0, M, (U,), device=dev, generator=g)
    items = N + (first[:, None] + 251 * torch.arange(P, device=dev)[None, :]) % M
    pool = torch.stack([users.repeat_interleave(P), items.reshape(-1)], 1)
    y_pool = (torch.rand(U * P, device=dev, generator=g) < 0.3).float()           # clicks
    strategy = "variance"
    start = m._flat.clone()

    def restore():
        m._flat.copy_(start)
        m.params_changed()

    def session():
        m.elicit_field_implicit(pool, y_pool, args.rounds, 0, w0=args.w0, strategy=strategy)

    def loop():
        restore()
        composed_loop(m, pool, y_pool, args.rounds, strategy, args.w0)

    def exact():
        m.elicit_field_exact(pool, y_pool, args.rounds, 0, strategy)

    calls = (("session", session), ("loop", loop), ("exact", exact))
    ts = {k: [] for k, _ in calls}
    for rep in range(args.warmup + args.reps):              # interleaved: a, b, c, a, b, c, ..
        for k, fn in calls:
            t = once(fn)
            if rep >= args.warmup:
                ts[k].append(t)
    restore()
    med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
    return {"respondents": U, "pool_rows": U * P, "F": 2, "d": m.d, "strategy": strategy, "rounds": args.rounds,
            "w0": args.w0, "warmup": args.warmup, "reps": args.reps,
            "implicit_session_ms": round(med["session"], 3), "composed_implicit_loop_ms": round(med["loop"], 3),
            "exact_session_ms": round(med["exact"], 3),
            "implicit_session_all_ms": [round(v, 3) for v in ts["session"]],
            "loop_over_session": round(med["loop"] / med["session"], 2),
            "session_over_exact_session": round(med["session"] / med["exact"], 2)}


def curve(args, dev):
    from fit_implicit_synthetic import planted_clicks
    from vae_amd.model import VFM
    n_u, n_i, d, n_resp, Q = 2000, 800, 16, 300, 10
    X = planted_clicks(n_u, n_i, 6, 30, seed=3)
    g = torch.Generator().manual_seed(4)
    resp = torch.randperm(n_u, generator=g)[:n_resp]
    mine = torch.isin(X[:, 0], resp)
    held = mine & (torch.rand(X.shape[0], generator=g) < 0.3)
    Xtr, Xpool, Xte = X[~mine].to(dev), X[mine & ~held].to(dev), X[held].to(dev)
    # the pool: the respondents' remaining clicks (answer 1) and as many items they did not click (answer 0)
    neg = torch.stack([Xpool[:, 0].cpu(), n_u + torch.randint(0, n_i, (Xpool.shape[0],), generator=g)], 1).to(dev)
    key = lambda x: x[:, 0] * (n_u + n_i) + x[:, 1]
    neg = neg[~torch.isin(key(neg), key(X.to(dev)))]
    order = torch.argsort(key(neg), stable=True)
    dup = torch.zeros(neg.shape[0], dtype=torch.bool, device=dev)
    dup[order[1:]] = key(neg)[order[1:]] == key(neg)[order[:-1]]
    neg = neg[~dup]
    pool = torch.cat([Xpool, neg])
    y_pool = torch.cat([torch.ones(Xpool.shape[0], device=dev), torch.zeros(neg.shape[0], device=dev)])
    torch.manual_seed(0)
    m = VFM(n_u, n_i, embedding_size=d, output="reg", device=dev)
    m.fit_implicit(Xtr, n_sweeps=args.sweeps, w0=args.w0)
    kw = dict(ks=(10,), strategies=("variance",), threshold=0.5, ineligible="drop")
    yte = torch.ones(Xte.shape[0], device=dev)
    c_exact = m.elicitation_ranking_curve_field(pool, y_pool, Q, 0, Xte, yte, 1, exact=True, reset=True, **kw)
    m.fold_in_implicit(pool[:0], y_pool[:0], 0, w0=args.w0, entities=resp.to(dev))    # the cold-start recipe
    c_imp = m.elicitation_ranking_curve_field(pool, y_pool, Q, 0, Xte, yte, 1, implicit=True, w0=args.w0, **kw)
    r4 = lambda v: [round(x, 4) for x in v]
    return {"curve_users": n_u, "curve_items": n_i, "curve_d": d, "curve_respondents": n_resp, "curve_rounds": Q,
            "curve_pool_rows": int(pool.shape[0]), "curve_queries": c_imp["n_queries"],
            "implicit_recall_at_10": r4(c_imp["variance"]["recall@10"]), "implicit_ndcg_at_10": r4(c_imp["variance"]["ndcg@10"]),
            "exact_recall_at_10": r4(c_exact["variance"]["recall@10"]), "exact_ndcg_at_10": r4(c_exact["variance"]["ndcg@10"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--respondents", type=int, default=10_000)
    ap.add_argument("--pool", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--w0", type=float, default=0.05, help="a starting value: nobody has measured a good one")
    ap.add_argument("--sweeps", type=int, default=8)
    ap.add_argument("--no-curve", action="store_true")
    ap.add_argument("--record", action="store_true", help="append the line to profiles/elicit_implicit_bench.jsonl")
    ap.add_argument("--note", default=None, help="kept in the line: what was measured, e.g. the commit")
    args = ap.parse_args()
    dev = torch.device("cuda")
    rec = {"shape": "ml20m_two_field", **timing(args, dev)}
    if not args.no_curve:
        rec.update(curve(args, dev))
    rec.update({"device": torch.cuda.get_device_name(0), "when": time.strftime("%Y-%m-%dT%H:%M:%S")})
    if args.note:
        rec["note"] = args.note
    print(json.dumps(rec), flush=True)
    if args.record:
        with open(os.path.join(ROOT, "profiles", "elicit_implicit_bench.jsonl"), "a") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

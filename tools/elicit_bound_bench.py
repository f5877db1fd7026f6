"""The bound field-form session (include/vfm_bound.h: vfm_elicit_bound_f32, `VFM.elicit_field_bound`) against the two
things it stands beside for a 'class' model, in one process:
  (a) `elicit_field_bound`: every round of every respondent in one launch;
  (b) the loop it replaces, composed from the public API: per round `select_next_questions_field` on the rows still
      unasked, then `fold_in_bound(field=..., reset=False)` of the answering respondents on everything they have answered
      so far (the `torch.isin` / `torch.cat` glue included);
  (c) `elicit_field(n_steps=--steps)`: the Adam session on the sampled objective, the only session a 'class' model had.

Two shapes, one JSON line each (appended to profiles/elicit_bound_bench.jsonl with --record):
  fraction  the students of the `fraction` test rows as a cold-start population, d = 5, 15 rounds (tools/elicit_bench.py's)
  ml20m     10,000 respondents x 100-row pools, F = 3 (user, item, format: ML-20M's user and item counts and 4 formats),
            d = 128, 20 rounds (tools/elicit_field_exact_bench.py's)
The tables are the initial ones scaled by 0.3; at ml20m the answers are drawn from the model's own mean prediction.
Strategy "mean", cold start (reset).  Times: the three calls interleaved (a, b, c, a, b, c, ..), HIP-event medians over
`--reps` rounds after `--warmup`, the whole public call each (argument checks, sorts, operand passes, kernels); every call
leaves the model as it found it.  Quality, with strategy "random" so that both sessions ask the same rows in the same
order: the sum over the respondents of the bound session's final B_e against the sum of `fold_in_bound_objective` on
those rows at the table rows the Adam session wrote.  n_iters = 8 is the untuned starting value.  No speed is promised."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from elicit_field_exact_bench import once  # noqa: E402


def composed_loop(m, pool, y_pool, field, rounds, strategy, n_iters):
    """The host-glued loop: the pool shrinks, the answered rows grow."""
    Xa, ya = pool[:0], y_pool[:0]
    for r in range(rounds):
        if pool.shape[0] == 0:
            break
        _, rows = m.select_next_questions_field(pool, field, n=1, strategy=strategy, seed=r)
        asked = rows[rows >= 0]
        keep = torch.ones(pool.shape[0], dtype=torch.bool, device=pool.device)
        keep[asked] = False
        Xa, ya = torch.cat([Xa, pool[asked]]), torch.cat([ya, y_pool[asked]])
        who = torch.isin(Xa[:, field], pool[asked][:, field])
        m.fold_in_bound(Xa[who], ya[who], field=field, n_iters=n_iters, reset=False)
        pool, y_pool = pool[keep], y_pool[keep]


def problem(shape, dev):
    """(model, pool [P, F], y_pool [P], rounds) of a shape."""
    from vae_amd.model import VFM
    torch.manual_seed(0)
    g = torch.Generator(device=dev).manual_seed(1)
    if shape == "fraction":
        from vae_amd.data import load_fraction
        N, M, _, Xte, _, yte = load_fraction(os.path.join(ROOT, "tests", "golden", "fraction"))
        m = VFM(N, M, embedding_size=5, output="class", device=dev)
        with torch.no_grad():
            m._flat.mul_(0.3)
        return m, torch.as_tensor(Xte).to(dev, torch.int64), torch.as_tensor(yte).to(dev, torch.float32), 15
    N, M, K, n_resp, per = 138_493, 26_744, 4, 10_000, 100
    m = VFM(field_sizes=[N, M, K], embedding_size=128, output="class", device=dev)
    with torch.no_grad():
        m._flat.mul_(0.3)
    R = n_resp * per
    users = torch.randperm(N, device=dev, generator=g)[:n_resp]
    pool = torch.stack([users.repeat_interleave(per), N + torch.randint(0, M, (R,), device=dev, generator=g),
                        N + M + torch.randint(0, K, (R,), device=dev, generator=g)], 1)
    truth, _, _ = m.field_moments(pool, 0)
    y_pool = (torch.rand(R, device=dev, generator=g) < torch.sigmoid(truth)).float()
    return m, pool, y_pool, 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--n-iters", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="fraction,ml20m")
    ap.add_argument("--record", action="store_true", help="append the lines to profiles/elicit_bound_bench.jsonl")
    ap.add_argument("--note", default=None, help="kept in the line: what was measured, e.g. the commit")
    args = ap.parse_args()
    dev = torch.device("cuda")
    for shape in args.shapes.split(","):
        m, pool, y_pool, rounds = problem(shape, dev)
        field, strategy = 0, "mean"
        ents = torch.unique(pool[:, field])
        start = m._flat.clone()

        def restore():
            m._flat.copy_(start)
            m.params_changed()

        def prior():
            restore()
            ent, bia, _ = m._views(m._flat)
            ent[ents, :m.d], ent[ents, m.d:], bia[ents, 0], bia[ents, 1] = 0.0, 1.0, 0.0, 1.0     # (|.| link: s = 1)
            m.params_changed()

        def bound():
            m.elicit_field_bound(pool, y_pool, rounds, field, strategy, n_iters=args.n_iters, reset=True)

        def loop():
            prior()
            composed_loop(m, pool, y_pool, field, rounds, strategy, args.n_iters)

        def adam():
            m.elicit_field(pool, y_pool, rounds, field, strategy, n_steps=args.steps, lr=0.05, reset=True)

        calls = (("bound", bound), ("loop", loop), ("adam", adam))
        ts = {k: [] for k, _ in calls}
        for rep in range(args.warmup + args.reps):          # interleaved: a, b, c, a, b, c, ..
            for k, fn in calls:
                t = once(fn)
                if rep >= args.warmup:
                    ts[k].append(t)
        restore()
        med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
        # quality on equal rows: "random" asks the same rows in both sessions
        b = m.elicit_field_bound(pool, y_pool, rounds, field, "random", seed=3, n_iters=args.n_iters, reset=True)
        a = m.elicit_field(pool, y_pool, rounds, field, "random", seed=3, n_steps=args.steps, lr=0.05, reset=True, write=True)
        same_rows = torch.equal(a["rows"], b["rows"]) and torch.equal(a["entities"], b["entities"])
        last = (b["rows"] >= 0).sum(1) - 1
        has = last >= 0
        B_bound = float(b["loss"][has, last[has]].double().sum())
        asked = b["rows"][b["rows"] >= 0]
        B_adam = float(m.fold_in_bound_objective(pool[asked], y_pool[asked], field=field)["loss"].double().sum())
        restore()
        assert torch.equal(m._flat, start)
        rec = {"shape": shape, "respondents": int(ents.numel()), "pool_rows": int(pool.shape[0]), "F": int(pool.shape[1]),
               "field": field, "d": m.d, "strategy": strategy, "rounds": rounds, "n_iters": args.n_iters,
               "steps": args.steps, "reps": args.reps,
               "bound_session_ms": round(med["bound"], 3), "composed_bound_loop_ms": round(med["loop"], 3),
               "adam_session_ms": round(med["adam"], 3),
               "loop_over_bound": round(med["loop"] / med["bound"], 2), "adam_over_bound": round(med["adam"] / med["bound"], 2),
               "sum_final_bound_session": round(B_bound, 3), "sum_bound_at_adam_rows": round(B_adam, 3),
               "bound_below_adam_by": round(1.0 - B_bound / B_adam, 4), "same_rows_asked": same_rows,
               "device": torch.cuda.get_device_name(0), "when": time.strftime("%Y-%m-%dT%H:%M:%S")}
        if args.note:
            rec["note"] = args.note
        print(json.dumps(rec), flush=True)
        if args.record:
            with open(os.path.join(ROOT, "profiles", "elicit_bound_bench.jsonl"), "a") as f:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

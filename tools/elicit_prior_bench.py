"""What a learnt field prior costs a session (include/vfm_elicit_prior.h): each of the exact, design and bound sessions
with `priors=` against `priors=None`, in one process.

Shapes: tools/elicit_field_exact_bench.py's and tools/elicit_bound_bench.py's ml20m shape -- 10,000 respondents x 100-row
pools, F = 3 (ML-20M's user and item counts and 4 formats), d = 128, 20 rounds, the initial tables scaled by 0.3, cold
start (reset) -- 'reg' for the exact and design sessions, 'class' (n_iters = 8) for the bound one.  The priors: the user
field at precision 1 / 0.3^2 and mean 0.05, the others at (0, 1).  Times: the two legs interleaved (none, priors, none,
priors, ..), HIP-event medians over `--reps` rounds after `--warmup`, the whole public call each; spread = (max - min) /
median of a leg's own repetitions.  One JSON line per session (appended to profiles/elicit_prior_bench.jsonl with
--record).  The expectation is a ratio inside the priors=None leg's own spread: the prior is one 2 (d + 1)-float load per
workgroup and a few FMAs per coordinate and round.  No speed is promised and no test asserts one."""
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


def problem(output, dev, respondents, per):
    from vae_amd.model import VFM
    torch.manual_seed(0)
    N, M, K = 138_493, 26_744, 4
    m = VFM(field_sizes=[N, M, K], embedding_size=128, output=output, device=dev)
    with torch.no_grad():
        m._flat.mul_(0.3)
    g = torch.Generator(device=dev).manual_seed(1)
    R = respondents * per
    users = torch.randperm(N, device=dev, generator=g)[:respondents]
    pool = torch.stack([users.repeat_interleave(per), N + torch.randint(0, M, (R,), device=dev, generator=g),
                        N + M + torch.randint(0, K, (R,), device=dev, generator=g)], 1)
    truth, _, _ = m.field_moments(pool, 0)
    y = truth + 0.5 * torch.randn(R, device=dev, generator=g) if output == "reg" else \
        (torch.rand(R, device=dev, generator=g) < torch.sigmoid(truth)).float()
    return m, pool, y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--respondents", type=int, default=10_000)
    ap.add_argument("--pool", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--n-iters", type=int, default=8)
    ap.add_argument("--sessions", default="exact,design,bound")
    ap.add_argument("--record", action="store_true", help="append the lines to profiles/elicit_prior_bench.jsonl")
    ap.add_argument("--note", default=None, help="kept in the line: what was measured, e.g. the commit")
    args = ap.parse_args()
    from vae_amd import sweep
    dev = torch.device("cuda")
    models = {}
    for name in args.sessions.split(","):
        output = "class" if name == "bound" else "reg"
        if output not in models:
            models[output] = problem(output, dev, args.respondents, args.pool)
        m, pool, y = models[output]
        priors = sweep.GroupPriors(m.F, m.d, dev)
        priors.mean[0] = 0.05
        priors.prec[0] = 1.0 / 0.3 ** 2
        start = m._flat.clone()

        def call(p):
            if name == "exact":
                m.elicit_field_exact(pool, y, args.rounds, 0, "variance", reset=True, priors=p)
            elif name == "design":
                m.elicit_field_design(pool, y, args.rounds, 0, reset=True, priors=p)
            else:
                m.elicit_field_bound(pool, y, args.rounds, 0, "mean", n_iters=args.n_iters, reset=True, priors=p)

        legs = (("none", None), ("priors", priors))
        ts = {k: [] for k, _ in legs}
        for rep in range(args.warmup + args.reps):          # interleaved: none, priors, none, priors, ..
            for k, p in legs:
                t = once(lambda: call(p))
                if rep >= args.warmup:
                    ts[k].append(t)
        assert torch.equal(m._flat, start)
        med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
        spread = {k: (max(v) - min(v)) / med[k] for k, v in ts.items()}
        rec = {"session": name, "respondents": args.respondents, "pool_rows": int(pool.shape[0]), "F": m.F, "d": m.d,
               "rounds": args.rounds, "reps": args.reps, "none_ms": round(med["none"], 3),
               "priors_ms": round(med["priors"], 3), "none_spread": round(spread["none"], 4),
               "priors_spread": round(spread["priors"], 4), "priors_over_none": round(med["priors"] / med["none"], 4),
               "device": torch.cuda.get_device_name(0), "when": time.strftime("%Y-%m-%dT%H:%M:%S")}
        if name == "bound":
            rec["n_iters"] = args.n_iters
        if args.note:
            rec["note"] = args.note
        print(json.dumps(rec), flush=True)
        if args.record:
            with open(os.path.join(ROOT, "profiles", "elicit_prior_bench.jsonl"), "a") as f:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

"""Bound fold-in (VFM.fold_in_bound, vfm_foldin_bound_f32) against fold_in(n_steps=200) on the sampled objective, the
only form a 'class' model had before, of the same checkout.

The two shapes of tools/foldin_bench.py with a 'class' model and labels in {0, 1}, one JSON line each (also appended to
profiles/foldin_bound_bench.jsonl with --write):
  fraction  536 students x 5 answers, d = 5 (the table shape of the `fraction` data: 536 + 20 entities)
  ml20m     10,000 users x 20 rows, d = 128, ML-20M table shape (138,493 + 26,744 entities)
Both calls start from the same parameters (the table is restored before each call, inside the timed span), in one
process, interleaved round by round: call_ms = HIP-event times of the whole public call, median and min over --reps
rounds after --warmup.  bound_after = the sum over the entities of B_e after 1 .. n_iters rounds; bound_at_adam = the
same sum from fold_in_bound_objective at the rows Adam wrote, which shows which of the two reaches the lower bound.
No speed is promised: eight rounds of a full assembly may well be slower than 200 Adam steps."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from foldin_exact_bench import interleaved, stats  # noqa: E402

SHAPES = {"fraction": (536, 20, 5, 536, 5), "ml20m": (138_493, 26_744, 128, 10_000, 20)}   # N, M, d, users, rows each


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--lr", type=float, default=0.05)
    ap.add_argument("--n-iters", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--shapes", default="fraction,ml20m")
    ap.add_argument("--write", action="store_true", help="append the lines to profiles/foldin_bound_bench.jsonl")
    ap.add_argument("--note", default=None, help="kept in the line: what was measured, e.g. the commit")
    args = ap.parse_args()
    from vae_amd.model import VFM
    dev = torch.device("cuda")
    lines = []
    for shape in args.shapes.split(","):
        N, M, d, n_users, per = SHAPES[shape]
        torch.manual_seed(0)
        m = VFM(N, M, embedding_size=d, output="class", device=dev)
        with torch.no_grad():
            m._flat.mul_(0.3)
        g = torch.Generator(device=dev).manual_seed(1)
        users = torch.randperm(N, device=dev, generator=g)[:n_users]
        u = users.repeat_interleave(per)
        X = torch.stack([u, N + torch.randint(0, M, (u.numel(),), device=dev, generator=g)], 1)
        y = (torch.rand(u.numel(), device=dev, generator=g) < 0.4).float()
        start = m._flat.clone()

        def adam():
            m._flat.copy_(start)
            return m.fold_in(X, y, n_steps=args.steps, lr=args.lr)

        def bound(n_iters=args.n_iters):
            m._flat.copy_(start)
            return m.fold_in_bound(X, y, n_iters=n_iters)

        t = interleaved({"adam": adam, "bound": bound}, args.warmup, args.reps)
        after = [float(bound(k)["loss"].double().sum()) for k in range(1, args.n_iters + 1)]
        adam()
        at_adam = float(m.fold_in_bound_objective(X, y)["loss"].double().sum())
        m._flat.copy_(start)
        at_start = float(m.fold_in_bound_objective(X, y)["loss"].double().sum())
        rec = {"shape": shape, "entities": n_users, "rows": int(X.shape[0]), "d": d, "steps": args.steps, "lr": args.lr,
               "n_iters": args.n_iters, "reps": args.reps,
               "fold_in_call_ms": stats(t["adam"]), "fold_in_bound_call_ms": stats(t["bound"]),
               "bound_over_adam": round(t["bound"][len(t["bound"]) // 2] / t["adam"][len(t["adam"]) // 2], 4),
               "bound_at_start": at_start, "bound_after": after, "bound_at_adam": at_adam,
               "device": torch.cuda.get_device_name(0), "when": time.strftime("%Y-%m-%dT%H:%M:%S")}
        if args.note:
            rec["note"] = args.note
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if args.write:
        with open(os.path.join(ROOT, "profiles", "foldin_bound_bench.jsonl"), "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

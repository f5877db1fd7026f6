"""Exact fold-in (VFM.fold_in_exact, vfm_foldin_solve_f32) against fold_in(n_steps=200) of the same checkout.

The 'reg' / closed-form shape of tools/foldin_bench.py and its heavy-entity variant, one JSON line each (also appended
to profiles/foldin_exact_bench.jsonl with --write):
  ml20m        10,000 users x 20 ratings, d = 128, ML-20M table shape (138,493 + 26,744 entities): every system dual 20 x 20
  ml20m_heavy  the same with one user of 5,000 ratings: one primal 129 x 129 system among the dual ones
Both calls start from the same parameters (the table is restored before each call, inside the timed span: a margin of
~0.1 ms on both sides), in one process, interleaved round by round: call_ms = HIP-event times of the whole public call
(argument checks, sort, partner tuples, operand prep, kernel), median and min over --reps rounds after --warmup;
launch_ms = the same for the operand prep + kernel alone (the torch op on prepared row lists).  gap = the per-entity
loss gap L_adam200 - L_exact, both losses evaluated by their own kernel at the parameters it wrote."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def interleaved(fns, warmup, reps):
    """{name: sorted times} of the callables, one of each per round."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(event_ms(fn))
    return {k: sorted(v) for k, v in ts.items()}


def stats(v):
    return {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--lr", type=float, default=0.05)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--shapes", default="ml20m,ml20m_heavy")
    ap.add_argument("--write", action="store_true", help="append the lines to profiles/foldin_exact_bench.jsonl")
    ap.add_argument("--note", default=None, help="kept in the line: what was measured, e.g. the commit")
    args = ap.parse_args()
    from vae_amd import _lib, foldin, ops
    from vae_amd.model import VFM
    dev = torch.device("cuda")
    lines = []
    for shape in args.shapes.split(","):
        torch.manual_seed(0)
        N, M, d = 138_493, 26_744, 128
        m = VFM(N, M, embedding_size=d, output="reg", device=dev)
        with torch.no_grad():
            m._flat.mul_(0.3)
        g = torch.Generator(device=dev).manual_seed(1)
        users = torch.randperm(N, device=dev, generator=g)[:10_000]
        n = torch.full((10_000,), 20, device=dev, dtype=torch.int64)
        if shape == "ml20m_heavy":
            n[7] = 5000
        u = users.repeat_interleave(n)
        X = torch.stack([u, N + torch.randint(0, M, (u.numel(),), device=dev, generator=g)], 1)
        y = torch.randint(1, 6, (u.numel(),), device=dev, generator=g).float()
        start = m._flat.clone()

        def adam():
            m._flat.copy_(start)
            return m.fold_in(X, y, n_steps=args.steps, lr=args.lr)

        def exact():
            m._flat.copy_(start)
            return m.fold_in_exact(X, y)

        t_call = interleaved({"adam": adam, "exact": exact}, args.warmup, args.reps)
        l_adam, l_exact = adam()["loss"].double(), exact()["loss"].double()
        gap = (l_adam - l_exact).cpu()

        # the launches alone, on row lists prepared once
        o = _lib.ops()
        xs, ys, ents, ptr, _ = foldin.row_lists(X, y, 0)
        op_x, row_op = foldin.partner_tuples(xs, 0)
        E = ents.numel()
        code = foldin.OBJECTIVES["closed_form"]
        ws_a = torch.empty(max(o.foldin_workspace_bytes(op_x.shape[0], d, code), 1), dtype=torch.uint8, device=dev)
        ws_e = torch.empty(max(o.foldin_solve_workspace_bytes(E, op_x.shape[0], d, -1), 1), dtype=torch.uint8, device=dev)
        loss = torch.empty(E, device=dev)
        ent, bia, scal = m._views(m._flat)

        def adam_launch():
            m._flat.copy_(start)
            o.foldin(ents, ptr, xs, ys, op_x, row_op, ent, bia, scal, ws_a, loss, None, 0, code, _lib.LIK_NORMAL, 0,
                     foldin.MODE_FIT, args.steps, 1, 0, -1, args.lr, 1.0, 0, 0)

        def exact_launch():
            m._flat.copy_(start)
            o.foldin_solve(ents, ptr, ys, op_x, row_op, ent, bia, scal, ws_e, loss, 0, code, _lib.LIK_NORMAL, 0, -1, 1.0)

        t_launch = interleaved({"adam": adam_launch, "exact": exact_launch}, args.warmup, args.reps)
        m._flat.copy_(start)
        rec = {"shape": shape, "entities": int(E), "rows": int(X.shape[0]), "d": d, "steps": args.steps, "lr": args.lr,
               "reps": args.reps,
               "fold_in_call_ms": stats(t_call["adam"]), "fold_in_exact_call_ms": stats(t_call["exact"]),
               "fold_in_launch_ms": stats(t_launch["adam"]), "fold_in_exact_launch_ms": stats(t_launch["exact"]),
               "gap_adam_minus_exact": {"min": float(gap.min()), "median": float(gap.median()), "max": float(gap.max())},
               "rel_gap_max": float((gap / l_exact.cpu()).max()),
               "device": torch.cuda.get_device_name(0), "when": time.strftime("%Y-%m-%dT%H:%M:%S")}
        if args.note:
            rec["note"] = args.note
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if args.write:
        with open(os.path.join(ROOT, "profiles", "foldin_exact_bench.jsonl"), "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

"""Elicitation sessions (include/vfm_elicit.h, `VFM.elicit`) against the loop they replace, composed from the public
API as examples/elicit_foldin.py composes it: per round `select_next_questions` on the rows still unasked, then
`fold_in` of the answering users on everything they have answered so far (the `torch.isin` / `torch.cat` glue included).

Two shapes, one JSON line each (appended to profiles/elicit_bench.jsonl with --record):
  fraction  the students of the `fraction` test rows as a cold-start population, d = 5, 'class' (sampled objective),
            15 rounds.
  ml20m     10,000 users with 100-row pools, d = 128, 'reg' (closed form), ML-20M table shape, 20 rounds.
Every round runs `--steps` Adam steps (default 200).  Times: HIP-event medians over `--reps` calls after `--warmup`, the
whole public call (argument checks, sorts, operand pass, kernel); both sides leave the model as they found it
(`write=False`; the loop restores the table before each call).  The split between the operand pass and the session
kernel is taken from one torch.profiler trace of the session call (kernel time by name); null if the profiler gives no
kernel records."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from foldin_bench import timed


def composed_loop(m, pool, y_pool, rounds, strategy, steps, lr, objective, reset):
    """The host-glued loop (examples/elicit_foldin.py): the pool shrinks, the answered rows grow."""
    Xa, ya = pool[:0], y_pool[:0]
    first = True
    for r in range(rounds):
        if pool.shape[0] == 0:
            break
        _, rows = m.select_next_questions(pool, n=1, strategy=strategy, seed=r)
        asked = rows[rows >= 0]
        keep = torch.ones(pool.shape[0], dtype=torch.bool, device=pool.device)
        keep[asked] = False
        Xa, ya = torch.cat([Xa, pool[asked]]), torch.cat([ya, y_pool[asked]])
        who = torch.isin(Xa[:, 0], pool[asked][:, 0])
        m.fold_in(Xa[who], ya[who], n_steps=steps, lr=lr, objective=objective, reset=reset and first)
        first = False
        pool, y_pool = pool[keep], y_pool[keep]


def kernel_split(fn):
    """{"operand_pass_ms", "session_kernel_ms"} of one call of fn, from a profiler trace; None where not found."""
    out = {"operand_pass_ms": None, "session_kernel_ms": None}
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        for ev in prof.key_averages():
            t = getattr(ev, "device_time_total", None)
            if t is None:
                t = getattr(ev, "cuda_time_total", 0.0)
            if "k_foldin_prep" in ev.key:
                out["operand_pass_ms"] = round((out["operand_pass_ms"] or 0.0) + t / 1e3, 4)
            elif "k_elicit" in ev.key:
                out["session_kernel_ms"] = round((out["session_kernel_ms"] or 0.0) + t / 1e3, 4)
    except Exception as e:                                  # (a profiler without kernel records: the split stays null)
        out["split_error"] = repr(e)[:200]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="fraction,ml20m")
    ap.add_argument("--record", action="store_true", help="append the lines to profiles/elicit_bench.jsonl")
    args = ap.parse_args()
    from vae_amd.model import VFM
    from vae_amd.data import load_fraction
    dev = torch.device("cuda")
    lines = []
    for shape in args.shapes.split(","):
        torch.manual_seed(0)
        if shape == "fraction":
            N, M, Xtr, Xte, ytr, yte = load_fraction(os.path.join(ROOT, "tests", "golden", "fraction"))
            m = VFM(N, M, embedding_size=5, output="class", device=dev)
            m.fit(torch.as_tensor(Xtr), torch.as_tensor(ytr), n_epochs=60, batch_size=100000, verbose=False)
            pool, y_pool = torch.as_tensor(Xte).to(dev), torch.as_tensor(yte).float().to(dev)
            objective, rounds, strategy = "sampled", 15, "variance"
        else:
            N, M = 138_493, 26_744
            m = VFM(N, M, embedding_size=128, output="reg", device=dev)
            with torch.no_grad():
                m._flat.mul_(0.3)
            g = torch.Generator(device=dev).manual_seed(1)
            users = torch.randperm(N, device=dev, generator=g)[:10_000]
            pool = torch.stack([users.repeat_interleave(100), N + torch.randint(0, M, (1_000_000,), device=dev, generator=g)], 1)
            y_pool = torch.randint(1, 6, (1_000_000,), device=dev, generator=g).float()
            objective, rounds, strategy = "closed_form", 20, "variance"
        start = m._flat.clone()

        def session():
            m.elicit(pool, y_pool, rounds, strategy, n_steps=args.steps, lr=0.05, objective=objective, reset=True)

        def loop():
            m._flat.copy_(start)
            m.params_changed()
            composed_loop(m, pool, y_pool, rounds, strategy, args.steps, 0.05, objective, True)

        t_sess = timed(session, args.warmup, args.reps)
        split = kernel_split(session)
        t_loop = timed(loop, args.warmup, args.reps)
        m._flat.copy_(start)
        m.params_changed()
        rec = {"shape": shape, "users": int(torch.unique(pool[:, 0]).numel()), "pool_rows": int(pool.shape[0]), "d": m.d,
               "objective": objective, "strategy": strategy, "rounds": rounds, "steps": args.steps,
               "session_ms": round(t_sess, 3), "composed_loop_ms": round(t_loop, 3),
               "loop_over_session": round(t_loop / t_sess, 2), **split,
               "device": torch.cuda.get_device_name(0), "when": time.strftime("%Y-%m-%dT%H:%M:%S")}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if args.record:
        with open(os.path.join(ROOT, "profiles", "elicit_bench.jsonl"), "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

"""Field-form elicitation sessions (include/vfm_elicit.h: vfm_elicit_field_f32, `VFM.elicit_field`) against the loop
they replace, composed from the public API: per round `select_next_questions_field` on the rows still unasked, then
`fold_in(field=...)` of the answering respondents on everything they have answered so far (the `torch.isin` /
`torch.cat` glue included).

One shape, one JSON line (appended to profiles/elicit_field_bench.jsonl with --record): 10,000 respondents x 100-row
pools, F = 3 (user, item, format: ML-20M's user and item counts and 4 formats), d = 128, 'reg' (closed form), 20 rounds
of `--steps` Adam steps (default 200), cold start.  Times: HIP-event medians over `--reps` calls after `--warmup`, the
whole public call (argument checks, sorts, operand passes, kernel); both sides leave the model as they found it
(`write=False`; the loop restores the table before each call).  The split between the operand passes and the session
kernel is taken from one torch.profiler trace of the session call; null if the profiler gives no kernel records."""
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


def composed_loop(m, pool, y_pool, field, rounds, strategy, steps, lr, objective, reset):
    """The host-glued loop: the pool shrinks, the answered rows grow."""
    Xa, ya = pool[:0], y_pool[:0]
    first = True
    for r in range(rounds):
        if pool.shape[0] == 0:
            break
        _, rows = m.select_next_questions_field(pool, field, n=1, strategy=strategy, seed=r)
        asked = rows[rows >= 0]
        keep = torch.ones(pool.shape[0], dtype=torch.bool, device=pool.device)
        keep[asked] = False
        Xa, ya = torch.cat([Xa, pool[asked]]), torch.cat([ya, y_pool[asked]])
        who = torch.isin(Xa[:, field], pool[asked][:, field])
        m.fold_in(Xa[who], ya[who], field=field, n_steps=steps, lr=lr, objective=objective, reset=reset and first)
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
            if "k_foldin_prep" in ev.key or "k_elicit_ctx_prep" in ev.key:
                out["operand_pass_ms"] = round((out["operand_pass_ms"] or 0.0) + t / 1e3, 4)
            elif "k_elicit_field" in ev.key:
                out["session_kernel_ms"] = round((out["session_kernel_ms"] or 0.0) + t / 1e3, 4)
    except Exception as e:                                  # (a profiler without kernel records: the split stays null)
        out["split_error"] = repr(e)[:200]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--respondents", type=int, default=10_000)
    ap.add_argument("--pool", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--record", action="store_true", help="append the line to profiles/elicit_field_bench.jsonl")
    args = ap.parse_args()
    from vae_amd.model import VFM
    dev = torch.device("cuda")
    torch.manual_seed(0)
    N, M, K = 138_493, 26_744, 4
    m = VFM(field_sizes=[N, M, K], embedding_size=128, output="reg", device=dev)
    with torch.no_grad():
        m._flat.mul_(0.3)
    g = torch.Generator(device=dev).manual_seed(1)
    R = args.respondents * args.pool
    users = torch.randperm(N, device=dev, generator=g)[:args.respondents]
    pool = torch.stack([users.repeat_interleave(args.pool), N + torch.randint(0, M, (R,), device=dev, generator=g),
                        N + M + torch.randint(0, K, (R,), device=dev, generator=g)], 1)
    y_pool = torch.randint(1, 6, (R,), device=dev, generator=g).float()
    field, objective, strategy = 0, "closed_form", "variance"
    start = m._flat.clone()

    def session():
        m.elicit_field(pool, y_pool, args.rounds, field, strategy, n_steps=args.steps, lr=0.05, objective=objective,
                       reset=True)

    def loop():
        m._flat.copy_(start)
        m.params_changed()
        composed_loop(m, pool, y_pool, field, args.rounds, strategy, args.steps, 0.05, objective, True)

    t_sess = timed(session, args.warmup, args.reps)
    split = kernel_split(session)
    t_loop = timed(loop, args.warmup, args.reps)
    m._flat.copy_(start)
    m.params_changed()
    rec = {"shape": "ml20m_formats", "respondents": args.respondents, "pool_rows": R, "F": 3, "field": field, "d": m.d,
           "objective": objective, "strategy": strategy, "rounds": args.rounds, "steps": args.steps,
           "session_ms": round(t_sess, 3), "composed_loop_ms": round(t_loop, 3),
           "loop_over_session": round(t_loop / t_sess, 2), **split,
           "device": torch.cuda.get_device_name(0), "when": time.strftime("%Y-%m-%dT%H:%M:%S")}
    print(json.dumps(rec), flush=True)
    if args.record:
        with open(os.path.join(ROOT, "profiles", "elicit_field_bench.jsonl"), "a") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

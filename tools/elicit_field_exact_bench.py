"""The exact field-form session (include/vfm_elicit.h: vfm_elicit_solve_f32, `VFM.elicit_field_exact`) against the two
things it stands beside, in one process:
  (a) `elicit_field_exact`: every round of every respondent in one launch;
  (b) the loop it replaces, composed from the public API: per round `select_next_questions_field` on the rows still
      unasked, then `fold_in_exact(field=...)` of the answering respondents on everything they have answered so far (the
      `torch.isin` / `torch.cat` glue included);
  (c) `elicit_field(n_steps=--steps)`: the Adam session on the same closed-form objective.

One shape, one JSON line (appended to profiles/elicit_field_exact_bench.jsonl with --record): tools/elicit_field_bench.py's
-- 10,000 respondents x 100-row pools, F = 3 (user, item, format: ML-20M's user and item counts and 4 formats), d = 128,
'reg', 20 rounds, cold start.  The answers are planted: the model's own mean prediction of each pool row under the
respondents' table rows plus N(0, 0.5^2) noise, so that a session from the prior has something to learn.  Times: the
three calls interleaved (a, b, c, a, b, c, ..), HIP-event medians over `--reps` rounds after `--warmup`, the whole public
call each (argument checks, sorts, operand passes, kernels); every call leaves the model as it found it.  The split of
(a) between the operand passes and the session kernel is taken from one torch.profiler trace; null if the profiler
gives no kernel records.  Quality: the per-round RMSE of `elicitation_curve_field_exact` and of
`elicitation_curve_field(n_steps=--steps)` on the rows still unasked, strategy "variance", values only."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def composed_loop(m, pool, y_pool, field, rounds, strategy):
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
        m.fold_in_exact(Xa[who], ya[who], field=field)
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
            if "k_foldin_prep" in ev.key or "k_foldin_solve_prep" in ev.key or "k_elicit_ctx_prep" in ev.key:
                out["operand_pass_ms"] = round((out["operand_pass_ms"] or 0.0) + t / 1e3, 4)
            elif "k_elicit_solve" in ev.key:
                out["session_kernel_ms"] = round((out["session_kernel_ms"] or 0.0) + t / 1e3, 4)
    except Exception as e:                                  # (a profiler without kernel records: the split stays null)
        out["split_error"] = repr(e)[:200]
    return out


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--respondents", type=int, default=10_000)
    ap.add_argument("--pool", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--record", action="store_true", help="append the line to profiles/elicit_field_exact_bench.jsonl")
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
    R = args.respondents * args.pool
    users = torch.randperm(N, device=dev, generator=g)[:args.respondents]
    pool = torch.stack([users.repeat_interleave(args.pool), N + torch.randint(0, M, (R,), device=dev, generator=g),
                        N + M + torch.randint(0, K, (R,), device=dev, generator=g)], 1)
    field, strategy = 0, "variance"
    truth, _, _ = m.field_moments(pool, field)
    y_pool = truth + 0.5 * torch.randn(R, device=dev, generator=g)
    start = m._flat.clone()

    def restore():
        m._flat.copy_(start)
        m.params_changed()

    def exact():
        m.elicit_field_exact(pool, y_pool, args.rounds, field, strategy, reset=True)

    def loop():
        restore()
        composed_loop(m, pool, y_pool, field, args.rounds, strategy)

    def adam():
        m.elicit_field(pool, y_pool, args.rounds, field, strategy, n_steps=args.steps, lr=0.05, objective="closed_form",
                       reset=True)

    calls = (("exact", exact), ("loop", loop), ("adam", adam))
    ts = {k: [] for k, _ in calls}
    for rep in range(args.warmup + args.reps):              # interleaved: a, b, c, a, b, c, ..
        for k, fn in calls:
            t = once(fn)
            if rep >= args.warmup:
                ts[k].append(t)
    restore()
    med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
    split = kernel_split(exact)
    c_exact = m.elicitation_curve_field_exact(pool, y_pool, args.rounds, field, strategies=(strategy,), reset=True)
    c_adam = m.elicitation_curve_field(pool, y_pool, args.rounds, field, strategies=(strategy,), n_steps=args.steps,
                                       lr=0.05, objective="closed_form", reset=True)
    assert torch.equal(m._flat, start)
    rec = {"shape": "ml20m_formats", "respondents": args.respondents, "pool_rows": R, "F": 3, "field": field, "d": m.d,
           "strategy": strategy, "rounds": args.rounds, "steps": args.steps, "reps": args.reps,
           "exact_session_ms": round(med["exact"], 3), "composed_exact_loop_ms": round(med["loop"], 3),
           "adam_session_ms": round(med["adam"], 3),
           "loop_over_exact": round(med["loop"] / med["exact"], 2), "adam_over_exact": round(med["adam"] / med["exact"], 2),
           **split,
           "rmse_exact": [round(v, 5) for v in c_exact[strategy]], "rmse_adam": [round(v, 5) for v in c_adam[strategy]],
           "device": torch.cuda.get_device_name(0), "when": time.strftime("%Y-%m-%dT%H:%M:%S")}
    if args.note:
        rec["note"] = args.note
    print(json.dumps(rec), flush=True)
    if args.record:
        with open(os.path.join(ROOT, "profiles", "elicit_field_exact_bench.jsonl"), "a") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

"""Fold-in (include/vfm_foldin.h) against a torch fp32 GPU composition of the same objective and against a refit.

Two shapes, one JSON line each (also appended to profiles/foldin_bench.jsonl with --write):
  fraction  536 students x 5 answers, d = 5, 'class' (sampled objective), the elicitation example's model; the refit is
            the example's `fit` over all training rows for epochs // 6 = 10 epochs.
  ml20m     10,000 users x 20 ratings, d = 128, 'reg' (closed form), ML-20M table shape (138,493 + 26,744 entities).
Every fold-in runs `--steps` Adam steps (default 200).  The composition is autograd of the objective batched over all
entities + torch.optim.Adam, the frozen row operands formed once outside the loop.  Times: HIP-event medians over `--reps`
calls after `--warmup`, the whole public call (argument checks, sort, operand prep, kernel) plus a restore of the table
before each call (a conservative margin: ~0.1 ms at the ML-20M shape)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def torch_composition(m, X, y, steps, lr, objective):
    """fp32 autograd + torch.optim.Adam of the fold-in objective of every entity of X[:, 0] at once."""
    link = (lambda s: s.abs()) if m.link == "abs" else torch.nn.functional.softplus
    d = m.d
    ent, bia, scal = m._views(m._flat)
    ents, idx = torch.unique(X[:, 0], return_inverse=True)
    it = X[:, 1]
    mu_i, sg_i = ent[it, :d], link(ent[it, d:])
    bw, sw2 = bia[it, 0], link(bia[it, 1]) ** 2
    prec = link(scal[0])
    m0, sg0 = scal[1], link(scal[2])
    th = [ent[ents, :d].clone().requires_grad_(), ent[ents, d:].clone().requires_grad_(),
          bia[ents, 0].clone().requires_grad_(), bia[ents, 1].clone().requires_grad_()]
    opt = torch.optim.Adam(th, lr=lr)
    for _ in range(steps):
        opt.zero_grad()
        mu, sg, mw, sgw = th[0], link(th[1]), th[2], link(th[3])
        if objective == "closed_form":
            E = m0 + bw + mw[idx] + (mu[idx] * mu_i).sum(1)
            A = sg_i ** 2
            V = sg0 ** 2 + sw2 + sgw[idx] ** 2 + (mu[idx] ** 2 * A + sg[idx] ** 2 * (A + mu_i ** 2)).sum(1)
            nll = 0.5 * prec * ((y - E) ** 2 + V) - 0.5 * torch.log(prec)
        else:
            eu = torch.randn(ents.numel(), d, device=X.device)
            ei = torch.randn(X.shape[0], d, device=X.device)
            ew = torch.randn(ents.numel(), device=X.device)
            pred = (m0 + sg0 * torch.randn((), device=X.device) + bw + link(bia[it, 1]) * torch.randn(X.shape[0], device=X.device)
                    + (mw + sgw * ew)[idx] + ((mu + sg * eu)[idx] * (mu_i + sg_i * ei)).sum(1))
            nll = torch.nn.functional.softplus(pred) - y * pred
        kl = (0.5 * (sg ** 2 + mu ** 2 - 1) - torch.log(sg)).sum() + (0.5 * (sgw ** 2 + mw ** 2 - 1) - torch.log(sgw)).sum()
        (nll.sum() + kl).backward()
        opt.step()
    return th


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="fraction,ml20m")
    ap.add_argument("--write", action="store_true", help="append the lines to profiles/foldin_bench.jsonl")
    ap.add_argument("--note", default=None, help="kept in the line: what was measured, e.g. the commit")
    args = ap.parse_args()
    from vae_amd.model import VFM
    from vae_amd.data import load_fraction
    dev = torch.device("cuda")
    lines = []
    for shape in args.shapes.split(","):
        torch.manual_seed(0)
        if shape == "fraction":
            N, M, Xtr, Xte, ytr, yte = load_fraction(os.path.join(ROOT, "tests", "golden", "fraction"))
            Xtr, ytr = torch.as_tensor(Xtr), torch.as_tensor(ytr)
            m = VFM(N, M, embedding_size=5, output="class", device=dev)
            m.fit(Xtr, ytr, n_epochs=60, batch_size=100000, verbose=False)
            g = torch.Generator().manual_seed(1)
            users = torch.arange(N)
            X = torch.stack([users.repeat_interleave(5), N + torch.randint(0, M, (5 * N,), generator=g)], 1).to(dev)
            y = (torch.rand(5 * N, generator=g) < 0.5).float().to(dev)
            objective, lr = "sampled", 0.05
            refit = lambda: m.fit(Xtr, ytr, n_epochs=10, batch_size=100000, verbose=False)
        else:
            N, M = 138_493, 26_744
            m = VFM(N, M, embedding_size=128, output="reg", device=dev)
            with torch.no_grad():
                m._flat.mul_(0.3)
            g = torch.Generator(device=dev).manual_seed(1)
            users = torch.randperm(N, device=dev, generator=g)[:10_000]
            X = torch.stack([users.repeat_interleave(20), N + torch.randint(0, M, (200_000,), device=dev, generator=g)], 1)
            y = torch.randint(1, 6, (200_000,), device=dev, generator=g).float()
            objective, lr, refit = "closed_form", 0.05, None
        start = m._flat.clone()

        def fold():
            m._flat.copy_(start)
            m.fold_in(X, y, n_steps=args.steps, lr=lr, objective=objective)

        t_fold = timed(fold, args.warmup, args.reps)
        m._flat.copy_(start)
        t_torch = timed(lambda: torch_composition(m, X, y, args.steps, lr, objective), 1, max(1, args.reps // 2))
        rec = {"shape": shape, "entities": int(torch.unique(X[:, 0]).numel()), "rows": int(X.shape[0]), "d": m.d,
               "objective": objective, "steps": args.steps, "fold_in_ms": round(t_fold, 3),
               "torch_composition_ms": round(t_torch, 3), "speedup_vs_torch": round(t_torch / t_fold, 2)}
        if refit is not None:
            m._flat.copy_(start)
            rec["refit_ms"] = round(timed(refit, 0, 1), 3)
        rec["device"] = torch.cuda.get_device_name(0)
        rec["when"] = time.strftime("%Y-%m-%dT%H:%M:%S")
        if args.note:
            rec["note"] = args.note
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if args.write:
        with open(os.path.join(ROOT, "profiles", "foldin_bench.jsonl"), "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Step time of the ELBO variants: the step as `VFMClosedForm.fit` runs it by default (VariantElbo.apply + backward +
torch.optim.Adam) against the fused step (variant_forward + vfm_variant_step_f32, `train_step`), in the same run.

The two are interleaved reading by reading (A B A B ...), each reading is `--iters` steps between two HIP events after
`--warmup` steps of both, and a point reports the median of `--readings` readings per side.  Both sides train the same
tables (timing only; the values are not compared here -- tests/test_gpu_variant_step.py does that).
Points: ML-20M shape (T = 138,493 + 26,744, d = 128, B = 100,000) closed form + priors and sampled + values; ML-100K shape
(T = 943 + 1,682) at d = 2 with fit's default batch of 8,000, closed form + priors.  Ids are uniform (synthetic_triples)
unless --zipf is given: the variant kernels walk a hot entity's list with one lane group, so a skewed batch measures that
walk on both sides.
usage: tools/variant_step_bench.py [--out profiles/variant_step_bench.jsonl] [--readings 7] [--iters 20] [--warmup 10]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

POINTS = [
    dict(name="ml20m_d128_closed_form_priors", sizes=[138493, 26744], d=128, B=100000, objective="closed_form", priors=True, values=False),
    dict(name="ml20m_d128_sampled_values", sizes=[138493, 26744], d=128, B=100000, objective="sampled", priors=False, values=True),
    dict(name="ml100k_d2_closed_form_priors", sizes=[943, 1682], d=2, B=8000, objective="closed_form", priors=True, values=False),
]


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters          # us per step


def make_sides(pt, dev, zipf=None, lr=0.02):
    from vae_amd import ops, _lib
    from vae_amd.data import synthetic_triples
    from vae_amd.variants import (VFMClosedForm, VariantElbo, VariantMoments, variant_forward, variant_adam_step,
                                  variant_step_workspace)
    sizes, d, B = pt["sizes"], pt["d"], pt["B"]
    X, y = synthetic_triples(sizes, B, seed=3, device=dev, zipf=zipf)
    y = y.to(torch.float32)
    if pt["objective"] == "closed_form":
        models = []
        for _ in range(2):                           # one model per side: neither pays for the other's parameter syncs
            torch.manual_seed(0)
            m = VFMClosedForm(sizes, d, alpha_0=1.0, device=dev)
            m.set_training_data(X)
            models.append(m)
        mu, mf = models
        plan = mu.plan(X, y)
        opt = torch.optim.Adam(mu.parameters(), lr=lr)

        def unfused():
            loss, _, _ = mu.elbo(plan=plan)
            opt.zero_grad()
            loss.backward()
            opt.step()

        def fused():
            mf.train_step(plan, lr)
        return unfused, fused
    T = sum(sizes)
    spec = ops.Spec(T=T, F=len(sizes), d=d, group_hi=tuple(int(v) for v in np.cumsum(sizes)), group_n=tuple(float(s) for s in sizes),
                    likelihood=_lib.LIK_NORMAL, nb_train=B)
    inv_occ = ops.inv_occ_from_counts(torch.bincount(X.reshape(-1), minlength=T))
    plan = ops.BatchPlan(spec, X, y, inv_occ)
    g = torch.Generator(device="cpu").manual_seed(1)
    ent = torch.cat([0.1 * torch.randn(T, d, generator=g), 0.2 * torch.ones(T, d)], 1).to(dev)
    bia = torch.cat([0.1 * torch.randn(T, 1, generator=g), 0.2 * torch.ones(T, 1)], 1).to(dev)
    sc = torch.tensor([1.0, 0.1, 0.2], device=dev)
    vals = (0.5 + torch.rand(B, len(sizes), generator=g)).to(dev) if pt["values"] else None
    leaves = [t.clone().requires_grad_(True) for t in (ent, bia, sc)]
    opt = torch.optim.Adam(leaves, lr=lr)
    step = [0]

    def unfused():
        step[0] += 1
        loss, _, _ = VariantElbo.apply(leaves[0], leaves[1], leaves[2], None, plan, inv_occ, pt["objective"], vals, None, 5, step[0])
        opt.zero_grad()
        loss.backward()
        opt.step()

    mo = VariantMoments(ent, bia, sc, None)
    ws, one, t = variant_step_workspace(plan), torch.ones(1, device=dev), [0]

    def fused():
        t[0] += 1
        st = variant_forward(plan, pt["objective"], ent, bia, sc, inv_occ, values=vals, seed=5, step=t[0])
        variant_adam_step(plan, st, ent, bia, sc, None, inv_occ, mo, lr, t[0], grad_out=one, workspace=ws)
    return unfused, fused


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "variant_step_bench.jsonl"))
    ap.add_argument("--readings", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--only", default="")
    ap.add_argument("--zipf", type=float, default=None, help="Zipf exponent of the non-user fields (default: uniform ids)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []
    for pt in POINTS:
        if a.only not in pt["name"]:
            continue
        unfused, fused = make_sides(pt, dev, a.zipf)
        for _ in range(a.warmup):
            unfused()
            fused()
        torch.cuda.synchronize()
        ru, rf = [], []
        for _ in range(a.readings):
            ru.append(timed(unfused, a.iters))
            rf.append(timed(fused, a.iters))
        mu, mf = statistics.median(ru), statistics.median(rf)
        rec = dict(point=pt["name"], T=sum(pt["sizes"]), d=pt["d"], B=pt["B"], objective=pt["objective"], priors=pt["priors"],
                   values=pt["values"], zipf=a.zipf, unfused_us=round(mu, 1), fused_us=round(mf, 1), speedup=round(mu / mf, 3),
                   unfused_readings_us=[round(v, 1) for v in ru], fused_readings_us=[round(v, 1) for v in rf],
                   readings=a.readings, iters=a.iters, warmup=a.warmup, device=torch.cuda.get_device_name(0))
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""fit_bound beside fit() on a 'class' model: J (VFM.bound_objective) and held-out log loss per sweep / per 5 epochs.

    python examples/fit_bound_synthetic.py [--rows 200000] [--sweeps 8] [--n-iters 8] [--learn-priors]

fit_bound trains by coordinate ascent on the Jaakkola-Jordan bound (per entity and field, n_iters rounds of one weighted
closed-form solve; then the global bias): there is no learning rate, no sampling and no seed, and J never increases.
fit() is the sampled-ELBO Adam loop of the reference.  The labels are drawn from a planted low-rank logit.

--learn-priors plants the two fields at different scales (factor std 0.3 for the users, 1.0 for the items, as in
fit_exact_synthetic.py) and gives every field a Gaussian prior N(mean, 1 / prec) per coordinate that fit_bound learns: each
field's rounds are followed by the prior's own closed-form minimiser (sweep.GroupPriors, learn_priors=True), and J is
bound_objective(priors=).  The learnt precisions of the factors are printed per sweep."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vae_amd.data import synthetic_triples  # noqa: E402
from vae_amd.model import VFM  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--sweeps", type=int, default=8)
    ap.add_argument("--d", type=int, default=16)
    ap.add_argument("--n-iters", type=int, default=8)
    ap.add_argument("--learn-priors", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda")
    sizes = (3000, 1000)
    X, _ = synthetic_triples(sizes, args.rows, seed=0, output="class", device=dev, zipf=1.0)
    g = torch.Generator(device=dev).manual_seed(1)
    U = torch.randn(sum(sizes), 8, device=dev, generator=g) * 0.8
    if args.learn_priors:
        U[:sizes[0]] *= 0.3 / 0.8
        U[sizes[0]:] *= 1.0 / 0.8
    logit = -0.5 + (3.0 if args.learn_priors else 1.0) * (U[X[:, 0]] * U[X[:, 1]]).sum(1)
    y = (torch.rand(args.rows, device=dev, generator=g) < torch.sigmoid(logit)).float()
    cut = int(0.9 * args.rows)
    Xtr, ytr, Xte, yte = X[:cut], y[:cut], X[cut:], y[cut:]

    def log_loss(m):
        return float(torch.nn.functional.binary_cross_entropy_with_logits(m.predictive_moments(Xte)[0], yte))

    torch.manual_seed(0)
    m = VFM(*sizes, embedding_size=args.d, output="class", device=dev)
    pr = None
    if args.learn_priors:
        from vae_amd import sweep
        pr = sweep.GroupPriors(2, args.d, dev)
    print(f"fit_bound  start    J {m.bound_objective(Xtr, ytr, priors=pr):14.2f}  held-out log loss {log_loss(m):.4f}")
    for s in range(args.sweeps):
        out = m.fit_bound(Xtr, ytr, n_sweeps=1, n_iters=args.n_iters, priors=pr, learn_priors=args.learn_priors)
        print(f"fit_bound  sweep {s + 1:2d} J {out['objective'][-1]:14.2f}  held-out log loss {log_loss(m):.4f}  "
              f"{out['ms'][0]:.1f} ms")
        if pr is not None:
            print("           mean learnt precision of the factors: users "
                  f"{float(pr.prec[0, 1:].mean()):.2f}, items {float(pr.prec[1, 1:].mean()):.2f}")
    torch.manual_seed(0)
    a = VFM(*sizes, embedding_size=args.d, output="class", device=dev)
    for s in range(args.sweeps):
        a.fit(Xtr, ytr, n_epochs=5, batch_size=20_000, verbose=False)
        print(f"fit        epoch {5 * (s + 1):2d} J {a.bound_objective(Xtr, ytr):14.2f}  held-out log loss {log_loss(a):.4f}")


if __name__ == "__main__":
    main()

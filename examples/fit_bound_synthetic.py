"""fit_bound beside fit() on a 'class' model: J (VFM.bound_objective) and held-out log loss per sweep / per 5 epochs.

    python examples/fit_bound_synthetic.py [--rows 200000] [--sweeps 8] [--n-iters 8]

fit_bound trains by coordinate ascent on the Jaakkola-Jordan bound (per entity and field, n_iters rounds of one weighted
closed-form solve; then the global bias): there is no learning rate, no sampling and no seed, and J never increases.
fit() is the sampled-ELBO Adam loop of the reference.  The labels are drawn from a planted low-rank logit."""
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
    args = ap.parse_args()
    dev = torch.device("cuda")
    sizes = (3000, 1000)
    X, _ = synthetic_triples(sizes, args.rows, seed=0, output="class", device=dev, zipf=1.0)
    g = torch.Generator(device=dev).manual_seed(1)
    U = torch.randn(sum(sizes), 8, device=dev, generator=g) * 0.8
    logit = -0.5 + (U[X[:, 0]] * U[X[:, 1]]).sum(1)
    y = (torch.rand(args.rows, device=dev, generator=g) < torch.sigmoid(logit)).float()
    cut = int(0.9 * args.rows)
    Xtr, ytr, Xte, yte = X[:cut], y[:cut], X[cut:], y[cut:]

    def log_loss(m):
        return float(torch.nn.functional.binary_cross_entropy_with_logits(m.predictive_moments(Xte)[0], yte))

    torch.manual_seed(0)
    m = VFM(*sizes, embedding_size=args.d, output="class", device=dev)
    print(f"fit_bound  start    J {m.bound_objective(Xtr, ytr):14.2f}  held-out log loss {log_loss(m):.4f}")
    for s in range(args.sweeps):
        out = m.fit_bound(Xtr, ytr, n_sweeps=1, n_iters=args.n_iters)
        print(f"fit_bound  sweep {s + 1:2d} J {out['objective'][-1]:14.2f}  held-out log loss {log_loss(m):.4f}  "
              f"{out['ms'][0]:.1f} ms")
    torch.manual_seed(0)
    a = VFM(*sizes, embedding_size=args.d, output="class", device=dev)
    for s in range(args.sweeps):
        a.fit(Xtr, ytr, n_epochs=5, batch_size=20_000, verbose=False)
        print(f"fit        epoch {5 * (s + 1):2d} J {a.bound_objective(Xtr, ytr):14.2f}  held-out log loss {log_loss(a):.4f}")


if __name__ == "__main__":
    main()

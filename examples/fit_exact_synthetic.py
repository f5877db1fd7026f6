"""fit_exact beside fit() on synthetic_triples: J (VFM.exact_objective) and test RMSE per sweep / per 5 epochs.

    python examples/fit_exact_synthetic.py [--rows 200000] [--sweeps 8] [--learn-priors]

fit_exact trains by exact coordinate ascent (one closed-form solve per entity and field, then the three scalars):
there is no learning rate, and J never increases.  fit() is the sampled-ELBO Adam loop of the reference.
--learn-priors runs fit_exact a second time with a learnt Gaussian prior per field (sweep.GroupPriors; each field's prior
block follows its solves) and prints J, the test RMSE and the learnt precisions per sweep beside the fixed N(0, 1) run;
the two J are different objectives (each run's own), the RMSE is comparable."""
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
    ap.add_argument("--learn-priors", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda")
    sizes = (3000, 1000)
    X, y = synthetic_triples(sizes, args.rows, seed=0, device=dev, zipf=1.0)
    cut = int(0.9 * args.rows)
    Xtr, ytr, Xte, yte = X[:cut], y[:cut], X[cut:], y[cut:]

    def rmse(m):
        return float(((m.predictive_moments(Xte)[0] - yte) ** 2).mean().sqrt())

    torch.manual_seed(0)
    m = VFM(*sizes, embedding_size=args.d, output="reg", device=dev)
    print(f"fit_exact  start    J {m.exact_objective(Xtr, ytr):14.2f}  test RMSE {rmse(m):.4f}")
    for s in range(args.sweeps):
        out = m.fit_exact(Xtr, ytr, n_sweeps=1)
        print(f"fit_exact  sweep {s + 1:2d} J {out['objective'][-1]:14.2f}  test RMSE {rmse(m):.4f}  {out['ms'][0]:.1f} ms")
    if args.learn_priors:
        from vae_amd import sweep
        torch.manual_seed(0)
        h = VFM(*sizes, embedding_size=args.d, output="reg", device=dev)
        pr = sweep.GroupPriors(h.F, h.d, dev)
        print(f"learnt     start    J {h.exact_objective(Xtr, ytr, priors=pr):14.2f}  test RMSE {rmse(h):.4f}")
        for s in range(args.sweeps):
            out = h.fit_exact(Xtr, ytr, n_sweeps=1, priors=pr, learn_priors=True)
            lo, hi = pr.prec.min(1).values.tolist(), pr.prec.max(1).values.tolist()
            print(f"learnt     sweep {s + 1:2d} J {out['objective'][-1]:14.2f}  test RMSE {rmse(h):.4f}  {out['ms'][0]:.1f} ms  "
                  f"prec per field [min, max] {[[round(a, 2), round(b, 2)] for a, b in zip(lo, hi)]}  clamped {out['clamped']}")
    torch.manual_seed(0)
    a = VFM(*sizes, embedding_size=args.d, output="reg", device=dev)
    for s in range(args.sweeps):
        a.fit(Xtr, ytr, n_epochs=5, batch_size=20_000, verbose=False)
        print(f"fit        epoch {5 * (s + 1):2d} J {a.exact_objective(Xtr, ytr):14.2f}  test RMSE {rmse(a):.4f}")


if __name__ == "__main__":
    main()

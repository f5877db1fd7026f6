"""fit_implicit on planted clicks: every user has a planted taste vector, clicks the items it likes best (y = 1 and
nothing else), and the held-out clicks are ranked against the whole catalog.  fit_exact sees only the observed rows, all
ones, and has nothing to learn; fit_implicit treats every other (user, item) pair as a row with target 0 and weight w0.

    python examples/fit_implicit_synthetic.py [--w0 0.05] [--sweeps 8] [--learn-priors]

--learn-priors: every field gets a Gaussian prior mean and precision per coordinate, set to its closed-form minimiser
of J_imp after the field's solves over ALL of the field's entities (DESIGN.md §4 "Hierarchical implicit sweeps").
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def planted_clicks(n_u, n_i, rank, per_user, seed):
    """Each user's per_user clicks: the items with the largest planted affinity plus Gumbel noise.  Distinct pairs."""
    g = torch.Generator().manual_seed(seed)
    U, V = torch.randn(n_u, rank, generator=g), torch.randn(n_i, rank, generator=g)
    noise = -torch.log(-torch.log(torch.rand(n_u, n_i, generator=g)))
    items = torch.topk(U @ V.T + noise, per_user, dim=1).indices
    users = torch.arange(n_u).repeat_interleave(per_user)
    return torch.stack([users, n_u + items.reshape(-1)], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1500)
    ap.add_argument("--items", type=int, default=600)
    ap.add_argument("--d", type=int, default=16)
    ap.add_argument("--w0", type=float, default=0.05, help="weight of an unobserved pair (a starting value, not tuned)")
    ap.add_argument("--sweeps", type=int, default=8)
    ap.add_argument("--learn-priors", action="store_true", help="learn each field's prior N(mean, 1 / prec)")
    args = ap.parse_args()
    from vae_amd.model import VFM
    dev = torch.device("cuda")
    X = planted_clicks(args.users, args.items, 6, 30, seed=0)
    held = torch.rand(X.shape[0], generator=torch.Generator().manual_seed(1)) < 0.2
    Xtr, Xte = X[~held].to(dev), X[held].to(dev)
    ones = lambda x: torch.ones(x.shape[0], device=dev)

    def recall(m):
        r = m.evaluate_ranking(Xte, ones(Xte), ks=(10,), exclude=Xtr, threshold=0.5)
        return r["recall@10"], r["ndcg@10"]

    torch.manual_seed(0)
    m = VFM(args.users, args.items, embedding_size=args.d, output="reg", device=dev)
    print("untrained: recall@10 %.4f ndcg@10 %.4f" % recall(m))
    out = m.fit_implicit(Xtr, n_sweeps=args.sweeps, w0=args.w0, learn_priors=args.learn_priors,
                         on_step=lambda s, w: print("  sweep %d: recall@10 %.4f ndcg@10 %.4f" % ((s,) + recall(m)))
                         if w == "scalars" else None)
    print("J_imp:", [round(v, 1) for v in out["objective"]])
    if args.learn_priors:
        for f, name in enumerate(("users", "items")):
            pr = out["priors"].prec[f].cpu()
            print("  learnt precisions of the %s: weight %.3g, factors %.3g .. %.3g (clamped coordinates: %d)"
                  % (name, float(pr[0]), float(pr[1:].min()), float(pr[1:].max()), out["clamped"][f]))
    torch.manual_seed(0)
    e = VFM(args.users, args.items, embedding_size=args.d, output="reg", device=dev)
    e.fit_exact(Xtr, ones(Xtr), n_sweeps=args.sweeps)
    print("fit_exact on the clicks alone: recall@10 %.4f ndcg@10 %.4f" % recall(e))


if __name__ == "__main__":
    main()

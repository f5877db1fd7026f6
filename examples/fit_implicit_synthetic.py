"""fit_implicit on planted clicks: every user has a planted taste vector, clicks the items it likes best (y = 1 and
nothing else), and the held-out clicks are ranked against the whole catalog.  fit_exact sees only the observed rows, all
ones, and has nothing to learn; fit_implicit treats every other (user, item) pair as a row with target 0 and weight w0.

    python examples/fit_implicit_synthetic.py [--w0 0.05] [--sweeps 8] [--learn-priors] [--counts [--alpha 5]]

--learn-priors: every field gets a Gaussian prior mean and precision per coordinate, set to its closed-form minimiser
of J_imp after the field's solves over ALL of the field's entities (DESIGN.md §4 "Hierarchical implicit sweeps").
--counts: every click comes with a planted play count that grows with the planted preference, and the model is fitted
with weights=sweep.hkv_weights(counts, w0, alpha) (DESIGN.md §4 "Weighted implicit sweeps") beside the binarised call.
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


def planted_counts(n_u, n_i, rank, per_user, seed, scale=4.0):
    """planted_clicks with a play count per click: 1 + Poisson(scale sigmoid(affinity / sqrt(rank))), so that a pair the
    user likes better is played more often.  Returns (X [R, 2], counts [R] fp32)."""
    g = torch.Generator().manual_seed(seed)
    U, V = torch.randn(n_u, rank, generator=g), torch.randn(n_i, rank, generator=g)
    noise = -torch.log(-torch.log(torch.rand(n_u, n_i, generator=g)))
    aff = U @ V.T
    items = torch.topk(aff + noise, per_user, dim=1).indices
    users = torch.arange(n_u).repeat_interleave(per_user)
    rate = scale * torch.sigmoid(aff[users, items.reshape(-1)] / rank ** 0.5)
    return torch.stack([users, n_u + items.reshape(-1)], 1), 1.0 + torch.poisson(rate, generator=g)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1500)
    ap.add_argument("--items", type=int, default=600)
    ap.add_argument("--d", type=int, default=16)
    ap.add_argument("--w0", type=float, default=0.05, help="weight of an unobserved pair (a starting value, not tuned)")
    ap.add_argument("--sweeps", type=int, default=8)
    ap.add_argument("--learn-priors", action="store_true", help="learn each field's prior N(mean, 1 / prec)")
    ap.add_argument("--counts", action="store_true", help="planted play counts as weights= (sweep.hkv_weights)")
    ap.add_argument("--alpha", type=float, default=5.0,
                    help="--counts: a click weighs w0 (1 + alpha count); at alpha = 1 / w0 that is w0 + count (a starting "
                         "value, not tuned: on these planted counts larger values cost held-out recall)")
    args = ap.parse_args()
    from vae_amd import sweep
    from vae_amd.model import VFM
    dev = torch.device("cuda")
    if args.counts:
        X, counts = planted_counts(args.users, args.items, 6, 30, seed=0)
    else:
        X, counts = planted_clicks(args.users, args.items, 6, 30, seed=0), None
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
    if args.counts:
        weights = sweep.hkv_weights(counts[~held], args.w0, args.alpha).to(dev)
        torch.manual_seed(0)
        c = VFM(args.users, args.items, embedding_size=args.d, output="reg", device=dev)
        outc = c.fit_implicit(Xtr, n_sweeps=args.sweeps, w0=args.w0, weights=weights, learn_priors=args.learn_priors)
        print("with weights = w0 (1 + %g counts), counts 1 .. %d: recall@10 %.4f ndcg@10 %.4f (binarised, above: %.4f %.4f)"
              % ((args.alpha, int(counts.max())) + recall(c) + recall(m)))
        print("J_imp with the weights:", [round(v, 1) for v in outc["objective"]])
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

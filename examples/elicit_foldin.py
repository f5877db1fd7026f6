#!/usr/bin/env python3
"""Preference elicitation on the `fraction` data set with fold-in: the loop of elicit_fraction.py, but after each round
the answering students are folded in (`VFM.fold_in`, every other parameter frozen) instead of refitting the whole model.
Prints the test AUC per round for both, side by side:

    python examples/elicit_foldin.py [rounds] [epochs] [strategy] [--exact | --bound]   (needs an MI355X; vae_amd has no CPU fallback)

The refit moves every student's and question's posterior on every Adam step (dense Adam); the fold-in moves only the
rows of the students who answered, warm-started from their current posteriors.

--exact: the same loop with 'reg' models (the 0/1 answers as a regression target, test RMSE in place of the AUC), whose
fold-in objective has a closed-form optimum: the students are folded in with `VFM.fold_in_exact`, one solve per student
in one launch, no n_steps and no lr to choose.

--bound: the 'class' models and the AUC of the default loop, the students folded in with `VFM.fold_in_bound`: a few rounds
of exact solves of the Jaakkola-Jordan bound of the Bernoulli likelihood, no lr, no sampling and no seed to choose."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from vae_amd.model import VFM
from vae_amd.data import load_fraction


def main():
    argv = [a for a in sys.argv[1:] if a not in ("--exact", "--bound")]
    exact, bound = "--exact" in sys.argv[1:], "--bound" in sys.argv[1:]
    if exact and bound:
        raise SystemExit("--exact ('reg' models) and --bound ('class' models) exclude each other")
    rounds = int(argv[0]) if len(argv) > 0 else 5
    epochs = int(argv[1]) if len(argv) > 1 else 60
    strategy = argv[2] if len(argv) > 2 else "variance"
    output, metric, name = ("reg", "rmse", "RMSE") if exact else ("class", "auc", "AUC")
    N, M, X_train, X_test, y_train, y_test = load_fraction(os.path.join(ROOT, "tests", "golden", "fraction"))
    X_train, X_test = torch.as_tensor(X_train), torch.as_tensor(X_test)
    y_train, y_test = torch.as_tensor(y_train), torch.as_tensor(y_test)
    models = {}
    for kind in ("refit", "fold_in"):
        torch.manual_seed(42)
        models[kind] = VFM(N, M, embedding_size=5, output=output, device="cuda")
        models[kind].fit(X_train, y_train, n_epochs=epochs, batch_size=100000, verbose=False)
    state = {k: (X_train.clone(), y_train.clone(), X_test.clone(), y_test.clone()) for k in models}
    auc = {k: models[k].evaluate(X_test, y_test)[metric] for k in models}
    print(f"{strategy}: round 0, {len(X_test)} unasked, test {name} refit {auc['refit']:.4f}  fold-in {auc['fold_in']:.4f}")
    for r in range(1, rounds + 1):
        for kind, model in models.items():
            Xt, yt, pool, y_pool = state[kind]
            _, rows = model.select_next_questions(pool, n=1, strategy=strategy, seed=r)
            asked = rows[rows >= 0].cpu()
            keep = torch.ones(len(pool), dtype=torch.bool)
            keep[asked] = False
            Xt, yt = torch.cat([Xt, pool[asked]]), torch.cat([yt, y_pool[asked]])
            if kind == "refit":
                model.fit(Xt, yt, n_epochs=max(1, epochs // 6), batch_size=100000, verbose=False)
            else:
                # every row of the answering students (their earlier answers too): their posteriors refitted alone
                who = torch.isin(Xt[:, 0], pool[asked][:, 0])
                if exact:
                    model.fold_in_exact(Xt[who], yt[who])
                elif bound:
                    model.fold_in_bound(Xt[who], yt[who])
                else:
                    model.fold_in(Xt[who], yt[who], n_steps=200, lr=0.05)
            pool, y_pool = pool[keep], y_pool[keep]
            state[kind] = (Xt, yt, pool, y_pool)
            auc[kind] = model.evaluate(pool, y_pool)[metric]
        print(f"{strategy}: round {r}, {len(state['refit'][2])} unasked, test {name} refit {auc['refit']:.4f}  "
              f"fold-in {auc['fold_in']:.4f}")


if __name__ == "__main__":
    main()

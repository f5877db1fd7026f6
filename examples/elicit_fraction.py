#!/usr/bin/env python3
"""Preference elicitation on the `fraction` data set (536 students x 20 questions, binary outcomes): the reference's
interactive loop (vfm.py:1236-1251) -- for each strategy `mean`, `random`, `variance`, fit, then in every round ask each
test student the question `select_next_questions` picks from the ones not yet asked, add the answers to the training
data, refit, and print the AUC on the questions still unasked:

    python examples/elicit_fraction.py [rounds] [epochs]          (needs an MI355X; vae_amd has no CPU fallback)

The scores are the closed-form predictive moments (include/vfm_rank.h): `mean` asks the question whose answer the model
is least sure of (probability closest to 0.5), `variance` the one of largest logit variance."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from vae_amd.model import VFM
from vae_amd.data import load_fraction


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    epochs = int(sys.argv[2]) if len(sys.argv) > 2 else 60
    N, M, X_train, X_test, y_train, y_test = load_fraction(os.path.join(ROOT, "tests", "golden", "fraction"))
    X_train, X_test = torch.as_tensor(X_train), torch.as_tensor(X_test)
    y_train, y_test = torch.as_tensor(y_train), torch.as_tensor(y_test)
    for strategy in ("mean", "random", "variance"):
        torch.manual_seed(42)
        model = VFM(N, M, embedding_size=5, output="class", device="cuda")
        Xt, yt = X_train.clone(), y_train.clone()
        pool, y_pool = X_test.clone(), y_test.clone()
        model.fit(Xt, yt, n_epochs=epochs, batch_size=100000, verbose=False)
        print(f"{strategy}: round 0, {len(pool)} questions unasked, test AUC {model.evaluate(pool, y_pool)['auc']:.4f}")
        for r in range(1, rounds + 1):
            _, rows = model.select_next_questions(pool, n=1, strategy=strategy, seed=r)
            asked = rows[rows >= 0].cpu()
            keep = torch.ones(len(pool), dtype=torch.bool)
            keep[asked] = False
            Xt, yt = torch.cat([Xt, pool[asked]]), torch.cat([yt, y_pool[asked]])
            pool, y_pool = pool[keep], y_pool[keep]
            model.fit(Xt, yt, n_epochs=max(1, epochs // 6), batch_size=100000, verbose=False)
            print(f"{strategy}: round {r}, asked {len(asked)}, {len(pool)} unasked, "
                  f"test AUC {model.evaluate(pool, y_pool)['auc']:.4f}")


if __name__ == "__main__":
    main()

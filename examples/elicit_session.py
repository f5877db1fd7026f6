#!/usr/bin/env python3
"""The reference's interactive experiment (vfm.py:1236-1251) on the `fraction` data set, as elicitation sessions: the
students of the test rows are treated as a cold-start population (their posteriors start from the prior), every one of
them is asked up to 15 questions picked by a strategy from the student's current posterior, and after each answer the
student's posterior alone is refitted -- all rounds of all students in one launch per strategy (`VFM.elicit`).  Prints
the test AUC on the questions still unasked after every round, once per strategy:

    python examples/elicit_session.py [questions] [epochs]     (needs an MI355X; vae_amd has no CPU fallback)

With --exact the same questionnaire runs on a 'reg' model of the 0/1 answers (the closed form needs the Gaussian
likelihood) and every answer is followed by the exact posterior instead of 200 Adam steps
(`VFM.elicit_field_exact`): the RMSE on the questions still unasked, beside the Adam session's on the same model.

    python examples/elicit_session.py --exact [questions] [epochs]

With --ranking the 'reg' model's exact sessions are also judged as a recommender: beside the RMSE curve, the NDCG@10 of
each student's correctly answered held-out questions in the ranking of all questions under the student's posterior of
every round (`VFM.elicitation_ranking_curve_field`: the posteriors stay outside the model, one launch per strategy).
Every student's test rows are split in two: the first half is the pool of questions, the second half is held out.

    python examples/elicit_session.py --ranking [questions] [epochs]

With --design the same split compares which question is asked: the NDCG@10 curves of random / variance / design side
by side, where "design" (`VFM.elicit_field_design`) asks the question that most reduces the predictive variance over
the student's held-out questions.

    python examples/elicit_session.py --design [questions] [epochs]

With --bound the 'class' model's questionnaire runs without Adam: every answer is followed by n_iters = 8 rounds of the
Jaakkola-Jordan bound's exact solves (`VFM.elicit_field_bound`; 8 is an untuned starting value): the AUC on the questions
still unasked, beside the Adam session's (200 steps on the sampled objective) on the same model.

    python examples/elicit_session.py --bound [questions] [epochs]

With --priors the model is trained by exact coordinate ascent with a learnt Gaussian prior per field
(`VFM.fit_exact(learn_priors=True)`; with --bound after it, `VFM.fit_bound(learn_priors=True)` on a 'class' model) and the
cold-start questionnaire (reset=True: every student starts at the prior) runs twice: under the learnt priors
(`priors=`) and under N(0, 1), side by side.

    python examples/elicit_session.py --priors [--bound] [questions] [sweeps]

With --implicit the correct answers are clicks: a 'reg' model is trained by `VFM.fit_implicit` on the training rows
answered correctly (every other (student, question) pair counts as target 0 with weight w0), the test students are
cold-started by the implicit recipe -- `fold_in_implicit` without rows gives them the base-only optimum -- and interviewed
by `VFM.elicit_field_implicit`, whose every fold is the optimum over all of a student's pairs.  Prints the NDCG@10 of the
held-out correct answers under every round's posteriors, beside the exact session's (reset=True) on the same model.

    python examples/elicit_session.py --implicit [questions] [sweeps]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from vae_amd.model import VFM
from vae_amd.data import load_fraction


def main_exact(argv):
    questions = int(argv[0]) if len(argv) > 0 else 15
    epochs = int(argv[1]) if len(argv) > 1 else 60
    N, M, X_train, X_test, y_train, y_test = load_fraction(os.path.join(ROOT, "tests", "golden", "fraction"))
    X_train, X_test = torch.as_tensor(X_train), torch.as_tensor(X_test)
    y_train, y_test = torch.as_tensor(y_train).float(), torch.as_tensor(y_test).float()
    torch.manual_seed(42)
    model = VFM(N, M, embedding_size=5, output="reg", device="cuda")
    model.fit(X_train, y_train, n_epochs=epochs, batch_size=100000, verbose=False)
    strategies = ("random", "variance")
    exact = model.elicitation_curve_field_exact(X_test, y_test, questions, 0, strategies, reset=True, seed=1)
    adam = model.elicitation_curve_field(X_test, y_test, questions, 0, strategies, n_steps=200, lr=0.05, reset=True, seed=1)
    print(f"{len(torch.unique(X_test[:, 0]))} students, {len(X_test)} questions in the pool; RMSE exact / Adam(200)")
    print("asked  " + "  ".join(f"{s:>26}" for s in strategies))
    for q in range(questions + 1):
        print(f"{q:5d}  " + "  ".join(f"{exact[s][q]:8.4f} / {adam[s][q]:8.4f} ({exact['n_unasked'][s][q]:5d})"
                                      for s in strategies))


def main_ranking(argv, design=False):
    questions = int(argv[0]) if len(argv) > 0 else 10
    epochs = int(argv[1]) if len(argv) > 1 else 60
    N, M, X_train, X_test, y_train, y_test = load_fraction(os.path.join(ROOT, "tests", "golden", "fraction"))
    X_train, X_test = torch.as_tensor(X_train), torch.as_tensor(X_test)
    y_train, y_test = torch.as_tensor(y_train).float(), torch.as_tensor(y_test).float()
    torch.manual_seed(42)
    model = VFM(N, M, embedding_size=5, output="reg", device="cuda")
    model.fit(X_train, y_train, n_epochs=epochs, batch_size=100000, verbose=False)
    # per student: the even test rows are asked about, the odd ones are held out for the ranking
    order = torch.sort(X_test[:, 0], stable=True).indices
    nth = torch.arange(len(order)) - torch.searchsorted(X_test[order, 0].contiguous(), X_test[order, 0].contiguous())
    ask, held = order[nth % 2 == 0], order[nth % 2 == 1]
    strategies = ("random", "variance", "design") if design else ("random", "variance")
    kw = dict(reset=True, seed=1, targets=X_test[held]) if design else dict(reset=True, seed=1)
    rmse = model.elicitation_curve_field_exact(X_test[ask], y_test[ask], questions, 0, strategies, **kw)
    ndcg = model.elicitation_ranking_curve_field(X_test[ask], y_test[ask], questions, 0, X_test[held], y_test[held], 1,
                                                 ks=(10,), strategies=strategies, exact=True, threshold=0.5,
                                                 ineligible="drop", **kw)
    print(f"{len(torch.unique(X_test[ask, 0]))} students, {len(ask)} questions in the pool, {len(held)} held out, "
          f"{ndcg['n_queries']} ranking queries per strategy; RMSE on the unasked / NDCG@10 of the held-out")
    print("asked  " + "  ".join(f"{s:>19}" for s in strategies))
    for q in range(questions + 1):
        print(f"{q:5d}  " + "  ".join(f"{rmse[s][q]:8.4f} / {ndcg[s]['ndcg@10'][q]:8.4f}" for s in strategies))


def main_implicit(argv):
    questions = int(argv[0]) if len(argv) > 0 else 10
    sweeps = int(argv[1]) if len(argv) > 1 else 8
    w0 = 0.1                                                 # an untuned starting value
    N, M, X_train, X_test, y_train, y_test = load_fraction(os.path.join(ROOT, "tests", "golden", "fraction"))
    X_train, X_test = torch.as_tensor(X_train), torch.as_tensor(X_test)
    y_train, y_test = torch.as_tensor(y_train).float(), torch.as_tensor(y_test).float()
    students = torch.unique(X_test[:, 0])
    clicks = X_train[y_train == 1]                           # (the students' own rows train the questions; the recipe below forgets the students)
    torch.manual_seed(42)
    model = VFM(N, M, embedding_size=5, output="reg", device="cuda")
    model.fit_implicit(clicks, n_sweeps=sweeps, w0=w0)
    order = torch.sort(X_test[:, 0], stable=True).indices
    nth = torch.arange(len(order)) - torch.searchsorted(X_test[order, 0].contiguous(), X_test[order, 0].contiguous())
    ask, held = order[nth % 2 == 0], order[nth % 2 == 1]
    strategies = ("random", "variance")
    kw = dict(ks=(10,), strategies=strategies, threshold=0.5, ineligible="drop", seed=1)
    exact = model.elicitation_ranking_curve_field(X_test[ask], y_test[ask], questions, 0, X_test[held], y_test[held], 1,
                                                  exact=True, reset=True, **kw)
    # the cold-start recipe: a student without answers sits at the base-only optimum, then reset=False
    model.fold_in_implicit(X_test[:0], y_test[:0], 0, w0=w0, entities=students)
    imp = model.elicitation_ranking_curve_field(X_test[ask], y_test[ask], questions, 0, X_test[held], y_test[held], 1,
                                                implicit=True, w0=w0, **kw)
    print(f"{len(students)} students, {len(ask)} questions in the pool, {len(held)} held out, {imp['n_queries']} ranking "
          f"queries per strategy; NDCG@10 of the held-out: implicit session / exact session")
    print("asked  " + "  ".join(f"{s:>19}" for s in strategies))
    for q in range(questions + 1):
        print(f"{q:5d}  " + "  ".join(f"{imp[s]['ndcg@10'][q]:8.4f} / {exact[s]['ndcg@10'][q]:8.4f}" for s in strategies))


def main_bound(argv):
    questions = int(argv[0]) if len(argv) > 0 else 15
    epochs = int(argv[1]) if len(argv) > 1 else 60
    N, M, X_train, X_test, y_train, y_test = load_fraction(os.path.join(ROOT, "tests", "golden", "fraction"))
    X_train, X_test = torch.as_tensor(X_train), torch.as_tensor(X_test)
    y_train, y_test = torch.as_tensor(y_train).float(), torch.as_tensor(y_test).float()
    torch.manual_seed(42)
    model = VFM(N, M, embedding_size=5, output="class", device="cuda")
    model.fit(X_train, y_train, n_epochs=epochs, batch_size=100000, verbose=False)
    strategies = ("mean", "random", "variance")
    bound = model.elicitation_curve_field_bound(X_test, y_test, questions, 0, strategies, n_iters=8, reset=True, seed=1)
    adam = model.elicitation_curve_field(X_test, y_test, questions, 0, strategies, n_steps=200, lr=0.05, reset=True, seed=1)
    print(f"{len(torch.unique(X_test[:, 0]))} students, {len(X_test)} questions in the pool; AUC bound(8) / Adam(200)")
    print("asked  " + "  ".join(f"{s:>26}" for s in strategies))
    for q in range(questions + 1):
        print(f"{q:5d}  " + "  ".join(f"{bound[s][q]:8.4f} / {adam[s][q]:8.4f} ({bound['n_unasked'][s][q]:5d})"
                                      for s in strategies))


def main_priors(argv):
    bound = bool(argv) and argv[0] == "--bound"
    argv = argv[1:] if bound else argv
    questions = int(argv[0]) if len(argv) > 0 else 15
    sweeps = int(argv[1]) if len(argv) > 1 else 10
    N, M, X_train, X_test, y_train, y_test = load_fraction(os.path.join(ROOT, "tests", "golden", "fraction"))
    X_train, X_test = torch.as_tensor(X_train), torch.as_tensor(X_test)
    y_train, y_test = torch.as_tensor(y_train).float(), torch.as_tensor(y_test).float()
    torch.manual_seed(42)
    model = VFM(N, M, embedding_size=5, output="class" if bound else "reg", device="cuda")
    fit = model.fit_bound if bound else model.fit_exact
    priors = fit(X_train, y_train, n_sweeps=sweeps, learn_priors=True)["priors"]
    strategies = ("random", "variance")
    curve = model.elicitation_curve_field_bound if bound else model.elicitation_curve_field_exact
    learnt = curve(X_test, y_test, questions, 0, strategies, reset=True, seed=1, priors=priors)
    std = curve(X_test, y_test, questions, 0, strategies, reset=True, seed=1)
    print(f"{len(torch.unique(X_test[:, 0]))} students, {len(X_test)} questions in the pool; the students' prior precisions "
          f"{[round(float(v), 2) for v in priors.prec[0]]}")
    print(f"{'AUC' if bound else 'RMSE'} on the unasked, cold start: learnt priors / N(0, 1)")
    print("asked  " + "  ".join(f"{s:>19}" for s in strategies))
    for q in range(questions + 1):
        print(f"{q:5d}  " + "  ".join(f"{learnt[s][q]:8.4f} / {std[s][q]:8.4f}" for s in strategies))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--priors":
        return main_priors(sys.argv[2:])
    if len(sys.argv) > 1 and sys.argv[1] == "--exact":
        return main_exact(sys.argv[2:])
    if len(sys.argv) > 1 and sys.argv[1] == "--implicit":
        return main_implicit(sys.argv[2:])
    if len(sys.argv) > 1 and sys.argv[1] == "--bound":
        return main_bound(sys.argv[2:])
    if len(sys.argv) > 1 and sys.argv[1] in ("--ranking", "--design"):
        return main_ranking(sys.argv[2:], design=sys.argv[1] == "--design")
    questions = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    epochs = int(sys.argv[2]) if len(sys.argv) > 2 else 60
    N, M, X_train, X_test, y_train, y_test = load_fraction(os.path.join(ROOT, "tests", "golden", "fraction"))
    X_train, X_test = torch.as_tensor(X_train), torch.as_tensor(X_test)
    y_train, y_test = torch.as_tensor(y_train), torch.as_tensor(y_test)
    torch.manual_seed(42)
    model = VFM(N, M, embedding_size=5, output="class", device="cuda")
    model.fit(X_train, y_train, n_epochs=epochs, batch_size=100000, verbose=False)
    strategies = ("mean", "random", "variance")
    curve = model.elicitation_curve(X_test, y_test, questions, strategies, n_steps=200, lr=0.05, reset=True, seed=1)
    print(f"{len(torch.unique(X_test[:, 0]))} students, {len(X_test)} questions in the pool")
    print("asked  " + "  ".join(f"{s:>16}" for s in strategies))
    for q in range(questions + 1):
        print(f"{q:5d}  " + "  ".join(f"{curve[s][q]:8.4f} ({curve['n_unasked'][s][q]:5d})" for s in strategies))


if __name__ == "__main__":
    main()

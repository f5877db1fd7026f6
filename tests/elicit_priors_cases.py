"""The planted cases of the sessions under learnt priors (tests/test_elicit_priors_cpu.py, tests/test_gpu_elicit_priors.py)
and the fp64 restatements that exist nowhere else: the design score under a prior.  CPU tensors only.

A case: 4 respondents of field 0 of a (12, 30, 3) model at d = 5, pools of 3 rows and 3 rounds -- every pool row is asked,
in an order the GPU decides --, histories of 0, 2, 7 and 3 rows (the respondent with 3 turns from the dual system to the
primal one in its last round), priors drawn by prior_reference.draw_priors with the precisions in [1, 16].  Because the
order is the GPU's, the CPU test walks every order (3! per respondent) and asserts the condition number of every matrix
a session could factor; the GPU test asserts it again for the order that was taken."""
import itertools

import numpy as np
import torch

import bound_prior_reference as BP
import bound_reference as BR
import prior_reference as PR
import solve_reference as R

COND_EXACT, COND_BOUND = 78.4, 1e3       # the caps tests/test_gpu_fit_priors.py and tests/test_gpu_fit_bound_priors.py assert
SIZES, D, Q, FIELD, KLW = (12, 30, 3), 5, 3, 0, 0.8
_SEEDS = {"exact": 11, "design": 12, "bound": 13}
_LINKS = {"exact": "softplus", "design": "abs", "bound": "softplus"}
N_ITERS = 4


def case(name):
    g = torch.Generator().manual_seed(_SEEDS[name])
    T = sum(SIZES)
    ent = (torch.randn(T, 2 * D, generator=g) * 0.5).float()
    bia = (torch.randn(T, 2, generator=g) * 0.5).float()
    scal = torch.tensor([1.3, 0.2, 0.3])
    resp = torch.randperm(SIZES[0], generator=g)[:4]
    n_ctx = SIZES[1] * SIZES[2]
    pool, hist = [], []
    for e, h in zip(resp.tolist(), (0, 2, 7, 3)):
        pick = torch.randperm(n_ctx, generator=g)[:Q + h]
        rows = torch.stack([torch.full_like(pick, e), SIZES[0] + pick // SIZES[2], SIZES[0] + SIZES[1] + pick % SIZES[2]], 1)
        pool.append(rows[:Q])
        hist.append(rows[Q:])
    pool, hist = torch.cat(pool), torch.cat(hist)
    output = "class" if name == "bound" else "reg"
    ans = (lambda n: torch.randn(n, generator=g) + 1.0) if output == "reg" else (lambda n: (torch.rand(n, generator=g) < 0.5).float())
    mean, prec = PR.draw_priors(len(SIZES), D, _SEEDS[name], 1.0)
    return dict(sizes=SIZES, d=D, Q=Q, field=FIELD, klw=KLW, link=_LINKS[name], output=output, ent=ent, bia=bia, scal=scal,
                pool=pool, y_pool=ans(pool.shape[0]), hist_x=hist, hist_y=ans(hist.shape[0]), mean=mean, prec=prec,
                n_iters=N_ITERS)


def rows_of(c, e, asked):
    """(x, y) of respondent e in fold order: its history in the given order, then the pool rows `asked` (indices into
    the caller's pool, in the order asked)."""
    f = c["field"]
    h = c["hist_x"][:, f] == e
    asked = torch.as_tensor(asked, dtype=torch.int64).reshape(-1)
    return torch.cat([c["hist_x"][h], c["pool"][asked]]), torch.cat([c["hist_y"][h], c["y_pool"][asked]])


def orders(c, e):
    """Every order in which respondent e's pool rows can be asked."""
    idx = torch.nonzero(c["pool"][:, c["field"]] == e).reshape(-1).tolist()
    return list(itertools.permutations(idx))


def prior_start(c):
    """(theta [d + 1], sig2 [d + 1]) a reset bound session starts a respondent at: the fp32 prior row read back in fp64."""
    f = c["field"]
    sg = np.sqrt(1.0 / c["prec"][f].numpy())
    s32 = BR.unlink64(sg, c["link"]).astype(np.float32).astype(np.float64)
    return c["mean"][f].numpy().copy(), R._link64(s32, c["link"]) ** 2


def start_of_row(c, theta_w, theta, s_w, s):
    """(theta, sig2) of an fp32 row [mu_w | mu], [s_w | s] as the next fold reads it."""
    th = np.concatenate([np.asarray(theta_w, np.float64).reshape(1), np.asarray(theta, np.float64)])
    sv = np.concatenate([np.asarray(s_w, np.float64).reshape(1), np.asarray(s, np.float64)])
    return th, R._link64(sv, c["link"]) ** 2


def bound_fold(c, x, y, e, start):
    """One fold of a bound session: n_iters rounds over (x, y) from `start` = (theta, sig2)."""
    f = c["field"]
    return BP.bound_rounds_fp64_prior(c["ent"], c["bia"], c["scal"], x, y, f, c["link"], c["klw"], e, c["n_iters"],
                                      c["mean"][f], c["prec"][f], start=start)


def design_v_prior(kl, prec, S, lam):
    return kl / (kl * lam + prec * S)


def design_scores_prior(S, W, n, Mq, Aq, kl, prec, lam):
    """design_restatement.scores under the prior's precisions lam [d + 1] (0: the weight): numpy fp64,
    (v_w(n) - v_w(n + 1)) + sum_k W_k (v_k(S_k) - v_k(S_k + a_qk)) with v_c(S) = kl / (kl lam_c + prec S)."""
    lam = np.asarray(lam, np.float64)
    a = Aq + Mq * Mq
    bias = design_v_prior(kl, prec, float(n), lam[0]) - design_v_prior(kl, prec, float(n) + 1.0, lam[0])
    drop = design_v_prior(kl, prec, S[None], lam[None, 1:]) - design_v_prior(kl, prec, S[None] + a, lam[None, 1:])
    return bias + (W[None] * drop).sum(1)

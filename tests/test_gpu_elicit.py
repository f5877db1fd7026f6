"""GPU: elicitation sessions (include/vfm_elicit.h) -- bitwise against the composition of select_next_questions and
fold_in it replaces (both objectives, both links, every strategy, d = 5 / 16 / 128, history, reset, an exhausted pool, a
user past the LDS stage), write=False leaves the model alone, independence of the other users and of the pool's order,
the per-round moments against predictive_moments, the fp64 restatement on a planted model, and the curve."""
import math

import numpy as np
import pytest
import torch

import elicit_restatement as R
from golden_util import rel_err
from test_gpu_foldin import _model

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _problem(m, n_users, pool_sizes, hist_sizes, seed):
    """A shuffled pool [P, 2] with the given rows per user (distinct items per user), answers, and a history."""
    g = torch.Generator().manual_seed(seed)
    N, M = m.field_sizes
    users = torch.randperm(N, generator=g)[:n_users]
    pool, hist = [], []
    for i, u in enumerate(users.tolist()):
        it = N + torch.randperm(M, generator=g)
        n, h = pool_sizes[i % len(pool_sizes)], hist_sizes[i % len(hist_sizes)]
        pool.append(torch.stack([torch.full((n,), u), it[:n]], 1))
        hist.append(torch.stack([torch.full((h,), u), it[n:n + h]], 1))
    pool, hist = torch.cat(pool), torch.cat(hist)
    pool = pool[torch.randperm(pool.shape[0], generator=g)]
    hist = hist[torch.randperm(hist.shape[0], generator=g)]
    ans = (lambda n: torch.randn(n, generator=g) + 1.0) if m.output == "reg" else \
        (lambda n: (torch.rand(n, generator=g) < 0.5).float())
    return pool.to(DEV), ans(pool.shape[0]).to(DEV), hist.to(DEV), ans(hist.shape[0]).to(DEV)


def _set_prior(m, users):
    from vae_amd import foldin
    d = m.d
    ent, bia, _ = m._views(m._flat)
    ent[users, :d] = 0.0
    ent[users, d:] = foldin.prior_s(m.link)
    bia[users, 0] = 0.0
    bia[users, 1] = foldin.prior_s(m.link)
    m.params_changed()


def _theta_rows(m, users):
    ent, bia, _ = m._views(m._flat)
    return torch.cat([ent[users], bia[users]], 1).clone()


def _composed(m, pool, y_pool, Q, strategy, hist, n_steps, lr, objective, S, seed, klw, reset):
    """The loop the session replaces, on the public pieces (modifies m): per round select_next_questions with seed + q
    on the rows still unasked, then foldin.run of the answering users on their history followed by everything they were
    asked so far, with t0 = q (n_steps + 1).  Returns rows, score, loss [U, Q], theta [U, Q, 2d + 2]."""
    from vae_amd import foldin, rank
    users = torch.unique(pool[:, 0])
    U, P = users.numel(), pool.shape[0]
    if reset:
        _set_prior(m, users)
    rows = torch.full((U, Q), -1, dtype=torch.int64, device=DEV)
    score = torch.full((U, Q), float("nan"), device=DEV)
    loss = torch.full((U, Q), float("nan"), device=DEV)
    theta = torch.empty(U, Q, 2 * m.d + 2, device=DEV)
    unasked = torch.ones(P, dtype=torch.bool, device=DEV)
    asked = torch.zeros(0, dtype=torch.int64, device=DEV)              # caller indices in the order asked
    hx, hy = hist if hist is not None else (pool[:0], y_pool[:0])
    for q in range(Q):
        idx = torch.nonzero(unasked).reshape(-1)
        if idx.numel():
            sub = pool[idx]
            us, r = m.select_next_questions(sub, 1, strategy, seed + q)
            ent, bia, scal = m._views(m._flat)
            _, _, sc = rank.predictive_moments(sub, ent, bia, scal, m.link, strategy, seed + q)
            upos = torch.searchsorted(users, us)
            rows[upos, q] = idx[r[:, 0]]
            score[upos, q] = sc[r[:, 0]]
            unasked[idx[r[:, 0]]] = False
            asked = torch.cat([asked, idx[r[:, 0]]])
            ha = torch.isin(hx[:, 0], us)
            aa = asked[torch.isin(pool[asked, 0], us)]
            X, y = torch.cat([hx[ha], pool[aa]]), torch.cat([hy[ha], y_pool[aa]])
            ents, ls, _, _ = foldin.run(m, X, y, 0, objective, S, seed, klw, foldin.MODE_FIT, n_steps, lr,
                                        t0=q * (n_steps + 1))
            assert torch.equal(ents, us)
            loss[upos, q] = ls
        theta[:, q] = _theta_rows(m, users)
    return users, rows, score, loss, theta


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


CASES = [  # output, objective, link, strategy, d, history, reset, n_samples
    ("reg", "closed_form", "abs", "variance", 5, True, False, 1),
    ("reg", "closed_form", "softplus", "top", 16, False, True, 1),
    ("reg", "closed_form", "abs", "random", 128, True, False, 1),
    ("reg", "closed_form", "softplus", "variance", 128, True, True, 1),
    ("class", "sampled", "softplus", "mean", 5, True, True, 1),
    ("class", "sampled", "abs", "variance", 16, False, False, 2),
    ("class", "sampled", "abs", "random", 128, True, False, 1),
    ("class", "sampled", "softplus", "top", 128, False, True, 1),
    ("reg", "sampled", "softplus", "variance", 5, False, False, 3),
    ("class", "sampled", "abs", "mean", 16, True, False, 1),
]


@pytest.mark.parametrize("output,objective,link,strategy,d,with_hist,reset,S", CASES)
def test_bitwise_against_the_composition(output, objective, link, strategy, d, with_hist, reset, S):
    Q, n_steps = 6, 9
    m = _model((40, 90), d, output, link, seed=d + len(strategy), rng_seed=3)
    # pools of 3 rows run out before Q; 60 history rows are past the LDS stage at every d (at most 43 rows fit)
    pool, y_pool, hx, hy = _problem(m, 11, [3, 9, 17, 30, 1], [60, 0, 4, 11] if with_hist else [0], seed=d)
    hist = (hx, hy) if with_hist else None
    start = m._flat.clone()
    users, rows, score, loss, theta = _composed(m, pool, y_pool, Q, strategy, hist, n_steps, 0.05, objective, S, 21,
                                                0.8, reset)
    final = m._flat.clone()
    m._flat.copy_(start)
    m.params_changed()
    out = m.elicit(pool, y_pool, Q, strategy, history=hist, n_steps=n_steps, lr=0.05, objective=objective, n_samples=S,
                   seed=21, kl_weight=0.8, reset=reset, write=True, return_theta=True)
    assert torch.equal(out["users"], users)
    assert torch.equal(out["rows"], rows)
    assert int((rows < 0).sum()) > 0 and int((rows[:, 0] >= 0).sum()) == users.numel()
    assert _same_bits(out["score"], score)                   # (NaN where nothing was left to ask, in both)
    assert _same_bits(out["loss"], loss)
    assert torch.equal(out["theta"], theta)
    assert torch.equal(m._flat, final)
    assert not torch.equal(final, start)


def test_lds_stage_size_does_not_matter():
    from vae_amd import elicit
    m = _model((40, 90), 16, "reg", "abs", seed=2)
    pool, y_pool, hx, hy = _problem(m, 7, [12, 5], [7, 0, 50], seed=4)
    kw = dict(history=(hx, hy), n_steps=8, return_theta=True, return_moments=True)
    a = elicit.run(m, pool, y_pool, 5, "variance", **kw)
    for cap in (0, 3):
        b = elicit.run(m, pool, y_pool, 5, "variance", lds_rows=cap, **kw)
        for k in a:
            assert _same_bits(a[k], b[k]) if a[k].dtype == torch.float32 else torch.equal(a[k], b[k]), (cap, k)


@pytest.mark.parametrize("output,objective", [("reg", "closed_form"), ("class", "sampled")])
def test_write_false_leaves_the_model_alone(output, objective):
    m = _model((40, 90), 16, output, "abs", seed=5)
    pool, y_pool, hx, hy = _problem(m, 9, [10, 4, 25], [3, 0], seed=1)
    before = m._flat.clone()
    kw = dict(history=(hx, hy), n_steps=10, objective=objective, return_theta=True, return_moments=True)
    a = m.elicit(pool, y_pool, 5, "variance", **kw)
    assert torch.equal(m._flat, before)
    b = m.elicit(pool, y_pool, 5, "variance", **kw)
    assert torch.equal(m._flat, before)
    for k in a:
        assert _same_bits(a[k], b[k]) if a[k].dtype == torch.float32 else torch.equal(a[k], b[k]), k
    assert bool(torch.isfinite(a["loss"][a["rows"] >= 0]).all())


@pytest.mark.parametrize("output,objective,strategy", [("reg", "closed_form", "variance"), ("class", "sampled", "mean"),
                                                       ("class", "sampled", "random")])
def test_independent_of_the_other_users_and_of_the_pool_order(output, objective, strategy):
    m = _model((40, 90), 16, output, "softplus", seed=6)
    pool, y_pool, hx, hy = _problem(m, 10, [14, 6, 2, 33], [5, 0, 45], seed=8)
    kw = dict(history=(hx, hy), n_steps=7, objective=objective, seed=4, return_theta=True)
    Q = 5
    full = m.elicit(pool, y_pool, Q, strategy, **kw)
    item_of = lambda o, p: torch.where(o["rows"] >= 0, p[o["rows"].clamp(min=0), 1], o["rows"])
    perm = torch.randperm(pool.shape[0], generator=torch.Generator().manual_seed(1)).to(DEV)
    shuf = m.elicit(pool[perm], y_pool[perm], Q, strategy, **kw)
    assert torch.equal(item_of(full, pool), item_of(shuf, pool[perm]))
    for k in ("score", "loss", "theta"):
        assert _same_bits(full[k], shuf[k]), k
    for i, u in enumerate(full["users"].tolist()):
        sel = pool[:, 0] == u
        hs = hx[:, 0] == u
        one = m.elicit(pool[sel], y_pool[sel], Q, strategy, **dict(kw, history=(hx[hs], hy[hs])))
        assert torch.equal(item_of(one, pool[sel]), item_of(full, pool)[i:i + 1])
        for k in ("score", "loss", "theta"):
            assert _same_bits(one[k], full[k][i:i + 1]), (u, k)


@pytest.mark.parametrize("output,objective,link,d", [("reg", "closed_form", "abs", 5), ("class", "sampled", "softplus", 128)])
def test_round_moments_are_predictive_moments_of_that_rounds_posterior(output, objective, link, d):
    m = _model((40, 90), d, output, link, seed=9)
    pool, y_pool, _, _ = _problem(m, 8, [11, 3, 20], [0], seed=2)
    Q = 4
    out = m.elicit(pool, y_pool, Q, "variance", n_steps=10, objective=objective, return_theta=True, return_moments=True)
    users = out["users"]
    ent, bia, _ = m._views(m._flat)
    for q in range(Q + 1):
        if q > 0:
            ent[users] = out["theta"][:, q - 1, :2 * d]
            bia[users] = out["theta"][:, q - 1, 2 * d:]
            m.params_changed()
        mean, var = m.predictive_moments(pool)
        assert _same_bits(out["logit_mean"][q], mean) and _same_bits(out["logit_var"][q], var), q


def test_against_the_fp64_restatement_on_a_planted_model():
    """Selections feed back, so a user is compared for as long as every round so far had a relative gap of at least tau
    between the best and the second-best score in the restatement; tau = 4 x the largest relative difference between
    the kernel's and the restatement's scores of round 0 (no fold yet: pure scoring error).  Generator (chosen on the
    CPU with the restatement alone): 32 cold-start users, 40-row pools, d = 8, 8 rounds of 20 Adam steps at lr = 0.01
    (the learning rate of test_trajectory_matches_fp64_adam, whose tolerance is used), planted item means of unit
    scale.  In the restatement the smallest relative gap of any user and round is 4.7e-4, so every user is compared
    through all rounds for any tau below that (share 100 %; the assertion asks for 80 %).
    Why lr = 0.01: the tolerance bounds fp32 rounding, and Adam's update m / sqrt(v) does not depend on the gradient's
    scale, so where a fit overshoots or converges within a round the absolute rounding noise of a gradient near zero
    becomes a relative one of the step.  A plain numpy fp32 transcription of the restatement (same selections, no
    kernel involved) is 2.5e-2 away from fp64 at lr = 0.05 -- no fp32 code can meet 1e-4 on those inputs -- and 3.7e-6
    away at lr = 0.01.
    Measured on an MI355X at lr = 0.05 (the first version of this test): tau = 7.9e-7, 32 of 32 users compared through
    all rounds with identical sequences, worst theta rel_err 1.6e-2.  At lr = 0.01: the same tau (round 0 does not depend on lr; measured
    7.9e-7 again), 32 of 32 users compared through all rounds, worst theta rel_err 2.8e-6."""
    from vae_amd.model import VFM
    N, M, d, Q, n_steps = 32, 300, 8, 8, 20
    torch.manual_seed(0)
    m = VFM(N, M, d, output="reg", device=DEV)
    g = torch.Generator().manual_seed(2)
    mu = torch.randn(N + M, d, generator=g)
    ent = torch.cat([mu, torch.full((N + M, d), 0.05)], 1)
    bia = torch.stack([torch.randn(N + M, generator=g) * 0.1, torch.full((N + M,), 0.05)], 1)
    m.entity_params.weight.data.copy_(ent)
    m.bias_params.weight.data.copy_(bia)
    m._flat[m._off_scal: m._off_scal + 3] = torch.tensor([4.0, 0.0, 0.05], device=DEV)
    pool = torch.stack([torch.arange(N).repeat_interleave(40),
                        torch.cat([N + torch.randperm(M, generator=g)[:40] for _ in range(N)])], 1)
    truth = (mu[pool[:, 0]] * mu[pool[:, 1]]).sum(1) + bia[pool[:, 0], 0] + bia[pool[:, 1], 0]
    y_pool = truth + 0.5 * torch.randn(pool.shape[0], generator=g)
    out = m.elicit(pool.to(DEV), y_pool.to(DEV), Q, "variance", n_steps=n_steps, lr=0.01, reset=True, return_theta=True,
                   return_moments=True)
    E, B, S = (t.detach().cpu().numpy().astype(np.float64) for t in (*m._views(m._flat)[:2], m._scalars()))
    rows, theta = out["rows"].cpu(), out["theta"].cpu().numpy()
    var0 = out["logit_var"][0].cpu().numpy()
    ref, tau = [], 0.0
    for u in range(N):
        sel = (pool[:, 0] == u).nonzero().reshape(-1)
        s = R.session(u, pool[sel, 1].numpy(), y_pool[sel].numpy(), Q, "variance", E, B, S, n_steps=n_steps, lr=0.01,
                      reset=True)
        ref.append((sel, s))
        tau = max(tau, float(np.max(np.abs(var0[sel.numpy()] - s["score0"]) / np.abs(s["score0"]))))
    tau *= 4.0
    print(f"tau = {tau:.3e}")
    through = 0
    worst = 0.0
    for u, (sel, s) in enumerate(ref):
        n_ok = 0
        while n_ok < Q and s["gap"][n_ok] >= tau:
            n_ok += 1
        through += n_ok == Q
        want = [int(sel[r]) if r >= 0 else -1 for r in s["rows"][:n_ok]]
        assert rows[u, :n_ok].tolist() == want, u
        for q in range(n_ok):
            t = s["theta"][q]
            for a, b in ((theta[u, q, :d], t[0]), (theta[u, q, d:2 * d], t[1]), (theta[u, q, 2 * d:], np.array(t[2:]))):
                worst = max(worst, rel_err(a, b))
    print(f"compared through all rounds: {through} of {N}; worst theta rel_err {worst:.3e}")
    assert through >= 0.8 * N                               # (the condition on the inputs)
    assert worst <= 1e-4                                    # test_trajectory_matches_fp64_adam's tolerance


def test_curve_random_strategy_equals_the_composed_loop():
    from vae_amd import elicit
    m = _model((40, 90), 16, "class", "abs", seed=12)
    pool, y_pool, _, _ = _problem(m, 12, [9, 15, 4], [0], seed=3)
    Q, n_steps = 4, 8
    start = m._flat.clone()
    c = m.elicitation_curve(pool, y_pool, Q, strategies=("random",), n_steps=n_steps, seed=5)
    assert torch.equal(m._flat, start)
    # by hand: the composed loop's model at round q, the metric on the rows still unasked
    users = torch.unique(pool[:, 0])
    for q in range(Q + 1):
        m._flat.copy_(start)
        m.params_changed()
        _, rows, _, _, _ = _composed(m, pool, y_pool, q, "random", None, n_steps, 0.05, "sampled", 1, 5, 1.0, False)
        keep = torch.ones(pool.shape[0], dtype=torch.bool, device=DEV)
        keep[rows[rows >= 0]] = False
        mean, var = m.predictive_moments(pool[keep])
        want = elicit.metric("class", mean, var, y_pool[keep])
        assert c["n_unasked"]["random"][q] == int(keep.sum())
        assert c["random"][q] == want, q
    assert len(c["random"]) == Q + 1 and all(0.0 <= v <= 1.0 for v in c["random"])

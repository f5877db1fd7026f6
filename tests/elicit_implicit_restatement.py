"""Restatement of the implicit field-form elicitation session (include/vfm_elicit_implicit.h: vfm_elicit_implicit_f32): a
helper of test_elicit_implicit_cpu.py / test_gpu_elicit_implicit.py, not a test.  The loop is
elicit_exact_restatement.session (score the pool with elicit_field_restatement.moments, ask the best row, fold) with the
fold of a round exchanged: implicit_reference.implicit_solve_fp64 (under a prior
implicit_prior_reference.implicit_solve_fp64_prior) over the history followed by the rows asked so far -- the optimum of
the respondent's share of J_imp from its dense row set, every partner a row.  Nothing is carried between rounds.

solve_f32 is a plain numpy float32 transcription of the same system (what fp32 rounding alone does to the choices, no
kernel involved); the planted cases are chosen so that the fp64 run alone keeps every round's best score GAP_FLOOR apart
from the runner-up."""
import math

import numpy as np
import torch

import elicit_exact_restatement as ER
import elicit_restatement as R
import implicit_prior_reference as IPR
import implicit_reference as IR

GAP_FLOOR = ER.GAP_FLOOR                 # best against second-best score, relative, in every round
ROUNDS = 6
W0, W1 = 0.125, 1.0                     # (fp32-representable: the C ABI takes the weights as floats)
USERS, ITEMS, RESPONDENTS, POOL = 12, 40, 8, 12


def _t64(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float64))


def _theta_of(sol, kind):
    th, sg = sol["theta"][0], sol["sigma"][0]
    s = IR.inv_link_t(sg, kind)
    return (th[1:].numpy(), s[1:].numpy(), float(th[0]), float(s[0])), float(sol["cond"][0])


def make_solve64(N, M, w0, w1, prior=None):
    """solve(e, X, y, ent, bia, scal, field, kind, klw) for ER.session: theta = (mu [d], s [d], mu_w, s_w) of respondent
    e at the optimum of its share of J_imp with the rows (X [n, 2], y [n]) observed, and cond(H).  prior: None or
    (m [d + 1], lam [d + 1]) of the respondents' field."""
    def solve(e, X, y, ent, bia, scal, field, kind, klw):
        a = (_t64(ent), _t64(bia), _t64(scal), torch.as_tensor(np.asarray(X, dtype=np.int64)).reshape(-1, 2), _t64(y),
             field, N, M, kind, w0, w1, klw)
        if prior is None:
            sol = IR.implicit_solve_fp64(*a, entities=[int(e)])
        else:
            sol = IPR.implicit_solve_fp64_prior(*a, prior[0], prior[1], entities=[int(e)])
        return _theta_of(sol, kind)
    return solve


def make_solve32(N, M, w0, w1, prior=None):
    """make_solve64's system in float32: operands, sums, system and solve all fp32."""
    f = np.float32

    def solve(e, X, y, ent, bia, scal, field, kind, klw):
        X = np.asarray(X, dtype=np.int64).reshape(-1, 2)
        d = ent.shape[1] // 2
        ids = np.arange(N, N + M) if field == 0 else np.arange(0, N)
        n = ids.size
        w, t = np.full(n, f(w0)), np.zeros(n, dtype=f)
        j = X[:, 1 - field] - ids[0]
        w[j], t[j] = f(w1), np.asarray(y, dtype=f)
        U = np.concatenate([np.ones((n, 1), dtype=f), ent[ids, :d].astype(f)], 1)
        A = np.concatenate([np.zeros((n, 1), dtype=f), R.link(ent[ids, d:], kind, f).astype(f) ** 2], 1)
        cm = (f(scal[1]) + bia[ids, 0].astype(f)).astype(f)
        prec, kl = f(R.link(scal[0], kind, f)), f(klw)
        m = np.zeros(d + 1, dtype=f) if prior is None else np.asarray(prior[0], dtype=f)
        lam = np.ones(d + 1, dtype=f) if prior is None else np.asarray(prior[1], dtype=f)
        H = (np.diag(kl * lam) + prec * ((U * w[:, None]).T @ U + np.diag((w[:, None] * A).sum(0, dtype=f)))).astype(f)
        b = (prec * (U.T @ (w * (t - cm))) + kl * lam * m).astype(f)
        th = np.linalg.solve(H, b).astype(f)
        sg = np.sqrt(kl / (kl * lam + prec * (w[:, None] * (A + U * U)).sum(0, dtype=f))).astype(f)
        s = sg if kind == "abs" else np.log(np.expm1(sg))
        return (th[1:], s[1:].astype(f), float(th[0]), float(s[0])), float(np.linalg.cond(H.astype(np.float64)))
    return solve


# name: link, strategy, field, history rows per respondent, d, prior?, generator seed (chosen on the CPU so that the fp64
# restatement alone keeps every round's gap above GAP_FLOOR: tests/test_elicit_implicit_cpu.py asserts it)
PLANTED = {
    "d5_abs": ("abs", "variance", 0, 0, 5, False, 1),
    "d16_softplus_history": ("softplus", "top", 0, 3, 16, False, 0),
    "d5_softplus_prior": ("softplus", "variance", 0, 0, 5, True, 2),
    "d16_abs_items": ("abs", "top", 1, 2, 16, False, 1),
}


def planted_case(name, seed=None):
    """The inputs of one planted case (numpy only, shared by the CPU conditioning test and the GPU test): USERS users,
    ITEMS items, the first RESPONDENTS ids of the respondents' field with POOL-row pools of distinct partners, planted
    partner means of norm about 1 (N(0, 1 / d) coordinates), respondent rows as a trained model would hold them, click
    targets 1 with noise.  Returns dict(ent, bia, scal fp32 tables, pool [P, 2], y_pool [P], hist_x [H, 2], hist_y [H],
    N, M, prior = None or (m, lam) fp32 [d + 1] of the respondents' field)."""
    kind, strategy, field, n_hist, d, with_prior, s0 = PLANTED[name]
    g = np.random.default_rng(1000 * sorted(PLANTED).index(name) + (s0 if seed is None else seed))
    N, M = USERS, ITEMS
    s_of = (lambda sig: sig) if kind == "abs" else (lambda sig: np.log(np.expm1(sig)))
    mu = g.normal(size=(N + M, d)) / math.sqrt(d)
    sig = g.uniform(0.1, 0.5, size=(N + M, d))
    ent = np.concatenate([mu, s_of(sig)], 1).astype(np.float32)
    bia = np.stack([g.normal(size=N + M) * 0.1, s_of(g.uniform(0.1, 0.4, size=N + M))], 1).astype(np.float32)
    scal = np.array([4.0 if kind == "abs" else math.log(math.expm1(4.0)), 0.1, s_of(0.2)], dtype=np.float32)
    lo, n_part = ((N, M) if field == 0 else (0, N))
    resp = np.arange(RESPONDENTS) + (0 if field == 0 else N)
    n_pool = min(POOL, n_part - n_hist)
    pool, hist = [], []
    for e in resp:
        partners = lo + g.permutation(n_part)[:n_pool + n_hist]
        for k, j in enumerate(partners):
            row = [int(e), int(j)] if field == 0 else [int(j), int(e)]
            (hist if k < n_hist else pool).append(row)
    pool = np.array(pool, dtype=np.int64).reshape(-1, 2)
    hist = np.array(hist, dtype=np.int64).reshape(-1, 2)
    order = g.permutation(pool.shape[0])                   # (the caller's pool order mixes the respondents)
    pool = pool[order]
    y_pool = (1.0 + 0.3 * g.normal(size=pool.shape[0])).astype(np.float32)
    hist_y = (1.0 + 0.3 * g.normal(size=hist.shape[0])).astype(np.float32)
    prior = None
    if with_prior:
        prior = ((0.2 * g.normal(size=d + 1)).astype(np.float32), g.uniform(0.5, 2.0, size=d + 1).astype(np.float32))
    return dict(ent=ent, bia=bia, scal=scal, pool=pool, y_pool=y_pool, hist_x=hist, hist_y=hist_y, N=N, M=M, prior=prior,
                kind=kind, strategy=strategy, field=field, d=d)


def planted_sessions(name, case, f32=False, klw=1.0):
    """The session of every respondent of the case, in ascending respondent order; each dict carries "sel" (the
    respondent's rows of case["pool"]), "entity" and "hist".  f32: the float32 transcription (moments and solve)."""
    kind, strategy, field = case["kind"], case["strategy"], case["field"]
    prior = case["prior"]
    if f32:
        E, B, S = case["ent"], case["bia"], case["scal"]
        kw = dict(moments=ER.moments_f32, solve=make_solve32(case["N"], case["M"], W0, W1, prior))
    else:
        E, B, S = (case[k].astype(np.float64) for k in ("ent", "bia", "scal"))
        p64 = None if prior is None else tuple(np.asarray(v, dtype=np.float64) for v in prior)
        kw = dict(solve=make_solve64(case["N"], case["M"], W0, W1, p64))
    out = []
    for e in np.unique(case["pool"][:, field]):
        sel = np.nonzero(case["pool"][:, field] == e)[0]
        hs = np.nonzero(case["hist_x"][:, field] == e)[0] if case["hist_x"].shape[0] else np.zeros(0, dtype=np.int64)
        s = ER.session(int(e), case["pool"][sel], case["y_pool"][sel], ROUNDS, strategy, E, B, S, field=field, kind=kind,
                       hist_x=case["hist_x"][hs], hist_y=case["hist_y"][hs], klw=klw, reset=False, **kw)
        s["sel"], s["entity"], s["hist"] = sel, int(e), hs
        out.append(s)
    return out


def block_gradient(case, s, q, klw=1.0):
    """max |d J_imp / d (the respondent's means and scale parameters)| of the dense brute-force objective at the
    restatement's theta after round q, the respondent's rows being the history and the rows asked up to round q."""
    N, M, kind, field = case["N"], case["M"], case["kind"], case["field"]
    e, d = s["entity"], case["d"]
    mu, sp, mw, sw = s["theta"][q]
    ent, bia, scal = _t64(case["ent"]).clone(), _t64(case["bia"]).clone(), _t64(case["scal"])
    ent[e, :d], ent[e, d:] = _t64(mu), _t64(sp)
    bia[e, 0], bia[e, 1] = float(mw), float(sw)
    ent.requires_grad_(True)
    bia.requires_grad_(True)
    x = torch.as_tensor(s["fold_x"][q])
    y = _t64(s["fold_y"][q])
    if case["prior"] is None:
        J = IR.brute_J(ent, bia, scal, x, y, N, M, kind, W0, W1, klw)
    else:
        mean, prec = torch.zeros(2, d + 1, dtype=torch.float64), torch.ones(2, d + 1, dtype=torch.float64)
        mean[field], prec[field] = _t64(case["prior"][0]), _t64(case["prior"][1])
        J = IPR.brute_J_prior(ent, bia, scal, x, y, N, M, kind, W0, W1, klw, mean, prec)
    J.backward()
    return max(float(ent.grad[e].abs().max()), float(bia.grad[e].abs().max()))

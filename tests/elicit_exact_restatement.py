"""Restatement of the exact field-form elicitation session (include/vfm_elicit.h: vfm_elicit_solve_f32): a helper of
test_elicit_exact_cpu.py / test_gpu_elicit_exact.py, not a test.  Built from two functions that exist already:
elicit_field_restatement.moments (the field-form moments of vfm_rank.h, fp64 numpy) scores the pool, and
test_foldin_exact_cpu.solve_fp64 (the closed-form optimum of L_e, fp64 torch) folds the answers in.  Every round solves
from the rows themselves: the history in its order, then the asked rows in the order asked.  Nothing is carried.

`session` takes the two functions as arguments, so that the same loop runs in another precision: moments_f32 / solve_f32
are plain numpy float32 transcriptions of the same formulas (what fp32 rounding alone does to the choices, no kernel
involved).
"""
import math

import numpy as np
import torch

import elicit_field_restatement as RF
import elicit_restatement as R
from test_foldin_exact_cpu import solve_fp64


def solve64(e, X, y, ent, bia, scal, field, kind, klw):
    """theta = (mu [d], s [d], mu_w, s_w) of entity e at the optimum of L_e on the rows (X [n, F], y [n]), and cond(H)."""
    X = torch.as_tensor(np.asarray(X, dtype=np.int64))
    sol = solve_fp64(torch.as_tensor(np.asarray(ent, dtype=np.float64)), torch.as_tensor(np.asarray(bia, dtype=np.float64)),
                     torch.as_tensor(np.asarray(scal, dtype=np.float64)), X, torch.as_tensor(np.asarray(y, dtype=np.float64)),
                     field, kind, klw)
    assert sol["entities"].tolist() == [int(e)]
    return (sol["mu"][0].numpy(), sol["s"][0].numpy(), float(sol["mu_w"][0]), float(sol["s_w"][0])), float(sol["cond"][0])


def _operands32(X, field, ent, bia, scal, kind):
    """RF.context_operands in float32: every product and sum rounded to fp32."""
    f = np.float32
    X = np.asarray(X, dtype=np.int64)
    d = ent.shape[1] // 2
    cols = [c for c in range(X.shape[1]) if c != field]
    m = np.stack([ent[X[:, c], :d].astype(f) for c in cols], 1)
    s2 = np.stack([R.link(ent[X[:, c], d:], kind, f) ** 2 for c in cols], 1).astype(f)
    M, A = m.sum(1, dtype=f), s2.sum(1, dtype=f)
    C = (f(2.0) * (s2 * (M[:, None, :] - m)).sum(1, dtype=f)).astype(f)
    EP = f(0.5) * (M * M - (m * m).sum(1, dtype=f))
    VP = (s2 * (M[:, None, :] - m) ** 2).sum(1, dtype=f)
    for a in range(len(cols)):
        for b in range(a + 1, len(cols)):
            VP = VP + s2[:, a] * s2[:, b]
    bw = sum(bia[X[:, c], 0].astype(f) for c in cols)
    sw2 = sum(R.link(bia[X[:, c], 1], kind, f) ** 2 for c in cols)
    c_mean = (f(scal[1]) + bw + EP.sum(1, dtype=f)).astype(f)
    c_var = (f(R.link(scal[2], kind, f)) ** 2 + sw2 + VP.sum(1, dtype=f)).astype(f)
    return M, A, C, c_mean, c_var


def moments_f32(theta, ent, bia, scal, X, field, kind):
    """RF.moments in float32."""
    f = np.float32
    mu, s, mw, sw = theta
    mu = np.asarray(mu, dtype=f)
    sg, sgw = R.link(s, kind, f).astype(f), f(R.link(sw, kind, f))
    M, A, C, c_mean, c_var = _operands32(X, field, ent, bia, scal, kind)
    mean = c_mean + f(mw) + M @ mu
    var = c_var + sgw * sgw + A @ (mu * mu) + (A + M * M) @ (sg * sg) + C @ mu
    return mean.astype(f), var.astype(f)


def solve_f32(e, X, y, ent, bia, scal, field, kind, klw):
    """solve64's primal form in float32 (operands, system and solve all fp32)."""
    f = np.float32
    X = np.asarray(X, dtype=np.int64)
    y = np.asarray(y, dtype=f)
    n = X.shape[0]
    M, A, C, c_mean, _ = _operands32(X, field, ent, bia, scal, kind)
    prec, kl = f(R.link(scal[0], kind, f)), f(klw)
    U = np.concatenate([np.ones((n, 1), dtype=f), M], 1)
    t = y - c_mean
    D = kl + prec * np.concatenate([np.zeros(1, dtype=f), A.sum(0, dtype=f)])
    b = prec * (U.T @ t - np.concatenate([np.zeros(1, dtype=f), f(0.5) * C.sum(0, dtype=f)]))
    H = (np.diag(D) + prec * (U.T @ U)).astype(f)
    th = np.linalg.solve(H, b.astype(f)).astype(f)
    sg_w = np.sqrt(kl / (kl + prec * f(n)))
    sg = np.sqrt(kl / (kl + prec * (A + M * M).sum(0, dtype=f)))
    inv = (lambda v: v) if kind == "abs" else (lambda v: np.log(np.expm1(v)))
    return (th[1:], inv(sg).astype(f), float(th[0]), float(inv(sg_w))), float(np.linalg.cond(H.astype(np.float64)))


def session(e, pool_x, pool_y, n_rounds, strategy, ent, bia, scal, field=0, key_col=None, kind="abs", hist_x=None,
            hist_y=(), klw=1.0, reset=False, uniform=None, moments=RF.moments, solve=solve64):
    """All rounds of respondent e over its pool rows pool_x [P, F].  Returns dict(rows [Q] pool positions or -1,
    score [Q], gap [Q] (relative gap of the chosen score to the runner-up), theta [Q] tuples (the posterior after each
    round), cond [Q] = cond(H) of each solve (NaN where nothing was asked), fold_x / fold_y: per round the rows solved
    on (None where nothing was asked), mean / var [Q + 1, P] as scored before each round)."""
    pool_x = np.asarray(pool_x, dtype=np.int64)
    F, d, P = pool_x.shape[1], ent.shape[1] // 2, pool_x.shape[0]
    if key_col is None:
        key_col = [c for c in range(F) if c != field][0]
    theta = R.prior_theta(d, kind) if reset else R.table_theta(ent, bia, e)
    asked = np.zeros(P, dtype=bool)
    f_x = [] if hist_x is None else [np.asarray(r, dtype=np.int64) for r in hist_x]
    f_y = [float(v) for v in hist_y]
    out = dict(rows=[], score=[], gap=[], theta=[], cond=[], fold_x=[], fold_y=[], mean=[], var=[])
    for q in range(n_rounds + 1):
        mean, var = moments(theta, ent, bia, scal, pool_x, field, kind) if P else (np.zeros(0), np.zeros(0))
        out["mean"].append(mean)
        out["var"].append(var)
        if q == n_rounds:
            break
        sc = R.score(strategy, mean, var, q, pool_x[:, key_col], uniform)
        best, gap = R.choose(sc, asked)
        out["rows"].append(best)
        out["gap"].append(gap)
        if best < 0:
            out["score"].append(math.nan)
            out["cond"].append(math.nan)
            out["fold_x"].append(None)
            out["fold_y"].append(None)
            out["theta"].append(theta)
            continue
        out["score"].append(float(sc[best]))
        asked[best] = True
        f_x.append(pool_x[best])
        f_y.append(float(pool_y[best]))
        theta, cond = solve(e, np.array(f_x), f_y, ent, bia, scal, field, kind, klw)
        out["cond"].append(cond)
        out["fold_x"].append(np.array(f_x))
        out["fold_y"].append(np.array(f_y))
        out["theta"].append(theta)
    return out


def brute_force(e, pool_x, pool_y, n_rounds, strategy, ent, bia, scal, field, kind, hist_x, hist_y, klw, reset):
    """The asked sequence by the two functions alone, nothing else of `session`: per round an argmax over the unasked
    rows' scores (numpy's argmax takes the first of equal values: the lower position), then solve_fp64 on all rows."""
    pool_x = np.asarray(pool_x, dtype=np.int64)
    d = ent.shape[1] // 2
    theta = R.prior_theta(d, kind) if reset else R.table_theta(ent, bia, e)
    left = list(range(pool_x.shape[0]))
    X = [np.asarray(r, dtype=np.int64) for r in hist_x]
    y = [float(v) for v in hist_y]
    rows = []
    for q in range(n_rounds):
        if not left:
            rows.append(-1)
            continue
        mean, var = RF.moments(theta, ent, bia, scal, pool_x[left], field, kind)
        p = left.pop(int(np.argmax({"top": mean, "variance": var}[strategy])))
        rows.append(p)
        X.append(pool_x[p])
        y.append(float(pool_y[p]))
        theta, _ = solve64(e, np.array(X), y, ent, bia, scal, field, kind, klw)
    return rows


# ---------------------------------------------------------------------------------------------------------------------
# the planted models of test_gpu_elicit_exact.py: the closed-form ('reg') generators of elicit_field_restatement
# ---------------------------------------------------------------------------------------------------------------------
PLANTED = ("closed_form_d5", "closed_form_d128")
PLANTED_ROUNDS = 6                       # d = 5 without history: n crosses d in round 5 (dual, then primal)
GAP_FLOOR = 1e-3                         # best against second-best score, relative, in every round


def planted_sessions(name, case, **kw):
    """The session of every respondent of RF.planted_case(name), in ascending respondent order; each dict carries "sel"
    (the respondent's rows of case["pool"]) and "entity".  kw: moments / solve for another precision."""
    _, _, kind, strategy, reset, _, _, field, _ = RF.PLANTED[name]
    cast = (lambda a: a.astype(np.float64)) if "solve" not in kw else (lambda a: a)
    E, B, S = (cast(case[k]) for k in ("ent", "bia", "scal"))
    out = []
    for e in np.unique(case["pool"][:, field]):
        sel = np.nonzero(case["pool"][:, field] == e)[0]
        hs = np.nonzero(case["hist_x"][:, field] == e)[0]
        s = session(int(e), case["pool"][sel], case["y_pool"][sel], PLANTED_ROUNDS, strategy, E, B, S, field=field,
                    kind=kind, hist_x=case["hist_x"][hs], hist_y=case["hist_y"][hs], reset=reset, **kw)
        s["sel"], s["entity"], s["hist"] = sel, int(e), hs
        out.append(s)
    return out

"""Restatement of the bound field-form elicitation session (include/vfm_bound.h: vfm_elicit_bound_f32): a helper of
test_elicit_bound_cpu.py / test_gpu_elicit_bound.py, not a test.  Built from functions that exist already:
elicit_field_restatement.moments (the field-form moments of vfm_rank.h, fp64 numpy) scores the pool, and
bound_reference.bound_rounds_fp64(start=...) (the rounds of the bound's two block minimisers, fp64 numpy) folds the
answers in, started at the posterior the round was scored from.  As in the kernel the posterior between two rounds is
what a table row would hold: the fold's fp64 result rounded to fp32 once.

  fold64        one fold: n_iters rounds from a given fp32 posterior on given rows
  session       all rounds of one respondent (optionally along a given sequence of rows: the GPU test replays the
                kernel's own choices, so a near-tie in the argmax cannot fail it)
  composition   the loop the session replaces, restated separately: an argmax over the rows still unasked, then
                bound_rounds_fp64(reset=False) on a table whose row holds the current posterior
  CASES, case   the inputs of the GPU fp64 test: CPU tensors only

No GPU is needed to import this module or to build a case."""
import math

import numpy as np
import torch

import bound_reference as BR
import elicit_field_restatement as RF
import elicit_restatement as R
import solve_reference as SR


def _f32(v):
    return np.asarray(v, np.float32).astype(np.float64)


def prior_theta32(d, kind):
    """The prior row as fp32 holds it: mu = 0, s = link^-1(1) rounded to fp32."""
    mu, s, mw, sw = R.prior_theta(d, kind)
    return mu, _f32(s), mw, float(_f32(sw))


def fold64(theta, e, X, y, ent, bia, scal, field, kind, klw, n_iters):
    """n_iters rounds of the bound for entity e on the rows (X [n, F], y [n]; column `field` of X holds e) from the
    posterior theta = (mu [d], s [d], mu_w, s_w).  Returns (the posterior after the rounds, rounded to fp32 once, as
    float64 arrays; bound_rounds_fp64's dict, unrounded)."""
    mu, s, mw, sw = theta
    th0 = np.concatenate([[mw], mu]).astype(np.float64)
    sg = SR._link64(np.concatenate([[sw], s]), kind)
    r = BR.bound_rounds_fp64(ent, bia, scal, np.asarray(X, np.int64), np.asarray(y, np.float32), field, kind, klw, int(e),
                             n_iters, start=(th0, sg * sg))
    t, st = _f32(r["theta"][-1]), _f32(r["s"][-1])
    return (t[1:], st[1:], float(t[0]), float(st[0])), r


def session(e, pool_x, pool_y, n_rounds, strategy, ent, bia, scal, field=0, key_col=None, kind="abs", hist_x=None,
            hist_y=(), klw=1.0, n_iters=8, reset=False, uniform=None, along=None, start=None):
    """All rounds of respondent e over its pool rows pool_x [P, F].  along: None, or [Q] pool positions (-1: nothing
    asked) to ask instead of the argmax; start: None, or per round the posterior the round's fold starts from (the
    kernel's returned fp32 theta of the round before; round 0: the table row or the prior) instead of this loop's own.
    Returns dict(rows [Q], score [Q], gap [Q], theta [Q] tuples (fp32 values), unrounded [Q] (theta [d + 1], s [d + 1])
    of each fold before the rounding or None, cond [Q] = the largest cond of the matrices the fold factored, B [Q] arrays
    [1 + n_iters] = B_e at the start and after each inner round, n [Q] fold rows, fold_x / fold_y per round, mean / var
    [Q + 1, P] as scored before each round)."""
    pool_x = np.asarray(pool_x, dtype=np.int64)
    F, d, P = pool_x.shape[1], ent.shape[1] // 2, pool_x.shape[0]
    if key_col is None:
        key_col = [c for c in range(F) if c != field][0]
    e64, b64 = np.asarray(ent, np.float64), np.asarray(bia, np.float64)
    theta = prior_theta32(d, kind) if reset else R.table_theta(e64, b64, e)
    asked = np.zeros(P, dtype=bool)
    f_x = [] if hist_x is None else [np.asarray(r, dtype=np.int64) for r in hist_x]
    f_y = [float(v) for v in hist_y]
    keys = ("rows", "score", "gap", "theta", "unrounded", "cond", "B", "n", "fold_x", "fold_y", "mean", "var")
    out = {k: [] for k in keys}
    for q in range(n_rounds + 1):
        mean, var = RF.moments(theta, e64, b64, scal, pool_x, field, kind) if P else (np.zeros(0), np.zeros(0))
        out["mean"].append(mean)
        out["var"].append(var)
        if q == n_rounds:
            break
        sc = R.score(strategy, mean, var, q, pool_x[:, key_col], uniform)
        best, gap = R.choose(sc, asked)
        if along is not None:
            best = int(along[q])
        out["rows"].append(best)
        out["gap"].append(gap)
        if best < 0:
            for k, v in (("score", math.nan), ("cond", math.nan), ("B", None), ("n", 0), ("fold_x", None), ("fold_y", None),
                         ("unrounded", None), ("theta", theta)):
                out[k].append(v)
            continue
        out["score"].append(float(sc[best]))
        asked[best] = True
        f_x.append(pool_x[best])
        f_y.append(float(pool_y[best]))
        theta, r = fold64(theta if start is None else start[q], e, np.array(f_x), f_y, ent, bia, scal, field, kind, klw,
                          n_iters)
        out["cond"].append(float(r["cond"].max()))
        out["B"].append(np.concatenate([[r["B_start"]], r["B"]]))
        out["n"].append(len(f_y))
        out["fold_x"].append(np.array(f_x))
        out["fold_y"].append(np.array(f_y))
        out["unrounded"].append((r["theta"][-1], r["s"][-1]))
        out["theta"].append(theta)
    return out


def composition(e, pool_x, pool_y, n_rounds, strategy, ent, bia, scal, field, kind, hist_x, hist_y, klw, n_iters, reset):
    """The composed loop by the pieces alone, nothing else of `session`: per round an argmax over the unasked rows'
    scores at the table row (numpy's argmax takes the first of equal values: the lower position), then
    bound_rounds_fp64(reset=False) on all rows from that table row, whose result is written back in fp32.  With reset
    the prior row is written first.  Returns (rows [Q], thetas [Q] tuples)."""
    pool_x = np.asarray(pool_x, dtype=np.int64)
    ent, bia = np.array(ent, np.float32), np.array(bia, np.float32)
    d = ent.shape[1] // 2
    if reset:
        mu, s, mw, sw = prior_theta32(d, kind)
        ent[e, :d], ent[e, d:], bia[e, 0], bia[e, 1] = mu, s, mw, sw
    left = list(range(pool_x.shape[0]))
    X = [np.asarray(r, dtype=np.int64) for r in hist_x]
    y = [float(v) for v in hist_y]
    rows, thetas = [], []
    for q in range(n_rounds):
        theta = R.table_theta(ent, bia, e)
        if not left:
            rows.append(-1)
            thetas.append(theta)
            continue
        mean, var = RF.moments(theta, ent.astype(np.float64), bia.astype(np.float64), scal, pool_x[left], field, kind)
        p = left.pop(int(np.argmax(R.score(strategy, mean, var))))
        rows.append(p)
        X.append(pool_x[p])
        y.append(float(pool_y[p]))
        r = BR.bound_rounds_fp64(ent, bia, scal, np.array(X), np.array(y, np.float32), field, kind, klw, int(e), n_iters)
        ent[e, :d], ent[e, d:], bia[e, 0], bia[e, 1] = r["theta"][-1][1:], r["s"][-1][1:], r["theta"][-1][0], r["s"][-1][0]
        thetas.append(R.table_theta(ent, bia, e))
    return rows, thetas


# ---------------------------------------------------------------------------------------------------------------------
# the inputs of the GPU fp64 test: solve_reference's tables (scale 0.5, the cases of the bound fold-in's own tests),
# 6 respondents with 8-row pools of distinct contexts, labels in {0, 1}, 6 rounds
# ---------------------------------------------------------------------------------------------------------------------
CASES = {  # name: field sizes, field, d, link, strategy, reset, history rows per respondent, n_iters, kl_weight, seed
    "d5": ((12, 40, 4), 0, 5, "abs", "variance", True, 0, 8, 1.0, 11),          # n crosses d in round 5: dual, then primal
    "d33": ((12, 40), 0, 33, "softplus", "mean", False, 3, 3, 0.7, 12),
    "d128": ((12, 40, 4), 1, 128, "softplus", "top", False, 3, 1, 1.0, 13),
}
CASE_RESPONDENTS, CASE_POOL, CASE_ROUNDS = 6, 8, 6


def case(name):
    """dict(sizes, field, d, link, strategy, reset, n_iters, kl_weight, ent, bia, scal (fp32 torch), pool [P, F], y_pool
    [P], hist_x [H, F], hist_y [H] (torch, CPU))."""
    sizes, field, d, link, strategy, reset, n_hist, n_iters, klw, seed = CASES[name]
    ent, bia, scal = SR.tables(sizes, d, seed)
    g = np.random.default_rng(seed)
    F = len(sizes)
    lo = [sum(sizes[:f]) for f in range(F)]
    cols = [f for f in range(F) if f != field]
    n_ctx = int(np.prod([sizes[f] for f in cols]))
    pool, hist = [], []
    for r in range(CASE_RESPONDENTS):
        pick = g.permutation(n_ctx)[:CASE_POOL + n_hist]                    # distinct contexts
        rows = np.zeros((len(pick), F), dtype=np.int64)
        rows[:, field] = lo[field] + r
        for f in reversed(cols):
            rows[:, f] = lo[f] + pick % sizes[f]
            pick = pick // sizes[f]
        pool.append(rows[:CASE_POOL])
        hist.append(rows[CASE_POOL:])
    pool, hist = np.concatenate(pool), np.concatenate(hist)
    lab = lambda n: torch.from_numpy((g.random(n) < 0.4).astype(np.float32))
    return dict(sizes=sizes, field=field, d=d, link=link, strategy=strategy, reset=reset, n_iters=n_iters, kl_weight=klw,
                ent=ent, bia=bia, scal=scal, pool=torch.from_numpy(pool), y_pool=lab(len(pool)),
                hist_x=torch.from_numpy(hist), hist_y=lab(len(hist)))


def case_sessions(c, along=None, start=None):
    """The session of every respondent of a case, in ascending respondent order; each dict carries "sel" (the
    respondent's rows of c["pool"]) and "entity".  along [U, Q]: positions in c["pool"] to ask (-1: nothing); start
    [U][Q]: the posterior each round's fold starts from."""
    ent, bia, scal = (c[k].numpy() for k in ("ent", "bia", "scal"))
    pool, yp, hx, hy = (c[k].numpy() for k in ("pool", "y_pool", "hist_x", "hist_y"))
    f = c["field"]
    out = []
    for u, e in enumerate(np.unique(pool[:, f])):
        sel = np.nonzero(pool[:, f] == e)[0]
        hs = np.nonzero(hx[:, f] == e)[0]
        al = None
        if along is not None:
            back = {int(p): i for i, p in enumerate(sel)}
            al = [back[int(p)] if p >= 0 else -1 for p in along[u]]
        s = session(int(e), pool[sel], yp[sel], CASE_ROUNDS, c["strategy"], ent, bia, scal, field=f, kind=c["link"],
                    hist_x=hx[hs], hist_y=hy[hs], klw=c["kl_weight"], n_iters=c["n_iters"], reset=c["reset"], along=al,
                    start=None if start is None else start[u])
        s["sel"], s["entity"], s["hist"] = sel, int(e), hs
        out.append(s)
    return out

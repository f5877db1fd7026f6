"""fp64 numpy restatement of the elicitation session in the field form (include/vfm_elicit.h: vfm_elicit_field_f32): a
helper of test_elicit_field_cpu.py / test_gpu_elicit_field.py, not a test.  Written from the formulas of vfm_rank.h (the
field form: context operands M, A, C, c_mean, c_var and the two moments) and vfm_foldin.h (the objective L_e, closed form
and sampled, and Adam), not from the kernel: every round recomputes the fold from the rows, nothing is carried.

A respondent e is an entity of column `field`; a row is a full row [F]; the other columns are its frozen context.  Tables
and theta as in elicit_restatement.py, whose link, Adam, KL, score and choose are used.  The sampled objective takes
eps(t) -> (eps_entity [T, d], eps_bias [T], eps_global) for draw key t (one draw per iteration); strategy "random" takes
uniform(q, key) -> float with key = row[key_col].
"""
import math

import numpy as np

import elicit_restatement as R


def context_operands(X, field, ent, bia, scal, kind):
    """Per row of X [n, F]: M, A, C [n, d] and c_mean, c_var [n] of its context (the columns but `field`)."""
    X = np.asarray(X, dtype=np.int64)
    d = ent.shape[1] // 2
    cols = [f for f in range(X.shape[1]) if f != field]
    m = np.stack([ent[X[:, f], :d].astype(np.float64) for f in cols], 1)              # [n, nq, d]
    s2 = np.stack([R.link(ent[X[:, f], d:], kind) ** 2 for f in cols], 1)
    M, A = m.sum(1), s2.sum(1)
    C = 2.0 * (s2 * (M[:, None, :] - m)).sum(1)
    EP = 0.5 * (M * M - (m * m).sum(1))
    VP = (s2 * (M[:, None, :] - m) ** 2).sum(1)
    for a in range(len(cols)):
        for b in range(a + 1, len(cols)):
            VP = VP + s2[:, a] * s2[:, b]
    bw = sum(bia[X[:, f], 0].astype(np.float64) for f in cols)
    sw2 = sum(R.link(bia[X[:, f], 1], kind) ** 2 for f in cols)
    c_mean = float(scal[1]) + bw + EP.sum(1)
    c_var = float(R.link(scal[2], kind)) ** 2 + sw2 + VP.sum(1)
    return M, A, C, c_mean, c_var


def moments(theta, ent, bia, scal, X, field, kind):
    """(mean [n], var [n]) of the rows X with column `field` held by an entity with `theta`."""
    mu, s, mw, sw = theta
    sg, sgw = R.link(s, kind), float(R.link(sw, kind))
    M, A, C, c_mean, c_var = context_operands(X, field, ent, bia, scal, kind)
    mean = c_mean + mw + M @ mu
    var = c_var + sgw ** 2 + A @ (mu * mu) + (A + M * M) @ (sg * sg) + C @ mu
    return mean, var


def fold(theta, e, X, y, ent, bia, scal, field, kind, output, objective, n_steps, lr, klw=1.0, eps=None, t0=0):
    """n_steps Adam updates (fresh moments) of entity e's theta on the rows (X [n, F], y [n]), e in column `field`.
    Returns (theta, L_e at the final parameters)."""
    X = np.asarray(X, dtype=np.int64)
    y = np.asarray(y, dtype=np.float64)
    d = theta[0].shape[0]
    n = X.shape[0]
    cols = [f for f in range(X.shape[1]) if f != field]
    prec = float(R.link(scal[0], kind))
    m0, sg0 = float(scal[1]), float(R.link(scal[2], kind))
    M, A, C, c_mean, c_var = context_operands(X, field, ent, bia, scal, kind)
    const = n * (R.LOG_2PI_HALF - 0.5 * math.log(prec)) if output == "reg" else 0.0

    def grad_fn(th, it):
        mu, s, mw, sw = th
        sg, sgw = R.link(s, kind), float(R.link(sw, kind))
        if objective == "closed_form":
            Ep = c_mean + mw + M @ mu
            Vp = c_var + sgw ** 2 + A @ (mu * mu) + (A + M * M) @ (sg * sg) + C @ mu
            L = np.sum(0.5 * prec * ((y - Ep) ** 2 + Vp)) + const
            res = Ep - y
            gmu = prec * (res @ M + mu * A.sum(0) + 0.5 * C.sum(0))
            gsg = prec * sg * (A + M * M).sum(0)
            gmw, gsw = prec * res.sum(), prec * n * sgw
        else:
            ee, eb, eg = (np.asarray(a, dtype=np.float64) for a in eps(t0 + it))
            ze = mu + sg * ee[e]
            zq = [ent[X[:, f], :d] + R.link(ent[X[:, f], d:], kind) * ee[X[:, f]] for f in cols]
            S = sum(zq)
            pair = 0.5 * (S * S - sum(z * z for z in zq)).sum(1)
            wq = sum(bia[X[:, f], 0] + R.link(bia[X[:, f], 1], kind) * eb[X[:, f]] for f in cols)
            pred = (m0 + sg0 * float(eg)) + (mw + sgw * eb[e]) + wq + S @ ze + pair
            if output == "reg":
                L = np.sum(0.5 * prec * (y - pred) ** 2) + const
                gp = prec * (pred - y)
            else:
                L = np.sum(np.logaddexp(0.0, pred) - y * pred)
                gp = 1.0 / (1.0 + np.exp(-pred)) - y
            acc = gp @ S
            gmu, gsg = acc, acc * ee[e]
            gmw, gsw = gp.sum(), gp.sum() * eb[e]
        kl, gk = R._kl(th, kind, klw)
        g = np.concatenate([gmu, gsg * R.dlink(s, kind), [gmw, gsw * float(R.dlink(sw, kind))]]) + gk
        return L + kl, g

    return R._adam(theta, grad_fn, n_steps, lr)


def session(e, pool_x, pool_y, n_rounds, strategy, ent, bia, scal, field=0, key_col=None, kind="abs", output="reg",
            objective="closed_form", hist_x=None, hist_y=(), n_steps=20, lr=0.05, klw=1.0, reset=False, eps=None, t0=0,
            uniform=None):
    """All rounds of respondent e over its pool rows pool_x [P, F].  Returns dict(rows [Q] pool positions or -1,
    score [Q], loss [Q], gap [Q] (relative gap of the chosen score to the runner-up), theta [Q] tuples, mean / var
    [Q + 1, P] as scored before each round, score0 [P])."""
    pool_x = np.asarray(pool_x, dtype=np.int64)
    pool_y = np.asarray(pool_y, dtype=np.float64)
    F = pool_x.shape[1]
    d = ent.shape[1] // 2
    P = pool_x.shape[0]
    if key_col is None:
        key_col = [f for f in range(F) if f != field][0]
    theta = R.prior_theta(d, kind) if reset else R.table_theta(ent, bia, e)
    asked = np.zeros(P, dtype=bool)
    f_x = [] if hist_x is None else [np.asarray(r, dtype=np.int64) for r in hist_x]
    f_y = [float(v) for v in hist_y]
    out = dict(rows=[], score=[], loss=[], gap=[], theta=[], mean=[], var=[])
    for q in range(n_rounds + 1):
        mean, var = moments(theta, ent, bia, scal, pool_x, field, kind) if P else (np.zeros(0), np.zeros(0))
        out["mean"].append(mean)
        out["var"].append(var)
        if q == n_rounds:
            break
        sc = R.score(strategy, mean, var, q, pool_x[:, key_col], uniform)
        if q == 0:
            out["score0"] = np.array(sc, dtype=np.float64)
        best, gap = R.choose(sc, asked)
        out["rows"].append(best)
        out["gap"].append(gap)
        if best < 0:
            out["score"].append(math.nan)
            out["loss"].append(math.nan)
            out["theta"].append(theta)
            continue
        out["score"].append(float(sc[best]))
        asked[best] = True
        f_x.append(pool_x[best])
        f_y.append(float(pool_y[best]))
        theta, loss = fold(theta, e, np.array(f_x), f_y, ent, bia, scal, field, kind, output, objective, n_steps, lr, klw,
                           eps, t0 + q * (n_steps + 1))
        out["loss"].append(loss)
        out["theta"].append(theta)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the planted models of test_gpu_elicit_field.py::test_against_the_fp64_restatement_on_a_planted_model
# ---------------------------------------------------------------------------------------------------------------------
PLANTED = {  # name: output, objective, link, strategy, reset, history rows per respondent, d, field, generator seed
    "closed_form_d5": ("reg", "closed_form", "abs", "variance", True, 0, 5, 0, 7),
    "closed_form_d128": ("reg", "closed_form", "softplus", "top", False, 3, 128, 1, 6),
    "sampled_d5": ("class", "sampled", "softplus", "top", False, 3, 5, 0, 5),
    "sampled_d128": ("reg", "sampled", "abs", "top", True, 0, 128, 0, 4),
}
PLANTED_SIZES = (12, 40, 4)              # users, items, formats
PLANTED_RESPONDENTS, PLANTED_POOL, PLANTED_ROUNDS, PLANTED_STEPS, PLANTED_LR = 8, 12, 4, 20, 0.01


def planted_case(name):
    """The inputs of one case of PLANTED (numpy only, shared by the CPU gap check and the GPU test): a three-field model
    in the manner of elicit_restatement.planted_case -- context means N(0, 1 / d) per coordinate (logits of unit scale)
    with sigma 0.05, the respondents' field N(0, 1) with sigma 0.3, noise sd 0.5 (precision 4); 8 respondents (the first
    ids of the folded field's range) with 12-row pools of distinct contexts and their history rows.  Returns
    dict(ent, bia, scal fp32 tables, pool [P, 3], y_pool [P], hist_x [H, 3], hist_y [H])."""
    output, objective, kind, strategy, reset, n_hist, d, field, seed = PLANTED[name]
    sizes = PLANTED_SIZES
    T = sum(sizes)
    lo = [sum(sizes[:f]) for f in range(3)]
    g = np.random.default_rng(1000 * seed + sorted(PLANTED).index(name))
    s_of = (lambda sig: sig) if kind == "abs" else (lambda sig: math.log(math.expm1(sig)))
    mu = g.normal(size=(T, d)) / math.sqrt(d)
    mu[lo[field]: lo[field] + sizes[field]] *= math.sqrt(d)
    s = np.full((T, d), s_of(0.05))
    s[lo[field]: lo[field] + sizes[field]] = s_of(0.3)
    ent = np.concatenate([mu, s], 1).astype(np.float32)
    bia = np.stack([g.normal(size=T) * 0.1, np.full(T, s_of(0.05))], 1).astype(np.float32)
    bia[lo[field]: lo[field] + sizes[field], 1] = s_of(0.3)
    scal = np.array([s_of(4.0), 0.0, s_of(0.05)], dtype=np.float32)
    cols = [f for f in range(3) if f != field]
    n_ctx = sizes[cols[0]] * sizes[cols[1]]
    pool, hist = [], []
    for r in range(PLANTED_RESPONDENTS):
        pick = g.permutation(n_ctx)[:PLANTED_POOL + n_hist]                 # distinct contexts: no tied scores
        rows = np.zeros((len(pick), 3), dtype=np.int64)
        rows[:, field] = lo[field] + r
        rows[:, cols[0]] = lo[cols[0]] + pick // sizes[cols[1]]
        rows[:, cols[1]] = lo[cols[1]] + pick % sizes[cols[1]]
        pool.append(rows[:PLANTED_POOL])
        hist.append(rows[PLANTED_POOL:])
    pool, hist = np.concatenate(pool), np.concatenate(hist)
    mu64 = ent[:, :d].astype(np.float64)

    def answers(x):
        z = [mu64[x[:, f]] for f in range(3)]
        truth = sum((z[a] * z[b]).sum(1) for a in range(3) for b in range(a + 1, 3)) + sum(bia[x[:, f], 0] for f in range(3))
        if output == "reg":
            return (truth + 0.5 * g.normal(size=len(x))).astype(np.float32)
        return (g.random(len(x)) < 1.0 / (1.0 + np.exp(-truth))).astype(np.float32)

    return dict(ent=ent, bia=bia, scal=scal, pool=pool, y_pool=answers(pool), hist_x=hist, hist_y=answers(hist))


def numpy_eps(case, seed=7):
    """eps(t) from numpy normals keyed on the draw key, rounded to fp32 as the kernel's draws are: the stand-in of the
    CPU gap check (the kernel's Philox stream needs a GPU)."""
    T, d = case["ent"].shape[0], case["ent"].shape[1] // 2
    cache = {}

    def f(t):
        if t not in cache:
            g = np.random.default_rng([seed, t])
            cache[t] = (g.normal(size=(T, d)).astype(np.float32), g.normal(size=T).astype(np.float32),
                        np.float32(g.normal()))
        return cache[t]
    return f


def planted_sessions(name, case, eps):
    """The fp64 session of every respondent of a planted case, in ascending respondent order: [(pool positions [n],
    session dict)]'s second parts carry "sel", the respondent's rows of case["pool"]."""
    output, objective, kind, strategy, reset, n_hist, d, field, seed = PLANTED[name]
    E, B, S = (case[k].astype(np.float64) for k in ("ent", "bia", "scal"))
    out = []
    for e in np.unique(case["pool"][:, field]):
        sel = np.nonzero(case["pool"][:, field] == e)[0]
        hs = np.nonzero(case["hist_x"][:, field] == e)[0]
        s = session(int(e), case["pool"][sel], case["y_pool"][sel], PLANTED_ROUNDS, strategy, E, B, S, field=field, kind=kind,
                    output=output, objective=objective, hist_x=case["hist_x"][hs], hist_y=case["hist_y"][hs],
                    n_steps=PLANTED_STEPS, lr=PLANTED_LR, reset=reset, eps=eps if objective == "sampled" else None)
        s["sel"], s["entity"] = sel, int(e)
        out.append(s)
    return out

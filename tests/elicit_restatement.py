"""fp64 numpy restatement of the elicitation session (include/vfm_elicit.h), two-field model: a helper of
test_elicit_cpu.py / test_gpu_elicit.py, not a test.

Two independent statements of the same semantics:
  * the single-round pieces -- `moments` (closed-form logit mean / variance of (u, item) pairs), `score`, `choose`,
    `fold` (n_steps Adam updates of one user's theta on a list of rows, recomputed from scratch);
  * `session`: all rounds of one user with the closed form's row sums carried from round to round (an asked row is
    appended to them, as the kernel does) and the fold-in written against those sums.
test_elicit_cpu.py checks that `session` agrees with a literal loop over the single-round pieces.

Tables: ent [T, 2d] = [mu | s], bia [T, 2] = [mu_w, s_w], scal [3] = alpha, global mean, global scale; sigma = link(s).
theta = (mu [d], s [d], mu_w, s_w) of the user.  The sampled objective takes eps(t) -> (eps_entity [T, d], eps_bias [T],
eps_global) for draw key t (one draw per iteration: n_samples = 1); strategy "random" takes uniform(q, item) -> float.
"""
import math

import numpy as np

LOG_2PI_HALF = 0.5 * math.log(2 * math.pi)


def link(s, kind, dtype=np.float64):
    s = np.asarray(s, dtype=dtype)
    return np.abs(s) if kind == "abs" else np.logaddexp(0.0, s)


def dlink(s, kind, dtype=np.float64):
    s = np.asarray(s, dtype=dtype)
    return np.where(s < 0, -1.0, 1.0).astype(dtype) if kind == "abs" else 1.0 / (1.0 + np.exp(-s))


def _scalar_of(dtype):
    """The scalar constructor of a working precision: float for float64 (the arithmetic of every caller that names no
    dtype, unchanged), the numpy scalar type otherwise (a Python float would carry scalar products in fp64)."""
    return float if np.dtype(dtype) == np.float64 else np.dtype(dtype).type


def prior_theta(d, kind):
    s1 = 1.0 if kind == "abs" else math.log(math.e - 1.0)
    return np.zeros(d), np.full(d, s1), 0.0, s1


def table_theta(ent, bia, u):
    d = ent.shape[1] // 2
    return ent[u, :d].astype(np.float64), ent[u, d:].astype(np.float64), float(bia[u, 0]), float(bia[u, 1])


def moments(theta, ent, bia, scal, items, kind):
    """(mean [n], var [n]) of the pairs (user with `theta`, item) for the item ids `items`."""
    mu, s, mw, sw = theta
    d = mu.shape[0]
    sg, sgw = link(s, kind), float(link(sw, kind))
    mi = ent[items, :d].astype(np.float64)
    si2 = link(ent[items, d:], kind) ** 2
    sbi = link(bia[items, 1], kind)
    mean = float(scal[1]) + mw + bia[items, 0].astype(np.float64) + mi @ mu
    var = float(link(scal[2], kind)) ** 2 + sgw ** 2 + sbi ** 2 + si2 @ (mu * mu) + (mi * mi + si2) @ (sg * sg)
    return mean, var


def score(strategy, mean, var, q=0, items=None, uniform=None):
    if strategy == "top":
        return mean
    if strategy == "variance":
        return var
    if strategy == "mean":
        return -np.abs(mean) / np.sqrt(1.0 + math.pi / 8.0 * var)
    return np.array([uniform(q, int(i)) for i in items], dtype=np.float64)


def choose(sc, asked):
    """(position of the best unasked score -- ties: the lower position; NaN never --, or -1; the relative gap to the
    runner-up, inf with fewer than two candidates)."""
    best, second = -1, -1
    for p in range(len(sc)):
        if asked[p] or np.isnan(sc[p]):
            continue
        if best < 0 or sc[p] > sc[best]:
            best, second = p, best
        elif second < 0 or sc[p] > sc[second]:
            second = p
    if best < 0:
        return -1, math.inf
    if second < 0:
        return best, math.inf
    den = max(abs(sc[best]), abs(sc[second]), 1e-300)
    return best, (sc[best] - sc[second]) / den


def _adam(theta, grad_fn, n_steps, lr, dtype=np.float64):
    p = np.concatenate([theta[0], theta[1], [theta[2], theta[3]]]).astype(dtype)
    d = theta[0].shape[0]
    m, v = np.zeros_like(p), np.zeros_like(p)
    unpack = lambda p: (p[:d], p[d:2 * d], p[2 * d], p[2 * d + 1])
    for it in range(n_steps):
        _, g = grad_fn(unpack(p), it)
        t = it + 1
        m = 0.9 * m + 0.1 * g
        v = 0.999 * v + 0.001 * g * g
        p = p - (lr / (1.0 - 0.9 ** t)) * m / (np.sqrt(v) / math.sqrt(1.0 - 0.999 ** t) + 1e-8)
    loss, _ = grad_fn(unpack(p), n_steps)
    th = unpack(p)
    return (th[0].copy(), th[1].copy(), float(th[2]), float(th[3])), float(loss)


def _kl(theta, kind, klw, dtype=np.float64):
    f = _scalar_of(dtype)
    mu, s, mw, sw = theta
    sg, sgw = link(s, kind, dtype), f(link(sw, kind, dtype))
    kl = np.sum(0.5 * (sg * sg + mu * mu - 1.0) - np.log(sg)) + 0.5 * (sgw * sgw + mw * mw - 1.0) - math.log(sgw)
    g = np.concatenate([klw * mu, klw * (sg - 1.0 / sg) * dlink(s, kind, dtype),
                        [klw * mw, klw * (sgw - 1.0 / sgw) * f(dlink(sw, kind, dtype))]])
    return klw * kl, g


def fold(theta, u, items, y, ent, bia, scal, kind, output, objective, n_steps, lr, klw=1.0, eps=None, t0=0,
         dtype=np.float64):
    """n_steps Adam updates (fresh moments) of the user's theta on the rows (items [n], y [n]); every quantity is
    recomputed from the rows at every step.  Returns (theta, loss at the final parameters).  dtype: the working
    precision of every array and scalar (float32: what rounding alone does to the fold, no kernel involved)."""
    f = _scalar_of(dtype)
    items = np.asarray(items, dtype=np.int64)
    y = np.asarray(y, dtype=dtype)
    d = theta[0].shape[0]
    prec = f(link(scal[0], kind, dtype))
    m0, sg0 = f(scal[1]), f(link(scal[2], kind, dtype))
    mi = ent[items, :d].astype(dtype)
    si = link(ent[items, d:], kind, dtype)
    bi, sbi = bia[items, 0].astype(dtype), link(bia[items, 1], kind, dtype)
    n = len(items)

    def grad_fn(th, it):
        mu, s, mw, sw = th
        sg, sgw = link(s, kind, dtype), f(link(sw, kind, dtype))
        if objective == "closed_form":
            A = si * si
            Ep = m0 + bi + mw + mi @ mu
            Vp = sg0 ** 2 + sbi ** 2 + sgw ** 2 + A @ (mu * mu) + (A + mi * mi) @ (sg * sg)
            L = np.sum(0.5 * prec * ((y - Ep) ** 2 + Vp)) + n * (LOG_2PI_HALF - 0.5 * math.log(prec))
            res = Ep - y
            gmu = prec * (res @ mi + mu * A.sum(0))
            gsg = prec * sg * (A + mi * mi).sum(0)
            gmw, gsw = prec * res.sum(), prec * n * sgw
        else:
            ee, eb, eg = (np.asarray(a, dtype=dtype) for a in eps(t0 + it))
            zu = mu + sg * ee[u]
            zi = mi + si * ee[items]
            pred = (m0 + sg0 * f(eg)) + (mw + sgw * eb[u]) + (bi + sbi * eb[items]) + zi @ zu
            if output == "reg":
                L = np.sum(0.5 * prec * (y - pred) ** 2) + n * (LOG_2PI_HALF - 0.5 * math.log(prec))
                gp = prec * (pred - y)
            else:
                L = np.sum(np.logaddexp(0.0, pred) - y * pred)
                gp = 1.0 / (1.0 + np.exp(-pred)) - y
            acc = gp @ zi
            gmu, gsg = acc, acc * ee[u]
            gmw, gsw = gp.sum(), gp.sum() * eb[u]
        kl, gk = _kl(th, kind, klw, dtype)
        g = np.concatenate([gmu, gsg * dlink(s, kind, dtype), [gmw, gsw * f(dlink(sw, kind, dtype))]]) + gk
        return L + kl, g

    return _adam(theta, grad_fn, n_steps, lr, dtype)


def session(u, pool_items, pool_y, n_rounds, strategy, ent, bia, scal, kind="abs", output="reg",
            objective="closed_form", hist_items=(), hist_y=(), n_steps=20, lr=0.05, klw=1.0, reset=False, eps=None,
            t0=0, uniform=None):
    """All rounds of user u.  Returns dict(rows [Q] pool positions or -1, score [Q], loss [Q], gap [Q] (relative gap of
    the chosen score to the runner-up), theta [Q] tuples, mean / var [Q + 1, P] as scored before each round, score0 [P]).
    The closed form's row sums are carried from round to round; the fold-in is written against them."""
    pool_items = np.asarray(pool_items, dtype=np.int64)
    pool_y = np.asarray(pool_y, dtype=np.float64)
    d = ent.shape[1] // 2
    P = len(pool_items)
    theta = prior_theta(d, kind) if reset else table_theta(ent, bia, u)
    asked = np.zeros(P, dtype=bool)
    f_items, f_y = [int(i) for i in hist_items], [float(v) for v in hist_y]
    prec = float(link(scal[0], kind))
    m0, sg0 = float(scal[1]), float(link(scal[2], kind))
    SA, SB, Scv = np.zeros(d), np.zeros(d), 0.0
    Ms, Cy = [], []

    def append(item, yv):
        nonlocal SA, SB, Scv
        M = ent[item, :d].astype(np.float64)
        A = link(ent[item, d:], kind) ** 2
        SA, SB = SA + A, SB + (A + M * M)
        Scv += sg0 ** 2 + float(link(bia[item, 1], kind)) ** 2
        Ms.append(M)
        Cy.append(m0 + float(bia[item, 0]) - yv)

    for it, yv in zip(f_items, f_y):
        append(it, yv)
    out = dict(rows=[], score=[], loss=[], gap=[], theta=[], mean=[], var=[])
    for q in range(n_rounds + 1):
        mean, var = moments(theta, ent, bia, scal, pool_items, kind)
        out["mean"].append(mean)
        out["var"].append(var)
        if q == n_rounds:
            break
        sc = score(strategy, mean, var, q, pool_items, uniform)
        if q == 0:
            out["score0"] = np.array(sc, dtype=np.float64)
        best, gap = choose(sc, asked)
        out["rows"].append(best)
        out["gap"].append(gap)
        if best < 0:
            out["score"].append(math.nan)
            out["loss"].append(math.nan)
            out["theta"].append(theta)
            continue
        out["score"].append(float(sc[best]))
        asked[best] = True
        f_items.append(int(pool_items[best]))
        f_y.append(float(pool_y[best]))
        append(f_items[-1], f_y[-1])
        if objective == "closed_form":
            Mm, cy, n = np.array(Ms), np.array(Cy), len(Ms)

            def grad_fn(th, it):
                mu, s, mw, sw = th
                sg, sgw = link(s, kind), float(link(sw, kind))
                res = cy + mw + Mm @ mu
                vq = np.sum(mu * mu * SA + sg * sg * SB)
                L = 0.5 * prec * (np.sum(res * res) + Scv + n * sgw * sgw + vq) + n * (LOG_2PI_HALF - 0.5 * math.log(prec))
                g = np.concatenate([prec * (res @ Mm + mu * SA), prec * sg * SB * dlink(s, kind),
                                    [prec * res.sum(), prec * n * sgw * float(dlink(sw, kind))]])
                kl, gk = _kl(th, kind, klw)
                return L + kl, g + gk

            theta, loss = _adam(theta, grad_fn, n_steps, lr)
        else:
            theta, loss = fold(theta, u, f_items, f_y, ent, bia, scal, kind, output, objective, n_steps, lr, klw, eps,
                               t0 + q * (n_steps + 1))
        out["loss"].append(loss)
        out["theta"].append(theta)
    return out


def closed_form_thetas_fp32(rows, pool_items, pool_y, ent, bia, scal, n_steps, lr):
    """A plain numpy fp32 transcription of the closed-form session's folds (|.| link, cold start, kl_weight 1, no
    history) along the GIVEN selections `rows`: what fp32 rounding alone does to the thetas, with no kernel involved.
    Returns [(mu, s, (mu_w, s_w))] per round.  The GPU test's tolerance is meaningful only where this stays well inside
    it (test_elicit_cpu.py checks that for the planted generator)."""
    f = np.float32
    d = ent.shape[1] // 2
    prec, m0 = f(abs(scal[0])), f(scal[1])
    p = np.concatenate([np.zeros(d, f), np.ones(d, f), [f(0), f(1)]]).astype(f)
    SA, SB, Ms, cy, out = np.zeros(d, f), np.zeros(d, f), [], [], []
    for r in rows:
        it = pool_items[r]
        M, A = ent[it, :d].astype(f), np.abs(ent[it, d:]).astype(f) ** 2
        SA, SB = SA + A, SB + (M * M + A)
        Ms.append(M)
        cy.append(f(m0 + f(bia[it, 0])) - f(pool_y[r]))
        Mm, c, n = np.array(Ms, f), np.array(cy, f), f(len(Ms))
        m, v = np.zeros_like(p), np.zeros_like(p)
        for t in range(1, n_steps + 1):
            mu, s, mw, sw = p[:d], p[d:2 * d], p[2 * d], p[2 * d + 1]
            sg, sgw = np.abs(s), abs(sw)
            res = (c + mw) + Mm @ mu
            g = np.concatenate([prec * (res @ Mm + mu * SA) + mu, (prec * sg * SB + (sg - f(1) / sg)) * np.sign(s),
                                [prec * res.sum(dtype=f) + mw, (prec * n * sgw + (sgw - f(1) / sgw)) * np.sign(sw)]]).astype(f)
            m = m + (g - m) * f(0.1)
            v = v * f(0.999) + (f(0.001) * g) * g
            den = np.sqrt(v) / f(math.sqrt(1.0 - 0.999 ** t)) + f(1e-8)
            p = (p + (-f(lr / (1.0 - 0.9 ** t)) * m) / den).astype(f)
        out.append((p[:d].copy(), p[d:2 * d].copy(), p[2 * d:].copy()))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the per-round fp64 check of test_gpu_elicit_shapes.py: its three generators and the walk along given selections
# ---------------------------------------------------------------------------------------------------------------------
FP64_CASES = {  # name: output, objective, link, strategy, reset, history rows per user, d
    "sampled_class_softplus_history_mean_d33": ("class", "sampled", "softplus", "mean", False, 12, 33),
    "sampled_reg_abs_reset_variance_d300": ("reg", "sampled", "abs", "variance", True, 0, 300),
    "closed_form_reg_softplus_history_top_d129": ("reg", "closed_form", "softplus", "top", False, 12, 129),
}
FP64_USERS, FP64_ITEMS, FP64_POOL, FP64_ROUNDS, FP64_STEPS, FP64_LR = 16, 120, 30, 5, 20, 0.01


def planted_case(name):
    """The inputs of one case of FP64_CASES (numpy only, so that the CPU conditioning test and the GPU test share
    them): 16 users, 120 items, 30-row pools, planted item means of norm about 1 at every d (N(0, 1 / d) coordinates:
    logits of unit scale), user means N(0, 1) with sigma 0.3, item sigmas 0.05, noise sd 0.5 (precision 4).  Returns
    dict(ent [T, 2d], bia [T, 2], scal [3] fp32 tables, pool [P, 2], y_pool [P], hist_x [H, 2], hist_y [H])."""
    output, objective, kind, strategy, reset, n_hist, d = FP64_CASES[name]
    N, M, P = FP64_USERS, FP64_ITEMS, FP64_POOL
    g = np.random.default_rng(100 + sorted(FP64_CASES).index(name))
    s_of = (lambda sig: sig) if kind == "abs" else (lambda sig: math.log(math.expm1(sig)))
    mu = g.normal(size=(N + M, d))
    mu[N:] /= math.sqrt(d)
    s = np.full((N + M, d), s_of(0.05))
    s[:N] = s_of(0.3)
    ent = np.concatenate([mu, s], 1).astype(np.float32)
    bia = np.stack([g.normal(size=N + M) * 0.1, np.full(N + M, s_of(0.05))], 1).astype(np.float32)
    bia[:N, 1] = s_of(0.3)
    scal = np.array([s_of(4.0), 0.0, s_of(0.05)], dtype=np.float32)
    pool, hist = [], []
    for u in range(N):
        it = N + g.permutation(M)
        pool.append(np.stack([np.full(P, u), it[:P]], 1))
        hist.append(np.stack([np.full(n_hist, u), it[P:P + n_hist]], 1))
    pool, hist = np.concatenate(pool).astype(np.int64), np.concatenate(hist).astype(np.int64)

    def answers(x):
        truth = (mu[x[:, 0]] * mu[x[:, 1]]).sum(1) + bia[x[:, 0], 0] + bia[x[:, 1], 0]
        if output == "reg":
            return (truth + 0.5 * g.normal(size=len(x))).astype(np.float32)
        return (g.random(len(x)) < 1.0 / (1.0 + np.exp(-truth))).astype(np.float32)

    return dict(ent=ent, bia=bia, scal=scal, pool=pool, y_pool=answers(pool), hist_x=hist, hist_y=answers(hist))


def rounds_along(name, case, u, rows, theta_before, eps, dtype=np.float64):
    """User u's session of `case` taken round by round along GIVEN selections, with no feedback between the rounds:
    rows [Q] positions in u's pool slice (-1: nothing asked), theta_before(q) -> the theta tuple round q starts from.
    Per round q with a row asked: (q, mean, var, score [n_pool] from theta_before(q), the unasked mask before the
    choice, theta after the fold of the history followed by rows[:q + 1] with t0 = q (n_steps + 1), its loss)."""
    output, objective, kind, strategy, reset, n_hist, d = FP64_CASES[name]
    E, B, S = (case[k].astype(np.float64) for k in ("ent", "bia", "scal"))
    sel = np.nonzero(case["pool"][:, 0] == u)[0]
    items, ys = case["pool"][sel, 1], case["y_pool"][sel]
    hs = np.nonzero(case["hist_x"][:, 0] == u)[0]
    f_items, f_y = list(case["hist_x"][hs, 1]), list(case["hist_y"][hs])
    unasked = np.ones(len(sel), dtype=bool)
    out = []
    for q, r in enumerate(rows):
        if r < 0:
            break
        th = theta_before(q)
        mean, var = moments(th, E, B, S, items, kind)
        sc = score(strategy, mean, var)
        mask = unasked.copy()
        unasked[r] = False
        f_items.append(items[r])
        f_y.append(ys[r])
        th_d = (th[0].astype(dtype), th[1].astype(dtype), th[2], th[3])
        th1, loss = fold(th_d, u, f_items, f_y, E, B, S, kind, output, objective, FP64_STEPS, FP64_LR, 1.0, eps,
                         q * (FP64_STEPS + 1), dtype=dtype)
        out.append((q, mean, var, sc, mask, th1, loss))
    return out

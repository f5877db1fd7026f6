"""fp64 reference of the implicit-feedback objective and its blocks (VFM.fit_implicit, include/vfm_implicit.h), written
from the dense definition: every (user, item) pair is a row, an observed pair with its target and weight w1, every other
pair with target 0 and weight w0.  Nothing here uses a Gram block but gram_J, the closed form the package evaluates,
which the CPU tests hold against brute_J.  Tables: ent [T, 2d] = mu | s, bia [T, 2] = mu_w | s_w, scal [3] = alpha,
m_0, s_0 (any float dtype; taken to fp64); users are ids [0, N), items [N, N + M)."""
import math

import torch

LOG_2PI_HALF = 0.5 * math.log(2.0 * math.pi)


def link_t(s, link):
    s = s.double()
    return s.abs() if link == "abs" else torch.nn.functional.softplus(s)


def inv_link_t(v, link):
    return v if link == "abs" else torch.log(torch.expm1(v))


def kl_t(mu, sg):
    return 0.5 * (sg * sg + mu * mu - 1.0) - torch.log(sg)


def dense_targets(x, y, N, M, w0, w1):
    """(Wgt [N, M], Y [N, M]) of the dense grid."""
    Wgt = torch.full((N, M), float(w0), dtype=torch.float64)
    Y = torch.zeros(N, M, dtype=torch.float64)
    if x.shape[0]:
        Wgt[x[:, 0], x[:, 1] - N] = float(w1)
        Y[x[:, 0], x[:, 1] - N] = y.double()
    return Wgt, Y


def pair_moments(ent, bia, scal, N, M, link):
    """(E pred [N, M], Var pred [N, M]) of every pair, differentiable."""
    d = ent.shape[1] // 2
    ent, bia, scal = ent.double(), bia.double(), scal.double()
    mu_u, mu_i = ent[:N, :d], ent[N:N + M, :d]
    su2, si2 = link_t(ent[:N, d:], link) ** 2, link_t(ent[N:N + M, d:], link) ** 2
    m = scal[1] + bia[:N, :1] + bia[N:N + M, 0][None, :] + mu_u @ mu_i.T
    v = (link_t(scal[2], link) ** 2 + link_t(bia[:N, 1], link)[:, None] ** 2 + link_t(bia[N:N + M, 1], link)[None, :] ** 2
         + (mu_u * mu_u) @ si2.T + su2 @ si2.T + su2 @ (mu_i * mu_i).T)
    return m, v


def kl_all(ent, bia, scal, link):
    d = ent.shape[1] // 2
    ent, bia, scal = ent.double(), bia.double(), scal.double()
    return (kl_t(ent[:, :d], link_t(ent[:, d:], link)).sum() + kl_t(bia[:, 0], link_t(bia[:, 1], link)).sum()
            + kl_t(scal[1], link_t(scal[2], link)))


def brute_J(ent, bia, scal, x, y, N, M, link, w0, w1, kl_weight):
    """J_imp over the dense N x M grid (differentiable in the tables)."""
    Wgt, Y = dense_targets(x, y, N, M, w0, w1)
    m, v = pair_moments(ent, bia, scal, N, M, link)
    prec = link_t(scal[0], link)
    rows = Wgt * (0.5 * prec * ((Y - m) ** 2 + v) - 0.5 * torch.log(prec) + LOG_2PI_HALF)
    return rows.sum() + kl_weight * kl_all(ent, bia, scal, link)


def gram_sums(ent, bia, scal, x, y, N, M, link, w0, w1):
    """(W, S1, S2) = sum w, sum w (y - (E pred - m0)), sum w ((y - E pred)^2 + Var pred) over all pairs through the two
    fields' Grams and first moments, corrected at the observed rows."""
    d = ent.shape[1] // 2
    ent, bia, scal = ent.double(), bia.double(), scal.double()
    m0, s0 = scal[1], link_t(scal[2], link)
    mu_u, mu_i = ent[:N, :d], ent[N:N + M, :d]
    su2, si2 = link_t(ent[:N, d:], link) ** 2, link_t(ent[N:N + M, d:], link) ** 2
    one = lambda n: torch.ones(n, 1, dtype=torch.float64)
    P = torch.cat([one(N), bia[:N, :1], mu_u], 1)
    Q = torch.cat([m0 + bia[N:N + M, :1], one(M), mu_i], 1)
    sum_m2 = ((P.T @ P) * (Q.T @ Q)).sum()
    sum_m = P.sum(0) @ Q.sum(0)
    sum_v = (N * M * s0 * s0 + M * (link_t(bia[:N, 1], link) ** 2).sum() + N * (link_t(bia[N:N + M, 1], link) ** 2).sum()
             + (mu_u * mu_u).sum(0) @ si2.sum(0) + su2.sum(0) @ (si2 + mu_i * mu_i).sum(0))
    R = x.shape[0]
    W = w0 * N * M + (w1 - w0) * R
    S1 = -w0 * (sum_m - N * M * m0)
    S2 = w0 * (sum_m2 + sum_v)
    if R:
        u, i = x[:, 0], x[:, 1]
        m = m0 + bia[u, 0] + bia[i, 0] + (ent[u, :d] * ent[i, :d]).sum(1)
        su, si = link_t(ent[u, d:], link) ** 2, link_t(ent[i, d:], link) ** 2
        v = (s0 * s0 + link_t(bia[u, 1], link) ** 2 + link_t(bia[i, 1], link) ** 2
             + (ent[u, :d] ** 2 * si + su * si + su * ent[i, :d] ** 2).sum(1))
        yd = y.double()
        S1 = S1 + (w1 * (yd - (m - m0)) + w0 * (m - m0)).sum()
        S2 = S2 + (w1 * ((yd - m) ** 2 + v) - w0 * (m * m + v)).sum()
    return W, S1, S2


def gram_J(ent, bia, scal, x, y, N, M, link, w0, w1, kl_weight):
    prec = link_t(scal[0], link)
    W, _, S2 = gram_sums(ent, bia, scal, x, y, N, M, link, w0, w1)
    return 0.5 * prec * S2 + W * (LOG_2PI_HALF - 0.5 * torch.log(prec)) + kl_weight * kl_all(ent, bia, scal, link)


def _partners(ent, bia, scal, field, N, M, link):
    """The partner field of `field`: (ids, u [n, d + 1], A [n, d + 1], c_mean [n], c_var [n])."""
    d = ent.shape[1] // 2
    ent, bia, scal = ent.double(), bia.double(), scal.double()
    ids = torch.arange(N, N + M) if field == 0 else torch.arange(0, N)
    n = ids.numel()
    u = torch.cat([torch.ones(n, 1, dtype=torch.float64), ent[ids, :d]], 1)
    A = torch.cat([torch.zeros(n, 1, dtype=torch.float64), link_t(ent[ids, d:], link) ** 2], 1)
    cm = scal[1] + bia[ids, 0]
    cv = link_t(scal[2], link) ** 2 + link_t(bia[ids, 1], link) ** 2
    return ids, u, A, cm, cv


def entity_rows(x, y, field, e, ids, w0, w1):
    """(w [n], y [n]) of entity e over all partners `ids` (a contiguous range)."""
    w = torch.full((ids.numel(),), float(w0), dtype=torch.float64)
    t = torch.zeros(ids.numel(), dtype=torch.float64)
    if x.shape[0]:
        sel = x[:, field] == e
        j = x[sel, 1 - field] - int(ids[0])
        w[j] = float(w1)
        t[j] = y[sel].double()
    return w, t


def system_fp64(ent, bia, scal, x, y, field, N, M, link, w0, w1, kl_weight, e):
    """(H [d + 1, d + 1], b [d + 1], SB' [d + 1]) of entity e from its dense row set."""
    ids, u, A, cm, cv = _partners(ent, bia, scal, field, N, M, link)
    w, t = entity_rows(x, y, field, e, ids, w0, w1)
    prec = link_t(scal[0], link)
    H = kl_weight * torch.eye(u.shape[1], dtype=torch.float64) + prec * (u.T @ (w[:, None] * u) + torch.diag((w[:, None] * A).sum(0)))
    b = prec * (u.T @ (w * (t - cm)))
    SB = (w[:, None] * (A + u * u)).sum(0)
    return H, b, SB


def entity_loss_fp64(ent, bia, scal, x, y, field, N, M, link, w0, w1, kl_weight, e, theta, sigma):
    """L_e at (theta, sigma) [d + 1] (column 0: the first-order weight), row by row over all partners."""
    ids, u, A, cm, cv = _partners(ent, bia, scal, field, N, M, link)
    w, t = entity_rows(x, y, field, e, ids, w0, w1)
    prec = link_t(scal[0], link)
    theta, sigma = theta.double(), sigma.double()
    res = t - cm - u @ theta
    var = cv + A @ (theta * theta) + (A + u * u) @ (sigma * sigma)
    rows = w * (0.5 * prec * (res * res + var) - 0.5 * torch.log(prec) + LOG_2PI_HALF)
    return rows.sum() + kl_weight * kl_t(theta, sigma).sum()


def implicit_solve_fp64(ent, bia, scal, x, y, field, N, M, link, w0, w1, kl_weight, entities=None):
    """The block minimiser of every entity of `entities` (default: the field's whole range): dict(ids [E],
    theta [E, d + 1], sigma [E, d + 1], cond [E] = cond_2(H))."""
    lo, hi = (0, N) if field == 0 else (N, N + M)
    ids = torch.arange(lo, hi) if entities is None else torch.as_tensor(entities, dtype=torch.int64)
    prec = link_t(scal[0], link)
    th, sg, cond = [], [], []
    for e in ids.tolist():
        H, b, SB = system_fp64(ent, bia, scal, x, y, field, N, M, link, w0, w1, kl_weight, e)
        th.append(torch.linalg.solve(H, b))
        sg.append(torch.sqrt(kl_weight / (kl_weight + prec * SB)))
        cond.append(torch.linalg.cond(H))
    return {"ids": ids, "theta": torch.stack(th), "sigma": torch.stack(sg), "cond": torch.stack(cond)}


def write_solution(ent, bia, sol, link, dtype=None):
    """The tables with sol's rows written (scales through the inverse link); dtype: round what is written."""
    ent, bia = ent.clone(), bia.clone()
    d = ent.shape[1] // 2
    ids = sol["ids"]
    s = inv_link_t(sol["sigma"], link)
    cast = (lambda v: v.to(dtype)) if dtype is not None else (lambda v: v)
    ent[ids, :d] = cast(sol["theta"][:, 1:]).to(ent.dtype)
    ent[ids, d:] = cast(s[:, 1:]).to(ent.dtype)
    bia[ids, 0] = cast(sol["theta"][:, 0]).to(bia.dtype)
    bia[ids, 1] = cast(s[:, 0]).to(bia.dtype)
    return ent, bia


def bias_block_fp64(ent, bia, scal, x, y, N, M, link, w0, w1, kl_weight):
    """scal with the global bias (mean, scale parameter) at its joint block minimiser."""
    prec = link_t(scal[0], link)
    W, S1, _ = gram_sums(ent, bia, scal, x, y, N, M, link, w0, w1)
    den = kl_weight + prec * W
    out = scal.clone().double()
    out[1] = prec * S1 / den
    out[2] = inv_link_t(torch.sqrt(kl_weight / den), link)
    return out.to(scal.dtype)


def precision_block_fp64(ent, bia, scal, x, y, N, M, link, w0, w1):
    W, _, S2 = gram_sums(ent, bia, scal, x, y, N, M, link, w0, w1)
    out = scal.clone().double()
    out[0] = inv_link_t(W / S2, link)
    return out.to(scal.dtype)


def planted(N, M, d, seed, scale=0.3, n_obs=None, dtype=torch.float64, scalars=(1.3, 0.2, 0.3)):
    """Tables with means of size `scale` and scales in [0.2, 0.6], and n_obs distinct observed pairs (every user id
    N - 1 and item id N + M - 1 unobserved when the grid allows)."""
    g = torch.Generator().manual_seed(seed)
    T = N + M
    ent = torch.cat([torch.randn(T, d, generator=g, dtype=torch.float64) * scale,
                     torch.rand(T, d, generator=g, dtype=torch.float64) * 0.4 + 0.2], 1)
    bia = torch.stack([torch.randn(T, generator=g, dtype=torch.float64) * scale,
                       torch.rand(T, generator=g, dtype=torch.float64) * 0.4 + 0.2], 1)
    scal = torch.tensor(scalars, dtype=torch.float64)
    nu, ni = max(N - 1, 1), max(M - 1, 1)
    n_obs = (nu * ni) // 3 if n_obs is None else n_obs
    pick = torch.randperm(nu * ni, generator=g)[:n_obs]
    x = torch.stack([pick // ni, N + pick % ni], 1)
    y = torch.randn(n_obs, generator=g, dtype=torch.float64) * 0.5 + 1.0
    return ent.to(dtype), bia.to(dtype), scal.to(dtype), x, y.to(dtype)

"""fp64 reference of the weighted implicit sweeps (VFM.fit_implicit(weights=), include/vfm_implicit_weights.h; DESIGN.md
§4 "Weighted implicit sweeps") for tests/test_fit_implicit_weights_cpu.py and tests/test_gpu_fit_implicit_weights.py,
written from the dense definition: a weight matrix Wgt [N, M] and a target matrix Y [N, M] over every (user, item) pair
-- an observed pair with its own weight and target, every other pair (w0, 0) -- and every block from rows or columns of
the two.  No Gram block, no g_r = w_r - w0, no correction at the observed rows anywhere in this file: the Gram form the
package evaluates is restated by the CPU tests and held against brute_J here.  CPU tensors only.

From implicit_reference come only helpers that know no weight: the links, pair_moments, kl_all, _partners,
write_solution, planted; from implicit_prior_reference the KL to a field prior and the prior block, which do not see
the likelihood.  A prior is the pair (m [d + 1], lam [d + 1]) or None for N(0, 1); the priors of a model are
(mean [2, d + 1], prec [2, d + 1]) or None."""
import torch

import implicit_prior_reference as IPR
import implicit_reference as IR

LOG_2PI_HALF = IR.LOG_2PI_HALF


def dense_targets(x, y, wts, N, M, w0):
    """(Wgt [N, M], Y [N, M]) of the dense grid: (wts[r], y[r]) at observed pair r, (w0, 0) elsewhere."""
    Wgt = torch.full((N, M), float(w0), dtype=torch.float64)
    Y = torch.zeros(N, M, dtype=torch.float64)
    if x.shape[0]:
        Wgt[x[:, 0], x[:, 1] - N] = wts.double()
        Y[x[:, 0], x[:, 1] - N] = y.double()
    return Wgt, Y


def _kl(ent, bia, scal, N, M, link, priors):
    if priors is None:
        return IR.kl_all(ent, bia, scal, link)
    return IPR.kl_all_prior(ent, bia, scal, N, M, link, priors[0], priors[1])


def brute_J(ent, bia, scal, x, y, wts, N, M, link, w0, kl_weight, priors=None):
    """J_imp over the dense N x M grid (differentiable in the tables and the priors)."""
    Wgt, Y = dense_targets(x, y, wts, N, M, w0)
    m, v = IR.pair_moments(ent, bia, scal, N, M, link)
    prec = IR.link_t(scal[0], link)
    rows = Wgt * (0.5 * prec * ((Y - m) ** 2 + v) - 0.5 * torch.log(prec) + LOG_2PI_HALF)
    return rows.sum() + kl_weight * _kl(ent, bia, scal, N, M, link, priors)


def entity_rows(x, y, wts, field, e, N, M, w0):
    """(w [n], t [n]) of entity e over all its partners in id order: a row (field 0) or a column (field 1) of the grid."""
    Wgt, Y = dense_targets(x, y, wts, N, M, w0)
    return (Wgt[e], Y[e]) if field == 0 else (Wgt[:, e - N], Y[:, e - N])


def system_fp64(ent, bia, scal, x, y, wts, field, N, M, link, w0, kl_weight, e, prior=None):
    """(H [d + 1, d + 1], b [d + 1], b_data [d + 1], SB' [d + 1]) of entity e from its dense row set:
    H = kl diag(lam) + prec sum_j w_j (u_j u_j^T + diag(0, A_j)), b = b_data + kl lam m, b_data = prec sum_j w_j t_j u_j."""
    ids, u, A, cm, cv = IR._partners(ent, bia, scal, field, N, M, link)
    w, t = entity_rows(x, y, wts, field, e, N, M, w0)
    prec = IR.link_t(scal[0], link)
    d1 = u.shape[1]
    m, lam = (torch.zeros(d1, dtype=torch.float64), torch.ones(d1, dtype=torch.float64)) if prior is None else \
        (torch.as_tensor(prior[0]).double(), torch.as_tensor(prior[1]).double())
    H = torch.diag(kl_weight * lam) + prec * (u.T @ (w[:, None] * u) + torch.diag((w[:, None] * A).sum(0)))
    b_data = prec * (u.T @ (w * (t - cm)))
    SB = (w[:, None] * (A + u * u)).sum(0)
    return H, b_data + kl_weight * lam * m, b_data, SB


def implicit_solve_fp64(ent, bia, scal, x, y, wts, field, N, M, link, w0, kl_weight, entities=None, prior=None):
    """The block minimiser of every entity of `entities` (default: the field's whole range): dict(ids [E],
    theta [E, d + 1], sigma [E, d + 1], cond [E] = cond_2(H))."""
    lo, hi = (0, N) if field == 0 else (N, N + M)
    ids = torch.arange(lo, hi) if entities is None else torch.as_tensor(entities, dtype=torch.int64)
    prec = IR.link_t(scal[0], link)
    th, sg, cond = [], [], []
    for e in ids.tolist():
        H, b, _, SB = system_fp64(ent, bia, scal, x, y, wts, field, N, M, link, w0, kl_weight, e, prior)
        lam = 1.0 if prior is None else torch.as_tensor(prior[1]).double()
        th.append(torch.linalg.solve(H, b))
        sg.append(torch.sqrt(kl_weight / (kl_weight * lam + prec * SB)))
        cond.append(torch.linalg.cond(H))
    return {"ids": ids, "theta": torch.stack(th), "sigma": torch.stack(sg), "cond": torch.stack(cond)}


def entity_loss_fp64(ent, bia, scal, x, y, wts, field, N, M, link, w0, kl_weight, e, theta, sigma, prior=None):
    """L_e at (theta, sigma) [d + 1] (column 0: the first-order weight), row by row over all partners."""
    ids, u, A, cm, cv = IR._partners(ent, bia, scal, field, N, M, link)
    w, t = entity_rows(x, y, wts, field, e, N, M, w0)
    prec = IR.link_t(scal[0], link)
    theta, sigma = theta.double(), sigma.double()
    res = t - cm - u @ theta
    var = cv + A @ (theta * theta) + (A + u * u) @ (sigma * sigma)
    rows = w * (0.5 * prec * (res * res + var) - 0.5 * torch.log(prec) + LOG_2PI_HALF)
    kl = IR.kl_t(theta, sigma) if prior is None else \
        IPR.kl_prior(theta, sigma, torch.as_tensor(prior[0]).double(), torch.as_tensor(prior[1]).double())
    return rows.sum() + kl_weight * kl.sum()


def dense_sums(ent, bia, scal, x, y, wts, N, M, link, w0):
    """(W, S1, S2) = sum w, sum w (y - (E pred - m0)), sum w ((y - E pred)^2 + Var pred) over the dense grid."""
    Wgt, Y = dense_targets(x, y, wts, N, M, w0)
    m, v = IR.pair_moments(ent, bia, scal, N, M, link)
    m0 = scal.double()[1]
    return Wgt.sum(), (Wgt * (Y - (m - m0))).sum(), (Wgt * ((Y - m) ** 2 + v)).sum()


def bias_block_fp64(ent, bia, scal, x, y, wts, N, M, link, w0, kl_weight):
    """scal with the global bias (mean, scale parameter) at its joint block minimiser."""
    prec = IR.link_t(scal[0], link)
    W, S1, _ = dense_sums(ent, bia, scal, x, y, wts, N, M, link, w0)
    den = kl_weight + prec * W
    out = scal.clone().double()
    out[1] = prec * S1 / den
    out[2] = IR.inv_link_t(torch.sqrt(kl_weight / den), link)
    return out.to(scal.dtype)


def precision_block_fp64(ent, bia, scal, x, y, wts, N, M, link, w0):
    W, _, S2 = dense_sums(ent, bia, scal, x, y, wts, N, M, link, w0)
    out = scal.clone().double()
    out[0] = IR.inv_link_t(W / S2, link)
    return out.to(scal.dtype)


def sweep_fp64(ent, bia, scal, x, y, wts, N, M, link, w0, kl_weight, priors=None, learn_priors=False, after=None):
    """One weighted implicit sweep on fp64 tables: field 0 (then its prior), field 1 (then its prior), the global bias,
    the precision.  after(what, ent, bia, scal, priors) follows every block; what: 0, ("prior", 0), 1, ("prior", 1),
    "bias", "precision".  Returns (ent, bia, scal, priors)."""
    ent, bia, scal = ent.double(), bia.double(), scal.double()
    if priors is not None:
        priors = (priors[0].double().clone(), priors[1].double().clone())
    for f in (0, 1):
        pr = None if priors is None else (priors[0][f], priors[1][f])
        sol = implicit_solve_fp64(ent, bia, scal, x, y, wts, f, N, M, link, w0, kl_weight, prior=pr)
        ent, bia = IR.write_solution(ent, bia, sol, link)
        if after:
            after(f, ent, bia, scal, priors)
        if learn_priors:
            priors[0][f], priors[1][f], _ = IPR.prior_block_fp64(ent, bia, f, N, M, link, priors[0][f])
            if after:
                after(("prior", f), ent, bia, scal, priors)
    scal = bias_block_fp64(ent, bia, scal, x, y, wts, N, M, link, w0, kl_weight)
    if after:
        after("bias", ent, bia, scal, priors)
    scal = precision_block_fp64(ent, bia, scal, x, y, wts, N, M, link, w0)
    if after:
        after("precision", ent, bia, scal, priors)
    return ent, bia, scal, priors


def draw_weights(n, w0, seed, ratio=16.0, n_floor=3):
    """n fp32 weights uniform in [w0, ratio w0], the first n_floor of a random order exactly w0 (w0: an fp32 value)."""
    g = torch.Generator().manual_seed(seed)
    w = (float(w0) * (1.0 + (ratio - 1.0) * torch.rand(n, generator=g, dtype=torch.float64))).float()
    w[torch.randperm(n, generator=g)[:min(n_floor, n)]] = float(w0)
    return w.clamp_min(float(w0))

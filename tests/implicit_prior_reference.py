"""fp64 reference of the hierarchical implicit sweeps (VFM.fit_implicit(priors=, learn_priors=True),
include/vfm_implicit_prior.h; DESIGN.md §4 "Hierarchical implicit sweeps") for tests/test_fit_implicit_priors_cpu.py and
tests/test_gpu_fit_implicit_priors.py: implicit_reference's blocks under a field prior N(m_c, 1 / lam_c), each from the
dense row set (a weight and a target per partner, no Gram block), the objective by brute force and in the Gram form,
the prior block over a field's whole id range and one sweep.  CPU tensors only.  A prior is the pair (m [d + 1],
lam [d + 1]), coordinate 0 the first-order weight; the priors of a model are (mean [2, d + 1], prec [2, d + 1]).

The KL to N(m, 1 / lam) is taken as KL(N(sqrt(lam) (mu - m), lam sg^2) || N(0, 1)) through implicit_reference.kl_t --
the same number as prior_reference.kl_prior_t (the CPU tests hold the two together) -- so that at m = 0, lam = 1 every
function here returns implicit_reference's result exactly."""
import torch

import implicit_reference as IR
import prior_reference as P


def _prior(m, lam):
    return torch.as_tensor(m).double(), torch.as_tensor(lam).double()


def kl_prior(mu, sg, m, lam):
    sl = torch.sqrt(lam)
    return IR.kl_t(sl * (mu - m), sl * sg)


def system_fp64_prior(ent, bia, scal, x, y, field, N, M, link, w0, w1, kl_weight, e, m, lam):
    """(H [d + 1, d + 1], b [d + 1], b_data [d + 1], SB' [d + 1]) of entity e from its dense row set under the prior:
    H = kl diag(lam) + prec sum_j w_j (u_j u_j^T + diag(0, A_j)), b = b_data + kl lam m, b_data = prec sum_j w_j t_j u_j."""
    m, lam = _prior(m, lam)
    ids, u, A, cm, cv = IR._partners(ent, bia, scal, field, N, M, link)
    w, t = IR.entity_rows(x, y, field, e, ids, w0, w1)
    prec = IR.link_t(scal[0], link)
    H = torch.diag(kl_weight * lam) + prec * (u.T @ (w[:, None] * u) + torch.diag((w[:, None] * A).sum(0)))
    b_data = prec * (u.T @ (w * (t - cm)))
    SB = (w[:, None] * (A + u * u)).sum(0)
    return H, b_data + kl_weight * lam * m, b_data, SB


def implicit_solve_fp64_prior(ent, bia, scal, x, y, field, N, M, link, w0, w1, kl_weight, m, lam, entities=None):
    """The block minimiser of every entity of `entities` (default: the field's whole range) under the prior:
    dict(ids [E], theta [E, d + 1], sigma [E, d + 1], cond [E] = cond_2(H))."""
    m, lam = _prior(m, lam)
    lo, hi = (0, N) if field == 0 else (N, N + M)
    ids = torch.arange(lo, hi) if entities is None else torch.as_tensor(entities, dtype=torch.int64)
    prec = IR.link_t(scal[0], link)
    th, sg, cond = [], [], []
    for e in ids.tolist():
        H, b, _, SB = system_fp64_prior(ent, bia, scal, x, y, field, N, M, link, w0, w1, kl_weight, e, m, lam)
        th.append(torch.linalg.solve(H, b))
        sg.append(torch.sqrt(kl_weight / (kl_weight * lam + prec * SB)))
        cond.append(torch.linalg.cond(H))
    return {"ids": ids, "theta": torch.stack(th), "sigma": torch.stack(sg), "cond": torch.stack(cond)}


def entity_loss_fp64_prior(ent, bia, scal, x, y, field, N, M, link, w0, w1, kl_weight, e, theta, sigma, m, lam):
    """L_e at (theta, sigma) [d + 1] under the prior, row by row over all partners."""
    m, lam = _prior(m, lam)
    ids, u, A, cm, cv = IR._partners(ent, bia, scal, field, N, M, link)
    w, t = IR.entity_rows(x, y, field, e, ids, w0, w1)
    prec = IR.link_t(scal[0], link)
    theta, sigma = theta.double(), sigma.double()
    res = t - cm - u @ theta
    var = cv + A @ (theta * theta) + (A + u * u) @ (sigma * sigma)
    rows = w * (0.5 * prec * (res * res + var) - 0.5 * torch.log(prec) + IR.LOG_2PI_HALF)
    return rows.sum() + kl_weight * kl_prior(theta, sigma, m, lam).sum()


def kl_all_prior(ent, bia, scal, N, M, link, mean, prec):
    """The KL of EVERY entity of both fields to its field's prior and of the global bias to N(0, 1) (differentiable in
    the tables and in the priors)."""
    d = ent.shape[1] // 2
    ent, bia, scal = ent.double(), bia.double(), scal.double()
    f = torch.cat([torch.zeros(N, dtype=torch.int64), torch.ones(M, dtype=torch.int64)])
    m, lam = mean.double()[f], prec.double()[f]                              # [T, d + 1]
    return (kl_prior(ent[:N + M, :d], IR.link_t(ent[:N + M, d:], link), m[:, 1:], lam[:, 1:]).sum()
            + kl_prior(bia[:N + M, 0], IR.link_t(bia[:N + M, 1], link), m[:, 0], lam[:, 0]).sum()
            + IR.kl_t(scal[1], IR.link_t(scal[2], link)))


def brute_J_prior(ent, bia, scal, x, y, N, M, link, w0, w1, kl_weight, mean, prec):
    """J_imp over the dense N x M grid under the priors (differentiable in the tables and the priors)."""
    Wgt, Y = IR.dense_targets(x, y, N, M, w0, w1)
    mm, v = IR.pair_moments(ent, bia, scal, N, M, link)
    pr = IR.link_t(scal[0], link)
    rows = Wgt * (0.5 * pr * ((Y - mm) ** 2 + v) - 0.5 * torch.log(pr) + IR.LOG_2PI_HALF)
    return rows.sum() + kl_weight * kl_all_prior(ent, bia, scal, N, M, link, mean, prec)


def gram_J_prior(ent, bia, scal, x, y, N, M, link, w0, w1, kl_weight, mean, prec):
    pr = IR.link_t(scal[0], link)
    W, _, S2 = IR.gram_sums(ent, bia, scal, x, y, N, M, link, w0, w1)
    return (0.5 * pr * S2 + W * (IR.LOG_2PI_HALF - 0.5 * torch.log(pr))
            + kl_weight * kl_all_prior(ent, bia, scal, N, M, link, mean, prec))


def prior_block_fp64(ent, bia, field, N, M, link, m_old, learn_mean=True, prec_min=1e-4, prec_max=1e4):
    """The prior block of `field` over its WHOLE id range (an entity without observed rows is in J_imp): m* = mean_e mu
    (learn_mean; else m_old), 1 / lam* = mean_e (sigma^2 + (mu - m*)^2), lam* clamped.  Returns (m* [d + 1],
    lam* clamped [d + 1], lam* unclamped [d + 1])."""
    ent, bia = ent.double(), bia.double()
    d = ent.shape[1] // 2
    lo, hi = (0, N) if field == 0 else (N, N + M)
    mu = torch.cat([bia[lo:hi, :1], ent[lo:hi, :d]], 1)
    sg = IR.link_t(torch.cat([bia[lo:hi, 1:], ent[lo:hi, d:]], 1), link)
    m = mu.mean(0) if learn_mean else torch.as_tensor(m_old).double()
    lam = 1.0 / (sg ** 2 + (mu - m) ** 2).mean(0)
    return m, lam.clamp(prec_min, prec_max), lam


def sweep_fp64_prior(ent, bia, scal, x, y, N, M, link, w0, w1, kl_weight, mean, prec, learn_priors=True, learn_mean=True,
                     prec_min=1e-4, prec_max=1e4, update_scalars=True, after=None):
    """One hierarchical implicit sweep on fp64 tables: field 0, prior 0, field 1, prior 1, the global bias, the
    precision.  after(what, ent, bia, scal, mean, prec) follows every block; what: 0, ("prior", 0), 1, ("prior", 1),
    "bias", "precision"."""
    ent, bia, scal = ent.double(), bia.double(), scal.double()
    mean, prec = mean.double().clone(), prec.double().clone()
    for f in (0, 1):
        sol = implicit_solve_fp64_prior(ent, bia, scal, x, y, f, N, M, link, w0, w1, kl_weight, mean[f], prec[f])
        ent, bia = IR.write_solution(ent, bia, sol, link)
        if after:
            after(f, ent, bia, scal, mean, prec)
        if learn_priors:
            mean[f], prec[f], _ = prior_block_fp64(ent, bia, f, N, M, link, mean[f], learn_mean, prec_min, prec_max)
            if after:
                after(("prior", f), ent, bia, scal, mean, prec)
    if update_scalars:
        scal = IR.bias_block_fp64(ent, bia, scal, x, y, N, M, link, w0, w1, kl_weight)
        if after:
            after("bias", ent, bia, scal, mean, prec)
        scal = IR.precision_block_fp64(ent, bia, scal, x, y, N, M, link, w0, w1)
        if after:
            after("precision", ent, bia, scal, mean, prec)
    return ent, bia, scal, mean, prec


def standard(d):
    return P.standard(2, d)

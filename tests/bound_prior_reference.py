"""fp64 restatement of the hierarchical bound sweeps (DESIGN.md §4 "Hierarchical bound sweeps";
include/vfm_bound_prior.h) for tests/test_fit_bound_priors_cpu.py and tests/test_gpu_fit_bound_priors.py: the bound
rounds of one entity under a field prior N(m_c, 1 / lam_c) (bound_reference.bound_rounds_fp64 with the three changed
lines and the prior start), B_e and J with the KL to that prior, one round's system in the split association, and the
sweep loop with prior_reference.prior_block_fp64 behind every field.  CPU tensors only.  A prior is the pair
(m [d + 1], lam [d + 1]), coordinate 0 the first-order weight; the priors of a model are (mean [F, d + 1],
prec [F, d + 1])."""
import numpy as np
import torch

import bound_reference as BR
import bound_sweep_restatement as BS
import fit_exact_restatement as FR
import prior_reference as PR
import solve_reference as R
from test_foldin_cpu import kl_t, link_t


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))


def kl_prior_sum_t(theta, sig2, m, lam):
    """sum_c KL(N(theta_c, sig2_c) || N(m_c, 1 / lam_c)), written so that at m = 0, lam = 1 every operation is
    bound_reference.kl_t's."""
    return (0.5 * (lam * sig2 + lam * (theta - m) * (theta - m) - 1.0) - 0.5 * torch.log(lam * sig2)).sum()


def bound_objective_t_prior(o, kl, theta, sigma, m, lam, xi=None):
    """bound_reference.bound_objective_t with the KL to N(m, 1 / lam): B_e(theta, sigma; xi), or with xi=None the
    collapsed B_e(theta, sigma).  torch fp64, autograd."""
    sig2 = sigma * sigma
    Ef, Vf = BR.moments_t(o, theta, sig2)
    if xi is None:
        x = torch.sqrt(Ef * Ef + Vf)
        rows = -(o["y"] - 0.5) * Ef + 0.5 * x + torch.log1p(torch.exp(-x))
    else:
        w = torch.from_numpy(BR.jj_weight(xi.numpy()))
        rows = -(o["y"] - 0.5) * Ef + 0.5 * w * (Ef * Ef + Vf - xi * xi) + 0.5 * xi + torch.log1p(torch.exp(-xi))
    return rows.sum() + kl * kl_prior_sum_t(theta, sig2, m, lam)


def bound_objective_fp64_prior(ent, bia, scal, x, y, field, link, kl_weight, entity, theta, s, m, lam):
    """The collapsed B_e of one entity under the prior at the means theta [d + 1] = (mu_w, mu) and the STORED scales
    s [d + 1] = (s_w, s), in fp64 (the arguments may be the fp32 values a kernel wrote)."""
    o = BR.entity_operands(ent, bia, scal, x, y, field, link, entity)
    th = _t(R._np(theta))
    sg = torch.from_numpy(R._link64(np.asarray(R._np(s), np.float64), link))
    return float(bound_objective_t_prior(o, R.f32(kl_weight), th, sg, _t(m), _t(lam)))


def bound_rounds_fp64_prior(ent, bia, scal, x, y, field, link, kl_weight, entity, n_iters, m, lam, reset=False,
                            start=None, form=None):
    """bound_reference.bound_rounds_fp64 under the prior N(m, 1 / lam): the start with reset is theta = m,
    sig2 = 1 / lam; D = kl lam + (0, sum w A); b += kl lam m; sig2 = kl / (kl lam + sum w (A + M^2)); B carries the KL to
    the prior.  The same dict, cond included."""
    o = BR.entity_operands(ent, bia, scal, x, y, field, link, entity)
    n, d = o["n"], o["d"]
    M, A, Cc, cm, cv, yr = (o[k].numpy() for k in ("M", "A", "C", "cm", "cv", "y"))
    m, lam = np.asarray(R._np(m), np.float64), np.asarray(R._np(lam), np.float64)
    mt, lt = _t(m), _t(lam)
    kl = R.f32(kl_weight)
    if start is not None:
        theta, sig2 = (np.array(v, np.float64) for v in start)
    elif reset:
        theta, sig2 = m.copy(), 1.0 / lam
    else:
        theta, sig2 = BR.table_start(ent, bia, link, entity)
    U = np.concatenate([np.ones((n, 1)), M], 1)
    B_of = lambda th, s2: float(bound_objective_t_prior(o, kl, torch.from_numpy(th), torch.from_numpy(np.sqrt(s2)), mt, lt))
    out = dict(n=n, d=d, theta=[], sig2=[], s=[], xi=[], w=[], cond=[], B=[], B_start=B_of(theta, sig2))
    dual = n <= d if form is None else form == "dual"
    for _ in range(n_iters):
        mu = theta[1:]
        Ef = cm + theta[0] + M @ mu
        Vf = cv + sig2[0] + (mu * mu * A + sig2[1:] * (A + M * M) + mu * Cc).sum(1)
        xi = np.sqrt(np.maximum(Ef * Ef + Vf, 0.0))
        w = BR.jj_weight(xi)
        D = kl * lam + np.concatenate([[0.0], (w[:, None] * A).sum(0)])
        b = U.T @ ((yr - 0.5) - w * cm) - np.concatenate([[0.0], 0.5 * (w[:, None] * Cc).sum(0)]) + kl * lam * m
        if dual:
            v = b / D
            K = np.diag(1.0 / w) + (U / D) @ U.T
            theta = v - (U.T @ np.linalg.solve(K, U @ v)) / D if n else v
            cond = float(np.linalg.cond(K)) if n else 1.0
        else:
            H = np.diag(D) + U.T @ (w[:, None] * U)
            theta = np.linalg.solve(H, b)
            cond = float(np.linalg.cond(H))
        sig2 = kl / (kl * lam + np.concatenate([[w.sum()], (w[:, None] * (A + M * M)).sum(0)]))
        out["theta"].append(theta)
        out["sig2"].append(sig2)
        out["s"].append(BR.unlink64(np.sqrt(sig2), link))
        out["xi"].append(xi)
        out["w"].append(w)
        out["cond"].append(cond)
        out["B"].append(B_of(theta, sig2))
    for k in ("theta", "sig2", "s", "xi", "w", "cond", "B"):
        out[k] = np.array(out[k])
    return out


def case_rounds_prior(c, k, n_iters, reset, m, lam):
    """bound_rounds_fp64_prior of entity number k of a bound_reference case."""
    return bound_rounds_fp64_prior(c["ent"], c["bia"], c["scal"], c["X"], c["y"], c["field"], c["link"], c["kl_weight"],
                                   int(c["ids"][k]), n_iters, m, lam, reset)


def chunked_round_fp64_prior(ent, bia, scal, x, y, field, link, kl_weight, entity, theta, sig2, chunk_rows, m, lam):
    """(H, b, SB) of one round in the split association (bound_sweep_restatement.chunked_round_fp64: the prior enters
    k_bsplit_solve alone, after the chunks' shares are added): H = T + diag(kl lam + SA), b = sum (..) u - (0, SC / 2) +
    kl lam m."""
    H, b, SB = BS.chunked_round_fp64(ent, bia, scal, x, y, field, link, kl_weight, entity, theta, sig2, chunk_rows)
    kl = R.f32(kl_weight)
    m, lam = np.asarray(R._np(m), np.float64), np.asarray(R._np(lam), np.float64)
    return H + np.diag(kl * lam - kl), b + kl * lam * m, SB


def objective_J_prior(ent, bia, scal, x, y, sizes, link, kl_weight, mean, prec):
    """bound_sweep_restatement.objective_J with every entity's KL to its field's prior (prior_reference.kl_prior_t); the
    global bias keeps N(0, 1).  torch fp64."""
    ent, bia, scal = ent.double(), bia.double(), scal.double()
    d = ent.shape[1] // 2
    Ep, Vp = FR.moments_fp64(ent, bia, scal, x, link)
    xi = BS.xi_of(Ep, Vp)
    J = (-(y.double() - 0.5) * Ep + 0.5 * xi + torch.log1p(torch.exp(-xi))).sum()
    seen = torch.unique(x)
    f = PR.field_of(sizes, seen)
    mu = torch.cat([bia[seen, :1], ent[seen, :d]], 1)
    sg = link_t(torch.cat([bia[seen, 1:], ent[seen, d:]], 1), link)
    kl = PR.kl_prior_t(mu, sg, mean.double()[f], prec.double()[f]).sum() + kl_t(scal[1], link_t(scal[2], link))
    return J + kl_weight * kl


def field_block_fp64_prior(ent, bia, scal, x, y, field, link, kl_weight, n_iters, m, lam):
    """bound_sweep_restatement.field_block_fp64 under the field's prior."""
    ent1, bia1 = ent.double().clone(), bia.double().clone()
    d = ent.shape[1] // 2
    rounds = {}
    for e in torch.unique(x[:, field]).tolist():
        r = bound_rounds_fp64_prior(ent, bia, scal, x, y, field, link, kl_weight, e, n_iters, m, lam, False)
        ent1[e, :d] = torch.from_numpy(r["theta"][-1][1:])
        ent1[e, d:] = torch.from_numpy(r["s"][-1][1:])
        bia1[e, 0], bia1[e, 1] = float(r["theta"][-1][0]), float(r["s"][-1][0])
        rounds[e] = r
    return ent1, bia1, rounds


def fit_bound_fp64_prior(ent, bia, scal, x, y, sizes, link, kl_weight, mean, prec, n_sweeps=3, n_iters=8,
                         learn_priors=True, learn_mean=True, prec_min=1e-4, prec_max=1e4, update_bias=True, after=None):
    """fit_bound's loop with priors: per field its block under (mean[f], prec[f]), then (learn_priors) the prior block
    prior_reference.prior_block_fp64 from the block's rows rounded to fp32 (the tables the device reads), the result
    rounded to fp32 as it is stored; after every sweep the bias block.  after(sweep, what, before, unrounded), both
    (ent, bia, scal, mean, prec), follows every block.  Returns the final fp32-valued (ent, bia, scal, mean, prec)."""
    r32 = BS.round32
    ent, bia, scal = r32(ent), r32(bia), r32(scal)
    mean, prec = r32(mean.double()).clone(), r32(prec.double()).clone()
    for sweep in range(n_sweeps):
        for f in range(x.shape[1]):
            e1, b1, _ = field_block_fp64_prior(ent, bia, scal, x, y, f, link, kl_weight, n_iters, mean[f], prec[f])
            if after:
                after(sweep, f, (ent, bia, scal, mean, prec), (e1, b1, scal, mean, prec))
            ent, bia = r32(e1), r32(b1)
            if learn_priors:
                m1, p1 = mean.clone(), prec.clone()
                m1[f], p1[f], _ = PR.prior_block_fp64(ent, bia, x, f, link, mean[f], learn_mean, prec_min, prec_max)
                if after:
                    after(sweep, ("prior", f), (ent, bia, scal, mean, prec), (ent, bia, scal, m1, p1))
                mean, prec = r32(m1), r32(p1)
        if update_bias:
            s1 = scal.clone()
            s1[1], s1[2], _ = BS.global_bias_fp64(ent, bia, scal, x, y, link, kl_weight)
            if after:
                after(sweep, "bias", (ent, bia, scal, mean, prec), (ent, bia, s1, mean, prec))
            scal = r32(s1)
    return ent, bia, scal, mean, prec


# ---------------------------------------------------------------------------------------------------------------------
# the priors of the GPU cases
# ---------------------------------------------------------------------------------------------------------------------
def case_priors(F, d):
    """(mean [F, d + 1], prec [F, d + 1]) of the unsplit, split and placement cases at embedding size d: means in
    [-0.5, 0.5] (the start theta = m is not zero), precisions log-uniform in [0.25, 16]."""
    return PR.draw_priors(F, d, 11 + d)

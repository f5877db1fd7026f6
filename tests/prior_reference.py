"""fp64 restatement of the hierarchical sweeps (DESIGN.md §4 "Hierarchical sweeps"; include/vfm_prior.h) for
tests/test_fit_priors_cpu.py and tests/test_gpu_fit_priors.py: the entity block under a field prior N(m_c, 1 / lam_c)
(solve_fp64_prior, written out from the block's formulas, not a call of solve_fp64), the prior block, the objective J and
the sweep.  CPU tensors only.  A prior is the pair (m [d + 1], lam [d + 1]), coordinate 0 the first-order weight; the
priors of a model are (mean [F, d + 1], prec [F, d + 1])."""
import numpy as np
import torch

import solve_reference as R
from test_foldin_cpu import kl_t, link_t, objective_fp64


def inv_link_t(v, link):
    return v if link == "abs" else torch.log(torch.expm1(v))


def kl_prior_t(mu, sg, m, lam):
    """KL(N(mu, sg^2) || N(m, 1 / lam)) = 1/2 (lam sg^2 + lam (mu - m)^2 - 1 - log(lam sg^2))."""
    return 0.5 * (lam * sg * sg + lam * (mu - m) ** 2 - 1.0 - torch.log(lam * sg * sg))


def standard(F, d):
    return torch.zeros(F, d + 1, dtype=torch.float64), torch.ones(F, d + 1, dtype=torch.float64)


def draw_priors(F, d, seed, prec_lo=0.25):
    """Non-trivial priors: means uniform in [-0.5, 0.5], precisions log-uniform in [prec_lo, 16] (prec_lo >= 0.25), as
    fp32 values (the tables the kernels read) held in fp64."""
    assert 0.25 <= prec_lo < 16.0
    g = torch.Generator().manual_seed(seed)
    mean = torch.rand(F, d + 1, generator=g, dtype=torch.float64) - 0.5
    prec = torch.exp(torch.rand(F, d + 1, generator=g, dtype=torch.float64) * np.log(16.0 / prec_lo) + np.log(prec_lo))
    return mean.float().double(), prec.float().clamp(prec_lo, 16.0).double()


def prec_lo_for(d):
    """The lower end of the precisions drawn for embedding size d, so that every factored matrix of the GPU cases stays
    under the condition number 78.4: an entity with n rows near d has cond(K) of about 1 + prec n / (kl lam) (the
    rank-one term of the first-order weight alone gives that), which at n = 137, prec = 1.3, kl = 0.7 needs lam >= 3.3
    and with the factors' own spectrum (as large again) and F = 3 (twice the partners' M^2) four times that.  d < 128: the
    whole range [0.25, 16]; d >= 128: [12, 16]."""
    return 0.25 if d < 128 else 12.0


def _operands(ent, bia, scal, x, field, link):
    """M, A, C [R, d] and c_mean [R] of every row from the frozen fields, fp64."""
    d = ent.shape[1] // 2
    Q = [f for f in range(x.shape[1]) if f != field]
    z = torch.zeros(1, x.shape[0], d, dtype=torch.float64)
    mq = torch.stack([ent[x[:, q], :d] for q in Q]) if Q else z
    sq2 = torch.stack([link_t(ent[x[:, q], d:], link) for q in Q]) ** 2 if Q else z
    M, A = mq.sum(0), sq2.sum(0)
    C = 2.0 * (sq2 * (M[None] - mq)).sum(0)
    cm = scal[1] + sum(bia[x[:, q], 0] for q in Q) + 0.5 * (M ** 2 - (mq ** 2).sum(0)).sum(1)
    return M, A, C, cm


def solve_fp64_prior(ent, bia, scal, x, y, field, link, kl_weight, m, lam, form="primal", entities=None):
    """The entity block: for every entity e of x[:, field] (or of `entities`: one without rows gets the prior row)
        D_c = kl lam_c + prec SA_c,  b_c = prec (bM_c - SC_c / 2) + kl lam_c m_c,  H = prec T + diag(D),  H theta = b,
        sigma_c^2 = kl / (kl lam_c + prec SB_c),
    with T = sum_r u_r u_r^T, u_r = (1, M_r), SA = (0, sum_r A_r), SB = (n, sum_r (A_r + M_r^2)), SC = (0, sum_r C_r),
    bM = sum_r t_r u_r, t_r = y_r - c_mean,r.  form "dual": the same theta through the n x n system
    K = I / prec + U D^-1 U^T.  Returns dict(entities, mu [E, d], s [E, d], mu_w [E], s_w [E], cond [E] = the condition
    number of the matrix the kernel factors: K for n <= d, else H)."""
    ent, bia, scal, y = ent.double(), bia.double(), scal.double(), y.double()
    m, lam = torch.as_tensor(m).double(), torch.as_tensor(lam).double()
    d = ent.shape[1] // 2
    kl = float(kl_weight)
    prec = link_t(scal[0], link)
    M, A, C, cm = _operands(ent, bia, scal, x, field, link)
    ents = torch.unique(x[:, field]) if entities is None else torch.as_tensor(entities)
    out = dict(entities=ents, mu=[], s=[], mu_w=[], s_w=[], cond=[])
    z1 = torch.zeros(1, dtype=torch.float64)
    for e in ents.tolist():
        r = x[:, field] == e
        n = int(r.sum())
        U = torch.cat([torch.ones(n, 1, dtype=torch.float64), M[r]], 1)
        t = y[r] - cm[r]
        SA = torch.cat([z1, A[r].sum(0)])
        SB = torch.cat([z1 + n, (A[r] + M[r] ** 2).sum(0)])
        SC = torch.cat([z1, C[r].sum(0)])
        D = kl * lam + prec * SA
        b = prec * (U.T @ t - 0.5 * SC) + kl * lam * m
        H = prec * (U.T @ U) + torch.diag(D)
        K = torch.eye(n, dtype=torch.float64) / prec + (U / D) @ U.T
        if form == "primal":
            theta = torch.linalg.solve(H, b)
        else:
            v = b / D
            theta = v - (U.T @ torch.linalg.solve(K, U @ v)) / D if n else v
        s = inv_link_t(torch.sqrt(kl / (kl * lam + prec * SB)), link)
        out["mu_w"].append(theta[0])
        out["mu"].append(theta[1:])
        out["s_w"].append(s[0])
        out["s"].append(s[1:])
        out["cond"].append(torch.linalg.cond(K) if 0 < n <= d else torch.linalg.cond(H))
    for k in ("mu", "s", "mu_w", "s_w", "cond"):
        out[k] = torch.stack(out[k]) if out[k] else torch.zeros(0, dtype=torch.float64)
    return out


def entity_objective_prior(ent, bia, scal, x, y, field, theta, link, kl_weight, m, lam):
    """L_e [E] under the prior: the rows' expected nll of objective_fp64 plus kl_weight KL to N(m, 1 / lam)."""
    ents, mu, s, mw, sw = theta
    m, lam = torch.as_tensor(m).double(), torch.as_tensor(lam).double()
    nll = objective_fp64(ent, bia, scal, x, y, field, theta, link, "reg", "closed_form", None, 0.0)
    kl = kl_prior_t(mu, link_t(s, link), m[1:], lam[1:]).sum(1) + kl_prior_t(mw, link_t(sw, link), m[0], lam[0])
    return nll + float(kl_weight) * kl


def field_of(sizes, ids):
    edges = torch.tensor(np.cumsum(sizes)[:-1].tolist(), dtype=torch.int64)
    return torch.bucketize(ids, edges, right=True)


def objective_J_prior(ent, bia, scal, x, y, sizes, link, kl_weight, mean, prec):
    """J: the rows' expected nll, kl_weight times the KL of every entity that occurs in x to its field's prior, and
    kl_weight times the KL of the global bias to N(0, 1)."""
    ent, bia, scal = ent.double(), bia.double(), scal.double()
    d = ent.shape[1] // 2
    e0 = torch.unique(x[:, 0])
    theta = (e0, ent[e0, :d], ent[e0, d:], bia[e0, 0], bia[e0, 1])
    J = objective_fp64(ent, bia, scal, x, y, 0, theta, link, "reg", "closed_form", None, 0.0).sum()
    seen = torch.unique(x)
    f = field_of(sizes, seen)
    mu = torch.cat([bia[seen, :1], ent[seen, :d]], 1)
    sg = link_t(torch.cat([bia[seen, 1:], ent[seen, d:]], 1), link)
    kl = kl_prior_t(mu, sg, mean.double()[f], prec.double()[f]).sum() + kl_t(scal[1], link_t(scal[2], link))
    return J + float(kl_weight) * kl


def prior_block_fp64(ent, bia, x, field, link, m_old, learn_mean=True, prec_min=1e-4, prec_max=1e4):
    """The prior block of (field, c) over the entities of the field that occur in x: m* = mean_e mu (learn_mean; else
    m_old), 1 / lam* = mean_e (s^2 + (mu - m*)^2), lam* clamped.  Returns (m* [d + 1], lam* clamped [d + 1],
    lam* unclamped [d + 1])."""
    ent, bia = ent.double(), bia.double()
    d = ent.shape[1] // 2
    e = torch.unique(x[:, field])
    mu = torch.cat([bia[e, :1], ent[e, :d]], 1)
    sg = link_t(torch.cat([bia[e, 1:], ent[e, d:]], 1), link)
    m = mu.mean(0) if learn_mean else torch.as_tensor(m_old).double()
    lam = 1.0 / (sg ** 2 + (mu - m) ** 2).mean(0)
    return m, lam.clamp(prec_min, prec_max), lam


def write_block(ent, bia, sol):
    ent, bia = ent.double().clone(), bia.double().clone()
    e = sol["entities"]
    ent[e] = torch.cat([sol["mu"], sol["s"]], 1)
    bia[e] = torch.stack([sol["mu_w"], sol["s_w"]], 1)
    return ent, bia


def sweep_fp64_prior(ent, bia, scal, x, y, sizes, link, kl_weight, mean, prec, learn_priors=True, learn_mean=True,
                     prec_min=1e-4, prec_max=1e4, update_scalars=True, after=None):
    """One hierarchical sweep on fp64 tables: per field its entity block, then (learn_priors) its prior block; then the
    global bias and the precision (fit_exact_restatement.scalars_block_fp64: they do not depend on the priors).
    after(what, ent, bia, scal, mean, prec) follows every block."""
    import fit_exact_restatement as FR
    ent, bia, scal = ent.double(), bia.double(), scal.double()
    mean, prec = mean.double().clone(), prec.double().clone()
    for f in range(x.shape[1]):
        ent, bia = write_block(ent, bia, solve_fp64_prior(ent, bia, scal, x, y, f, link, kl_weight, mean[f], prec[f]))
        if after:
            after(f, ent, bia, scal, mean, prec)
        if learn_priors:
            mean[f], prec[f], _ = prior_block_fp64(ent, bia, x, f, link, mean[f], learn_mean, prec_min, prec_max)
            if after:
                after(("prior", f), ent, bia, scal, mean, prec)
    if update_scalars:
        scal = FR.scalars_block_fp64(ent, bia, scal, x, y, link, kl_weight)
        if after:
            after("scalars", ent, bia, scal, mean, prec)
    return ent, bia, scal, mean, prec


def cond_of_the_factored_prior(ent, bia, scal, x, y, field, link, kl_weight, entity, m, lam):
    """cond of the matrix the kernel factors for this entity under the prior, from the fp32 tables in numpy fp64 (the
    pieces of solve_reference.system64 with D = kl lam + prec SA)."""
    s = R.system64(ent, bia, scal, x, y, field, link, kl_weight, entity)
    n, d, prec = s["n"], s["d"], s["prec"]
    D = s["kl"] * np.asarray(lam, np.float64) + (s["D"] - s["kl"])
    U = np.concatenate([np.ones((n, 1)), s["M"]], 1)
    if 0 < n <= d:
        return float(np.linalg.cond(np.eye(n) / prec + (U / D) @ U.T))
    return float(np.linalg.cond(np.diag(D) + prec * (U.T @ U)))

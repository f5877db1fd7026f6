"""fp64 restatement of VFM.fit_exact (vae_amd/sweep.py, DESIGN.md §4 "Exact sweeps") for tests/test_fit_exact_cpu.py and
tests/test_gpu_fit_exact.py: the objective J from objective_fp64's expressions, the scalars' block minimisers, one sweep
from solve_fp64 per field, and the chunk-wise assembly of one entity's system.  CPU tensors only."""
import numpy as np
import torch

import solve_reference as R
from test_foldin_cpu import LOG_2PI_HALF, kl_t, link_t, objective_fp64
from test_foldin_exact_cpu import solve_fp64


def inv_link_t(v, link):
    return v if link == "abs" else torch.log(torch.expm1(v))


def objective_J(ent, bia, scal, x, y, link="abs", kl_weight=1.0):
    """J: sum_e L_e of objective_fp64 over field 0's entities (the rows' expected nll and those entities' KL), the KL of
    the entities of the other fields that occur in x, and the KL of the global bias."""
    ent, bia, scal = ent.double(), bia.double(), scal.double()
    d = ent.shape[1] // 2
    e0 = torch.unique(x[:, 0])
    theta = (e0, ent[e0, :d], ent[e0, d:], bia[e0, 0], bia[e0, 1])
    J = objective_fp64(ent, bia, scal, x, y, 0, theta, link, "reg", "closed_form", None, kl_weight).sum()
    if x.shape[1] > 1:
        o = torch.unique(x[:, 1:])
        J = J + kl_weight * (kl_t(ent[o, :d], link_t(ent[o, d:], link)).sum() + kl_t(bia[o, 0], link_t(bia[o, 1], link)).sum())
    return J + kl_weight * kl_t(scal[1], link_t(scal[2], link))


def moments_fp64(ent, bia, scal, x, link="abs"):
    """(E pred [R], Var pred [R]) over every random variable of each row: objective_fp64's closed form with no field
    singled out."""
    ent, bia, scal = ent.double(), bia.double(), scal.double()
    d = ent.shape[1] // 2
    F = x.shape[1]
    mq = torch.stack([ent[x[:, q], :d] for q in range(F)])
    sq2 = torch.stack([link_t(ent[x[:, q], d:], link) for q in range(F)]) ** 2
    M, A = mq.sum(0), sq2.sum(0)
    pm = 0.5 * (M ** 2 - (mq ** 2).sum(0)).sum(1)
    pv = (0.5 * (A ** 2 - (sq2 ** 2).sum(0)) + (sq2 * (M[None] - mq) ** 2).sum(0)).sum(1)
    Ep = scal[1] + sum(bia[x[:, q], 0] for q in range(F)) + pm
    Vp = link_t(scal[2], link) ** 2 + sum(link_t(bia[x[:, q], 1], link) ** 2 for q in range(F)) + pv
    return Ep, Vp


def global_bias_fp64(ent, bia, scal, x, y, link="abs", kl_weight=1.0):
    """(m0*, s0*): the joint minimiser of J over the global bias, s0* through the link's inverse."""
    scal = scal.double()
    prec, n = link_t(scal[0], link), x.shape[0]
    Ep, _ = moments_fp64(ent, bia, scal, x, link)
    den = kl_weight + prec * n
    m0 = prec * (y.double() - (Ep - scal[1])).sum() / den
    return m0, inv_link_t(torch.sqrt(kl_weight / den), link)


def precision_fp64(ent, bia, scal, x, y, link="abs"):
    """alpha* = link^-1(N / sum_r ((y_r - E pred_r)^2 + Var pred_r))."""
    Ep, Vp = moments_fp64(ent, bia, scal, x, link)
    return inv_link_t(x.shape[0] / ((y.double() - Ep) ** 2 + Vp).sum(), link)


def field_block_fp64(ent, bia, scal, x, y, field, link="abs", kl_weight=1.0):
    """Field `field`'s block: solve_fp64 over all rows.  Returns (ent, bia) with the solved rows written, and sol."""
    sol = solve_fp64(ent, bia, scal, x, y, field, link, kl_weight)
    ent, bia = ent.double().clone(), bia.double().clone()
    e = sol["entities"]
    ent[e] = torch.cat([sol["mu"], sol["s"]], 1)
    bia[e] = torch.stack([sol["mu_w"], sol["s_w"]], 1)
    return ent, bia, sol


def scalars_block_fp64(ent, bia, scal, x, y, link="abs", kl_weight=1.0):
    """The scalars' block in fit_exact's order: the global bias, then the precision at the new bias."""
    scal = scal.double().clone()
    m0, s0 = global_bias_fp64(ent, bia, scal, x, y, link, kl_weight)
    scal[1], scal[2] = m0, s0
    scal[0] = precision_fp64(ent, bia, scal, x, y, link)
    return scal


def sweep_fp64(ent, bia, scal, x, y, link="abs", kl_weight=1.0, fields=None, update_scalars=True, after=None):
    """One sweep on fp64 tables; after(what, ent, bia, scal) is called after every block."""
    ent, bia, scal = ent.double(), bia.double(), scal.double()
    for f in (range(x.shape[1]) if fields is None else fields):
        ent, bia, _ = field_block_fp64(ent, bia, scal, x, y, f, link, kl_weight)
        if after:
            after(f, ent, bia, scal)
    if update_scalars:
        scal = scalars_block_fp64(ent, bia, scal, x, y, link, kl_weight)
        if after:
            after("scalars", ent, bia, scal)
    return ent, bia, scal


def system_fp64(ent, bia, scal, x, y, field, link, kl_weight, entity):
    """(H [d + 1, d + 1], b [d + 1]) of solve_fp64's primal form for one entity (numpy fp64, from the fp32 tables)."""
    s = R.system64(ent, bia, scal, x, y, field, link, kl_weight, entity)
    U = np.concatenate([np.ones((s["n"], 1)), s["M"]], 1)
    return np.diag(s["D"]) + s["prec"] * (U.T @ U), s["b"]


def chunked_system_fp64(ent, bia, scal, x, y, field, link, kl_weight, entity, chunk_rows):
    """The same system as k_split_assemble and k_split_solve form it: per chunk of chunk_rows rows, in row order, the
    shares T = sum u u^T, SA = sum A, sum t u and SC = sum C; the shares added in chunk order; H = prec T + diag(kl +
    prec SA), b = prec (sum t u - SC / 2)."""
    xr, yr = R.entity_rows(x, y, field, entity)
    M, A, Cc, cm = R.operands64(ent, bia, scal, xr, field, link)
    n, d = M.shape
    prec = float(R._link64(R._np(scal, np.float32)[0], link))
    kl = R.f32(kl_weight)
    T, SA, tu, SC = np.zeros((d + 1, d + 1)), np.zeros(d + 1), np.zeros(d + 1), np.zeros(d + 1)
    for r0 in range(0, n, chunk_rows):
        Tc, SAc, tuc, SCc = np.zeros((d + 1, d + 1)), np.zeros(d + 1), np.zeros(d + 1), np.zeros(d + 1)
        for i in range(r0, min(r0 + chunk_rows, n)):
            u = np.concatenate([[1.0], M[i]])
            Tc += np.outer(u, u)
            SAc[1:] += A[i]
            SCc[1:] += Cc[i]
            tuc += (yr[i] - cm[i]) * u
        T, SA, tu, SC = T + Tc, SA + SAc, tu + tuc, SC + SCc
    return prec * T + np.diag(kl + prec * SA), prec * (tu - 0.5 * SC)


def moment_error_bounds(ent, bia, scal, x, link="abs"):
    """(e_mean [R], e_var [R]): bounds on the error of an fp32 evaluation of (E pred, Var pred) from the fp32 tables, by
    the running-error rule: every one of at most n_ops roundings costs 2^-24 of a partial sum, and every partial sum of
    E pred is at most S = |m0| + sum_f |w_f| + sum_k (sum_f |m_fk|)^2, of Var pred at most V = sg0^2 + sum_f sigma_wf^2 +
    sum_k (A_k^2 + A_k (sum_f |m_fk|)^2).  n_ops: F (d + 2) additions of table values plus 3 (mean) or 8 (variance)
    operations per coordinate and 4 for the scalars."""
    ent, bia, scal = ent.double(), bia.double(), scal.double()
    d, F = ent.shape[1] // 2, x.shape[1]
    am = sum(ent[x[:, q], :d].abs() for q in range(F))
    A = sum(link_t(ent[x[:, q], d:], link) ** 2 for q in range(F))
    S = scal[1].abs() + sum(bia[x[:, q], 0].abs() for q in range(F)) + (am ** 2).sum(1)
    V = link_t(scal[2], link) ** 2 + sum(link_t(bia[x[:, q], 1], link) ** 2 for q in range(F)) + (A ** 2 + A * am ** 2).sum(1)
    return (F * (d + 2) + 3 * d + 4) * 2.0 ** -24 * S, (F * (d + 2) + 8 * d + 4) * 2.0 ** -24 * V


def scalar_abs_terms(ent, bia, scal, x, y, link="abs"):
    """Absolute terms for the scalars fit_exact writes from fp32 moments, at the tables (ent, bia, scal) the block read:
    (for m0: a weighted mean, weights summing to at most 1, of residuals each off by at most e_mean;  for alpha: the
    relative error of sum_r q_r, q = (y - E pred)^2 + Var pred, at most sum_r (2 |res_r| e_mean,r + e_mean,r^2 +
    e_var,r) / sum_r q_r, times prec, times the derivative of the link's inverse)."""
    em, ev = moment_error_bounds(ent, bia, scal, x, link)
    Ep, Vp = moments_fp64(ent, bia, scal, x, link)
    res = (y.double() - Ep).abs()
    q = (res ** 2 + Vp).sum()
    prec = x.shape[0] / q
    rel = float((2 * res * em + em ** 2 + ev).sum() / q)
    dinv = 1.0 if link == "abs" else float(1.0 / (1.0 - torch.exp(-prec)))
    return float(em.max()), float(prec) * rel * dinv

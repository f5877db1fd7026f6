"""fp64 references and case builders for the tests of the bound fold-in (include/vfm_bound.h, VFM.fold_in_bound):
tests/test_foldin_bound_cpu.py checks the references themselves and the conditions on the inputs, and
tests/test_gpu_foldin_bound.py runs the same cases on the kernel.

  jj_weight, jj_bound         w = 2 lambda(xi) (the series below 1e-3) and the Jaakkola-Jordan bound of one row
  c_var64                     c_var of the rows in fp64 from the fp32 tables (operands64 of solve_reference.py has the rest)
  entity_operands             everything one entity's problem needs, as torch fp64 tensors
  bound_objective_t           B_e(theta, sigma; xi) or, with xi=None, the collapsed B_e(theta, sigma): torch fp64, autograd
  bound_objective_fp64        the collapsed B_e of one entity at given parameters (stored scales), a float
  bound_rounds_fp64           n_iters rounds from the table row, the prior or a given start: theta, sigma^2, the stored
                              scales, xi, w, the factored matrix' condition number and B_e after every round
  bound_case, GPU_*           the cases of the GPU tests: CPU tensors only

No GPU is needed to import this module or to build a case."""
import math

import numpy as np
import torch

import solve_reference as R

SERIES_BELOW = 1e-3


def jj_weight(xi):
    """w = 2 lambda(xi) = tanh(xi / 2) / (2 xi); 1/4 - xi^2 / 48 below 1e-3."""
    xi = np.asarray(xi, np.float64)
    safe = np.where(xi < SERIES_BELOW, 1.0, xi)
    return np.where(xi < SERIES_BELOW, 0.25 - xi * xi / 48.0, np.tanh(0.5 * safe) / (2.0 * safe))


def jj_weight_tanh(xi):
    xi = np.asarray(xi, np.float64)
    return np.tanh(0.5 * xi) / (2.0 * xi)


def nll(y, f):
    """-y f + log(1 + e^f), stable."""
    f = np.asarray(f, np.float64)
    return -y * f + np.maximum(f, 0.0) + np.log1p(np.exp(-np.abs(f)))


def jj_bound(y, f, xi):
    """-(y - 1/2) f + xi / 2 + log(1 + e^-xi) + lambda(xi) (f^2 - xi^2)."""
    f, xi = np.asarray(f, np.float64), np.asarray(xi, np.float64)
    return -(y - 0.5) * f + 0.5 * xi + np.log1p(np.exp(-xi)) + 0.5 * jj_weight(xi) * (f * f - xi * xi)


def c_var64(ent, bia, scal, xr, field, link):
    """c_var [n] of the rows xr in fp64 from the fp32 tables: the global bias' and the partners' first-order variances
    and the variance of the partners' pair term (k_foldin_prep's sum with the links in fp64)."""
    ent, bia, scal = R._np(ent, np.float32), R._np(bia, np.float32), R._np(scal, np.float32)
    d = ent.shape[1] // 2
    Q = [f for f in range(xr.shape[1]) if f != field]
    n = xr.shape[0]
    cv = np.full(n, float(R._link64(scal[2], link)) ** 2)
    for f in Q:
        cv = cv + R._link64(bia[xr[:, f], 1], link) ** 2
    sm, ss, sss = np.zeros((n, d)), np.zeros((n, d)), np.zeros((n, d))
    for f in Q:
        m = ent[xr[:, f], :d].astype(np.float64)
        s2 = R._link64(ent[xr[:, f], d:], link) ** 2
        sm, ss, sss = sm + m, ss + s2, sss + s2 * s2
    lin = np.zeros((n, d))
    for f in Q:
        m = ent[xr[:, f], :d].astype(np.float64)
        s2 = R._link64(ent[xr[:, f], d:], link) ** 2
        lin = lin + s2 * (sm - m) ** 2
    for k in range(d):
        cv = cv + 0.5 * (ss[:, k] * ss[:, k] - sss[:, k]) + lin[:, k]
    return cv


def entity_operands(ent, bia, scal, x, y, field, link, entity):
    """dict(n, d, M, A, C [n, d], cm, cv, y [n]) of one entity's rows, torch fp64, the rows in the kernel's order."""
    xr, yr = R.entity_rows(x, y, field, entity)
    M, A, Cc, cm = R.operands64(ent, bia, scal, xr, field, link)
    cv = c_var64(ent, bia, scal, xr, field, link)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64))
    return dict(n=M.shape[0], d=M.shape[1], M=t(M), A=t(A), C=t(Cc), cm=t(cm), cv=t(cv), y=t(yr))


def moments_t(o, theta, sig2):
    """(E f [n], Var f [n]) at the means theta [d + 1] = (mu_w, mu) and the variances sig2 [d + 1]."""
    mu = theta[1:]
    Ef = o["cm"] + theta[0] + o["M"] @ mu
    Vf = o["cv"] + sig2[0] + (mu * mu * o["A"] + sig2[1:] * (o["A"] + o["M"] ** 2) + mu * o["C"]).sum(1)
    return Ef, Vf


def kl_t(theta, sig2):
    return (0.5 * (sig2 + theta * theta - 1.0) - 0.5 * torch.log(sig2)).sum()


def bound_objective_t(o, kl, theta, sigma, xi=None):
    """B_e in torch fp64.  xi [n]: B_e(theta, sigma; xi) of the header; None: xi at its optimum, the collapsed form."""
    sig2 = sigma * sigma
    Ef, Vf = moments_t(o, theta, sig2)
    if xi is None:
        x = torch.sqrt(Ef * Ef + Vf)
        rows = -(o["y"] - 0.5) * Ef + 0.5 * x + torch.log1p(torch.exp(-x))
    else:
        w = torch.from_numpy(jj_weight(xi.numpy()))
        rows = -(o["y"] - 0.5) * Ef + 0.5 * w * (Ef * Ef + Vf - xi * xi) + 0.5 * xi + torch.log1p(torch.exp(-xi))
    return rows.sum() + kl * kl_t(theta, sig2)


def unlink64(sigma, link):
    sigma = np.asarray(sigma, np.float64)
    return sigma if link == "abs" else np.log(np.expm1(sigma))


def bound_objective_fp64(ent, bia, scal, x, y, field, link, kl_weight, entity, theta, s):
    """The collapsed B_e of one entity at the means theta [d + 1] = (mu_w, mu) and the STORED scales s [d + 1] =
    (s_w, s), in fp64 (the arguments may be the fp32 values a kernel wrote)."""
    o = entity_operands(ent, bia, scal, x, y, field, link, entity)
    th = torch.from_numpy(np.asarray(R._np(theta), np.float64))
    sg = torch.from_numpy(R._link64(np.asarray(R._np(s), np.float64), link))
    return float(bound_objective_t(o, R.f32(kl_weight), th, sg))


def table_start(ent, bia, link, entity):
    """(theta [d + 1], sig2 [d + 1]) of the entity's current row in the fp32 tables."""
    ent, bia = R._np(ent, np.float32), R._np(bia, np.float32)
    d = ent.shape[1] // 2
    e = int(entity)
    theta = np.concatenate([[bia[e, 0]], ent[e, :d]]).astype(np.float64)
    sg = R._link64(np.concatenate([[bia[e, 1]], ent[e, d:]]), link)
    return theta, sg * sg


def bound_rounds_fp64(ent, bia, scal, x, y, field, link, kl_weight, entity, n_iters, reset=False, start=None, form=None):
    """n_iters rounds of the two block minimisers for one entity in numpy fp64.  The start: `start` = (theta, sig2), else
    the prior with reset, else the entity's row in the tables.  form: None = the kernel's rule (dual while n <= d),
    "dual" or "primal".  Returns dict(n, d, theta [n_iters, d + 1], sig2 [n_iters, d + 1], s [n_iters, d + 1] (stored
    scales), xi [n_iters, n], w [n_iters, n] (the xi block each round started from), cond [n_iters] of the matrix
    factored, B [n_iters] = the collapsed B_e after each round, B_start)."""
    o = entity_operands(ent, bia, scal, x, y, field, link, entity)
    n, d = o["n"], o["d"]
    M, A, Cc, cm, cv, yr = (o[k].numpy() for k in ("M", "A", "C", "cm", "cv", "y"))
    kl = R.f32(kl_weight)
    if start is not None:
        theta, sig2 = (np.array(v, np.float64) for v in start)
    elif reset:
        theta, sig2 = np.zeros(d + 1), np.ones(d + 1)
    else:
        theta, sig2 = table_start(ent, bia, link, entity)
    U = np.concatenate([np.ones((n, 1)), M], 1)
    out = dict(n=n, d=d, theta=[], sig2=[], s=[], xi=[], w=[], cond=[], B=[],
               B_start=float(bound_objective_t(o, kl, torch.from_numpy(theta), torch.from_numpy(np.sqrt(sig2)))))
    dual = n <= d if form is None else form == "dual"
    for _ in range(n_iters):
        mu = theta[1:]
        Ef = cm + theta[0] + M @ mu
        Vf = cv + sig2[0] + (mu * mu * A + sig2[1:] * (A + M * M) + mu * Cc).sum(1)
        xi = np.sqrt(np.maximum(Ef * Ef + Vf, 0.0))
        w = jj_weight(xi)
        D = kl + np.concatenate([[0.0], (w[:, None] * A).sum(0)])
        b = U.T @ ((yr - 0.5) - w * cm) - np.concatenate([[0.0], 0.5 * (w[:, None] * Cc).sum(0)])
        if dual:
            v = b / D
            K = np.diag(1.0 / w) + (U / D) @ U.T
            theta = v - (U.T @ np.linalg.solve(K, U @ v)) / D if n else v
            cond = float(np.linalg.cond(K)) if n else 1.0
        else:
            H = np.diag(D) + U.T @ (w[:, None] * U)
            theta = np.linalg.solve(H, b)
            cond = float(np.linalg.cond(H))
        sig2 = kl / (kl + np.concatenate([[w.sum()], (w[:, None] * (A + M * M)).sum(0)]))
        out["theta"].append(theta)
        out["sig2"].append(sig2)
        out["s"].append(unlink64(np.sqrt(sig2), link))
        out["xi"].append(xi)
        out["w"].append(w)
        out["cond"].append(cond)
        out["B"].append(float(bound_objective_t(o, kl, torch.from_numpy(theta), torch.from_numpy(np.sqrt(sig2)))))
    for k in ("theta", "sig2", "s", "xi", "w", "cond", "B"):
        out[k] = np.array(out[k])
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the cases of the GPU tests: solve_reference's builders (tables(scale=0.5)) with labels in {0, 1}
# ---------------------------------------------------------------------------------------------------------------------
def bound_case(sizes, field, d, link, counts, seed, kl_weight=1.0, **kw):
    """solve_reference.case with y drawn from {0, 1}; an entity whose number is in kw['all_equal'] answers 1 always."""
    all_equal = kw.pop("all_equal", ())
    c = R.case(sizes, field, d, link, counts, seed, kl_weight, **kw)
    g = torch.Generator().manual_seed(seed + 2)
    c["y"] = (torch.rand(c["X"].shape[0], generator=g) < 0.4).float()
    for k in all_equal:
        c["y"][c["X"][:, field] == int(c["ids"][k])] = 1.0
    return c


GPU_DS = (1, 8, 9, 33, 128)              # each W / CPL bucket edge of shape_of: W = 8 | 16 | 64 (CPL 1) | 64 (CPL 2)
GPU_ITERS = ((1, False), (1, True), (8, False), (8, True))       # (n_iters, reset)


def shape_counts(d):
    """n = 1, d - 1, d (the last dual), d + 1 (the first primal); the distinct positive ones."""
    return sorted({n for n in (1, d - 1, d, d + 1) if n >= 1})


def shape_case(d, link, F):
    sizes = (12, 40) if F == 2 else (12, 40, 25)
    return bound_case(sizes, 0, d, link, shape_counts(d), seed=100 + d + 7 * F + (link == "softplus"),
                      kl_weight=1.0 if F == 2 else 0.7)


def slab_case():
    """d = VFM_FOLDIN_SOLVE_LDS_DIM, n = d + 1: the primal system of d + 1 does not fit in LDS."""
    return bound_case((6, 300), 0, R.LDS, "abs", [R.LDS + 1], seed=211)


LDS_DIM_D = 5
LDS_DIMS = (-1, 0, 3)


def lds_dim_case():
    return bound_case((12, 40, 9), 0, LDS_DIM_D, "softplus", [1, 3, 4, 5, 6, 11], seed=223, kl_weight=0.7)


def bitwise_case():
    """2 SLABS + 37 entities at d = 5 (solve_reference.bitwise_counts), labels in {0, 1}."""
    return bound_case((2 * R.SLABS + 60, 30, 7), 0, R.BITWISE_D, "softplus", R.bitwise_counts(), seed=71, kl_weight=0.75)


def case_rounds(c, k, n_iters, reset):
    """bound_rounds_fp64 of entity number k of a case."""
    return bound_rounds_fp64(c["ent"], c["bia"], c["scal"], c["X"], c["y"], c["field"], c["link"], c["kl_weight"],
                             int(c["ids"][k]), n_iters, reset)

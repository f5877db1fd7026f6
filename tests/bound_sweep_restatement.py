"""fp64 restatement of VFM.fit_bound (vae_amd/sweep.py, DESIGN.md §4 "Bound sweeps") for tests/test_fit_bound_cpu.py and
tests/test_gpu_fit_bound.py: the objective J, the global bias' block minimiser under the bound, one field's block from
bound_reference.bound_rounds_fp64, the sweep loop, the chunk-wise assembly of one round's system, and the cases of the
split rounds.  CPU tensors only; no GPU is needed to import this module.

The tables between two blocks hold fp32 values, as on the device, where every block's rows are rounded to fp32 once: a
block reads fp32 tables (exactly representable in the fp64 tensors used here) and returns unrounded fp64 rows, and the
loop rounds them before the next block.  "A block does not increase J" is a statement about the unrounded rows."""
import numpy as np
import torch

import bound_reference as BR
import fit_exact_restatement as FR
import solve_reference as R
from test_foldin_cpu import kl_t, link_t

CHUNK = 8
SPLIT_DS = (1, 8, 9, 33, 128)
ITERS = ((1, False), (1, True), (8, False), (8, True))       # (n_iters, reset)


def xi_of(Ep, Vp):
    return torch.sqrt(torch.clamp(Ep * Ep + Vp, min=0.0))


def jj_weight_t(xi):
    return torch.from_numpy(BR.jj_weight(xi.detach().numpy()))


def objective_J(ent, bia, scal, x, y, link="abs", kl_weight=1.0):
    """J = sum_r [-(y_r - 1/2) E f_r + xi_r / 2 + log1p(e^-xi_r)] + kl (KL of every entity in x and of the global
    bias), xi_r = sqrt((E f_r)^2 + Var f_r), the moments over every random variable of the row.  torch fp64, autograd."""
    ent, bia, scal = ent.double(), bia.double(), scal.double()
    d = ent.shape[1] // 2
    Ep, Vp = FR.moments_fp64(ent, bia, scal, x, link)
    xi = xi_of(Ep, Vp)
    J = (-(y.double() - 0.5) * Ep + 0.5 * xi + torch.log1p(torch.exp(-xi))).sum()
    o = torch.unique(x)
    kl = kl_t(ent[o, :d], link_t(ent[o, d:], link)).sum() + kl_t(bia[o, 0], link_t(bia[o, 1], link)).sum()
    return J + kl_weight * (kl + kl_t(scal[1], link_t(scal[2], link)))


def bias_bound_t(ent, bia, scal, x, y, link, kl_weight, xi):
    """The bound at fixed xi as a function of the tables (autograd): for the gradient test of the bias block."""
    ent, bia, scal = ent.double(), bia.double(), scal.double()
    Ep, Vp = FR.moments_fp64(ent, bia, scal, x, link)
    w = jj_weight_t(xi)
    rows = -(y.double() - 0.5) * Ep + 0.5 * w * (Ep * Ep + Vp - xi * xi) + 0.5 * xi + torch.log1p(torch.exp(-xi))
    return rows.sum() + kl_weight * kl_t(scal[1], link_t(scal[2], link))


def global_bias_fp64(ent, bia, scal, x, y, link="abs", kl_weight=1.0):
    """(m0*, s0*, xi): the joint minimiser over the global bias of the bound at xi of the current posterior, s0* through
    the link's inverse."""
    scal = scal.double()
    Ep, Vp = FR.moments_fp64(ent, bia, scal, x, link)
    xi = xi_of(Ep, Vp)
    w = jj_weight_t(xi)
    den = kl_weight + w.sum()
    m0 = ((y.double() - 0.5) - w * (Ep - scal[1])).sum() / den
    return m0, FR.inv_link_t(torch.sqrt(kl_weight / den), link), xi


W_SLOPE = 1.0 / 23.0                     # |d w / d xi| <= 1 / 23 for every xi >= 0 (test_fit_bound_cpu.py checks a grid)


def bias_abs_terms(ent, bia, scal, x, y, link="abs", kl_weight=1.0):
    """Absolute terms (for m0, for the stored s0) of a bias block computed from fp32 moments, at the tables the block
    read.  With e_mean, e_var of fit_exact_restatement.moment_error_bounds: xi_r is off by at most dxi_r =
    (|E f_r| e_mean,r + e_var,r / 2) / xi_r + 2^-23 xi_r (xi_r >= sqrt(Var f_r) > 0), w_r by at most dw_r = dxi_r / 23.
    num = sum_r ((y_r - 1/2) - w_r rest_r) is off by at most sum_r (dw_r |rest_r| + w_r e_mean,r), den = kl + sum w by at
    most sum_r dw_r; m0 = num / den by at most dnum / den + |m0| dden / den; s0 = sqrt(kl / den) by at most
    s0 dden / (2 den), times the derivative of the link's inverse."""
    scal = scal.double()
    em, ev = FR.moment_error_bounds(ent, bia, scal, x, link)
    Ep, Vp = FR.moments_fp64(ent, bia, scal, x, link)
    xi = xi_of(Ep, Vp)
    dxi = (Ep.abs() * em + 0.5 * ev) / xi + 2.0 ** -23 * xi
    dw = W_SLOPE * dxi
    w = jj_weight_t(xi)
    den = kl_weight + w.sum()
    rest = Ep - scal[1]
    m0 = ((y.double() - 0.5) - w * rest).sum() / den
    t_m0 = float(((dw * rest.abs() + w * em).sum() + m0.abs() * dw.sum()) / den)
    s0 = float(torch.sqrt(kl_weight / den))
    dinv = 1.0 if link == "abs" else 1.0 / (1.0 - np.exp(-s0))
    return t_m0, float(0.5 * s0 * dw.sum() / den) * dinv


def field_block_fp64(ent, bia, scal, x, y, field, link="abs", kl_weight=1.0, n_iters=8):
    """Field `field`'s block: n_iters bound rounds of every entity of the column over all rows, from its current row.
    ent, bia: fp64 tensors holding fp32 values.  Returns (ent, bia) fp64 with the unrounded rows written, and per entity
    the bound_rounds_fp64 result."""
    ent1, bia1 = ent.double().clone(), bia.double().clone()
    d = ent.shape[1] // 2
    rounds = {}
    for e in torch.unique(x[:, field]).tolist():
        r = BR.bound_rounds_fp64(ent, bia, scal, x, y, field, link, kl_weight, e, n_iters, False)
        ent1[e, :d] = torch.from_numpy(r["theta"][-1][1:])
        ent1[e, d:] = torch.from_numpy(r["s"][-1][1:])
        bia1[e, 0], bia1[e, 1] = float(r["theta"][-1][0]), float(r["s"][-1][0])
        rounds[e] = r
    return ent1, bia1, rounds


def round32(t):
    return t.float().double()


def fit_bound_fp64(ent, bia, scal, x, y, link="abs", kl_weight=1.0, n_sweeps=3, n_iters=8, fields=None, update_bias=True,
                   after=None):
    """fit_bound's loop.  after(sweep, what, before = (ent, bia, scal), unrounded = (ent, bia, scal)) is called after
    every block with the fp32-valued tables the block read and the fp64 tables it produced; the next block reads the
    latter rounded to fp32.  Returns the final fp32-valued tables."""
    ent, bia, scal = round32(ent), round32(bia), round32(scal)
    for sweep in range(n_sweeps):
        for f in (range(x.shape[1]) if fields is None else fields):
            e1, b1, _ = field_block_fp64(ent, bia, scal, x, y, f, link, kl_weight, n_iters)
            if after:
                after(sweep, f, (ent, bia, scal), (e1, b1, scal))
            ent, bia = round32(e1), round32(b1)
        if update_bias:
            s1 = scal.clone()
            s1[1], s1[2], _ = global_bias_fp64(ent, bia, scal, x, y, link, kl_weight)
            if after:
                after(sweep, "bias", (ent, bia, scal), (ent, bia, s1))
            scal = round32(s1)
    return ent, bia, scal


def chunked_round_fp64(ent, bia, scal, x, y, field, link, kl_weight, entity, theta, sig2, chunk_rows):
    """(H, b, SB) of one round at the iterate (theta, sig2) as k_bsplit_assemble and k_bsplit_solve form them: per chunk
    of chunk_rows rows, in row order, the shares T = sum w u u^T, SA = sum w A, SB = sum w (A + M^2) (coordinate 0: sum
    w), sum ((y - 1/2) - w c_mean) u and SC = sum w C; the shares added in chunk order; H = T + diag(kl + SA),
    b = sum (..) u - (0, SC / 2)."""
    o = BR.entity_operands(ent, bia, scal, x, y, field, link, entity)
    n, d = o["n"], o["d"]
    M, A, Cc, cm, cv, yr = (o[k].numpy() for k in ("M", "A", "C", "cm", "cv", "y"))
    kl = R.f32(kl_weight)
    mu = theta[1:]
    Ef = cm + theta[0] + M @ mu
    Vf = cv + sig2[0] + (mu * mu * A + sig2[1:] * (A + M * M) + mu * Cc).sum(1)
    w = BR.jj_weight(np.sqrt(np.maximum(Ef * Ef + Vf, 0.0)))
    T, SA, SB, tu, SC = np.zeros((d + 1, d + 1)), np.zeros(d + 1), np.zeros(d + 1), np.zeros(d + 1), np.zeros(d + 1)
    for r0 in range(0, n, chunk_rows):
        Tc, SAc, SBc, tuc, SCc = (np.zeros((d + 1, d + 1)), np.zeros(d + 1), np.zeros(d + 1), np.zeros(d + 1),
                                  np.zeros(d + 1))
        for i in range(r0, min(r0 + chunk_rows, n)):
            u = np.concatenate([[1.0], M[i]])
            Tc += w[i] * np.outer(u, u)
            SAc[1:] += w[i] * A[i]
            SBc[1:] += w[i] * (A[i] + M[i] * M[i])
            SBc[0] += w[i]
            SCc[1:] += w[i] * Cc[i]
            tuc += ((yr[i] - 0.5) - w[i] * cm[i]) * u
        T, SA, SB, tu, SC = T + Tc, SA + SAc, SB + SBc, tu + tuc, SC + SCc
    return T + np.diag(kl + SA), tu - 0.5 * SC, SB


# ---------------------------------------------------------------------------------------------------------------------
# the cases of the split rounds (tests/test_gpu_fit_bound.py), CPU tensors only
# ---------------------------------------------------------------------------------------------------------------------
def split_counts(d):
    """d + 1 (at the threshold: not split), d + 2, around a chunk edge, 40 chunks, and one chunk where d allows."""
    k = d // CHUNK + 2
    c = [d + 1, d + 2, CHUNK * k - 1, CHUNK * k, CHUNK * k + 1, CHUNK * 40]
    return c + [CHUNK - 1] if d + 2 <= CHUNK - 1 else c


def split_sizes(F, n_ent):
    return (n_ent + 3, 60) if F == 2 else (n_ent + 3, 40, 7)


def split_case(d, link, F):
    counts = split_counts(d)
    return BR.bound_case(split_sizes(F, len(counts)), 0, d, link, counts, seed=300 + d + F,
                         kl_weight=0.7 if F == 3 else 1.0)


def placement_case(d, link):
    """The triangle in LDS (d = LDS - 1) and in the workgroup's slab (d = LDS)."""
    return BR.bound_case((6, 300), 0, d, link, [d + 2, CHUNK * (d // CHUNK + 2) + 1], seed=400 + d)


def mixed_case():
    """300 light entities of 3 .. 14 rows and two heavy ones (100 and 61 rows), d = 8, F = 3, softplus."""
    counts = [3 + g % 12 for g in range(300)]
    counts[17], counts[200] = 100, 61
    return BR.bound_case((320, 40, 7), 0, 8, "softplus", counts, seed=55, kl_weight=0.7)


def fit_case(F):
    """(sizes, X, y) of the fit_bound runs: 300 users x 12 items (x 3 formats), about 9 rows a user in item order;
    users 0 and 1 answer every item 5 times over (60 rows: heavy at split_rows = 40), user 299 and item 11 never occur."""
    sizes = (300, 12) if F == 2 else (300, 12, 4)
    g = torch.Generator().manual_seed(17 + F)
    rows = [(u, i) for u in range(299) for i in range(11) if u < 2 or (u + i) % 5 != 0]
    rows += [(u, i) for u in range(2) for i in range(11)] * 4 + [(u, 0) for u in range(2)] * 5
    X = torch.tensor(rows)
    X[:, 1] += 300
    if F == 3:
        X = torch.cat([X, 312 + torch.randint(0, 3, (X.shape[0], 1), generator=g)], 1)
    X = X[torch.randperm(X.shape[0], generator=g)]
    y = (torch.rand(X.shape[0], generator=g) < 0.4).float()
    return sizes, X, y

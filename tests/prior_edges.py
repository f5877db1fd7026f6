"""Case builders and references for the PRIOR instances of the solvers over the priors' own range and at the solver's
widths: tests/test_prior_edges_cpu.py checks the references and the conditions on the inputs, and
tests/test_gpu_prior_edges.py runs the same cases on the kernels.  CPU tensors only.

  edge_priors                      priors at the ends of the learner's clamp [1e-4, 1e4]: flat, sharp, mixed (three
                                   rotations), far
  optimum_mp_prior                 one entity's optimum under N(m, 1 / lam) with mpmath at 50 digits, written out
  dual_fp64_prior_in_kernel_order  numpy fp64 restatements of solve_body's two paths under a prior, the sums and the
  primal_fp64_prior_in_kernel_order  Cholesky in the kernel's order; both take one of MISTAKES, planted
  scale_abs_term_wide              solve_reference.scale_abs_term re-derived for sigma in [0.01, 100]
  exact_range_references           part 2's cases with their references, cached
  bound_range_case / bound_cond    part 3's cases and the condition that keeps their bound tight
  width_priors / bound_wide_case   part 4: the parent's edge cases with drawn priors whose factored matrices stay under
                                   cond 1e3
  session_case / session_reference_*  part 5: sessions at d = 8 (range), 33, 129 and LDS (wide) and one fold's reference

A prior is the pair (m [d + 1], lam [d + 1]), coordinate 0 the first-order weight, fp32 values held in fp64."""
import functools
import math

import numpy as np
import torch

import bound_reference as BR
import elicit_priors_cases as EC
import prior_reference as P
import solve_reference as R

CHUNK = 8
LAM_LO, LAM_HI = R.f32(1e-4), R.f32(1e4)                   # the learner's default clamp (prec_min, prec_max)
KINDS = ("flat", "sharp", "mixed0", "mixed1", "mixed2", "far")
MIXED = ("mixed0", "mixed1", "mixed2")
MISTAKES = ("b_without_the_mean", "lam_without_kl", "weight_from_coordinate_1", "prior_read_one_late")


# ---------------------------------------------------------------------------------------------------------------------
# 1. the priors
# ---------------------------------------------------------------------------------------------------------------------
def edge_priors(F, d, kind, seed=0):
    """(mean [F, d + 1], prec [F, d + 1]) as prior_reference.draw_priors returns them.  flat: every lam = 1e-4; sharp:
    every lam = 1e4; mixed<r>: lam_c = (1e-4, 1, 1e4)[(c + r) % 3], so that over r = 0, 1, 2 the weight coordinate takes
    each value once ("mixed" is mixed0); far: lam = 1.  The means of every kind are uniform in [-3, 3], distinct per
    coordinate: a prior that is constant across coordinates cannot see an indexing error."""
    kind = "mixed0" if kind == "mixed" else kind
    assert kind in KINDS, kind
    g = torch.Generator().manual_seed(7000 + 131 * seed + 17 * KINDS.index(kind) + d)
    mean = torch.rand(F, d + 1, generator=g, dtype=torch.float64) * 6.0 - 3.0
    if kind in MIXED:
        cyc = torch.tensor([1e-4, 1.0, 1e4], dtype=torch.float64)
        prec = cyc[(torch.arange(d + 1) + int(kind[-1])) % 3].expand(F, d + 1).clone()
    else:
        prec = torch.full((F, d + 1), {"flat": 1e-4, "sharp": 1e4, "far": 1.0}[kind], dtype=torch.float64)
    return mean.float().double(), prec.float().double()


def _mistaken(m, lam, mistake):
    """The prior as a kernel with `mistake` would read it (the two mistakes that are about where the prior is read)."""
    m, lam = np.array(R._np(m), np.float64), np.array(R._np(lam), np.float64)
    if mistake == "weight_from_coordinate_1":
        m[0], lam[0] = m[1], lam[1]
    elif mistake == "prior_read_one_late":
        m, lam = np.roll(m, -1), np.roll(lam, -1)
    else:
        assert mistake in (None,) + MISTAKES, mistake
    return m, lam


# ---------------------------------------------------------------------------------------------------------------------
# 2. the 50-digit reference under a prior
# ---------------------------------------------------------------------------------------------------------------------
_SHIFT = 149 + 2                                            # every fp32 value, and a sum of up to 4, is k 2^-_SHIFT


def mp_system(ent, bia, scal, x, y, field, link, kl_weight, entity):
    """What optimum_mp_prior needs of one entity that does not depend on the prior, mpmath at 50 digits:
    dict(n, d, prec, kl, T = sum_r u_r u_r^T, bM = sum_r t_r u_r, SA, SB, SC).  T is summed exactly: the entries of
    u_r = (1, sum of the partners' fp32 means) are integers times 2^-151, so their products are summed as integers and
    rounded once."""
    mpm = R._mpmath()
    mp = mpm.mp
    ent_, bia_, scal_ = R._np(ent, np.float32), R._np(bia, np.float32), R._np(scal, np.float32)
    d = ent_.shape[1] // 2
    d1 = d + 1
    xr, yr = R.entity_rows(x, y, field, entity)
    n = xr.shape[0]
    Q = [f for f in range(xr.shape[1]) if f != field]
    assert len(Q) <= 4
    with mp.workdps(50):
        F_ = lambda v: mpm.mpf(float(v))
        lk = (lambda s: abs(s)) if link == "abs" else (lambda s: mpm.log(1 + mpm.exp(s)))
        prec, kl = lk(F_(scal_[0])), F_(R.f32(kl_weight))
        zero = mpm.mpf(0)
        SA, SB, SC, bM = [zero] * d1, [zero] * d1, [zero] * d1, [zero] * d1
        SB[0] = mpm.mpf(n)
        Ui = np.empty((n, d1), dtype=object)
        for r in range(n):
            cm = F_(scal_[1])
            for f in Q:
                cm += F_(bia_[xr[r, f], 0])
            u = [mpm.mpf(1)]
            Ui[r, 0] = 1 << _SHIFT
            rowA, rowB, rowC = [], [], []
            for k in range(d):
                ms = [F_(ent_[xr[r, f], k]) for f in Q]
                s2 = [lk(F_(ent_[xr[r, f], d + k])) ** 2 for f in Q]
                sm = sum(ms, zero)
                A = sum(s2, zero)
                Cc = 2 * sum((s2[i] * (sm - ms[i]) for i in range(len(Q))), zero)
                cm += (sm * sm - sum((v * v for v in ms), zero)) / 2
                u.append(sm)
                Ui[r, k + 1] = sum(int(math.ldexp(float(ent_[xr[r, f], k]), _SHIFT)) for f in Q)
                rowA.append(A)
                rowB.append(A + sm * sm)
                rowC.append(Cc)
            t = F_(yr[r]) - cm
            for k in range(d):
                SA[k + 1] += rowA[k]
                SB[k + 1] += rowB[k]
                SC[k + 1] += rowC[k]
            for c in range(d1):
                bM[c] += t * u[c]
        Ti = Ui.T.dot(Ui) if n else np.zeros((d1, d1), dtype=object)
        T = mpm.zeros(d1, d1)
        for i in range(d1):
            for j in range(i + 1):
                T[i, j] = T[j, i] = mpm.ldexp(mpm.mpf(int(Ti[i, j])), -2 * _SHIFT)
    return dict(n=n, d=d, prec=prec, kl=kl, T=T, bM=bM, SA=SA, SB=SB, SC=SC)


def optimum_mp_prior(ent, bia, scal, x, y, field, link, kl_weight, entity, m, lam, system=None):
    """One entity's closed-form optimum under the prior N(m_c, 1 / lam_c) (include/vfm_prior.h) from the fp32 tables and
    the fp32 prior with mpmath at 50 digits, written out from the block's formulas:
        D_c = kl lam_c + prec SA_c,  b_c = prec (bM_c - SC_c / 2) + kl lam_c m_c,  H = prec T + diag(D),  H theta = b,
        sigma_c^2 = kl / (kl lam_c + prec SB_c),  s = link^-1(sigma).
    H is symmetric positive definite: solved by mpmath's Cholesky.  `system`: mp_system of the same entity, where one
    entity is solved under several priors.  For small systems (d + 1 <= 65).  Returns dict(n, theta [d + 1] = (mu_w, mu),
    s [d + 1] = (s_w, s), sigma [d + 1], rounded to fp64, cond = the condition number of the matrix the kernel factors)."""
    mpm = R._mpmath()
    mp = mpm.mp
    sy = mp_system(ent, bia, scal, x, y, field, link, kl_weight, entity) if system is None else system
    n, d = sy["n"], sy["d"]
    d1 = d + 1
    assert d1 <= 65, "optimum_mp_prior is for small systems"
    m_, lam_ = np.asarray(R._np(m), np.float64), np.asarray(R._np(lam), np.float64)
    assert m_.shape == (d1,) and lam_.shape == (d1,) and (lam_ > 0).all()
    with mp.workdps(50):
        prec, kl = sy["prec"], sy["kl"]
        kll = [kl * mpm.mpf(float(v)) for v in lam_]
        H = prec * sy["T"]
        b = mpm.zeros(d1, 1)
        for c in range(d1):
            H[c, c] += kll[c] + prec * sy["SA"][c]
            b[c] = prec * (sy["bM"][c] - sy["SC"][c] / 2) + kll[c] * mpm.mpf(float(m_[c]))
        theta = mpm.cholesky_solve(H, b)
        inv = (lambda s: s) if link == "abs" else (lambda s: mpm.log(mpm.expm1(s)))
        sigma = [mpm.sqrt(kl / (kll[c] + prec * sy["SB"][c])) for c in range(d1)]
        s = np.array([float(inv(v)) for v in sigma])
        sigma = np.array([float(v) for v in sigma])
        theta = np.array([float(theta[c]) for c in range(d1)])
    cond = P.cond_of_the_factored_prior(ent, bia, scal, x, y, field, link, kl_weight, entity, m_, lam_)
    return dict(n=n, theta=theta, s=s, sigma=sigma, cond=cond)


# ---------------------------------------------------------------------------------------------------------------------
# the kernel's two paths under a prior, restated in numpy fp64
# ---------------------------------------------------------------------------------------------------------------------
def system64_prior(ent, bia, scal, x, y, field, link, kl_weight, entity, m, lam, mistake=None):
    """solve_reference.system64 under the prior (phase A of solve_body, PRIOR): the row sums sequential in row order,
    kll = kl lam, D = kll + prec SA, b = prec (bM - SC / 2) + kll m.  dict(n, d, prec, kl, M, D, b, SB, kll), kll the
    term of the scales' denominator.  `mistake`: one of MISTAKES, planted."""
    xr, yr = R.entity_rows(x, y, field, entity)
    M, A, Cc, cm = R.operands64(ent, bia, scal, xr, field, link)
    n, d = M.shape
    prec = float(R._link64(R._np(scal, np.float32)[0], link))
    kl = R.f32(kl_weight)
    SA, SB, SC, bM = np.zeros(d + 1), np.zeros(d + 1), np.zeros(d + 1), np.zeros(d + 1)
    for i in range(n):
        t = yr[i] - cm[i]
        SA[1:] += A[i]
        SB[1:] += A[i] + M[i] * M[i]
        SC[1:] += Cc[i]
        bM[1:] += t * M[i]
        bM[0] += t
    SB[0] = float(n)
    m, lam = _mistaken(m, lam, mistake)
    kll = kl * lam
    b = prec * (bM - 0.5 * SC)
    if mistake != "b_without_the_mean":
        b = b + kll * m
    if mistake == "lam_without_kl":
        kll = lam.copy()
    return dict(n=n, d=d, prec=prec, kl=kl, M=M, D=kll + prec * SA, b=b, SB=SB, kll=kll)


def _chol_in_kernel_order(L):
    """chol_solve of vfm_foldin_solve_body.hpp on L [m + 1, m] (rows 0 .. m - 1: the lower triangle; row m: the
    right-hand side): the left-looking Cholesky with the right-hand side as one more row and 1 / sqrt of the pivot, then
    the back substitution column by column.  Returns the solution [m]."""
    m = L.shape[1]
    L = L.copy()
    dv = np.zeros(m)
    for j in range(m):
        sjj = L[j, j]
        for k in range(j):
            sjj -= L[j, k] * L[j, k]
        rinv = 1.0 / math.sqrt(sjj)
        dv[j] = rinv
        sij = L[j + 1:, j].copy()
        for k in range(j):
            sij -= L[j + 1:, k] * L[j, k]
        L[j + 1:, j] = sij * rinv
    yv, xv = L[m].copy(), np.zeros(m)
    for j in range(m - 1, -1, -1):
        xj = yv[j] * dv[j]
        yv[:j] -= L[j, :j] * xj
        xv[j] = xj
    return xv


def dual_fp64_prior_in_kernel_order(ent, bia, scal, x, y, field, link, kl_weight, entity, m, lam, mistake=None):
    """solve_reference.dual_fp64_in_kernel_order under the prior: theta [d + 1] of an entity with n <= d rows by phases
    A-D of the kernel's dual path with D and b of system64_prior."""
    s = system64_prior(ent, bia, scal, x, y, field, link, kl_weight, entity, m, lam, mistake)
    n, d, prec, M = s["n"], s["d"], s["prec"], s["M"]
    assert n <= d, "the dual path is taken for n <= d"
    Di = 1.0 / s["D"]
    bv = s["b"] / s["D"]
    if n == 0:
        return bv
    Lm = np.zeros((n + 1, n))
    K = R._wave_dot((M[:, None, :] * M[None, :, :]) * Di[None, None, 1:]) + Di[0]
    K[np.arange(n), np.arange(n)] += 1.0 / prec
    Lm[:n] = np.tril(K)
    Lm[n] = R._wave_dot(M * bv[None, 1:]) + bv[0]
    xv = _chol_in_kernel_order(Lm)
    acc = np.zeros(d + 1)
    for i in range(n):
        acc[0] += xv[i]
        acc[1:] += M[i] * xv[i]
    return bv - Di * acc


def primal_fp64_prior_in_kernel_order(ent, bia, scal, x, y, field, link, kl_weight, entity, m, lam, mistake=None):
    """theta [d + 1] of an entity with n > d rows by the kernel's primal path: H_ij = prec sum_r u_ri u_rj (+ D_i on the
    diagonal), every element's sum sequential in row order, b as the right-hand side row, the same Cholesky."""
    s = system64_prior(ent, bia, scal, x, y, field, link, kl_weight, entity, m, lam, mistake)
    n, d, prec, M = s["n"], s["d"], s["prec"], s["M"]
    U = np.concatenate([np.ones((n, 1)), M], 1)
    acc = np.zeros((d + 1, d + 1))
    for r in range(n):
        acc += U[r][:, None] * U[r][None, :]
    H = prec * acc + np.diag(s["D"])
    return _chol_in_kernel_order(np.concatenate([np.tril(H), s["b"][None]], 0))


def restatement_fp64_prior(ent, bia, scal, x, y, field, link, kl_weight, entity, m, lam, mistake=None):
    """(theta [d + 1], s [d + 1]) of one entity as solve_body computes them before its rounding to fp32: the dual path
    for n <= d, else the primal one, and phase D's scales."""
    s = system64_prior(ent, bia, scal, x, y, field, link, kl_weight, entity, m, lam, mistake)
    path = dual_fp64_prior_in_kernel_order if s["n"] <= s["d"] else primal_fp64_prior_in_kernel_order
    theta = path(ent, bia, scal, x, y, field, link, kl_weight, entity, m, lam, mistake)
    sg = np.sqrt(s["kl"] / (s["kll"] + s["prec"] * s["SB"]))
    return theta, BR.unlink64(sg, link)


# ---------------------------------------------------------------------------------------------------------------------
# the scales' absolute term over the range
# ---------------------------------------------------------------------------------------------------------------------
def scale_abs_term_wide(n, ref):
    """solve_reference.scale_abs_term re-derived for sigma in [0.01, 100], u = 2^-53.

    sigma_c^2 = kl / (kl lam_c + prec SB_c).  SB_c is a sum of n positive terms A + M^2, each with at most two roundings,
    added in n - 1 more: relative error (n + 1) u in either order.  prec itself (the link of a stored scalar), the
    products prec SB and kl lam, their sum (both positive: no cancellation) and the division add at most 2 + 1 + 1 + 1 +
    1 = 6 u.  The square root halves the total and adds its own rounding: d sigma / sigma <= ((n + 7) / 2 + 1) u
    = (n / 2 + 4.5) u.
    Under "abs" s = sigma: the error is relative, at most (n / 2 + 4.5) u |s|.
    Under softplus s = log(expm1(sigma)), ds / dsigma = 1 / (1 - exp(-sigma)), so a relative error delta of sigma moves s
    by g(sigma) delta with g(sigma) = sigma / (1 - exp(-sigma)) = sigma + sigma / expm1(sigma):
      sigma <= 1:  g is increasing, g(1) = 1.582: the 1.6 of scale_abs_term.  For sigma down to 0.01 (and to 0) g falls
                   to 1, while |s| = |log(expm1(0.01))| = 4.6 grows: max(1, |s|) covers it, nothing to add;
      sigma > 1:   g(sigma) <= sigma + 1, and s = sigma + log(1 - exp(-sigma)) >= sigma - 0.459, so g(sigma) <= |s| +
                   1.459 <= 2.46 max(1, |s|): at sigma = 100 the error of s is 100 times that of sigma <= 1, but
                   relative to |s| = 100 it is 2.46 / 1.6 of it.
    expm1 and log add a rounding each: u in the argument of log, which is u absolute in s, and u |s|.  One side:
    (2.46 (n / 2 + 4.5) + 2) u max(1, |s|) <= (1.25 n + 14) u max(1, |s|); as in scale_abs_term once for the kernel and
    once for the oracle, doubled.  (scale_abs_term's (n + 8) u is below this for every n: the term grows, by 2.46 / 1.6
    in n's factor and by the roundings of the prior's denominator.)  Beside 2^-23 |s| it is nothing: 7e-14 at n = 81."""
    ref = np.abs(np.asarray(R._np(ref), np.float64))
    return 4.0 * (1.25 * n + 14.0) * 2.0 ** -53 * max(1.0, float(ref.max()) if ref.size else 0.0)


# ---------------------------------------------------------------------------------------------------------------------
# 2. exact solves over the range: the cases and their references
# ---------------------------------------------------------------------------------------------------------------------
RANGE_DS = (8, 64)
RANGE_KL = {2: R.f32(1.6), 3: R.f32(0.7)}                  # (not 1: at kl = 1 "lam in place of kl lam" is no mistake)


def split_count(d):
    return CHUNK * (d // CHUNK + 2) + 1


def exact_range_counts(d):
    """solve_reference.kcond_counts -- n = 1, d / 2 with every other row a duplicate, d (the largest dual), d + 1 (the
    smallest primal) -- and the one entity the split solver takes at split_rows = 0, chunk_rows = CHUNK."""
    return R.kcond_counts(d) + [split_count(d)]


def exact_range_kinds(d, link, F):
    """The kinds a (d, link, F) table is solved under: all six, the three rotations of mixed included."""
    return KINDS


def exact_range_case(d, link, F):
    sizes = (8, 200) if F == 2 else (8, 40, 25)
    return R.case(sizes, 0, d, link, exact_range_counts(d), seed=1200 + d + 7 * F + (link == "softplus"),
                  kl_weight=RANGE_KL[F], dup=False, dup_every_other=(1,))


def _args(c, k):
    return (c["ent"], c["bia"], c["scal"], c["X"], c["y"], c["field"], c["link"], c["kl_weight"], int(c["ids"][k]))


@functools.lru_cache(maxsize=None)
def _range_systems(d, link, F):
    c = exact_range_case(d, link, F)
    return c, [mp_system(*_args(c, k)) for k in range(len(c["counts"]))]


@functools.lru_cache(maxsize=None)
def exact_range_references(d, link, F, kind):
    """(case, (m, lam) of the case's field, per entity dict(n, ref = optimum_mp_prior's result, restated = (theta, s) of
    the kernel-order fp64 restatement, e_ref = max |restated theta - ref theta|, the yardstick of the means))."""
    c, systems = _range_systems(d, link, F)
    mean, prec = edge_priors(F, d, kind)
    m, lam = mean[c["field"]].numpy(), prec[c["field"]].numpy()
    out = []
    for k, n in enumerate(c["counts"]):
        ref = optimum_mp_prior(*_args(c, k), m, lam, system=systems[k])
        assert ref["n"] == n
        restated = restatement_fp64_prior(*_args(c, k), m, lam)
        out.append(dict(n=n, ref=ref, restated=restated, e_ref=float(np.abs(restated[0] - ref["theta"]).max())))
    return c, (m, lam), out


def reference_objective(c, k, theta, s, m, lam):
    """L_e of entity number k of case c at (theta, s) [d + 1] under the prior: prior_reference.entity_objective_prior."""
    e = int(c["ids"][k])
    sel = c["X"][:, c["field"]] == e
    th = (torch.tensor([e]), torch.as_tensor(theta[None, 1:]).double(), torch.as_tensor(s[None, 1:]).double(),
          torch.as_tensor(theta[:1]).double(), torch.as_tensor(s[:1]).double())
    return float(P.entity_objective_prior(c["ent"], c["bia"], c["scal"], c["X"][sel], c["y"][sel].double(), c["field"], th,
                                          c["link"], c["kl_weight"], m, lam)[0])


def exact_criterion(r, theta32, s32):
    """Part 2's criterion for one entity: the means by 2^-23 |ref| + 8 e_ref (test_conditioning_of_the_dual_path's), the
    scales by scale_abs_term_wide.  Returns (ok, worst ratio of the means, worst ratio of the scales)."""
    ok_t, w_t = R.elementwise_ok(theta32, r["ref"]["theta"], 8.0 * r["e_ref"])
    ok_s, w_s = R.elementwise_ok(s32, r["ref"]["s"], scale_abs_term_wide(r["n"], r["ref"]["s"]))
    return ok_t and ok_s, w_t, w_s


# ---------------------------------------------------------------------------------------------------------------------
# 3. bound solves over the range
# ---------------------------------------------------------------------------------------------------------------------
BOUND_DS = (8, 33)


def bound_range_counts(d):
    """bound_reference.shape_counts plus the one entity the split solver takes.  (test_prior_edges_cpu asserts
    bound_tight for every (d, kind) pair at these counts.)"""
    return BR.shape_counts(d) + [split_count(d)]


def bound_range_case(d, link, F=3):
    sizes = (12, 40) if F == 2 else (12, 40, 25)
    return BR.bound_case(sizes, 0, d, link, bound_range_counts(d), seed=1400 + d + 7 * F + (link == "softplus"),
                         kl_weight=RANGE_KL[F])


def bound_rounds_mistaken(c, k, n_iters, reset, m, lam, mistake, start=None):
    """bound_rounds_fp64_prior of entity number k with one of MISTAKES planted, round by round: the mistaken round is
    the reference's own round (started where the mistaken one stands) under the prior the mistake reads, with b or kll
    changed.  Returns (theta, s) after n_iters rounds."""
    o = BR.entity_operands(c["ent"], c["bia"], c["scal"], c["X"], c["y"], c["field"], c["link"], int(c["ids"][k]))
    n, d = o["n"], o["d"]
    M, A, Cc, cm, cv, yr = (o[q].numpy() for q in ("M", "A", "C", "cm", "cv", "y"))
    kl = R.f32(c["kl_weight"])
    m0, lam0 = np.asarray(R._np(m), np.float64), np.asarray(R._np(lam), np.float64)
    if start is not None:
        theta, sig2 = (np.array(v, np.float64) for v in start)
    else:
        theta, sig2 = (m0.copy(), 1.0 / lam0) if reset else BR.table_start(c["ent"], c["bia"], c["link"], int(c["ids"][k]))
    m, lam = _mistaken(m0, lam0, mistake)
    kll = lam.copy() if mistake == "lam_without_kl" else kl * lam
    U = np.concatenate([np.ones((n, 1)), M], 1)
    for _ in range(n_iters):
        mu = theta[1:]
        Ef = cm + theta[0] + M @ mu
        Vf = cv + sig2[0] + (mu * mu * A + sig2[1:] * (A + M * M) + mu * Cc).sum(1)
        w = BR.jj_weight(np.sqrt(np.maximum(Ef * Ef + Vf, 0.0)))
        D = kll + np.concatenate([[0.0], (w[:, None] * A).sum(0)])
        b = U.T @ ((yr - 0.5) - w * cm) - np.concatenate([[0.0], 0.5 * (w[:, None] * Cc).sum(0)])
        if mistake != "b_without_the_mean":
            b = b + kl * lam * m
        theta = np.linalg.solve(np.diag(D) + U.T @ (w[:, None] * U), b)
        sig2 = kl / (kll + np.concatenate([[w.sum()], (w[:, None] * (A + M * M)).sum(0)]))
    return theta, BR.unlink64(np.sqrt(sig2), c["link"])


def bound_criterion(d, n_iters, r, theta32, s32):
    """test_gpu_fit_bound_priors._check's elementwise criterion for the rounds r of one entity.  Returns (ok, worst)."""
    at = n_iters * R.solve_abs_term(d, float(r["cond"].max()), r["theta"][-1])
    ok_t, w_t = R.elementwise_ok(theta32, r["theta"][-1], at)
    ok_s, w_s = R.elementwise_ok(s32, r["s"][-1], at + R.scale_abs_term(r["n"], r["s"][-1]))
    return ok_t and ok_s, max(w_t, w_s)


def bound_tight(d, n_iters, cond_max, ref):
    """Part 3's condition: the solves' absolute term stays below one fp32 rounding of the largest mean, so that the
    bound of test_gpu_fit_bound_priors._check is as tight as under its cond <= 1e3."""
    ref = np.asarray(ref, np.float64)
    return n_iters * R.solve_abs_term(d, cond_max, ref) <= R.EPS32 * float(np.abs(ref).max())


def bound_cond_cap(d, n_iters):
    """The largest cond_max that bound_tight accepts: 2^-23 / (n_iters 4 (d + 1) 2^-52)."""
    return R.EPS32 / (n_iters * 4.0 * (d + 1) * R.EPS64)


# ---------------------------------------------------------------------------------------------------------------------
# 4. widths and storage under a prior
# ---------------------------------------------------------------------------------------------------------------------
WIDTH_COND = 1e3                                            # test_gpu_solve_edges._check's own cap
WIDTH_PREC_LO = {"width": 0.25, "largest_dual": 1.0, "past_cap": 0.25, "bound_wide": 0.25}
BITWISE_KIND = "mixed1"


def width_priors(c, name, seed=5):
    """draw_priors for the case c of the parent's edge suite, the precisions from [WIDTH_PREC_LO[name], 16]."""
    return P.draw_priors(len(c["sizes"]), c["d"], seed + c["d"], WIDTH_PREC_LO[name])


def case_conds_prior(c, m, lam, which=None):
    which = range(len(c["counts"])) if which is None else which
    return [P.cond_of_the_factored_prior(*_args(c, k), m, lam) for k in which]


def bound_wide_counts(d):
    return [R.FB - 1, R.FB + 1, d, d + 1]


def bound_wide_case(link):
    return BR.bound_case((8, 12, 300), 1, 300, link, bound_wide_counts(300), seed=1500 + (link == "softplus"))


# ---------------------------------------------------------------------------------------------------------------------
# 5. sessions under a prior beyond d = 5
# ---------------------------------------------------------------------------------------------------------------------
SESSION_SIZES, SESSION_NAMES = (12, 60, 3), ("exact", "design", "bound")
WIDE_DS = (33, 129, R.LDS)
RANGE_D, RANGE_Q, RANGE_KINDS = 8, 3, MIXED + ("flat",)


def session_shape(d):
    """(history rows of the long respondent, rounds).  d = 8 and 33: d - 2 rows and 3 rounds, n = d - 1, d (dual), d + 1
    (primal).  d = 129: LDS - 3 rows and 4 rounds; its system is the primal one of 130 <= LDS throughout, so at this d
    nothing leaves LDS.  d = LDS: solve_reference.session_cases' (LDS, LDS - 2, 4), whose system goes LDS - 1, LDS (dual,
    in LDS), LDS + 1, LDS + 1 (primal, in the slab): the crossing mid-session."""
    if d == 129:
        return R.LDS - 3, 4
    if d == R.LDS:
        return R.LDS - 2, 4
    return d - 2, 3


def session_case(name, d, prior="drawn"):
    """elicit_priors_cases.case at embedding size d: 4 respondents of field 0 of a (12, 60, 3) model, pools of Q rows (every
    pool row is asked, in an order the GPU decides), histories of 0, 2, 7 and session_shape(d)[0] rows.  prior: "drawn"
    (prior_reference.draw_priors, the precisions in [max(1, prec_lo_for(d)), 16]; the tables' scale is 0.3 for d >= 128,
    which keeps every factored matrix under elicit_priors_cases.COND_EXACT) or a kind of edge_priors.  The same keys as
    elicit_priors_cases.case, and long = the respondent with the long history."""
    sizes, F = SESSION_SIZES, len(SESSION_SIZES)
    H, Q = session_shape(d)
    seed = 1600 + 3 * d + SESSION_NAMES.index(name)
    g = torch.Generator().manual_seed(seed)
    T = sum(sizes)
    scale = 0.3 if d >= 128 else 0.5
    ent = (torch.randn(T, 2 * d, generator=g) * scale).float()
    bia = (torch.randn(T, 2, generator=g) * scale).float()
    scal = torch.tensor([1.3, 0.2, 0.3])
    resp = torch.randperm(sizes[0], generator=g)[:4]
    n_ctx = sizes[1] * sizes[2]
    pool, hist = [], []
    for e, h in zip(resp.tolist(), (0, 2, 7, H)):
        pick = torch.randperm(n_ctx, generator=g)[:Q + h]
        rows = torch.stack([torch.full_like(pick, e), sizes[0] + pick // sizes[2], sizes[0] + sizes[1] + pick % sizes[2]], 1)
        pool.append(rows[:Q])
        hist.append(rows[Q:])
    pool, hist = torch.cat(pool), torch.cat(hist)
    output = "class" if name == "bound" else "reg"
    ans = (lambda n: torch.randn(n, generator=g) + 1.0) if output == "reg" else (lambda n: (torch.rand(n, generator=g) < 0.5).float())
    y_pool, hist_y = ans(pool.shape[0]), ans(hist.shape[0])
    mean, prec = P.draw_priors(F, d, seed, max(1.0, P.prec_lo_for(d))) if prior == "drawn" else edge_priors(F, d, prior)
    return dict(sizes=sizes, d=d, Q=Q, field=0, klw=EC.KLW, link=EC._LINKS[name], output=output, ent=ent, bia=bia, scal=scal,
                pool=pool, y_pool=y_pool, hist_x=hist, hist_y=hist_y, mean=mean, prec=prec, n_iters=EC.N_ITERS, long=resp[3].item(),
                H=H)


def session_view(c, x, y, e):
    """The rows (x, y) of respondent e as a one-entity fold-in case (the keys _args and bound_rounds_mistaken read)."""
    return dict(ent=c["ent"], bia=c["bia"], scal=c["scal"], X=x, y=y, field=c["field"], link=c["link"], kl_weight=c["klw"],
                ids=torch.tensor([e]), d=c["d"])


def session_prior(c):
    f = c["field"]
    return c["mean"][f].numpy(), c["prec"][f].numpy()


def session_reference_mp(c, x, y, e):
    """Part 2's reference of one fold of a range session: dict(n, ref, restated, e_ref) as exact_range_references."""
    m, lam = session_prior(c)
    a = _args(session_view(c, x, y, e), 0)
    ref = optimum_mp_prior(*a, m, lam)
    restated = restatement_fp64_prior(*a, m, lam)
    return dict(n=ref["n"], ref=ref, restated=restated, e_ref=float(np.abs(restated[0] - ref["theta"]).max()))


def session_reference_fp64(c, x, y):
    """The wide sessions' reference of one fold: (theta [d + 1], s [d + 1], cond, n) from solve_fp64_prior."""
    m, lam = session_prior(c)
    ref = P.solve_fp64_prior(c["ent"], c["bia"], c["scal"], x, y, c["field"], c["link"], R.f32(c["klw"]), m, lam)
    rt = np.concatenate([[float(ref["mu_w"][0])], ref["mu"][0].numpy()])
    rs = np.concatenate([[float(ref["s_w"][0])], ref["s"][0].numpy()])
    return rt, rs, float(ref["cond"][0]), x.shape[0]


def wide_criterion(d, rt, rs, cond, n, theta32, s32):
    """test_gpu_elicit_priors' criterion of an exact posterior.  Returns (ok, worst)."""
    ok_t, w_t = R.elementwise_ok(theta32, rt, R.solve_abs_term(d, cond, rt))
    ok_s, w_s = R.elementwise_ok(s32, rs, R.scale_abs_term(n, rs))
    return ok_t and ok_s, max(w_t, w_s)


def session_start(c, e, reset):
    """(theta, sig2) a bound session starts respondent e at: the prior row with reset, else its table row."""
    return EC.prior_start(c) if reset else BR.table_start(c["ent"], c["bia"], c["link"], e)


def pool_order(c, e):
    return torch.nonzero(c["pool"][:, c["field"]] == e).reshape(-1).tolist()

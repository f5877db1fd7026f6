"""References and case builders for the tests of solve_body (vae_amd/csrc_rank/vfm_foldin_solve_body.hpp) at its own
edges: tests/test_solve_edges_cpu.py checks the references and the conditions on the inputs, and
tests/test_gpu_solve_edges.py runs the same cases on the kernels.

  optimum_mp                   one entity's closed-form optimum from the fp32 tables with mpmath at 50 digits
  dual_fp64_in_kernel_order    numpy fp64 restatement of the kernel's dual path (phases A-D), its sums in the kernel's order
  elementwise_ok               |got_i - ref_i| <= 2^-23 |ref_i| + abs_term for every element
  solve_abs_term               4 (d + 1) 2^-52 cond max|ref|: the backward-error bound of an fp64 Cholesky solve, once
                               for the kernel, once for the fp64 oracle, doubled
  LDS, SLABS, FB               the solver's constants, read from include/vfm_foldin.h and vfm_foldin_body.hpp

Every edge of the builders below is an expression in LDS, SLABS and FB, so the cases move with the code.  No GPU is
needed to import this module or to build a case: the tables are CPU tensors which the GPU tests copy into a model."""
import functools
import math
import os
import re

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS32, EPS64 = 2.0 ** -23, 2.0 ** -52


# ---------------------------------------------------------------------------------------------------------------------
# the solver's constants and the rules that depend on them
# ---------------------------------------------------------------------------------------------------------------------
def read_solver_constants(root=ROOT):
    """(LDS, SLABS, FB) from the text of include/vfm_foldin.h and vae_amd/csrc_rank/vfm_foldin_body.hpp under root."""
    hdr = open(os.path.join(root, "include", "vfm_foldin.h")).read()
    body = open(os.path.join(root, "vae_amd", "csrc_rank", "vfm_foldin_body.hpp")).read()
    lds = re.findall(r"#define\s+VFM_FOLDIN_SOLVE_LDS_DIM\s+(\d+)", hdr)
    slabs = re.findall(r"#define\s+VFM_FOLDIN_SOLVE_SLABS\s+(\d+)", hdr)
    fb = re.findall(r"constexpr\s+int\s+FB\s*=\s*(\d+)\s*;", body)
    assert len(lds) == 1 and len(slabs) == 1 and len(fb) == 1, (lds, slabs, fb)
    return int(lds[0]), int(slabs[0]), int(fb[0])


LDS, SLABS, FB = read_solver_constants()


def f32(v):
    """v as the kernel receives it through a float argument."""
    return float(np.float32(v))


def tri(m):
    return m * (m + 1) // 2


def solve_dim(n, d):
    """The size of the system of an entity with n rows: the dual n x n while n <= d, else the primal (d + 1) x (d + 1)."""
    return n if n <= d else d + 1


def cap_dim_of(d, lds_dim=-1, lds=None):
    fit = min(d + 1, LDS if lds is None else lds)
    return fit if lds_dim < 0 or lds_dim > fit else lds_dim


def storage(n, d, lds_dim=-1, lds=None):
    """Where the triangle of an entity with n rows lives: "lds" or "slab"."""
    return "lds" if solve_dim(n, d) <= cap_dim_of(d, lds_dim, lds) else "slab"


def has_slabs(d, lds_dim=-1, lds=None):
    """The rule that decides whether a launch has slabs at all, and with them a capped grid."""
    return d + 1 > cap_dim_of(d, lds_dim, lds)


# ---------------------------------------------------------------------------------------------------------------------
# the row operands and the system of one entity in numpy fp64 (k_foldin_solve_prep's sums, field by field)
# ---------------------------------------------------------------------------------------------------------------------
def _np(t, dtype=None):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.astype(dtype) if dtype is not None else a


def _link64(s, link):
    s = np.asarray(s, np.float64)
    return np.abs(s) if link == "abs" else np.maximum(s, 0.0) + np.log1p(np.exp(-np.abs(s)))


def entity_rows(x, y, field, entity):
    """(partner rows [n, F] int64, y [n] fp64 of the fp32 answers) of one entity, in the order of x: the order of the
    kernel's row list, which is a stable sort by the folded id."""
    x, y = _np(x), _np(y, np.float32)
    sel = x[:, field] == int(entity)
    return x[sel], y[sel].astype(np.float64)


def operands64(ent, bia, scal, xr, field, link):
    """M, A, C [n, d] and c_mean [n] of the rows xr in fp64 from the fp32 tables."""
    ent, bia, scal = _np(ent, np.float32), _np(bia, np.float32), _np(scal, np.float32)
    d = ent.shape[1] // 2
    Q = [f for f in range(xr.shape[1]) if f != field]
    n = xr.shape[0]
    sm, smm, ss = np.zeros((n, d)), np.zeros((n, d)), np.zeros((n, d))
    cm = np.full(n, float(scal[1]))
    for f in Q:
        cm = cm + bia[xr[:, f], 0].astype(np.float64)
    for f in Q:
        m = ent[xr[:, f], :d].astype(np.float64)
        sg = _link64(ent[xr[:, f], d:], link)
        sm, smm, ss = sm + m, smm + m * m, ss + sg * sg
    cov = np.zeros((n, d))
    for f in Q:
        m = ent[xr[:, f], :d].astype(np.float64)
        sg = _link64(ent[xr[:, f], d:], link)
        cov = cov + sg * sg * (sm - m)
    for k in range(d):
        cm = cm + 0.5 * (sm[:, k] * sm[:, k] - smm[:, k])
    return sm, ss, 2.0 * cov, cm


def system64(ent, bia, scal, x, y, field, link, kl_weight, entity):
    """The pieces of one entity's system in fp64, the row sums sequential in row order (phase A): dict(n, d, prec, kl,
    M [n, d], D [d + 1], b [d + 1], SB [d + 1])."""
    xr, yr = entity_rows(x, y, field, entity)
    M, A, Cc, cm = operands64(ent, bia, scal, xr, field, link)
    n, d = M.shape
    prec = float(_link64(_np(scal, np.float32)[0], link))
    kl = f32(kl_weight)
    SA, SB, SC, bM = np.zeros(d + 1), np.zeros(d + 1), np.zeros(d + 1), np.zeros(d + 1)
    for i in range(n):
        t = yr[i] - cm[i]
        SA[1:] += A[i]
        SB[1:] += A[i] + M[i] * M[i]
        SC[1:] += Cc[i]
        bM[1:] += t * M[i]
        bM[0] += t
    SB[0] = float(n)
    return dict(n=n, d=d, prec=prec, kl=kl, M=M, D=kl + prec * SA, b=prec * (bM - 0.5 * SC), SB=SB)


def conds(ent, bia, scal, x, y, field, link, kl_weight, entity):
    """(cond(H), cond(K) or None): the 2-norm condition numbers of the primal matrix and, for n <= d, of the dual matrix
    K = I / prec + U D^-1 U^T the kernel factors in its place."""
    s = system64(ent, bia, scal, x, y, field, link, kl_weight, entity)
    n, d = s["n"], s["d"]
    U = np.concatenate([np.ones((n, 1)), s["M"]], 1)
    H = np.diag(s["D"]) + s["prec"] * (U.T @ U)
    cK = None
    if n <= d:
        cK = float(np.linalg.cond(np.eye(n) / s["prec"] + (U / s["D"]) @ U.T)) if n else 1.0
    return float(np.linalg.cond(H)), cK


def cond_of_the_factored(ent, bia, scal, x, y, field, link, kl_weight, entity):
    """cond of the matrix the kernel factors for this entity: cond(K) for n <= d, else cond(H)."""
    cH, cK = conds(ent, bia, scal, x, y, field, link, kl_weight, entity)
    return cH if cK is None else cK


# ---------------------------------------------------------------------------------------------------------------------
# the 50-digit reference
# ---------------------------------------------------------------------------------------------------------------------
def _mpmath():
    try:
        import mpmath
    except ImportError:
        import pytest
        pytest.skip("mpmath is not installed: the 50-digit reference of the exact fold-in cannot be computed")
    return mpmath


def optimum_mp(ent, bia, scal, x, y, field, link, kl_weight, entity):
    """One entity's closed-form optimum (include/vfm_foldin.h) from the fp32 tables with mpmath at 50 digits: the
    operands, H, b, the LU solve and the scales' closed form, log(expm1(.)) included.  For small systems (d + 1 <= 65).
    Returns dict(n, theta [d + 1] = (mu_w, mu), s [d + 1] = (s_w, s) rounded to fp64, cond_H, cond_K (None for n > d))."""
    mpm = _mpmath()
    mp = mpm.mp
    ent_, bia_, scal_ = _np(ent, np.float32), _np(bia, np.float32), _np(scal, np.float32)
    d = ent_.shape[1] // 2
    assert d + 1 <= 65, "optimum_mp is for small systems"
    xr, yr = entity_rows(x, y, field, entity)
    n = xr.shape[0]
    Q = [f for f in range(xr.shape[1]) if f != field]
    with mp.workdps(50):
        F_ = lambda v: mpm.mpf(float(v))
        lk = (lambda s: abs(s)) if link == "abs" else (lambda s: mpm.log(1 + mpm.exp(s)))
        prec, kl = lk(F_(scal_[0])), F_(f32(kl_weight))
        d1 = d + 1
        U, SA, SB, SC, t = [], [mpm.mpf(0)] * d1, [mpm.mpf(0)] * d1, [mpm.mpf(0)] * d1, []
        SB[0] = mpm.mpf(n)
        for r in range(n):
            cm = F_(scal_[1])
            for f in Q:
                cm += F_(bia_[xr[r, f], 0])
            u = [mpm.mpf(1)]
            for k in range(d):
                ms = [F_(ent_[xr[r, f], k]) for f in Q]
                s2 = [lk(F_(ent_[xr[r, f], d + k])) ** 2 for f in Q]
                sm = sum(ms, mpm.mpf(0))
                A = sum(s2, mpm.mpf(0))
                Cc = 2 * sum((s2[i] * (sm - ms[i]) for i in range(len(Q))), mpm.mpf(0))
                cm += (sm * sm - sum((m * m for m in ms), mpm.mpf(0))) / 2
                u.append(sm)
                SA[k + 1] += A
                SB[k + 1] += A + sm * sm
                SC[k + 1] += Cc
            U.append(u)
            t.append(F_(yr[r]) - cm)
        H = mpm.zeros(d1, d1)
        b = mpm.zeros(d1, 1)
        for i in range(d1):
            for j in range(i + 1):
                v = prec * sum((U[r][i] * U[r][j] for r in range(n)), mpm.mpf(0))
                if i == j:
                    v += kl + prec * SA[i]
                H[i, j] = H[j, i] = v
            b[i] = prec * (sum((t[r] * U[r][i] for r in range(n)), mpm.mpf(0)) - SC[i] / 2)
        theta = mpm.lu_solve(H, b)
        inv = (lambda s: s) if link == "abs" else (lambda s: mpm.log(mpm.expm1(s)))
        s = [inv(mpm.sqrt(kl / (kl + prec * SB[c]))) for c in range(d1)]
        theta = np.array([float(theta[c]) for c in range(d1)])
        s = np.array([float(v) for v in s])
    cH, cK = conds(ent, bia, scal, x, y, field, link, kl_weight, entity)
    return dict(n=n, theta=theta, s=s, cond_H=cH, cond_K=cK)


# ---------------------------------------------------------------------------------------------------------------------
# the kernel's dual path restated in numpy fp64
# ---------------------------------------------------------------------------------------------------------------------
def _wave_dot(V):
    """sum over the last axis as a wave does it: lane l adds elements l, l + 64, .. in order, then the xor butterfly."""
    k = V.shape[-1]
    pad = (-k) % 64
    if pad:
        V = np.concatenate([V, np.zeros(V.shape[:-1] + (pad,))], -1)
    V = V.reshape(V.shape[:-1] + (-1, 64))
    acc = np.zeros(V.shape[:-2] + (64,))
    for c in range(V.shape[-2]):
        acc = acc + V[..., c, :]
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., lane ^ o]
    return acc[..., 0]


def dual_fp64_in_kernel_order(ent, bia, scal, x, y, field, link, kl_weight, entity):
    """theta [d + 1] of an entity with n <= d rows by the kernel's dual path in numpy fp64, phase by phase: A the row sums
    in row order, D, 1 / D and D^-1 b; B the packed K = I / prec + U D^-1 U^T and U D^-1 b with a wave's summation order;
    C the left-looking Cholesky with the right-hand side as one more row and 1 / sqrt of the pivot, then the back
    substitution column by column; D theta = D^-1 b - D^-1 U^T z.  (numpy does not contract a * b + c: the roundings
    differ from the device's where it fuses, which the factor on e_ref in the tests allows for.)"""
    s = system64(ent, bia, scal, x, y, field, link, kl_weight, entity)
    n, d, prec, M = s["n"], s["d"], s["prec"], s["M"]
    assert n <= d, "the dual path is taken for n <= d"
    Di = 1.0 / s["D"]
    bv = s["b"] / s["D"]
    m = n
    L = np.zeros((m + 1, m))                               # rows 0 .. m - 1: the triangle; row m: the right-hand side
    if m:
        P = (M[:, None, :] * M[None, :, :]) * Di[None, None, 1:]
        K = _wave_dot(P) + Di[0]
        K[np.arange(m), np.arange(m)] += 1.0 / prec
        L[:m] = np.tril(K)
        L[m] = _wave_dot(M * bv[None, 1:]) + bv[0]
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
    yv, xv = L[m].copy() if m else np.zeros(0), np.zeros(m)
    for j in range(m - 1, -1, -1):
        xj = yv[j] * dv[j]
        yv[:j] -= L[j, :j] * xj
        xv[j] = xj
    theta = np.zeros(d + 1)
    acc = np.zeros(d + 1)
    for i in range(m):
        acc[0] += xv[i]
        acc[1:] += M[i] * xv[i]
    theta[:] = bv - Di * acc
    return theta


# ---------------------------------------------------------------------------------------------------------------------
# the metric
# ---------------------------------------------------------------------------------------------------------------------
def elementwise_ok(got_f32, ref, abs_term):
    """(ok, worst): ok iff |got_i - ref_i| <= 2^-23 |ref_i| + abs_term for every i; worst = the largest
    |got_i - ref_i| / (2^-23 |ref_i| + abs_term), for printing.  2^-23 |ref_i| is one fp32 rounding, doubled because ref
    may sit on a rounding boundary.  A NaN or infinity on either side is not ok."""
    got = np.asarray(_np(got_f32), np.float64).reshape(-1)
    ref = np.asarray(_np(ref), np.float64).reshape(-1)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not (np.isfinite(got).all() and np.isfinite(ref).all()):
        return False, float("inf")
    err = np.abs(got - ref)
    bound = EPS32 * np.abs(ref) + float(abs_term)
    ratio = np.where(err == 0.0, 0.0, err / np.where(bound > 0.0, bound, 1.0))
    ratio = np.where((bound == 0.0) & (err > 0.0), np.inf, ratio)
    return bool((err <= bound).all()), float(ratio.max()) if ratio.size else 0.0


def solve_abs_term(d, cond, ref):
    """4 (d + 1) 2^-52 cond max|ref|: the textbook backward-error bound of an fp64 Cholesky solve, once for the kernel
    and once for the fp64 oracle, doubled.  cond: cond(H) for a primal entity, cond(K) for a dual one."""
    ref = np.abs(np.asarray(_np(ref), np.float64))
    return 4.0 * (d + 1) * EPS64 * float(cond) * (float(ref.max()) if ref.size else 0.0)


def scale_abs_term(n, ref):
    """The scales have no solve in them: sigma_k^2 = kl / (kl + prec sum_r (A_rk + M_rk^2)), a sum of n positive terms in
    fp64 (relative error at most n 2^-53 in either order), a division, a square root and, under softplus,
    log(expm1(sigma)), whose derivative times sigma is at most 1.6 for sigma <= 1: an absolute error of at most
    (n + 8) 2^-53 max(1, |s|) for the kernel and as much for the oracle, doubled."""
    ref = np.abs(np.asarray(_np(ref), np.float64))
    return 4.0 * (n + 8) * 2.0 ** -53 * max(1.0, float(ref.max()) if ref.size else 0.0)


# ---------------------------------------------------------------------------------------------------------------------
# case builders: CPU tensors only
# ---------------------------------------------------------------------------------------------------------------------
def tables(sizes, d, seed, scale=0.5, scalars=(1.3, 0.2, 0.3)):
    """fp32 tables (ent [T, 2d], bia [T, 2], scal [3]) drawn as test_gpu_foldin._model draws them."""
    T = sum(sizes)
    g = torch.Generator().manual_seed(seed)
    ent = torch.randn(T, 2 * d, generator=g) * scale
    bia = torch.randn(T, 2, generator=g) * scale
    return ent, bia, torch.tensor(scalars, dtype=torch.float32)


def rows_with_counts(sizes, field, counts, seed, dup=True, dup_every_other=()):
    """Rows X [R, F], y [R] in which entity number k of `field` (ascending ids, so k is also its place in the launch)
    has counts[k] rows, the partners uniform in their fields; with dup, two rows of every entity of 7 rows or more are
    copies of its first; an entity whose number is in dup_every_other has every other row a copy of the row before it.
    The rows are shuffled so that the entities interleave."""
    g = torch.Generator().manual_seed(seed)
    lo = [sum(sizes[:f]) for f in range(len(sizes))]
    assert len(counts) <= sizes[field]
    ids = lo[field] + torch.sort(torch.randperm(sizes[field], generator=g)[:len(counts)]).values
    rows = []
    for k, n in enumerate(counts):
        x = torch.stack([torch.full((n,), int(ids[k])) if f == field
                         else lo[f] + torch.randint(0, sizes[f], (n,), generator=g) for f in range(len(sizes))], 1)
        if k in dup_every_other:
            x[1::2] = x[0:n - n % 2:2]
        elif dup and n >= 7:
            x[-1] = x[0]
            x[-2] = x[0]
        rows.append(x)
    X = torch.cat(rows) if rows else torch.zeros(0, len(sizes), dtype=torch.int64)
    X = X[torch.randperm(X.shape[0], generator=g)]
    y = torch.randn(X.shape[0], generator=g) + 3.0
    return X, y, ids


def case(sizes, field, d, link, counts, seed, kl_weight=1.0, **kw):
    """One fold-in case: dict(sizes, field, d, link, kl_weight, counts, ent, bia, scal, X, y, ids)."""
    tk = {k: kw.pop(k) for k in ("scale", "scalars") if k in kw}
    ent, bia, scal = tables(sizes, d, seed, **tk)
    X, y, ids = rows_with_counts(sizes, field, counts, seed + 1, **kw)
    return dict(sizes=tuple(sizes), field=field, d=d, link=link, kl_weight=f32(kl_weight), counts=list(counts), ent=ent,
                bia=bia, scal=scal, X=X, y=y, ids=ids)


# ---- 3.1: storage and width edges in one launch
def width_counts(d, lds=None, fb=None):
    lds, fb = LDS if lds is None else lds, FB if fb is None else fb
    return [1, lds - 1, lds, lds + 1, fb - 1, fb, fb + 1, d - 1, d, d + 1]


def largest_dual_counts(d, fb=None):
    return [(FB if fb is None else fb) + 1, d - 1, d, d + 1]


def width_case(link):
    return case((400, 12, 300), 1, 300, link, width_counts(300), seed=31 + (link == "softplus"))


def largest_dual_case(link):
    # (kl_weight = 2: cond(K) is about 1 + prec n / kl_weight, which at n = 512 would pass 1e3 under softplus with 1)
    return case((600, 8, 500), 1, 512, link, largest_dual_counts(512), seed=41 + (link == "softplus"), kl_weight=2.0)


# ---- 3.2: the slab rule
def slab_rule_ds(lds=None):
    """(the largest d without slabs, the smallest with), by the rule d + 1 > cap_dim."""
    lds = LDS if lds is None else lds
    return lds - 1, lds


def slab_rule_counts(d):
    return [d - 1, d, d + 1, d + 40]


def slab_rule_case(d, link):
    return case((30, 400), 0, d, link, slab_rule_counts(d), seed=51 + d)


def past_cap_counts(d, slabs=None, lds=None):
    """SLABS + 5 entities: five row counts cycling over the first SLABS, and each of the last five of the other storage
    than the entity SLABS places before it, which the same block solved first."""
    slabs = SLABS if slabs is None else slabs
    cyc = [1, d - 1, d, d + 1, d + 40]
    counts = [cyc[g % 5] for g in range(slabs)]
    for b in range(5):
        first = storage(counts[b], d, lds=lds)
        counts.append(next(c for c in reversed(cyc) if storage(c, d, lds=lds) != first))
    return counts


def past_cap_case(link="abs"):
    d = slab_rule_ds()[1]
    return case((SLABS + 40, 400), 0, d, link, past_cap_counts(d), seed=61)


# ---- 3.3: past the slab grid cap, bitwise
BITWISE_D = 5
BITWISE_LDS_DIMS = (-1, 0, 3)


def bitwise_counts(slabs=None):
    slabs = SLABS if slabs is None else slabs
    return [1 + g % 12 for g in range(2 * slabs + 37)]


def bitwise_case():
    return case((2 * SLABS + 60, 30, 7), 0, BITWISE_D, "softplus", bitwise_counts(), seed=71, kl_weight=0.75)


def bitwise_sample(E):
    """16 of the E entities for the comparison with fp64: one of each trip of block 0 and 13 drawn."""
    g = torch.Generator().manual_seed(5)
    rest = torch.randperm(E, generator=g).tolist()
    picks = [0, SLABS, 2 * SLABS]
    picks += [r for r in rest if r not in picks][:13]
    return sorted(picks)


def case_conds(c, which=None):
    """cond of the matrix the kernel factors, for the entities number `which` (default: all) of a case."""
    which = range(len(c["counts"])) if which is None else which
    return [cond_of_the_factored(c["ent"], c["bia"], c["scal"], c["X"], c["y"], c["field"], c["link"], c["kl_weight"],
                                 int(c["ids"][k])) for k in which]


# ---- 3.4: sessions across the same edges: (d, history rows, rounds)
def session_cases(lds=None, fb=None):
    lds, fb = LDS if lds is None else lds, FB if fb is None else fb
    return [(200, lds - 2, 5), (300, fb - 2, 4), (lds - 1, lds - 3, 4), (lds, lds - 2, 4)]


def session_systems(d, n_hist, Q):
    """The size and the storage of the system of each round of the respondent with n_hist history rows."""
    return [(solve_dim(n_hist + q + 1, d), storage(n_hist + q + 1, d)) for q in range(Q)]


# ---- 3.5: the conditioning of the dual path
KCOND_KL = f32(1e-4)
KCOND_DS = (8, 64)


def kcond_counts(d):
    """n = 1, d / 2 with every other row a duplicate, d (the largest dual) and d + 1 (the primal control)."""
    return [1, d // 2, d, d + 1]


def kcond_case(d, link):
    """Planted tables for the use on a trained model: a small kl_weight and a sharp likelihood (prec about 50), the
    partners' scales spread log-uniformly from 1e-3 to 2.  K = I / prec + U D^-1 U^T with D_0 = kl_weight alone."""
    sizes = (8, 200)
    c = case(sizes, 0, d, link, kcond_counts(d), seed=81 + d + (link == "softplus"), kl_weight=KCOND_KL, dup=False,
             dup_every_other=(1,), scalars=(50.0, 0.2, 0.3))
    g = torch.Generator().manual_seed(7 + d)
    sig = torch.exp(torch.rand(sum(sizes), d, generator=g) * (math.log(2.0) - math.log(1e-3)) + math.log(1e-3))
    c["ent"][:, d:] = sig if link == "abs" else torch.log(torch.expm1(sig.double())).float()
    return c


@functools.lru_cache(maxsize=None)
def kcond_references(d, link):
    """(case, per entity dict(n, ref = optimum_mp's result, e_ref)): e_ref, the yardstick of a dual entity, is the
    max-abs distance of dual_fp64_in_kernel_order from optimum_mp on the same inputs (None for the primal control)."""
    c = kcond_case(d, link)
    out = []
    for k, n in enumerate(c["counts"]):
        args = (c["ent"], c["bia"], c["scal"], c["X"], c["y"], c["field"], link, c["kl_weight"], int(c["ids"][k]))
        ref = optimum_mp(*args)
        assert ref["n"] == n
        e_ref = float(np.abs(dual_fp64_in_kernel_order(*args) - ref["theta"]).max()) if n <= d else None
        out.append(dict(n=n, ref=ref, e_ref=e_ref))
    return c, out

"""Case builders, references and input conditions for the tests of the implicit-feedback solves
(vae_amd/csrc_rank/vfm_implicit.hip) at their own edges: tests/test_implicit_edges_cpu.py checks the references and the
conditions each case must meet, tests/test_gpu_implicit_edges.py runs the same cases on the kernels.

  Reference, reference()       the fp64 solve and loss of any of the four forms (plain, prior, weights, prior_weights)
                               from the dense definition, the partner field's operands built once per case
  existing_reference()         the same through implicit_reference / implicit_prior_reference /
                               implicit_weights_reference as they are (the CPU file holds the two together at d = 9)
  compare()                    the project's elementwise bound on the rows of a solve
  optimum_mp()                 one entity's optimum with mpmath at 50 digits (the conditioning cases)
  LDS, SLABS, FB, GRID_CAP     the constants, parsed from the sources

Every edge below is an expression in LDS, SLABS, FB and GRID_CAP.  CPU tensors only: nothing here needs a GPU."""
import functools
import math
import os
import re

import numpy as np
import torch

import implicit_prior_reference as IPR
import implicit_reference as IR
import implicit_weights_reference as IWR
import prior_reference as P
import solve_reference as R
from test_gpu_fit_implicit import CHUNK, KLW, W0, W1, _case

LDS, SLABS, FB = R.LDS, R.SLABS, R.FB
FORMS = ("plain", "prior", "weights", "prior_weights")
LINKS = ("abs", "softplus")
RATIO = 16.0                                             # weights in [W0, 16 W0]
TL = 4                                                   # the edge of a register tile of share_of


def read_grid_cap(root=R.ROOT):
    """The grid cap of k_implicit_base, k_implicit_chunks and (without slabs) k_implicit_solve.  Each of the two entry
    points of vfm_implicit.hip states it in a `gcap` of its own: every statement must give the one value."""
    src = open(os.path.join(root, "vae_amd", "csrc_rank", "vfm_implicit.hip")).read()
    caps = re.findall(r"const\s+int64_t\s+gcap\s*=\s*\(int64_t\)\s*1\s*<<\s*(\d+)\s*;", src)
    assert caps and len(set(caps)) == 1, caps
    return 1 << int(caps[0])


GRID_CAP = read_grid_cap()


def trips(n, stride=None):
    """The trips of `for (c = tid; c < n; c += FB)` of the busiest thread."""
    return -(-n // (FB if stride is None else stride))


def tiles(d):
    """The 4 x 4 register tiles of the packed triangle of d + 1."""
    return R.tri((d + 1 + TL - 1) // TL)


def threshold(split_rows, d):
    """sweep.resolve_split_rows for an integer: an entity with more observed rows goes through chunk slabs."""
    return max(split_rows, d + 1)


# ---------------------------------------------------------------------------------------------------------------------
# the fp64 reference of the four forms, the partner field's operands built once
# ---------------------------------------------------------------------------------------------------------------------
def prior_of(c, field):
    """(m [d + 1], lam [d + 1]) fp64 of the folded field, or None."""
    return None if c.get("prior") is None else (c["prior"][0][field], c["prior"][1][field])


class Reference:
    """The dense definition of one case and form: every partner of the folded entity is a row, an observed one with
    its target and weight (W1, or its own under a weights form), every other with target 0 and weight W0; under a prior
    form the entity's prior is the folded field's N(m, 1 / lam).  tab: the tables the kernel reads."""

    def __init__(self, tab, c, form, field=None):
        assert form in FORMS
        self.c, self.form = c, form
        self.field = f = c["field"] if field is None else field
        self.N, self.M, self.link = c["N"], c["M"], c["link"]
        self.klw, self.w0 = c.get("klw", KLW), W0
        ent, bia, scal = tab
        self.ids, self.u, self.A, self.cm, self.cv = IR._partners(ent, bia, scal, f, self.N, self.M, self.link)
        self.prec = IR.link_t(scal[0], self.link)
        d1 = self.u.shape[1]
        pr = prior_of(c, f) if "prior" in form else None
        self.m, self.lam = (torch.zeros(d1, dtype=torch.float64), torch.ones(d1, dtype=torch.float64)) if pr is None else \
            (pr[0].double(), pr[1].double())
        x = c["x"]
        self.wr = c["w"].double() if "weights" in form else torch.full((x.shape[0],), float(W1), dtype=torch.float64)
        self.order = torch.sort(x[:, f], stable=True).indices if x.shape[0] else torch.zeros(0, dtype=torch.int64)
        self.key = x[self.order, f].contiguous() if x.shape[0] else torch.zeros(0, dtype=torch.int64)

    def rows(self, e):
        """(w [n], t [n]) of entity e over all partners."""
        n = self.ids.numel()
        w = torch.full((n,), float(self.w0), dtype=torch.float64)
        t = torch.zeros(n, dtype=torch.float64)
        lo, hi = torch.searchsorted(self.key, torch.tensor([e, e + 1])).tolist()
        if hi > lo:
            r = self.order[lo:hi]
            j = self.c["x"][r, 1 - self.field] - int(self.ids[0])
            w[j] = self.wr[r]
            t[j] = self.c["y"][r].double()
        return w, t

    def system(self, e):
        """(H, b, SB' [d + 1]): H = kl diag(lam) + prec sum_j w_j (u_j u_j^T + diag(0, A_j)), b = prec sum_j w_j
        (t_j - c_mean_j) u_j + kl lam m."""
        w, t = self.rows(e)
        u, A = self.u, self.A
        H = torch.diag(self.klw * self.lam) + self.prec * (u.T @ (w[:, None] * u) + torch.diag((w[:, None] * A).sum(0)))
        b = self.prec * (u.T @ (w * (t - self.cm))) + self.klw * self.lam * self.m
        return H, b, (w[:, None] * (A + u * u)).sum(0)

    def solve(self, ids):
        ids = torch.as_tensor(ids, dtype=torch.int64)
        th, sg, cond = [], [], []
        for e in ids.tolist():
            H, b, SB = self.system(e)
            th.append(torch.linalg.solve(H, b))
            sg.append(torch.sqrt(self.klw / (self.klw * self.lam + self.prec * SB)))
            cond.append(torch.linalg.cond(H))
        return {"ids": ids, "theta": torch.stack(th), "sigma": torch.stack(sg), "cond": torch.stack(cond)}

    def loss(self, e, theta, sigma):
        """L_e at (theta, sigma) [d + 1], row by row over all partners."""
        w, t = self.rows(e)
        theta, sigma = theta.double(), sigma.double()
        res = t - self.cm - self.u @ theta
        var = self.cv + self.A @ (theta * theta) + (self.A + self.u * self.u) @ (sigma * sigma)
        rows = w * (0.5 * self.prec * (res * res + var) - 0.5 * torch.log(self.prec) + IR.LOG_2PI_HALF)
        return float(rows.sum() + self.klw * IPR.kl_prior(theta, sigma, self.m, self.lam).sum())


def reference(form, tab, c, ids, field=None):
    """The dispatcher: (the fp64 solve of the entities ids, loss(e, theta, sigma) in fp64) of any of the four forms."""
    ref = Reference(tab, c, form, field)
    return ref.solve(ids), ref.loss


def existing_reference(form, tab, c, ids, field=None):
    """reference() through the three reference modules as they are (a Python loop per entity, the partners rebuilt)."""
    f = c["field"] if field is None else field
    klw = c.get("klw", KLW)
    a = (*tab, c["x"], c["y"])
    g = (f, c["N"], c["M"], c["link"])
    pr = prior_of(c, f)
    if form == "plain":
        return (IR.implicit_solve_fp64(*a, *g, W0, W1, klw, entities=ids),
                lambda e, th, sg: float(IR.entity_loss_fp64(*a, *g, W0, W1, klw, e, th, sg)))
    if form == "prior":
        return (IPR.implicit_solve_fp64_prior(*a, *g, W0, W1, klw, *pr, entities=ids),
                lambda e, th, sg: float(IPR.entity_loss_fp64_prior(*a, *g, W0, W1, klw, e, th, sg, *pr)))
    pr = pr if form == "prior_weights" else None
    return (IWR.implicit_solve_fp64(*a, c["w"], *g, W0, klw, entities=ids, prior=pr),
            lambda e, th, sg: float(IWR.entity_loss_fp64(*a, c["w"], *g, W0, klw, e, th, sg, pr)))


def compare(c, sol, theta, s, field=None, cond_range=(0.0, 1e3)):
    """The rows (theta [E, d + 1], s [E, d + 1], fp32) of sol's entities against sol per element:
    |got - ref| <= 2^-23 |ref| + 4 (d + 1) 2^-52 cond(H) max|ref| for the means, scale_abs_term over 2 n_dense for the
    raw scales, after the condition on cond(H).  Returns (worst ratio, list of the entities that miss)."""
    f = c["field"] if field is None else field
    d, link = c["d"], c["link"]
    cond = sol["cond"]
    assert cond_range[0] <= float(cond.min()) and float(cond.max()) <= cond_range[1], (cond.min(), cond.max())
    n_dense = c["M"] if f == 0 else c["N"]
    rs = IR.inv_link_t(sol["sigma"], link)
    worst, bad = 0.0, []
    for i, e in enumerate(sol["ids"].tolist()):
        rt = sol["theta"][i].numpy()
        ok_t, w_t = R.elementwise_ok(theta[i], rt, R.solve_abs_term(d, float(cond[i]), rt))
        ok_s, w_s = R.elementwise_ok(s[i], rs[i].numpy(), R.scale_abs_term(2 * n_dense, rs[i].numpy()))
        if not (ok_t and ok_s):
            bad.append((e, w_t, w_s))
        worst = max(worst, w_t, w_s)
    return worst, bad


def rounded(sol, link):
    """The reference itself as a kernel would write it: (theta, raw scales) rounded to fp32."""
    return sol["theta"].float(), IR.inv_link_t(sol["sigma"], link).float()


# ---------------------------------------------------------------------------------------------------------------------
# case builders
# ---------------------------------------------------------------------------------------------------------------------
def edge_case(n_folded, n_partner, d, link, counts, seed, field=0, **kw):
    """test_gpu_fit_implicit._case with what the four forms need: c["w"], a weight per row in [W0, 16 W0], and c["prior"]
    = (mean [2, d + 1], prec [2, d + 1]), fp32 values held in fp64 (means in [-0.5, 0.5], precisions in
    prior_reference.prec_lo_for(d) .. 16)."""
    c = _case(n_folded, n_partner, d, link, counts, seed, field=field)
    c["w"] = IWR.draw_weights(c["x"].shape[0], W0, seed + 7, RATIO)
    c["prior"] = P.draw_priors(2, d, seed + 11, P.prec_lo_for(d))
    c.update(kw)
    return c


def folded_ids(c):
    lo = 0 if c["field"] == 0 else c["N"]
    return torch.arange(lo, lo + len(c["counts"]))


# ---- 1. width: d = 300 and d = 512
WIDTH_DS = (300, 512)


def width_counts(d):
    return [0, 1, FB - 1, FB + 1, d + 2, CHUNK * (d // CHUNK + 2) + 1]


def width_partners(d):
    return 2 * d + 40 if d < 512 else 600


def width_split(d):
    return d + 3


@functools.lru_cache(maxsize=None)
def width_case(d, link):
    counts = width_counts(d)
    return edge_case(len(counts), width_partners(d), d, link, counts, seed=1300 + d + (link == "softplus"))


# ---- 2. the slab rule past its grid cap at a real slab d
PAST_CAP_PARTNERS = 48


def past_cap_counts(n=PAST_CAP_PARTNERS):
    """Entities 0 .. 4 and SLABS .. SLABS + 4 have observed rows; every other of the SLABS + 15 has none, so that the
    call of the entities without rows has SLABS + 5 of them and blocks 0 .. 4 solve twice.  (With SLABS + 5 entities
    in all the empty call would have SLABS - 5.  The catalog is smaller than d + 1, so no entity here can be split: the
    chunk form at a slab d is the width case's.)"""
    counts = [0] * (SLABS + 15)
    counts[:5] = [1, 3, n // 2, n - 1, n]
    counts[SLABS:SLABS + 5] = [n, 2, 5, n - 15, 1]
    return counts


@functools.lru_cache(maxsize=None)
def past_cap_case():
    counts = past_cap_counts()
    return edge_case(len(counts), PAST_CAP_PARTNERS, LDS, "abs", counts, seed=1400)


# ---- 3. past the slab grid cap, bitwise, through lds_dim
BITWISE_D, BITWISE_LDS_DIMS = R.BITWISE_D, R.BITWISE_LDS_DIMS
BITWISE_SPLIT, BITWISE_PARTNERS = 20, 130
BITWISE_HEAVY = (100, 61, 47)


def bitwise_counts():
    """Three runs of ids, one per call the plan makes, each long enough for its call to pass the slab grid cap:
    2 SLABS + 37 light entities of 1 .. 11 rows (block 0 takes the entities 0, SLABS and 2 SLABS of the call), 2 SLABS + 1
    heavy ones (more than BITWISE_SPLIT rows: the chunk form), those of 100, 61 and 47 rows at block 0's first, second
    and third trip, and SLABS + 5 without rows.  (One population of 2 SLABS + 37 with counts 0 .. 11 and three heavy
    entities gives calls of about 500, 3 and 46 entities: only the first passes the cap, and block 0 has no third trip.)"""
    light = [1 + g % 11 for g in range(2 * SLABS + 37)]
    heavy = [BITWISE_SPLIT + 1 + g % 3 for g in range(2 * SLABS + 1)]
    for k, n in enumerate(BITWISE_HEAVY):
        heavy[k * SLABS] = n
    return light + heavy + [0] * (SLABS + 5)


def bitwise_calls(counts=None):
    """The entity numbers of the light, the heavy-group and the empty call, in the order of each launch (ascending ids)."""
    counts = bitwise_counts() if counts is None else counts
    thr = threshold(BITWISE_SPLIT, BITWISE_D)
    light = [g for g, n in enumerate(counts) if 0 < n <= thr]
    heavy = [g for g, n in enumerate(counts) if n > thr]
    empty = [g for g, n in enumerate(counts) if n == 0]
    return light, heavy, empty


@functools.lru_cache(maxsize=None)
def bitwise_case():
    counts = bitwise_counts()
    return edge_case(len(counts), BITWISE_PARTNERS, BITWISE_D, "softplus", counts, seed=1500)


def bitwise_sample(c):
    """16 entities for the comparison with fp64, picked as solve_reference.bitwise_sample picks: block 0's three trips
    of the light call, of the heavy call and one entity without rows of the first and of the second trip, the rest drawn."""
    light, heavy, empty = bitwise_calls(c["counts"])
    picks = [call[k * SLABS] for call in (light, heavy) for k in range(3)] + [empty[0], empty[SLABS]]
    g = torch.Generator().manual_seed(5)
    rest = torch.randperm(len(c["counts"]), generator=g).tolist()
    picks += [r for r in rest if r not in picks][:16 - len(picks)]
    return sorted(picks)


def row_lists(c, ids):
    """The row-list form of the entities ids (valid ids of field 0, in the order given): (partner [R], y [R], w [R],
    row_ptr [E + 1]), an entity's rows in the order of c["x"]."""
    x = c["x"]
    order = torch.sort(x[:, 0], stable=True).indices
    key = x[order, 0].contiguous()
    ids = torch.as_tensor(ids, dtype=torch.int64)
    lo, hi = torch.searchsorted(key, ids), torch.searchsorted(key, ids + 1)
    sel = torch.cat([order[a:b] for a, b in zip(lo.tolist(), hi.tolist())]) if ids.numel() else order[:0]
    ptr = torch.zeros(ids.numel() + 1, dtype=torch.int64)
    torch.cumsum(hi - lo, 0, out=ptr[1:])
    return x[sel, 1].contiguous(), c["y"][sel].contiguous(), c["w"][sel].contiguous(), ptr


# ---- 4. the 2^20 caps of the base and the chunk pass
CAP_FORMS = ("plain", "weights")
CAP_ENTITIES = 64


def cap_partners():
    return GRID_CAP + 3


def cap_rows_per_entity():
    """So that the CAP_ENTITIES entities have more than GRID_CAP rows together, a row per chunk."""
    return GRID_CAP // CAP_ENTITIES + 1


@functools.lru_cache(maxsize=None)
def cap_case():
    """d = 1, abs, CAP_ENTITIES folded entities and GRID_CAP + 3 partners; every entity has cap_rows_per_entity() distinct
    partners, a run of consecutive ids from a start of its own (wrapping), so that the rows are cheap to draw."""
    E, n, k = CAP_ENTITIES, cap_partners(), cap_rows_per_entity()
    g = torch.Generator().manual_seed(1600)
    T = E + n                                                          # (tables drawn as implicit_reference.planted draws)
    ent = torch.cat([torch.randn(T, 1, generator=g, dtype=torch.float64) * 0.3,
                     torch.rand(T, 1, generator=g, dtype=torch.float64) * 0.4 + 0.2], 1).float()
    bia = torch.stack([torch.randn(T, generator=g, dtype=torch.float64) * 0.3,
                       torch.rand(T, generator=g, dtype=torch.float64) * 0.4 + 0.2], 1).float()
    scal = torch.tensor((1.3, 0.2, 0.3), dtype=torch.float32)
    start = torch.randint(0, n, (E,), generator=g)
    j = (start[:, None] + 7 * torch.arange(k)[None, :]) % n            # (distinct while 7 k < n)
    assert 7 * k < n
    x = torch.stack([torch.arange(E)[:, None].expand(E, k).reshape(-1), E + j.reshape(-1)], 1)
    y = (torch.randn(E * k, generator=g) * 0.5 + 1.0).float()
    c = dict(N=E, M=n, d=1, link="abs", field=0, ent=ent, bia=bia, scal=scal, x=x, y=y, counts=[k] * E, sizes=(E, n))
    c["w"] = IWR.draw_weights(E * k, W0, 1607, RATIO)
    c["prior"] = None
    return c


def base_fp64(c):
    """(the base block of the partner field of field 0 [imp_doubles(d)], the sum of the absolute terms of each element)
    in numpy fp64 from the tables: [triangle of sum u u^T | sum A | sum (A + M^2), n for coordinate 0 | sum t u | sum q]
    with u = (1, mu), t = -c_mean, q = c_mean^2 + c_var."""
    d, N, M = c["d"], c["N"], c["M"]
    ent, bia, scal = (t.double().numpy() for t in (c["ent"], c["bia"], c["scal"]))
    lk = lambda s: R._link64(s, c["link"])
    mu = ent[N:N + M, :d]
    u = np.concatenate([np.ones((M, 1)), mu], 1)
    A = np.concatenate([np.zeros((M, 1)), lk(ent[N:N + M, d:]) ** 2], 1)
    cm = scal[1] + bia[N:N + M, 0]
    cv = lk(scal[2]) ** 2 + lk(bia[N:N + M, 1]) ** 2
    out, mag = [], []
    for i in range(d + 1):
        for j in range(i + 1):
            out.append((u[:, i] * u[:, j]).sum())
            mag.append(np.abs(u[:, i] * u[:, j]).sum())
    SB = (A + u * u)
    SB[:, 0] = 1.0
    for v in (A, SB, -cm[:, None] * u):
        out += list(v.sum(0))
        mag += list(np.abs(v).sum(0))
    out.append((cm * cm + cv).sum())
    mag.append((cm * cm + cv).sum())
    return np.array(out), np.array(mag)


# ---- 5. conditioning
COND_DS, COND_KL = R.KCOND_DS, R.KCOND_KL
COND_FORMS = ("plain", "weights")
COND_RANGE = (1e5, 1e7)
COND_PARTNERS = {8: 100, 64: 200}


def cond_counts(d):
    return [0, 3, d + 2, CHUNK * (d // CHUNK + 2) + 1]


def cond_split(d):
    return d + 3


@functools.lru_cache(maxsize=None)
def cond_case(d, link):
    """A trained catalog: the partners' means B z_j plus noise of size 1e-3 with B of rank d / 2, every scale of the
    catalog about 1e-3 (abs: raw +-1e-3, either sign; softplus: raw in [-7, -6]) and kl_weight = 1e-4."""
    counts = cond_counts(d)
    n = COND_PARTNERS[d]
    c = edge_case(len(counts), n, d, link, counts, seed=1700 + d + (link == "softplus"), klw=COND_KL)
    N = c["N"]
    g = torch.Generator().manual_seed(1750 + d)
    k = d // 2
    B = torch.randn(d, k, generator=g, dtype=torch.float64) * (0.3 / math.sqrt(k))
    z = torch.randn(n, k, generator=g, dtype=torch.float64)
    mu = z @ B.T + 1e-3 * torch.randn(n, d, generator=g, dtype=torch.float64)
    r = torch.rand(n, d + 1, generator=g, dtype=torch.float64)
    if link == "abs":
        sign = torch.where(torch.rand(n, d + 1, generator=g) < 0.5, -1.0, 1.0).double()
        raw = sign * (0.5e-3 + 1e-3 * r)
    else:
        raw = -7.0 + r
    c["ent"][N:N + n, :d] = mu.float()
    c["ent"][N:N + n, d:] = raw[:, 1:].float()
    c["bia"][N:N + n, 1] = raw[:, 0].float()
    return c


@functools.lru_cache(maxsize=None)
def _catalog_mp(d, link):
    """The catalog of cond_case(d, link) in mpmath: per partner u [d + 1], A [d + 1], c_mean, and the sums over every
    partner that all entities share: G = sum u u^T (lower triangle), sum A, sum c_mean u."""
    mpm = R._mpmath()
    c = cond_case(d, link)
    N, M = c["N"], c["M"]
    ent, bia, scal = (t.numpy() for t in (c["ent"], c["bia"], c["scal"]))
    with mpm.mp.workdps(50):
        F_ = lambda v: mpm.mpf(float(v))
        lk = (lambda s: abs(s)) if link == "abs" else (lambda s: mpm.log(1 + mpm.exp(s)))
        U = [[mpm.mpf(1)] + [F_(v) for v in ent[N + j, :d]] for j in range(M)]
        A = [[mpm.mpf(0)] + [lk(F_(v)) ** 2 for v in ent[N + j, d:]] for j in range(M)]
        cm = [F_(scal[1]) + F_(bia[N + j, 0]) for j in range(M)]
        cols = [[U[j][i] for j in range(M)] for i in range(d + 1)]
        G = [[mpm.fsum(a * b for a, b in zip(cols[i], cols[k])) for k in range(i + 1)] for i in range(d + 1)]
        sA = [mpm.fsum(A[j][i] for j in range(M)) for i in range(d + 1)]
        sC = [mpm.fsum(cm[j] * cols[i][j] for j in range(M)) for i in range(d + 1)]
        prec, kl = lk(F_(scal[0])), F_(c["klw"])
    return dict(U=U, A=A, cm=cm, G=G, sA=sA, sC=sC, prec=prec, kl=kl)


def optimum_mp(d, link, form, e):
    """Entity e of cond_case(d, link) under the plain or the weights form with mpmath at 50 digits from the fp32 table
    values: H = kl I + prec sum_j w_j (u_j u_j^T + diag(0, A_j)) and b = prec sum_j w_j (t_j - c_mean_j) u_j over every
    partner j (the sum over the catalog at weight W0 is shared by the entities and the observed rows add w_r - W0 and
    w_r y_r to it, which at 50 digits is the dense sum), the LU solve, sigma_c^2 = kl / (kl + prec sum_j w_j (A_j + u_j^2))
    and the inverse link.  Returns dict(theta [d + 1], s [d + 1]) rounded to fp64."""
    assert form in COND_FORMS
    mpm = R._mpmath()
    c = cond_case(d, link)
    cat = _catalog_mp(d, link)
    d1 = d + 1
    x, N = c["x"], c["N"]
    sel = (x[:, 0] == e).nonzero().reshape(-1).tolist()
    with mpm.mp.workdps(50):
        F_ = lambda v: mpm.mpf(float(v))
        w0, prec, kl = F_(W0), cat["prec"], cat["kl"]
        H = mpm.zeros(d1, d1)
        for i in range(d1):
            for k in range(i + 1):
                H[i, k] = w0 * cat["G"][i][k]
        dA = [w0 * v for v in cat["sA"]]
        b = [-w0 * v for v in cat["sC"]]
        SB = [w0 * (cat["sA"][i] + cat["G"][i][i]) for i in range(d1)]
        for r in sel:
            j = int(x[r, 1]) - N
            wr = F_(c["w"][r]) if form == "weights" else F_(W1)
            g, u, A = wr - w0, cat["U"][j], cat["A"][j]
            gu = [g * v for v in u]
            for i in range(d1):
                for k in range(i + 1):
                    H[i, k] += gu[i] * u[k]
                dA[i] += g * A[i]
                SB[i] += g * (A[i] + u[i] * u[i])
                b[i] += (wr * F_(c["y"][r]) - g * cat["cm"][j]) * u[i]
        for i in range(d1):
            for k in range(i + 1):
                H[i, k] = H[k, i] = prec * H[i, k]
            H[i, i] += kl + prec * dA[i]
        theta = mpm.lu_solve(H, mpm.matrix([prec * v for v in b]))
        inv = (lambda s: s) if link == "abs" else (lambda s: mpm.log(mpm.expm1(s)))
        s = [inv(mpm.sqrt(kl / (kl + prec * SB[i]))) for i in range(d1)]
        return dict(theta=np.array([float(theta[i]) for i in range(d1)]), s=np.array([float(v) for v in s]))


@functools.lru_cache(maxsize=None)
def cond_references(d, link, form):
    """(case, sol): the fp64 solve's conditions and ids with theta and sigma replaced by the mpmath optimum; sol["fp64"]
    keeps the torch fp64 theta for the CPU file."""
    c = cond_case(d, link)
    tab = (c["ent"], c["bia"], c["scal"])
    sol, _ = reference(form, tab, c, folded_ids(c))
    mp = [optimum_mp(d, link, form, e) for e in sol["ids"].tolist()]
    out = dict(sol, fp64=sol["theta"], fp64_sigma=sol["sigma"])
    out["theta"] = torch.tensor(np.stack([m["theta"] for m in mp]))
    s = torch.tensor(np.stack([m["s"] for m in mp]))
    out["sigma"] = IR.link_t(s, link)                                  # (compare() takes sigma and inverts the link)
    out["s"] = s
    return c, out


# ---- 6. signed and small raw scales
SIGN_D = 9
SOFTPLUS_RAW_RANGE = (-8.0, 3.0)
SOFTPLUS_S0 = -3.0


def sign_counts():
    """The d = 9 case of test_gpu_fit_implicit.test_solve_matches_fp64."""
    split = threshold(20, SIGN_D)
    k = split // CHUNK + 2
    return [0, 1, SIGN_D, SIGN_D + 1, split, split + 1, CHUNK * k - 1, CHUNK * k, CHUNK * k + 1, CHUNK * 40]


@functools.lru_cache(maxsize=None)
def sign_case(link, field):
    counts = sign_counts()
    return edge_case(len(counts) + 1, CHUNK * 40 + 5, SIGN_D, link, counts, seed=500 + SIGN_D, field=field)


def flipped(c):
    """c with the sign of every second raw scale of both tables, of scal[0] (the precision) and of scal[2] flipped."""
    f = dict(c, ent=c["ent"].clone(), bia=c["bia"].clone(), scal=c["scal"].clone())
    d = c["d"]
    flat = f["ent"][:, d:].reshape(-1)                                  # (a copy: every second element of the block)
    flat[1::2] *= -1.0
    f["ent"][:, d:] = flat.reshape(-1, d)
    f["bia"][1::2, 1] *= -1.0
    f["scal"][0] *= -1.0
    f["scal"][2] *= -1.0
    return f


@functools.lru_cache(maxsize=None)
def small_scale_case(field):
    """sign_case("softplus", field) with every raw scale of both tables uniform in SOFTPLUS_RAW_RANGE -- the negative raw
    values a solve itself writes -- and scal[2] = SOFTPLUS_S0."""
    c = sign_case("softplus", field)
    c = dict(c, ent=c["ent"].clone(), bia=c["bia"].clone(), scal=c["scal"].clone())
    g = torch.Generator().manual_seed(1800 + field)
    lo, hi = SOFTPLUS_RAW_RANGE
    d = c["d"]
    c["ent"][:, d:] = (lo + (hi - lo) * torch.rand(c["ent"].shape[0], d, generator=g)).float()
    c["bia"][:, 1] = (lo + (hi - lo) * torch.rand(c["bia"].shape[0], generator=g)).float()
    c["scal"][2] = SOFTPLUS_S0
    return c

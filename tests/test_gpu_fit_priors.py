"""GPU: the exact solves under a learnt field prior (include/vfm_prior.h; VFM.fold_in_exact(priors=),
VFM.fold_in_objective(priors=), VFM.exact_objective(priors=)) and the hierarchical sweeps of
VFM.fit_exact(learn_priors=True), against the fp64 restatement of tests/prior_reference.py.

Bounds: those of tests/test_gpu_fit_exact.py.  Rows written by a solve: per element |got - ref| <= 2^-23 |ref| +
4 (d + 1) 2^-52 cond max|ref| against solve_fp64_prior (solve_reference.elementwise_ok / solve_abs_term /
scale_abs_term); the priors are drawn with means in [-0.5, 0.5] and precisions in [0.25, 16], and the condition number of
every matrix that is factored is computed in fp64 and asserted under COND_MAX = 78.4, the worst DESIGN.md records for the
cases of the bound sweeps' tests; for d >= 128 that needs the precisions drawn from the upper part of their range
(prior_reference.prec_lo_for).  Losses and J: 1e-5 relative.  The prior block, computed by torch in fp64 and rounded once:
2^-23 |ref| (elementwise_ok with no absolute term).  J after a block: J_after <= J_before + 1e-9 |J_before|.

Every test here fails on the parent of this feature: the priors= arguments and the entry points do not exist there."""
import functools

import numpy as np
import pytest
import torch

import fit_exact_restatement as FR
import prior_reference as P
import solve_reference as R
from test_gpu_solve_edges import _model_of, _written, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
LINKS = ["abs", "softplus"]
CHUNK = 8
COND_MAX = 78.4


def _priors_of(c, seed, standard=False):
    from vae_amd import sweep
    F, d = len(c["sizes"]), c["d"]
    pr = sweep.GroupPriors(F, d, DEV)
    if not standard:
        mean, prec = P.draw_priors(F, d, seed, P.prec_lo_for(d))
        pr.load_state_dict({"mean": mean.float(), "prec": prec.float()})
    return pr


def _fold(c, m, pr, X=None, y=None, **kw):
    X, y = (c["X"], c["y"]) if X is None else (X, y)
    return m.fold_in_exact(X.to(DEV), y.to(DEV), field=c["field"], kl_weight=c["kl_weight"], priors=pr, **kw)


def _check(c, m, loss, pr, what, which=None):
    """The written rows of the entities number `which` of case c (default: all) against solve_fp64_prior per element,
    the returned loss against the restated L_e at the written rows.  Returns the worst elementwise ratio."""
    which = list(range(len(c["counts"]))) if which is None else list(which)
    ids = c["ids"][which]
    field, link, klw, d = c["field"], c["link"], c["kl_weight"], c["d"]
    pm, pl = pr.mean[field].cpu().double(), pr.prec[field].cpu().double()
    sel = torch.isin(c["X"][:, field], ids)
    X, y = c["X"][sel], c["y"][sel]
    sol = P.solve_fp64_prior(c["ent"], c["bia"], c["scal"], X, y, field, link, klw, pm, pl)
    assert torch.equal(sol["entities"], ids)
    theta, s = _written(m, ids)
    worst, worst_cond = 0.0, 0.0
    for i, k in enumerate(which):
        n = c["counts"][k]
        cond = P.cond_of_the_factored_prior(c["ent"], c["bia"], c["scal"], X, y, field, link, klw, int(ids[i]), pm.numpy(),
                                            pl.numpy())
        assert cond < COND_MAX, (what, n, cond)
        rt = np.concatenate([[float(sol["mu_w"][i])], sol["mu"][i].numpy()])
        rs = np.concatenate([[float(sol["s_w"][i])], sol["s"][i].numpy()])
        ok_t, w_t = R.elementwise_ok(theta[i], rt, R.solve_abs_term(d, cond, rt))
        ok_s, w_s = R.elementwise_ok(s[i], rs, R.scale_abs_term(n, rs))
        assert ok_t and ok_s, (what, n, w_t, w_s)
        worst, worst_cond = max(worst, w_t, w_s), max(worst_cond, cond)
    th = (ids, theta[:, 1:].double(), s[:, 1:].double(), theta[:, 0].double(), s[:, 0].double())
    L = P.entity_objective_prior(c["ent"], c["bia"], c["scal"], X, y.double(), field, th, link, klw, pm, pl)
    el = rel_err(loss.cpu()[which].numpy(), L.numpy())
    print(f"PRIOR {what} {link} d={d}: worst ratio {worst:.3f}, worst cond {worst_cond:.1f}, loss rel_err {el:.2e}")
    assert el <= 1e-5, el
    return worst


def _sizes(F, n_ent):
    return (n_ent + 3, 60) if F == 2 else (n_ent + 3, 40, 7)


def _planted(d):
    """The scale of the planted tables: solve_reference.tables' 0.5, and 0.35 for d >= 128, where the spectrum of the rows'
    own sum_r u_r u_r^T (320 rows, F = 3) alone passes COND_MAX at 0.5 whatever the prior."""
    return dict(scale=0.35) if d >= 128 else {}


def unsplit_counts(d):
    """Around d + 1 (the largest dual, the smallest primal), one row, and past a chunk edge."""
    return sorted({n for n in (1, d - 1, d, d + 1, d + 2, CHUNK * (d // CHUNK + 2) + 1) if n >= 1})


def split_counts(d):
    """d + 1 (at the threshold: not split), d + 2, around a chunk edge, one chunk (where d allows) and 40 chunks."""
    k = d // CHUNK + 2
    c = [d + 1, d + 2, CHUNK * k - 1, CHUNK * k, CHUNK * k + 1, CHUNK * 40]
    return c + [CHUNK - 1] if d + 2 <= CHUNK - 1 else c


# ---------------------------------------------------------------------------------------------------------------------
# the two solves against the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [2, 3])
@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("d", [1, 8, 9, 33, 128])
def test_unsplit_prior_solve_matches_fp64(d, link, F):
    counts = unsplit_counts(d)
    c = R.case(_sizes(F, len(counts)), 0, d, link, counts, seed=900 + d + F, kl_weight=0.7 if F == 3 else 1.0, **_planted(d))
    m, pr = _model_of(c), _priors_of(c, 11 + d)
    out = _fold(c, m, pr)
    assert torch.equal(out["entities"].cpu(), c["ids"]) and out["rows"].tolist() == counts
    _check(c, m, out["loss"], pr, f"unsplit F={F}")


@pytest.mark.parametrize("F", [2, 3])
@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("d", [1, 8, 9, 33, 128])
def test_split_prior_solve_matches_fp64(d, link, F):
    counts = split_counts(d)
    c = R.case(_sizes(F, len(counts)), 0, d, link, counts, seed=300 + d + F, kl_weight=0.7 if F == 3 else 1.0, **_planted(d))
    m, pr = _model_of(c), _priors_of(c, 13 + d)
    out = _fold(c, m, pr, split_rows=0, chunk_rows=CHUNK)
    assert torch.equal(out["entities"].cpu(), c["ids"]) and out["rows"].tolist() == counts
    _check(c, m, out["loss"], pr, f"split F={F}")


@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("d", [R.LDS - 1, R.LDS])
def test_prior_solves_with_the_triangle_in_lds_and_in_the_slab(d, link):
    assert R.has_slabs(d) == (d == R.LDS)
    counts = [d, d + 1, d + 2, CHUNK * (d // CHUNK + 2) + 1]
    c = R.case((7, 300), 0, d, link, counts, seed=400 + d, **_planted(d))
    pr = _priors_of(c, 17 + d)
    m = _model_of(c)
    _check(c, m, _fold(c, m, pr)["loss"], pr, "unsplit lds/slab")
    m = _model_of(c)
    _check(c, m, _fold(c, m, pr, split_rows=0, chunk_rows=CHUNK)["loss"], pr, "split lds/slab")


# ---------------------------------------------------------------------------------------------------------------------
# the tie to the parent: the standard prior gives its bits
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mixed(link):
    """300 light entities of 1 .. 12 rows and two heavy ones (100 and 61 rows), d = 8, F = 3."""
    counts = [1 + g % 12 for g in range(300)]
    counts[17], counts[200] = 100, 61
    c = R.case((320, 40, 7), 0, 8, link, counts, seed=55, kl_weight=0.7)
    m = _model_of(c)
    return c, m, m._flat.clone()


@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("kw", [dict(), dict(split_rows=20, chunk_rows=CHUNK)], ids=["unsplit", "split"])
def test_standard_prior_gives_the_bits_of_no_prior(kw, link):
    c, m, start = _mixed(link)
    m._flat.copy_(start)
    ref = _fold(c, m, None, **kw)
    flat = m._flat.clone()
    m._flat.copy_(start)
    out = _fold(c, m, _priors_of(c, 0, standard=True), **kw)
    assert not torch.equal(flat, start)
    assert torch.equal(m._flat, flat) and torch.equal(out["loss"], ref["loss"])
    # ... and another prior does not
    m._flat.copy_(start)
    _fold(c, m, _priors_of(c, 3), **kw)
    assert not torch.equal(m._flat, flat)
    m._flat.copy_(start)


def test_an_entitys_bits_depend_on_its_rows_and_the_prior_alone():
    c, m, start = _mixed("softplus")
    pr = _priors_of(c, 3)
    kw = dict(split_rows=20, chunk_rows=CHUNK)
    m._flat.copy_(start)
    out = _fold(c, m, pr, **kw)
    flat = m._flat.clone()
    for g in (0, 17, 200, 299):                                # light and heavy: alone = among 300 others
        e = int(c["ids"][g])
        sel = c["X"][:, 0] == e
        m._flat.copy_(start)
        alone = _fold(c, m, pr, c["X"][sel], c["y"][sel], **kw)
        assert torch.equal(alone["loss"], out["loss"][g:g + 1])
        d = m.d
        assert torch.equal(m._flat[e * 2 * d:(e + 1) * 2 * d], flat[e * 2 * d:(e + 1) * 2 * d])
        assert torch.equal(m._flat[m._off_bias + 2 * e: m._off_bias + 2 * e + 2], flat[m._off_bias + 2 * e: m._off_bias + 2 * e + 2])
    m._flat.copy_(start)


# ---------------------------------------------------------------------------------------------------------------------
# the objectives
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("link", LINKS)
def test_fold_in_objective_under_priors_matches_the_restatement(link):
    c = R.case((12, 40, 7), 0, 9, link, [1, 5, 9, 10, 11, 30], seed=950, kl_weight=0.7)
    m, pr = _model_of(c), _priors_of(c, 21)
    ids, d, f = c["ids"], 9, 0
    start = m._flat.clone()
    loss, grads = m.fold_in_objective(c["X"].to(DEV), c["y"].to(DEV), field=f, kl_weight=0.7, priors=pr)
    assert torch.equal(m._flat, start) and torch.equal(grads["entities"].cpu(), ids)
    ent, bia = c["ent"].double(), c["bia"].double()
    th = [t.clone().requires_grad_(True) for t in (ent[ids, :d], ent[ids, d:], bia[ids, 0], bia[ids, 1])]
    L = P.entity_objective_prior(c["ent"], c["bia"], c["scal"], c["X"], c["y"].double(), f, (ids, *th), link, c["kl_weight"],
                                 pr.mean[f].cpu().double(), pr.prec[f].cpu().double())
    L.sum().backward()
    assert rel_err(loss.cpu().numpy(), L.detach().numpy()) <= 1e-5
    assert rel_err(grads["entity"].cpu().numpy(), torch.cat([th[0].grad, th[1].grad], 1).numpy()) <= 1e-5
    assert rel_err(grads["bias"].cpu().numpy(), torch.stack([th[2].grad, th[3].grad], 1).numpy()) <= 1e-5
    # at the optimum it is the loss the solve returned, and the standard prior is the parent's objective bit for bit
    out = _fold(c, m, pr)
    loss2, _ = m.fold_in_objective(c["X"].to(DEV), c["y"].to(DEV), field=f, kl_weight=0.7, priors=pr)
    assert rel_err(loss2.cpu().numpy(), out["loss"].cpu().numpy()) <= 1e-5


def _tables(m):
    return m.entity_params.weight.detach().cpu().clone(), m.bias_params.weight.detach().cpu().clone(), m._scalars().cpu().clone()


@pytest.mark.parametrize("F", [2, 3])
@pytest.mark.parametrize("link", LINKS)
def test_exact_objective_under_priors_matches_the_restatement(link, F):
    c = R.case(_sizes(F, 20), 0, 8, link, [5 + g for g in range(20)], seed=500 + F, kl_weight=0.7)
    m, pr = _model_of(c), _priors_of(c, 23)
    J = m.exact_objective(c["X"].to(DEV), c["y"].to(DEV), kl_weight=0.7, priors=pr)
    ref = float(P.objective_J_prior(*_tables(m), c["X"], c["y"].double(), c["sizes"], link, R.f32(0.7), pr.mean.cpu(),
                                    pr.prec.cpu()))
    print(f"J under priors {link} F={F}: {J:.9g} against {ref:.9g}, rel {abs(J - ref) / abs(ref):.2e}")
    assert abs(J - ref) <= 1e-5 * abs(ref)
    std = m.exact_objective(c["X"].to(DEV), c["y"].to(DEV), kl_weight=0.7, priors=_priors_of(c, 0, standard=True))
    none = m.exact_objective(c["X"].to(DEV), c["y"].to(DEV), kl_weight=0.7)
    assert abs(std - none) <= 1e-12 * abs(none) and abs(J - none) > 1e-3 * abs(none)


# ---------------------------------------------------------------------------------------------------------------------
# an entity without rows, and the guards
# ---------------------------------------------------------------------------------------------------------------------
class _Raw:
    """The operands of one unsplit and one split prior call on a small case, through torch.ops.vfm_hip."""

    def __init__(self, link):
        from vae_amd import _lib, foldin, ops, sweep
        self.flags = ops.FLAG_LINK_SOFTPLUS if link == "softplus" else 0
        self.c = c = R.case((8, 60), 0, 8, link, [30, 41, 12, 25], seed=700, kl_weight=0.7)
        self.m = m = _model_of(c)
        self.pr = _priors_of(c, 29)
        self.start = m._flat.clone()
        x, y = foldin.check_args_exact(m, c["X"].to(DEV), c["y"].to(DEV), 0, 0.7)
        self.p = sweep.SweepPlan(m, x, y, 0, split_rows=0, chunk_rows=CHUNK)
        self.light = sweep.SweepPlan(m, x, y, 0)
        self.o, self.obj = _lib.ops(), foldin.OBJECTIVES["closed_form"]
        _, _, self.cptr, self.tab = self.p.groups[0]

    def split(self, ents=None, cptr=None, tab=None):
        p, m, o = self.p, self.m, self.o
        ents = p.ents if ents is None else ents
        cptr, tab = self.cptr if cptr is None else cptr, self.tab if tab is None else tab
        m._flat.copy_(self.start)
        ent, bia, scal = m._views(m._flat)
        ws = torch.zeros(max(o.foldin_split_workspace_bytes(tab.shape[0], ents.numel(), p.op_x.shape[0], m.d, -1), 1),
                         dtype=torch.uint8, device=DEV)
        loss = torch.full((max(ents.numel(), 1),), -7.0, device=DEV)
        o.foldin_solve_split_prior(ents, cptr, tab, p.ys, p.op_x, p.row_op, ent, bia, scal, ws, loss, self.pr.row(0), 0,
                                   self.flags, -1, 0.7)
        torch.cuda.synchronize()
        return m._flat.clone(), loss

    def unsplit(self, ents=None, ptr=None):
        p, m, o = self.light, self.m, self.o
        ents, ptr = p.ents if ents is None else ents, p.ptr if ptr is None else ptr
        m._flat.copy_(self.start)
        ent, bia, scal = m._views(m._flat)
        ws = torch.zeros(max(o.foldin_solve_workspace_bytes(ents.numel(), p.op_x.shape[0], m.d, -1), 1),
                         dtype=torch.uint8, device=DEV)
        loss = torch.full((max(ents.numel(), 1),), -7.0, device=DEV)
        o.foldin_solve_prior(ents, ptr, p.ys, p.op_x, p.row_op, ent, bia, scal, ws, loss, self.pr.row(0), 0, self.obj,
                             0, self.flags, -1, 0.7)
        torch.cuda.synchronize()
        return m._flat.clone(), loss


def _row(m, flat, e):
    d = m.d
    return torch.cat([flat[m._off_bias + 2 * e: m._off_bias + 2 * e + 1], flat[e * 2 * d:e * 2 * d + d],
                      flat[m._off_bias + 2 * e + 1: m._off_bias + 2 * e + 2], flat[e * 2 * d + d:(e + 1) * 2 * d]]).cpu()


@pytest.mark.parametrize("link", LINKS)
def test_guards_and_the_entity_without_rows(link):
    r = _Raw(link)
    m, d, E = r.m, r.m.d, r.p.E
    pm, pl = r.pr.mean[0].cpu().double(), r.pr.prec[0].cpu().double()
    want_s = P.inv_link_t(pl ** -0.5, link).numpy()
    T = m.T
    for name, run, ents_of in (("split", r.split, r.p.ents), ("unsplit", r.unsplit, r.light.ents)):
        flat0, loss0 = run()
        assert torch.isfinite(loss0).all() and not torch.equal(flat0, r.start)
        # a bad entity id in front and behind: a NaN loss, nothing written, the others bit for bit
        ents = torch.cat([torch.tensor([-3], device=DEV), ents_of, torch.tensor([T + 2], device=DEV)])
        if name == "split":
            nch = r.tab.shape[0]
            tab = torch.cat([r.tab[:1], r.tab, r.tab[:2]]).clone()
            tab[1:1 + nch, 0] += 1
            tab[0, 0], tab[-2:, 0] = 0, E + 1
            cptr = torch.cat([torch.tensor([0], device=DEV), r.cptr + 1, torch.tensor([nch + 3], device=DEV)])
            flat, loss = run(ents=ents, cptr=cptr, tab=tab)
        else:
            ptr = torch.cat([r.light.ptr[:1], r.light.ptr, r.light.ptr[-1:]])
            flat, loss = run(ents, ptr)
        assert bool(torch.isnan(loss[0])) and bool(torch.isnan(loss[-1])) and torch.equal(loss[1:-1], loss0[:E]), name
        assert torch.equal(flat, flat0), name
        # no rows at all: every entity gets the prior row, mu = m and sigma = lam^-1/2 through the link's inverse
        if name == "split":
            flat, loss = run(cptr=torch.zeros(E + 1, dtype=torch.int64, device=DEV),
                             tab=torch.zeros(0, 3, dtype=torch.int64, device=DEV))
        else:
            flat, loss = run(ents_of, torch.zeros(E + 1, dtype=torch.int64, device=DEV))
        for e in ents_of.tolist():
            row = _row(m, flat, e)
            assert torch.equal(row[:d + 1], r.pr.mean[0].cpu()), name
            assert R.elementwise_ok(row[d + 1:], want_s, R.scale_abs_term(0, want_s))[0], name
        # (KL to the prior at the prior is 0 up to the fp32 rounding of sigma: each coordinate within a few 2^-23)
        # v = sqrt(lam) sigma is 1 within four roundings (the square root, the stored s, its link, the product): |v - 1|
        # <= 4 2^-24.  The first-order terms of 1/2 (v^2 - 1) - log v cancel in exact arithmetic, not in fp32: v^2 - 1
        # carries 2 |v - 1| + 2^-23, halved, and log v carries |v - 1| + 2^-24: under 8 2^-23 per coordinate
        assert float(loss[:E].abs().max()) <= (d + 1) * 8 * R.EPS32, name
        # E = 0: nothing written
        if name == "split":
            flat, loss = run(ents=ents_of[:0], cptr=r.cptr[:1], tab=r.tab)
        else:
            flat, loss = run(ents_of[:0], r.light.ptr[:1])
        assert torch.equal(flat, r.start) and bool((loss == -7.0).all()), name
    del pm


# ---------------------------------------------------------------------------------------------------------------------
# fit_exact(learn_priors=True), block by block
# ---------------------------------------------------------------------------------------------------------------------
KLW = R.f32(0.7)


def _fit_data(F):
    sizes = (13, 10) if F == 2 else (13, 10, 4)
    g = torch.Generator().manual_seed(9)
    rows = [(u, i) for i in range(9) for u in range(12) if i == 0 or (u + i) % 4 != 0]
    X = torch.tensor(rows)
    X[:, 1] += 13
    if F == 3:
        X = torch.cat([X, 23 + torch.randint(0, 3, (X.shape[0], 1), generator=g)], 1)
    X = X[torch.randperm(X.shape[0], generator=g)]
    y = torch.randn(X.shape[0], generator=g) + 3.0
    return sizes, X, y, g


def _state(m, pr):
    return _tables(m) + (pr.mean.cpu().clone(), pr.prec.cpu().clone())


@functools.lru_cache(maxsize=None)
def _fit_run(F, link, learn_mean=True):
    """3 hierarchical sweeps on test_gpu_fit_exact's data: 12 users x 9 items (x 3 formats), d = 8; item 0 has 12 rows
    (split at split_rows = 9, chunk_rows = 4); user 12, item 9 and format 3 never occur.  Returns the model, its start,
    the rows and per block (sweep, what, state before, state after), a state being (ent, bia, scal, mean, prec)."""
    from vae_amd import sweep
    sizes, X, y, g = _fit_data(F)
    ent, bia, scal = R.tables(sizes, 8, seed=600 + F)
    c = dict(sizes=sizes, d=8, link=link, ent=ent, bia=bia, scal=scal)
    m = _model_of(c)
    m._ensure_opt_state()
    m._adam_m.copy_(torch.randn(m._adam_m.shape, generator=g).to(DEV))
    m._adam_v.copy_(torch.rand(m._adam_v.shape, generator=g).to(DEV))
    start = dict(flat=m._flat.clone(), adam_m=m._adam_m.clone(), adam_v=m._adam_v.clone())
    pr = sweep.GroupPriors(F, 8, DEV)
    if not learn_mean:
        pr.mean.copy_(P.draw_priors(F, 8, 31)[0].float())
    blocks, prev = [], [_state(m, pr)]

    def on_step(s, what):
        now = _state(m, pr)
        blocks.append((s, what, prev[0], now))
        prev[0] = now

    out = m.fit_exact(X.to(DEV), y.to(DEV), n_sweeps=3, kl_weight=KLW, split_rows=9, chunk_rows=4, on_step=on_step,
                      priors=pr, learn_priors=True, learn_mean=learn_mean)
    return m, start, X, y, blocks, out, pr, sizes


@pytest.mark.parametrize("learn_mean", [True, False])
@pytest.mark.parametrize("F", [2, 3])
@pytest.mark.parametrize("link", LINKS)
def test_every_block_of_a_hierarchical_sweep_is_its_exact_minimiser(link, F, learn_mean):
    m, start, X, y, blocks, out, pr, sizes = _fit_run(F, link, learn_mean)
    d = 8
    order = [w for f in range(F) for w in (f, ("prior", f))] + ["scalars"]
    assert [(s, w) for s, w, _, _ in blocks] == [(s, w) for s in range(3) for w in order]
    assert out["priors"] is pr and out["clamped"] == {f: 0 for f in range(F)}
    worst = worst_p = worst_cond = 0.0
    for s_i, what, (e0, b0, s0, mn0, pc0), (e1, b1, s1, mn1, pc1) in blocks:
        if what == "scalars":
            assert torch.equal(e0, e1) and torch.equal(b0, b1) and torch.equal(mn0, mn1) and torch.equal(pc0, pc1)
            m0, sg0 = FR.global_bias_fp64(e0, b0, s0, X, y, link, KLW)
            t_m0, _ = FR.scalar_abs_terms(e0, b0, s0, X, y, link)
            assert R.elementwise_ok(s1[1:2], [float(m0)], t_m0)[0]
            assert R.elementwise_ok(s1[2:3], [float(sg0)], R.scale_abs_term(1, [float(sg0)]))[0]
            at = torch.stack([s0[0], s1[1], s1[2]])
            _, t_a = FR.scalar_abs_terms(e0, b0, at, X, y, link)
            assert R.elementwise_ok(s1[0:1], [float(FR.precision_fp64(e0, b0, at, X, y, link))], t_a)[0]
            continue
        assert torch.equal(s0, s1)
        if isinstance(what, tuple):                            # the prior block: from the tables before it
            f = what[1]
            assert torch.equal(e0, e1) and torch.equal(b0, b1)
            rm, rl, raw = P.prior_block_fp64(e0, b0, X, f, link, mn0[f], learn_mean)
            assert torch.equal(rl, raw)
            ok_m, w_m = R.elementwise_ok(mn1[f], rm.numpy(), 0.0)
            ok_l, w_l = R.elementwise_ok(pc1[f], rl.numpy(), 0.0)
            assert ok_m and ok_l, (s_i, what, w_m, w_l)
            if not learn_mean:
                assert torch.equal(mn1[f], mn0[f])
            keep = [g for g in range(F) if g != f]
            assert torch.equal(mn0[keep], mn1[keep]) and torch.equal(pc0[keep], pc1[keep])
            worst_p = max(worst_p, w_m, w_l)
            continue
        assert torch.equal(mn0, mn1) and torch.equal(pc0, pc1)
        pm, pl = mn0[what].double(), pc0[what].double()
        sol = P.solve_fp64_prior(e0, b0, s0, X, y, what, link, KLW, pm, pl)
        ids = sol["entities"]
        other = torch.ones(e0.shape[0], dtype=torch.bool)
        other[ids] = False
        assert torch.equal(e0[other], e1[other]) and torch.equal(b0[other], b1[other])
        for i, e in enumerate(ids.tolist()):
            cond = P.cond_of_the_factored_prior(e0, b0, s0, X, y, what, link, KLW, e, pm.numpy(), pl.numpy())
            n = int((X[:, what] == e).sum())
            rt = np.concatenate([[float(sol["mu_w"][i])], sol["mu"][i].numpy()])
            rs = np.concatenate([[float(sol["s_w"][i])], sol["s"][i].numpy()])
            ok_t, w_t = R.elementwise_ok(torch.cat([b1[e, :1], e1[e, :d]]), rt, R.solve_abs_term(d, cond, rt))
            ok_s, w_s = R.elementwise_ok(torch.cat([b1[e, 1:], e1[e, d:]]), rs, R.scale_abs_term(n, rs))
            assert ok_t and ok_s, (s_i, what, e, w_t, w_s, cond)
            worst, worst_cond = max(worst, w_t, w_s), max(worst_cond, cond)
    print(f"HFIT {link} F={F} learn_mean={learn_mean}: worst ratio of the field blocks {worst:.3f} (cond up to "
          f"{worst_cond:.1f}), of the prior blocks {worst_p:.3f}; learnt prec {pr.prec.cpu().numpy().round(3).tolist()}")


@pytest.mark.parametrize("learn_mean", [True, False])
@pytest.mark.parametrize("F", [2, 3])
@pytest.mark.parametrize("link", LINKS)
def test_J_never_increases_and_unseen_rows_and_adam_state_stay(link, F, learn_mean):
    m, start, X, y, blocks, out, pr, sizes = _fit_run(F, link, learn_mean)
    yd = y.double()
    J = [float(P.objective_J_prior(*blocks[0][2][:3], X, yd, sizes, link, KLW, *blocks[0][2][3:]))]
    for s_i, what, _, now in blocks:
        Ja = float(P.objective_J_prior(*now[:3], X, yd, sizes, link, KLW, *now[3:]))
        assert Ja <= J[-1] + 1e-9 * abs(J[-1]), (s_i, what, Ja, J[-1])
        J.append(Ja)
    per_sweep = [J[0]] + J[2 * F + 1::2 * F + 1]
    assert out["sweeps"] == 3 and len(out["ms"]) == 3 and len(out["objective"]) == 4
    for got, ref in zip(out["objective"], per_sweep):
        assert abs(got - ref) <= 1e-5 * abs(ref), (got, ref)
    print(f"HFIT {link} F={F} learn_mean={learn_mean}: J per sweep {out['objective']}")
    seen = torch.unique(X)
    unseen = torch.ones(m.T, dtype=torch.bool)
    unseen[seen] = False
    assert int(unseen.sum()) >= 2
    e0, b0 = blocks[0][2][:2]
    e1, b1 = blocks[-1][3][:2]
    assert torch.equal(e0[unseen], e1[unseen]) and torch.equal(b0[unseen], b1[unseen])
    assert not torch.equal(e0[~unseen], e1[~unseen])
    assert torch.equal(m._adam_m, start["adam_m"]) and torch.equal(m._adam_v, start["adam_v"])


def test_given_priors_without_learning_are_left_alone_and_are_solved_under():
    from vae_amd import sweep
    m, start, X, y, _, _, _, sizes = _fit_run(2, "abs")
    now = m._flat.clone()
    m._flat.copy_(start["flat"])
    pr = sweep.GroupPriors(2, 8, DEV)
    mean, prec = P.draw_priors(2, 8, 37)
    pr.load_state_dict({"mean": mean.float(), "prec": prec.float()})
    keep = pr.state_dict()
    whats = []
    t0 = _tables(m)
    out = m.fit_exact(X.to(DEV), y.to(DEV), n_sweeps=1, kl_weight=KLW, fields=(1,), update_scalars=False, split_rows=9,
                      chunk_rows=4, priors=pr, on_step=lambda s, w: whats.append((s, w)))
    assert whats == [(0, 1)] and out["priors"] is pr and "clamped" not in out
    assert torch.equal(pr.mean, keep["mean"]) and torch.equal(pr.prec, keep["prec"])
    e1, b1, _ = _tables(m)
    sol = P.solve_fp64_prior(*t0, X, y, 1, "abs", KLW, mean[1], prec[1])
    ids = sol["entities"]
    assert rel_err(e1[ids].numpy(), torch.cat([sol["mu"], sol["s"]], 1).numpy()) <= 1e-6
    ref = float(P.objective_J_prior(e1, b1, t0[2], X, y.double(), sizes, "abs", KLW, mean, prec))
    assert abs(out["objective"][-1] - ref) <= 1e-5 * abs(ref)
    m._flat.copy_(now)


def test_prec_max_binds_and_is_reported():
    """Users whose answers carry almost no information about their factors (a sharp prior, few rows) end within a
    narrow band of the prior mean: 1 / lam* falls below 1 / prec_max = 1 / 4, the clamp binds and is counted."""
    from vae_amd import sweep
    m, start, X, y, _, _, _, sizes = _fit_run(2, "abs")
    now = m._flat.clone()
    m._flat.copy_(start["flat"])
    pr = sweep.GroupPriors(2, 8, DEV)
    before = _tables(m)
    states = []
    out = m.fit_exact(X.to(DEV), y.to(DEV), n_sweeps=1, kl_weight=KLW, fields=(0,), update_scalars=False, priors=pr,
                      learn_priors=True, prec_min=1.0, prec_max=4.0,
                      on_step=lambda s, w: states.append((w, _tables(m), pr.prec.cpu().clone())))
    assert [w for w, _, _ in states] == [0, ("prior", 0)]
    e1, b1, _ = states[0][1]
    _, lam, raw = P.prior_block_fp64(e1, b1, X, 0, "abs", torch.zeros(9), True, 1.0, 4.0)
    n_bind = int(((raw < 1.0) | (raw > 4.0)).sum())
    assert int((raw > 4.0).sum()) >= 1, raw
    assert out["clamped"] == {0: n_bind}
    assert R.elementwise_ok(states[1][2][0], lam.numpy(), 0.0)[0] and float(states[1][2][0].max()) == 4.0
    assert torch.equal(pr.prec[1].cpu(), torch.ones(9))
    del before
    m._flat.copy_(now)

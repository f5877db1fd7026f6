"""GPU: the bound solves under a field prior (include/vfm_bound_prior.h: vfm_foldin_bound_prior_f32,
vfm_foldin_bound_split_prior_f32; VFM.fold_in_bound / fold_in_bound_objective / bound_objective / fit_bound with
priors=) against the fp64 restatement of tests/bound_prior_reference.py.

Bounds: those of test_gpu_foldin_bound.py and test_gpu_fit_bound.py, restated against the prior reference.  Rows
rel_err <= 1e-4, loss <= 1e-5 against the fp64 B_e (KL to the prior) at the written rows; per element
|got - ref| <= 2^-23 |ref| + n_iters solve_abs_term(d, cond_max, ref) for the means and the same plus scale_abs_term for
the scales, after asserting cond <= 1e3 of every round's factored matrix (tests/test_fit_bound_priors_cpu.py computes
them on the CPU: at most 40.9 unsplit and 81.6 split, at d = 128).  The prior block: 2^-23 |ref| (computed in fp64 on the
device, rounded once).  The bias block: bound_sweep_restatement.bias_abs_terms.  J after a block:
J_after <= J_before + 1e-5 |J_before|, both from fp32 moments.  The priors of the cases have means in [-0.5, 0.5], so
the start theta = m is not zero, and precisions in [0.25, 16].

Measured on an MI355X (the printed BPRI lines): worst elementwise ratio 0.498 for the unsplit rounds and 0.497 for the
split rounds (1 = at the bound; the reference itself rounded to fp32 gives at most 0.5), rows within 5.8e-8 and losses
within 8.6e-8 relative; bound_objective(priors=) within 1.3e-8 of the restatement; of fit_bound's blocks the field
blocks 0.498, the prior blocks 0.479, the bias blocks 0.050; the largest relative step of J over a block -4.3e-8 (none
rose)."""
import functools

import numpy as np
import pytest
import torch

import bound_prior_reference as BP
import bound_reference as BR
import bound_sweep_restatement as BS
import prior_reference as PR
import solve_reference as R
from golden_util import rel_err
from test_gpu_fit_bound import _rows_of, _tables
from test_gpu_foldin_bound import _model_of, _written

pytestmark = pytest.mark.gpu
DEV = "cuda"
LINKS = ["abs", "softplus"]
CHUNK = BS.CHUNK


def _priors_of(c, values=None):
    """A GroupPriors on the device for case c: bound_prior_reference.case_priors, `values` = (mean, prec), or with
    values="standard" the N(0, 1) it is created at."""
    from vae_amd import sweep
    F, d = len(c["sizes"]), c["d"]
    pr = sweep.GroupPriors(F, d, DEV)
    if values != "standard":
        mean, prec = BP.case_priors(F, d) if values is None else values
        pr.load_state_dict({"mean": mean.float(), "prec": prec.float()})
    return pr


def _fold(c, m, pr, n_iters=8, reset=False, X=None, y=None, **kw):
    X, y = (c["X"], c["y"]) if X is None else (X, y)
    return m.fold_in_bound(X.to(DEV), y.to(DEV), field=c["field"], kl_weight=c["kl_weight"], n_iters=n_iters, reset=reset,
                           priors=pr, **kw)


def _check(c, m, loss, pr, n_iters, reset, what, which=None):
    """test_gpu_foldin_bound._check against the prior reference: the written rows of the entities number `which` of
    case c against bound_rounds_fp64_prior (relative and per element), the loss against the fp64 B_e under the prior at
    the written rows.  Returns (worst elementwise ratio, rows rel_err, loss rel_err)."""
    which = list(range(len(c["counts"]))) if which is None else list(which)
    ids, d, f = c["ids"][which], c["d"], c["field"]
    pm, pl = pr.mean[f].cpu().double(), pr.prec[f].cpu().double()
    theta, s = _written(m, ids)
    worst, Bref, rt, rs = 0.0, [], [], []
    for i, k in enumerate(which):
        r = BP.case_rounds_prior(c, k, n_iters, reset, pm, pl)
        assert r["n"] == c["counts"][k] and float(r["cond"].max()) <= 1e3
        rt.append(r["theta"][-1])
        rs.append(r["s"][-1])
        at = n_iters * R.solve_abs_term(d, float(r["cond"].max()), r["theta"][-1])
        ok_t, w_t = R.elementwise_ok(theta[i], r["theta"][-1], at)
        ok_s, w_s = R.elementwise_ok(s[i], r["s"][-1], at + R.scale_abs_term(r["n"], r["s"][-1]))
        worst = max(worst, w_t, w_s)
        assert ok_t and ok_s, (what, r["n"], w_t, w_s)
        Bref.append(BP.bound_objective_fp64_prior(c["ent"], c["bia"], c["scal"], c["X"], c["y"], f, c["link"],
                                                  c["kl_weight"], int(ids[i]), theta[i], s[i], pm, pl))
    e_rows = max(rel_err(theta.numpy(), np.array(rt)), rel_err(s.numpy(), np.array(rs)))
    e_loss = rel_err(loss.cpu()[which].numpy(), np.array(Bref))
    print(f"BPRI {what} {c['link']} F={len(c['sizes'])} d={d} n_iters={n_iters} reset={int(reset)}: rows {e_rows:.2e} "
          f"loss {e_loss:.2e} worst elementwise ratio {worst:.3f}")
    assert e_rows <= 1e-4, e_rows
    assert e_loss <= 1e-5, e_loss
    return worst, e_rows, e_loss


# ---------------------------------------------------------------------------------------------------------------------
# against fp64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [2, 3])
@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("d", BR.GPU_DS)
def test_unsplit_rounds_under_a_prior_match_fp64(d, link, F):
    c = BR.shape_case(d, link, F)
    m, pr = _model_of(c), _priors_of(c)
    start = m._flat.clone()
    worst = 0.0
    for n_iters, reset in BR.GPU_ITERS:
        m._flat.copy_(start)
        out = _fold(c, m, pr, n_iters, reset)
        assert torch.equal(out["entities"].cpu(), c["ids"]) and out["rows"].tolist() == c["counts"]
        worst = max(worst, _check(c, m, out["loss"], pr, n_iters, reset, "unsplit")[0])
    print(f"BPRI unsplit worst d={d} {link} F={F}: {worst:.3f}")


@pytest.mark.parametrize("F", [2, 3])
@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("d", BS.SPLIT_DS)
def test_split_rounds_under_a_prior_match_fp64(d, link, F):
    c = BS.split_case(d, link, F)
    m, pr = _model_of(c), _priors_of(c)
    start = m._flat.clone()
    worst = 0.0
    for n_iters, reset in BS.ITERS:
        m._flat.copy_(start)
        out = _fold(c, m, pr, n_iters, reset, split_rows=0, chunk_rows=CHUNK)
        assert torch.equal(out["entities"].cpu(), c["ids"]) and out["rows"].tolist() == c["counts"]
        worst = max(worst, _check(c, m, out["loss"], pr, n_iters, reset, "split")[0])
    print(f"BPRI split worst d={d} {link} F={F}: {worst:.3f}")


@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("d", [R.LDS - 1, R.LDS])
def test_triangle_in_lds_and_in_the_slab(d, link):
    assert R.has_slabs(d) == (d == R.LDS)
    c = BR.bound_case((6, 300), 0, d, link, [d + 1], seed=211 + d)      # (slab_case's shape: n = d + 1, the first primal)
    m, pr = _model_of(c), _priors_of(c)
    assert R.storage(d + 1, d) == ("slab" if d == R.LDS else "lds")
    out = _fold(c, m, pr, 8, True)
    _check(c, m, out["loss"], pr, 8, True, "unsplit lds/slab")
    c = BS.placement_case(d, link)
    m = _model_of(c)
    out = _fold(c, m, pr, 8, True, split_rows=0, chunk_rows=CHUNK)
    assert out["rows"].tolist() == c["counts"]
    _check(c, m, out["loss"], pr, 8, True, "split lds/slab")


# ---------------------------------------------------------------------------------------------------------------------
# bits
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mixed():
    c = BS.mixed_case()
    m = _model_of(c)
    return c, m, m._flat.clone()


@pytest.mark.parametrize("reset", [False, True])
@pytest.mark.parametrize("kw", [dict(), dict(split_rows=20, chunk_rows=CHUNK)], ids=["unsplit", "split"])
def test_standard_prior_gives_the_bits_of_no_prior(kw, reset):
    c, m, start = _mixed()
    X, y = c["X"].to(DEV), c["y"].to(DEV)
    m._flat.copy_(start)
    plain = _fold(c, m, None, 8, reset, **kw)
    flat = m._flat.clone()
    obj_plain = m.fold_in_bound_objective(X, y, field=0, kl_weight=c["kl_weight"])
    J_plain = m.bound_objective(X, y, kl_weight=c["kl_weight"])
    std = _priors_of(c, "standard")
    m._flat.copy_(start)
    out = _fold(c, m, std, 8, reset, **kw)
    assert torch.equal(m._flat, flat) and torch.equal(out["loss"], plain["loss"])
    assert torch.equal(out["entities"], plain["entities"]) and torch.equal(out["rows"], plain["rows"])
    obj = m.fold_in_bound_objective(X, y, field=0, kl_weight=c["kl_weight"], priors=std)
    assert torch.equal(obj["loss"], obj_plain["loss"])
    J = m.bound_objective(X, y, kl_weight=c["kl_weight"], priors=std)
    assert J == J_plain                                        # (fp64 on the device, the same operations)
    # a non-standard prior gives other bits
    pr = _priors_of(c)
    m._flat.copy_(start)
    other = _fold(c, m, pr, 8, reset, **kw)
    assert not torch.equal(m._flat, flat) and not torch.equal(other["loss"], plain["loss"])
    assert not torch.equal(m.fold_in_bound_objective(X, y, field=0, kl_weight=c["kl_weight"], priors=pr)["loss"],
                           m.fold_in_bound_objective(X, y, field=0, kl_weight=c["kl_weight"])["loss"])
    m._flat.copy_(start)


@pytest.mark.parametrize("kw", [dict(), dict(split_rows=20, chunk_rows=CHUNK)], ids=["unsplit", "split"])
def test_objective_mode_returns_the_folds_loss_and_nothing_else_is_touched(kw):
    c, m, start = _mixed()
    X, y = c["X"].to(DEV), c["y"].to(DEV)
    pr = _priors_of(c)
    state = pr.state_dict()
    m._flat.copy_(start)
    out = _fold(c, m, pr, 8, False, **kw)
    flat = m._flat.clone()
    obj = m.fold_in_bound_objective(X, y, field=0, kl_weight=c["kl_weight"], priors=pr)
    if not kw:                                                 # (the split loss sums its rows chunk by chunk)
        assert torch.equal(obj["loss"], out["loss"])
    else:
        light = torch.tensor([g for g in range(300) if g not in (17, 200)], device=DEV)
        assert torch.equal(obj["loss"][light], out["loss"][light])
        assert rel_err(obj["loss"].cpu().numpy(), out["loss"].cpu().numpy()) <= 1e-5
    assert torch.equal(obj["entities"], out["entities"]) and torch.equal(m._flat, flat)
    assert torch.equal(pr.mean, state["mean"]) and torch.equal(pr.prec, state["prec"])
    changed = torch.zeros(m._n_flat, dtype=torch.bool, device=DEV)
    for e in out["entities"].tolist():
        changed[e * 2 * m.d:(e + 1) * 2 * m.d] = True
        changed[m._off_bias + 2 * e: m._off_bias + 2 * e + 2] = True
    assert torch.equal(m._flat[~changed], start[~changed]) and int((~changed).sum()) > 0
    assert not torch.equal(m._flat[changed], start[changed])
    _check(c, m, out["loss"], pr, 8, False, "mixed", which=[0, 1, 2, 17, 200])
    m._flat.copy_(start)


@pytest.mark.parametrize("kw", [dict(), dict(split_rows=0, chunk_rows=CHUNK)], ids=["unsplit", "split"])
def test_reset_starts_at_the_prior_not_at_zero_one(kw):
    c = BR.bound_case((8, 60), 0, 8, "softplus", [30, 41, 12, 25], seed=700, kl_weight=0.7)
    m, pr = _model_of(c), _priors_of(c)
    pm, pl = pr.mean[0].cpu().double(), pr.prec[0].cpu().double()
    out = _fold(c, m, pr, 1, True, **kw)
    _check(c, m, out["loss"], pr, 1, True, "reset")
    theta, s = _written(m, c["ids"])
    for k in range(4):                                         # the reference started at (0, 1) is somewhere else
        e = int(c["ids"][k])
        r = BP.bound_rounds_fp64_prior(c["ent"], c["bia"], c["scal"], c["X"], c["y"], 0, "softplus", 0.7, e, 1, pm, pl,
                                       start=(np.zeros(9), np.ones(9)))
        at = R.solve_abs_term(8, float(r["cond"].max()), r["theta"][-1])
        assert not R.elementwise_ok(theta[k], r["theta"][-1], at)[0], k


# ---------------------------------------------------------------------------------------------------------------------
# the entity without rows, through the ops
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reset", [0, 1])
@pytest.mark.parametrize("link", LINKS)
def test_an_entity_without_rows_gets_the_prior(link, reset):
    """mu = m, s = link^-1(lam^-1/2) rounded to fp32, loss 0.  The loss is kl sum_c of an fp32 KL at v = sqrtf(lam)
    link(s) = 1 + delta, |delta| <= 4 eps32 (a rounding each of sqrtf, the stored s, the link and the product), which is
    delta^2 / 2 exactly and is evaluated as (v^2 - 1) / 2 - log v: each term is delta to within 2 eps32, so a coordinate
    is off by at most 8 eps32."""
    from vae_amd import _lib, foldin, ops, sweep
    c = BR.bound_case((8, 60), 0, 8, link, [30, 41, 12, 25], seed=700, kl_weight=0.7)
    m, pr = _model_of(c), _priors_of(c)
    d, o = m.d, _lib.ops()
    flags = ops.FLAG_LINK_SOFTPLUS if link == "softplus" else 0
    empty = torch.tensor([i for i in range(8) if i not in c["ids"].tolist()][:1], device=DEV)
    prior = pr.row(0).to(DEV)
    x, y = foldin.check_args_bound(m, c["X"].to(DEV), c["y"].to(DEV), 0, 0.7, 8)
    want_mu = prior[0].cpu()
    want_s = 1.0 / np.sqrt(prior[1].cpu().double().numpy())
    want_s = want_s if link == "abs" else np.log(np.expm1(want_s))

    def check(flat, loss_e):
        row = _rows_of(m, flat, int(empty)).cpu()
        assert torch.equal(torch.cat([row[2 * d:2 * d + 1], row[:d]]), want_mu)
        assert R.elementwise_ok(torch.cat([row[2 * d + 1:], row[d:2 * d]]), want_s, 0.0)[0]
        assert abs(float(loss_e)) <= 0.7 * (d + 1) * 8 * R.EPS32, float(loss_e)

    # unsplit: the id behind the others with an empty row range
    start = m._flat.clone()
    xs, ys, ents, ptr, _ = foldin.row_lists(x, y, 0)
    op_x, row_op = foldin.partner_tuples(xs, 0)
    ents2, ptr2 = torch.cat([ents, empty]), torch.cat([ptr, ptr[-1:]])
    ent, bia, scal = m._views(m._flat)
    ws = torch.zeros(o.foldin_bound_workspace_bytes(5, ys.numel(), op_x.shape[0], d, -1), dtype=torch.uint8, device=DEV)
    loss = torch.full((5,), -7.0, device=DEV)
    o.foldin_bound_prior(ents2, ptr2, ys, op_x, row_op, ent, bia, scal, ws, loss, prior, 0, foldin.OBJECTIVES["closed_form"],
                         _lib.LIK_BERNOULLI, flags, -1, 0.7, 8, reset, foldin.MODE_FIT)
    torch.cuda.synchronize()
    check(m._flat, loss[4])
    ref = m._flat.clone()
    m._flat.copy_(start)
    out = _fold(c, m, pr, 8, bool(reset))                      # the four others: the bits of a call without it
    for e in c["ids"].tolist():
        assert torch.equal(_rows_of(m, m._flat, e), _rows_of(m, ref, e))
    assert torch.equal(out["loss"], loss[:4])
    # split: the id behind the others without chunks
    m._flat.copy_(start)
    p = sweep.SweepPlan(m, x, y, 0, 0, CHUNK, bound=True)
    assert p.n_light == 0 and len(p.groups) == 1
    _, _, cptr, tab = p.groups[0]
    ents2, cptr2 = torch.cat([p.ents, empty]), torch.cat([cptr, cptr[-1:]])
    ws = torch.zeros(o.foldin_bound_split_workspace_bytes(tab.shape[0], 5, p.ys.numel(), p.op_x.shape[0], d, -1),
                     dtype=torch.uint8, device=DEV)
    loss = torch.full((5,), -7.0, device=DEV)
    ent, bia, scal = m._views(m._flat)
    o.foldin_bound_split_prior(ents2, cptr2, tab, p.ys, p.op_x, p.row_op, ent, bia, scal, ws, loss, prior, 0, flags, -1, 0.7,
                               8, reset)
    torch.cuda.synchronize()
    check(m._flat, loss[4])
    assert bool(torch.isfinite(loss).all())


# ---------------------------------------------------------------------------------------------------------------------
# the bound session keeps its bits (it runs the PRIOR = false instantiation of bound_body)
# ---------------------------------------------------------------------------------------------------------------------
def test_bound_sessions_bits_are_unchanged():
    from test_gpu_elicit_bound import _against_the_composition
    from test_gpu_elicit_field import _problem
    from test_gpu_foldin import _model
    m = _model((40, 90), 8, "class", "softplus", seed=12, rng_seed=3)
    pool, y_pool, hx, hy = _problem(m, 0, 5, [3, 9, 6], [4, 0], seed=8)
    out = _against_the_composition(m, pool, y_pool, 3, 0, "variance", (hx, hy), False, 2)
    assert out["entities"].numel() == 5 and int((out["rows"][:, 0] >= 0).sum()) == 5


# ---------------------------------------------------------------------------------------------------------------------
# the objective
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [2, 3])
@pytest.mark.parametrize("link", LINKS)
def test_bound_objective_under_priors_matches_the_restatement(link, F):
    c = BR.bound_case(BS.split_sizes(F, 20), 0, 8, link, [5 + g for g in range(20)], seed=500 + F, kl_weight=0.7)
    m, pr = _model_of(c), _priors_of(c)
    before = m._flat.clone()
    J = m.bound_objective(c["X"].to(DEV), c["y"].to(DEV), kl_weight=0.7, priors=pr)
    ref = float(BP.objective_J_prior(*_tables(m), c["X"], c["y"], c["sizes"], link, R.f32(0.7), pr.mean.cpu(), pr.prec.cpu()))
    J0 = m.bound_objective(c["X"].to(DEV), c["y"].to(DEV), kl_weight=0.7)
    print(f"BPRI J {link} F={F}: {J:.9g} against {ref:.9g}, rel {abs(J - ref) / abs(ref):.2e} (N(0, 1): {J0:.9g})")
    assert abs(J - ref) <= 1e-5 * abs(ref) and abs(J - J0) > 1e-3 * abs(J0)
    assert torch.equal(m._flat, before)


# ---------------------------------------------------------------------------------------------------------------------
# fit_bound with learnt priors, block by block
# ---------------------------------------------------------------------------------------------------------------------
KLW = R.f32(0.7)
N_ITERS = 2
FIT_KW = dict(kl_weight=KLW, n_iters=N_ITERS, split_rows=40, chunk_rows=16)


def _fit_model(F, link):
    sizes, X, y = BS.fit_case(F)
    ent, bia, scal = R.tables(sizes, 8, seed=600 + F)
    return _model_of(dict(sizes=sizes, d=8, link=link, ent=ent, bia=bia, scal=scal)), sizes, X, y


@functools.lru_cache(maxsize=None)
def _fit_run(F, link):
    """3 hierarchical sweeps on bound_sweep_restatement.fit_case, d = 8, from a given GroupPriors at N(0, 1).  Returns
    the rows, per block (sweep, what, state before, state after, J before, J after) with state = (ent, bia, scal, mean,
    prec) on the CPU, fit_bound's result and the GroupPriors passed in."""
    from vae_amd import sweep
    m, sizes, X, y = _fit_model(F, link)
    pr = sweep.GroupPriors(F, 8, DEV)
    Xd, yd = X.to(DEV), y.to(DEV)
    state = lambda: (*_tables(m), pr.mean.cpu().clone(), pr.prec.cpu().clone())
    blocks, prev = [], [state(), m.bound_objective(Xd, yd, kl_weight=KLW, priors=pr)]

    def on_step(sweep_i, what):
        now, J = state(), m.bound_objective(Xd, yd, kl_weight=KLW, priors=pr)
        blocks.append((sweep_i, what, prev[0], now, prev[1], J))
        prev[0], prev[1] = now, J

    out = m.fit_bound(Xd, yd, n_sweeps=3, on_step=on_step, priors=pr, learn_priors=True, **FIT_KW)
    return sizes, X, y, blocks, out, pr


@pytest.mark.parametrize("F", [2, 3])
@pytest.mark.parametrize("link", LINKS)
def test_every_block_of_a_hierarchical_bound_sweep_is_the_restatement_s(link, F):
    sizes, X, y, blocks, out, pr = _fit_run(F, link)
    d = 8
    whats = [w for f in range(F) for w in (f, ("prior", f))] + ["bias"]
    assert [(b[0], b[1]) for b in blocks] == [(s, w) for s in range(3) for w in whats]
    assert out["priors"] is pr and out["clamped"] == {f: 0 for f in range(F)}
    worst = worst_p = worst_b = 0.0
    for sweep_i, what, (e0, b0, s0, m0, p0), (e1, b1, s1, m1, p1), _, _ in blocks:
        if what == "bias":
            assert torch.equal(e0, e1) and torch.equal(b0, b1) and torch.equal(s0[0], s1[0])
            assert torch.equal(m0, m1) and torch.equal(p0, p1)
            g0, sg0, _ = BS.global_bias_fp64(e0, b0, s0, X, y, link, KLW)
            t_m0, t_s0 = BS.bias_abs_terms(e0, b0, s0, X, y, link, KLW)
            ok, w1 = R.elementwise_ok(s1[1:2], [float(g0)], t_m0)
            assert ok, ("m0", w1)
            ok, w2 = R.elementwise_ok(s1[2:3], [float(sg0)], t_s0 + R.scale_abs_term(1, [float(sg0)]))
            assert ok, ("s0", w2)
            worst_b = max(worst_b, w1, w2)
            continue
        assert torch.equal(s0, s1)
        if isinstance(what, tuple):                            # the prior block: fp64 on the device, rounded once
            f = what[1]
            assert torch.equal(e0, e1) and torch.equal(b0, b1)
            rm, rl, raw = PR.prior_block_fp64(e0, b0, X, f, link, m0[f].double())
            assert torch.equal(rl, raw)                        # (no clamp binds)
            ok_m, w_m = R.elementwise_ok(m1[f], rm.numpy(), 0.0)
            ok_l, w_l = R.elementwise_ok(p1[f], rl.numpy(), 0.0)
            assert ok_m and ok_l, (sweep_i, what, w_m, w_l)
            worst_p = max(worst_p, w_m, w_l)
            other = [g for g in range(F) if g != f]
            assert torch.equal(m0[other], m1[other]) and torch.equal(p0[other], p1[other])
            continue
        assert torch.equal(m0, m1) and torch.equal(p0, p1)
        ids = torch.unique(X[:, what])
        other = torch.ones(e0.shape[0], dtype=torch.bool)
        other[ids] = False
        assert torch.equal(e0[other], e1[other]) and torch.equal(b0[other], b1[other])
        for e in ids.tolist():
            r = BP.bound_rounds_fp64_prior(e0, b0, s0, X, y, what, link, KLW, e, N_ITERS, m0[what].double(),
                                           p0[what].double(), False)
            cond = float(r["cond"].max())
            assert cond <= 1e3, cond
            rt, rs = r["theta"][-1], r["s"][-1]
            at = N_ITERS * R.solve_abs_term(d, cond, rt)
            ok_t, w_t = R.elementwise_ok(torch.cat([b1[e, :1], e1[e, :d]]), rt, at)
            ok_s, w_s = R.elementwise_ok(torch.cat([b1[e, 1:], e1[e, d:]]), rs, at + R.scale_abs_term(r["n"], rs))
            assert ok_t and ok_s, (sweep_i, what, e, w_t, w_s)
            worst = max(worst, w_t, w_s)
    print(f"BPRI fit {link} F={F}: worst elementwise ratio of the field blocks {worst:.3f}, of the prior blocks "
          f"{worst_p:.3f}, of the bias blocks {worst_b:.3f}; learnt prec of field 0 {pr.prec[0].tolist()}")


@pytest.mark.parametrize("F", [2, 3])
@pytest.mark.parametrize("link", LINKS)
def test_J_never_increases_over_a_hierarchical_bound_sweep(link, F):
    sizes, X, y, blocks, out, pr = _fit_run(F, link)
    worst = -1e30
    for sweep_i, what, _, _, Jb, Ja in blocks:
        worst = max(worst, (Ja - Jb) / abs(Jb))
        assert Ja <= Jb + 1e-5 * abs(Jb), (sweep_i, what, Ja, Jb)
    assert out["sweeps"] == 3 and len(out["objective"]) == 4 and out["objective"][-1] < out["objective"][0]
    per_sweep = [blocks[0][4]] + [b[5] for b in blocks if b[1] == "bias"]
    assert out["objective"] == per_sweep                      # (the same kernel on the same tables and priors)
    ref = float(BP.objective_J_prior(*blocks[-1][3][:3], X, y, sizes, link, KLW, *blocks[-1][3][3:]))
    assert abs(out["objective"][-1] - ref) <= 1e-5 * abs(ref)
    print(f"BPRI fit {link} F={F}: J per sweep {out['objective']}, largest relative step of a block {worst:.2e}")


def test_clamps_are_counted_means_can_stay_and_priors_none_creates_them():
    from vae_amd import sweep
    m, sizes, X, y = _fit_model(2, "abs")
    Xd, yd = X.to(DEV), y.to(DEV)
    start = m._flat.clone()
    # prec_min = 1e3, above the precisions the blocks of the first sweep ask for (a second sweep under the clamped prior
    # asks for values just under 1e3): the count is that of the restatement's unclamped values at the tables each prior
    # block read
    whats, expect = [], {0: 0, 1: 0}

    def on_step(s, w):
        whats.append(w)
        if isinstance(w, tuple):
            e, b, _ = _tables(m)
            _, _, raw = PR.prior_block_fp64(e, b, X, w[1], "abs", torch.zeros(9), True, 1e3, 1e4)
            assert float(raw.max()) < 0.9e3                    # (none near the clamp: the count is not a rounding matter)
            expect[w[1]] += int((raw < 1e3).sum())

    out = m.fit_bound(Xd, yd, n_sweeps=1, learn_priors=True, prec_min=1e3, on_step=on_step, **FIT_KW)
    assert isinstance(out["priors"], sweep.GroupPriors) and out["clamped"] == expect == {0: 9, 1: 9}
    assert bool((out["priors"].prec == 1e3).all()) and str(out["priors"].prec.device).startswith("cuda")
    assert whats == [0, ("prior", 0), 1, ("prior", 1), "bias"]
    # learn_mean=False leaves the means untouched
    m._flat.copy_(start)
    pr = sweep.GroupPriors(2, 8, DEV)
    g = torch.Generator().manual_seed(3)
    pr.mean.copy_((torch.rand(2, 9, generator=g) - 0.5).to(DEV))
    means = pr.mean.clone()
    out = m.fit_bound(Xd, yd, n_sweeps=1, priors=pr, learn_priors=True, learn_mean=False, **FIT_KW)
    assert torch.equal(pr.mean, means) and not bool((pr.prec == 1.0).any()) and out["clamped"] == {0: 0, 1: 0}
    # given priors without learning are solved under and left alone; no "clamped" then
    m._flat.copy_(start)
    state = pr.state_dict()
    out = m.fit_bound(Xd, yd, n_sweeps=1, priors=pr, **FIT_KW)
    assert out["priors"] is pr and "clamped" not in out
    assert torch.equal(pr.mean, state["mean"]) and torch.equal(pr.prec, state["prec"])
    under = m._flat.clone()
    m._flat.copy_(start)
    plain = m.fit_bound(Xd, yd, n_sweeps=1, **FIT_KW)
    assert "priors" not in plain and not torch.equal(m._flat, under)

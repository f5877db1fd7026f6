"""GPU: the implicit-feedback solve with a confidence weight per observed pair (include/vfm_implicit_weights.h:
VFM.fold_in_implicit(weights=), implicit_objective(weights=), fit_implicit(weights=)) against the fp64 reference of
tests/implicit_weights_reference.py, which solves every entity from a dense [N, M] weight matrix.

Cases and bounds: those of tests/test_gpu_fit_implicit.py (CHUNK = 16, W0 = f32(0.15), KLW = f32(0.7), its _case and
_counts).  The weights are fp32, uniform in [W0, 16 W0], a few rows exactly W0 (implicit_weights_reference.draw_weights).
Rows written by a solve: per element |got - ref| <= 2^-23 |ref| + 4 (d + 1) 2^-52 cond(H) max|ref|
(solve_reference.elementwise_ok / solve_abs_term) after asserting cond(H) <= 1e3 on the reference's own matrix, the
scales with solve_reference.scale_abs_term over 2 n_dense.  Losses and J_imp: 1e-5 relative.  J_imp after a block:
J_after <= J_before + 1e-9 |J_before|.  The cap on cond(H) is a condition on the inputs: with the reference alone, on the
CPU, before any GPU run, the worst is 5.8 over the solve cases at d = 1 .. 128, 6.9 at the LDS / slab crossing, 6.2 over
the five catalog sizes, 4.7 under a prior and 7.0 at the start of the sweeps, against the parent's 5.6 at w1 / w0 = 8.3:
the weight range [W0, 16 W0] did not have to be narrowed.

Every test here fails on the parent of this feature: weights= is a TypeError there and the op does not exist.

Measured on an MI355X: worst elementwise ratio of the solve 0.499 over d = 1, 8, 9, 33, 128, 134, 135, both links, both
fields, the five catalog sizes and d = 8, 33 under a prior (1 = at the bound; the reference itself rounded to fp32 gives
at most 0.5), of the field blocks of three fit_implicit(weights=) sweeps 0.486 and of their prior blocks 0.483; losses
within 5.9e-8 and J_imp within 2.1e-8 relative; worst cond(H) 6.9."""
import ctypes as C

import pytest
import torch

import implicit_reference as IR
import implicit_weights_reference as IWR
import prior_reference as P
import solve_reference as R
from test_gpu_fit_implicit import (CHUNK, KLW, W0, W1, _case, _counts, _model_of, _rows_of, _tables_of, _written)

pytestmark = pytest.mark.gpu
DEV = "cuda"
LINKS = ["abs", "softplus"]
RATIO = 16.0


def _wcase(*a, **kw):
    """test_gpu_fit_implicit._case with c["w"]: a weight per row in [W0, 16 W0], three of them exactly W0."""
    c = _case(*a, **kw)
    c["w"] = IWR.draw_weights(c["x"].shape[0], W0, kw["seed"] + 7, RATIO)
    return c


def _priors_of(d, seed):
    from vae_amd import sweep
    pr = sweep.GroupPriors(2, d, DEV)
    mean, prec = P.draw_priors(2, d, seed, P.prec_lo_for(d))                 # means in [-0.5, 0.5], precisions in [0.25, 16]
    pr.load_state_dict({"mean": mean.float(), "prec": prec.float()})
    return pr


def _row64(pr, field):
    return None if pr is None else (pr.mean[field].cpu().double(), pr.prec[field].cpu().double())


def _fold(c, m, pr=None, field=None, w=True, **kw):
    """w True: the case's weights; None: the call without weights= (w1 = W1); else the tensor given."""
    kw.setdefault("chunk_rows", CHUNK)
    if pr is not None:
        kw["priors"] = pr
    if w is None:
        kw["w1"] = W1
    else:
        kw["weights"] = (c["w"] if w is True else w).to(DEV)
    return m.fold_in_implicit(c["x"].to(DEV), c["y"].to(DEV), c["field"] if field is None else field, w0=W0,
                              kl_weight=KLW, **kw)


def reference_of(tab, c, ids, field=None, pr=None, w=None):
    """implicit_solve_fp64 of the case (CPU only: the cap on cond(H) is asserted here, on the reference's matrix)."""
    field = c["field"] if field is None else field
    sol = IWR.implicit_solve_fp64(*tab, c["x"], c["y"], c["w"] if w is None else w, field, c["N"], c["M"], c["link"], W0,
                                  KLW, entities=ids, prior=pr)
    assert float(sol["cond"].max()) <= 1e3, sol["cond"]
    return sol


def _check(tab, c, m, out, what, field=None, pr=None, w=None):
    """The rows of out["entities"] written into m against the reference from the tables `tab` per element, out["loss"]
    against entity_loss_fp64 at the written rows and, under a prior, the sensitivity of the parent test: the fp64 optimum
    under N(0, 1) misses the bound for every entity.  Returns (worst ratio, worst loss error)."""
    field = c["field"] if field is None else field
    ent, bia, scal = tab
    N, M, d, link = c["N"], c["M"], c["d"], c["link"]
    wts = c["w"] if w is None else w
    prior = _row64(pr, field)
    ids = out["entities"].cpu()
    sol = reference_of(tab, c, ids, field, prior, wts)
    std = reference_of(tab, c, ids, field, None, wts) if prior is not None else None
    theta, s = _written(m, ids)
    n_dense = M if field == 0 else N
    rs = IR.inv_link_t(sol["sigma"], link)
    worst, worst_l = 0.0, 0.0
    for i, e in enumerate(ids.tolist()):
        rt = sol["theta"][i].numpy()
        abs_t, abs_s = R.solve_abs_term(d, float(sol["cond"][i]), rt), R.scale_abs_term(2 * n_dense, rs[i].numpy())
        ok_t, w_t = R.elementwise_ok(theta[i], rt, abs_t)
        ok_s, w_s = R.elementwise_ok(s[i], rs[i].numpy(), abs_s)
        assert ok_t and ok_s, (what, e, int(out["rows"][i]), w_t, w_s)
        worst = max(worst, w_t, w_s)
        if std is not None:
            miss_t = not R.elementwise_ok(std["theta"][i], rt, abs_t)[0]
            miss_s = not R.elementwise_ok(IR.inv_link_t(std["sigma"][i], link), rs[i].numpy(), abs_s)[0]
            assert miss_t and miss_s, (what, e, "the N(0, 1) optimum is within the bound: the case does not see the prior")
        L = float(IWR.entity_loss_fp64(ent, bia, scal, c["x"], c["y"], wts, field, N, M, link, W0, KLW, e, theta[i],
                                       IR.link_t(s[i], link), prior))
        err = abs(float(out["loss"][i]) - L) / abs(L)
        assert err <= 1e-5, (what, e, float(out["loss"][i]), L)
        worst_l = max(worst_l, err)
    print(f"IMPLICIT-WEIGHTS {what} {link} d={d} field={field}: worst ratio {worst:.3f}, loss rel_err {worst_l:.2e}, "
          f"worst cond {float(sol['cond'].max()):.1f}")
    return worst, worst_l


# ---------------------------------------------------------------------------------------------------------------------
# the solve against implicit_solve_fp64 of the dense weight matrix
# ---------------------------------------------------------------------------------------------------------------------
def solve_case(d, link, field):
    from vae_amd import sweep
    split = sweep.resolve_split_rows(20, d)                                # (max(20, d + 1))
    counts = _counts(d, split)
    return _wcase(len(counts) + 1, CHUNK * 40 + 5, d, link, counts, seed=500 + d, field=field), counts


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("d", [1, 8, 9, 33, 128])
def test_weighted_solve_matches_fp64(d, link, field):
    c, counts = solve_case(d, link, field)
    m = _model_of(c)
    tab = _tables_of(m)
    out = _fold(c, m, split_rows=20)
    assert out["rows"].tolist() == counts + [0] and out["entities"].numel() == len(counts) + 1
    _check(tab, c, m, out, "solve")


def lds_case(d, link):
    return _wcase(4, 200, d, link, [0, d + 2, CHUNK * (d // CHUNK + 2) + 1], seed=600 + d)


@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("d", [R.LDS - 1, R.LDS])
def test_triangle_in_lds_and_in_the_slab_with_weights(d, link):
    c = lds_case(d, link)
    m = _model_of(c)
    tab = _tables_of(m)
    assert R.has_slabs(d) == (d == R.LDS)
    out = _fold(c, m, split_rows=d + 3)                                    # the second in its workgroup, the third in chunks
    _check(tab, c, m, out, "lds/slab")


def catalog_cases(n_partner):
    d = 8
    counts = sorted({0, 1, min(n_partner, d + 1), n_partner})
    return [_wcase(len(counts), n_partner, d, link, counts, seed=700 + n_partner, field=field)
            for link, field in (("abs", 0), ("softplus", 1))]


@pytest.mark.parametrize("n_partner", [1, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5])
def test_catalog_sizes_with_weights(n_partner):
    for c in catalog_cases(n_partner):
        m = _model_of(c)
        tab = _tables_of(m)
        out = _fold(c, m, split_rows=0)
        _check(tab, c, m, out, f"catalog {n_partner}")


@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("d", [8, 33])
def test_weighted_solve_under_a_prior(d, link):
    """PRIOR x WROW.  _check asserts that the N(0, 1) optimum misses the bound: the case sees the prior."""
    c, counts = solve_case(d, link, 0)
    m, pr = _model_of(c), _priors_of(d, 31 + d)
    tab = _tables_of(m)
    out = _fold(c, m, pr, split_rows=20)
    assert out["rows"].tolist() == counts + [0]
    _check(tab, c, m, out, "prior", pr=pr)


# ---------------------------------------------------------------------------------------------------------------------
# exact structure and bits
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("link", LINKS)
def test_rows_of_weight_w0_and_target_0_are_no_rows_bit_for_bit(link):
    """An entity whose rows all weigh exactly W0 with target 0 adds exact zeros to w0 base: it gets the row and the loss
    of the same entity without rows, once in the row-list form (7 rows) and once in the chunk form (45 rows)."""
    c = _wcase(5, 60, 8, link, [7, 45, 5, 30], seed=820)
    null = (c["x"][:, 0] == 0) | (c["x"][:, 0] == 1)
    c["w"][null] = W0
    c["y"][null] = 0.0
    m = _model_of(c)
    start = m._flat.clone()
    out = _fold(c, m, split_rows=20)
    assert out["rows"].tolist() == [7, 45, 5, 30, 0]
    flat = m._flat.clone()
    m._flat.copy_(start)
    keep = ~null
    less = m.fold_in_implicit(c["x"][keep].to(DEV), c["y"][keep].to(DEV), 0, w0=W0, kl_weight=KLW,
                              weights=c["w"][keep].to(DEV), split_rows=20, chunk_rows=CHUNK)
    assert less["rows"].tolist() == [0, 0, 5, 30, 0]
    assert torch.equal(m._flat, flat) and torch.equal(less["loss"], out["loss"])
    assert not torch.equal(_rows_of(m, flat, 0), _rows_of(m, start, 0))
    # ... and the unweighted call without those rows writes entities 0 and 1 the same way: w0 base alone
    m._flat.copy_(start)
    plain = m.fold_in_implicit(c["x"][keep].to(DEV), c["y"][keep].to(DEV), 0, w0=W0, w1=W1, kl_weight=KLW,
                               split_rows=20, chunk_rows=CHUNK)
    for e in (0, 1, 4):
        assert torch.equal(_rows_of(m, m._flat, e), _rows_of(m, flat, e)) and torch.equal(plain["loss"][e], out["loss"][e])
    assert not torch.equal(_rows_of(m, m._flat, 3), _rows_of(m, flat, 3))     # (the weights are read)


@pytest.mark.parametrize("link", LINKS)
def test_constant_weights_meet_the_unweighted_reference(link):
    """weights = full(W1) and the call with w1 = W1 solve the same problem: both within the elementwise bound of the same
    fp64 reference and the objectives within 1e-10 relative.  They need not be bitwise equal: sum (g u) u^T and
    dw sum u u^T round differently."""
    c = _wcase(8, 70, 9, link, [0, 1, 9, 10, 21, 40, 70], seed=830)
    full = torch.full_like(c["w"], W1)
    ref_c = dict(c, w=full)
    X, y = c["x"].to(DEV), c["y"].to(DEV)
    res = {}
    for name, w in (("weights", full), ("w1", None)):
        m = _model_of(c)
        tab = _tables_of(m)
        out = _fold(c, m, w=w, split_rows=20)
        res[name] = (_check(tab, ref_c, m, out, f"constant ({name})"), m._flat.clone())
        # the dense reference with W1 everywhere is implicit_reference's (W0, W1) problem
        ids = out["entities"].cpu()
        a = IR.implicit_solve_fp64(*tab, c["x"], c["y"], 0, c["N"], c["M"], link, W0, W1, KLW, entities=ids)
        b = reference_of(tab, ref_c, ids)
        assert torch.allclose(a["theta"], b["theta"], rtol=1e-11, atol=1e-13)
        Jw = m.implicit_objective(X, y, w0=W0, kl_weight=KLW, weights=full.to(DEV))
        J1 = m.implicit_objective(X, y, w0=W0, w1=W1, kl_weight=KLW)
        print(f"IMPLICIT-WEIGHTS constant objective {link} ({name}): rel diff {abs(Jw - J1) / abs(J1):.2e}")
        assert abs(Jw - J1) <= 1e-10 * abs(J1), (Jw, J1)
    print(f"IMPLICIT-WEIGHTS constant {link}: bitwise equal rows: {torch.equal(res['weights'][1], res['w1'][1])}")


def _mixed_case():
    """test_gpu_fit_implicit._mixed's population on a model of its own, with weights: 60 entities of 0 .. 11 observed
    rows and three heavy ones (100, 61 and 47 rows), d = 8, softplus."""
    counts = [g % 12 for g in range(60)]
    counts[17], counts[40], counts[41] = 100, 61, 47
    c = _wcase(60, 130, 8, "softplus", counts, seed=55)
    m = _model_of(c)
    return c, m, m._flat.clone()


def test_bits_with_weights_do_not_depend_on_the_call():
    c, m, start = _mixed_case()
    kw = dict(split_rows=20)
    out = _fold(c, m, **kw)
    flat = m._flat.clone()
    assert out["rows"].tolist() == c["counts"]
    m._flat.copy_(start)
    again = _fold(c, m, **kw)                                              # repeated calls
    assert torch.equal(m._flat, flat) and torch.equal(again["loss"], out["loss"])
    m._flat.copy_(start)
    parent = _fold(c, m, w=None, **kw)                                     # ... and the weights are read
    assert not torch.equal(m._flat, flat) and not torch.equal(parent["loss"], out["loss"])
    # groups: a workspace cap that holds one heavy entity's chunks at a time
    from vae_amd import _lib, sweep
    one = _lib.load().vfm_implicit_solve_weights_workspace_bytes(1, 6, 8, -1)  # (7, 4 and 3 chunks: no two fit together)
    x, y, _, _ = sweep.check_implicit_args(m, c["x"].to(DEV), c["y"].to(DEV), W0, 1.0, KLW, weights=c["w"])
    plan = sweep.ImplicitPlan(m, x, y, 0, None, 20, CHUNK, one, weights=c["w"].to(DEV))
    assert len(plan.obs.groups) == 3 and plan.obs.n_light == 52 and plan.empty.numel() == 5
    m._flat.copy_(start)
    grouped = _fold(c, m, max_workspace_bytes=one, **kw)
    assert torch.equal(m._flat, flat) and torch.equal(grouped["loss"], out["loss"])
    # two entity subsets: each entity's bytes are those of the one call
    for sub in (list(range(0, 30)), list(range(30, 60))):
        m._flat.copy_(start)
        part = _fold(c, m, entities=sub, **kw)
        assert part["entities"].tolist() == sub and torch.equal(part["loss"], out["loss"][sub[0]:sub[-1] + 1])
        for e in sub:
            assert torch.equal(_rows_of(m, m._flat, e), _rows_of(m, flat, e)), e
        other = (sub[0] + 30) % 60
        assert torch.equal(_rows_of(m, m._flat, other), _rows_of(m, start, other))       # nothing else is written
    # alone: a heavy entity, a light one, one without rows
    for e in (17, 40, 5, 0, 59):
        m._flat.copy_(start)
        alone = _fold(c, m, entities=[e], **kw)
        assert alone["entities"].tolist() == [e] and alone["rows"].tolist() == [c["counts"][e]]
        assert torch.equal(alone["loss"], out["loss"][e:e + 1]), e
        assert torch.equal(_rows_of(m, m._flat, e), _rows_of(m, flat, e)), e


@pytest.mark.parametrize("link", LINKS)
def test_weights_none_is_the_parent_bit_for_bit(link):
    counts = [0, 1, 5, 9, 10, 21, 40, 100, 61]                             # no rows, the row-list form, the chunk form
    c = _wcase(len(counts) + 1, 130, 8, link, counts, seed=56)
    m = _model_of(c)
    start = m._flat.clone()
    X, y = c["x"].to(DEV), c["y"].to(DEV)
    for kw in (dict(split_rows=20), dict(split_rows=None), dict(split_rows=0, chunk_rows=7)):
        kw.setdefault("chunk_rows", CHUNK)
        m._flat.copy_(start)
        parent = m.fold_in_implicit(X, y, 0, w0=W0, w1=W1, kl_weight=KLW, **kw)
        flat = m._flat.clone()
        m._flat.copy_(start)
        got = m.fold_in_implicit(X, y, 0, w0=W0, w1=W1, kl_weight=KLW, weights=None, **kw)
        assert torch.equal(m._flat, flat) and torch.equal(got["loss"], parent["loss"]) and not torch.equal(flat, start)
    m._flat.copy_(start)
    a = m.fit_implicit(X, y, 2, w0=W0, w1=W1, kl_weight=KLW, split_rows=20, chunk_rows=CHUNK)
    flat = m._flat.clone()
    m._flat.copy_(start)
    b = m.fit_implicit(X, y, 2, w0=W0, w1=W1, kl_weight=KLW, split_rows=20, chunk_rows=CHUNK, weights=None)
    assert torch.equal(m._flat, flat) and a["objective"] == b["objective"]
    assert m.implicit_objective(X, y, w0=W0, w1=W1, kl_weight=KLW, weights=None) == \
        m.implicit_objective(X, y, w0=W0, w1=W1, kl_weight=KLW)


# ---------------------------------------------------------------------------------------------------------------------
# the objective and the sweeps
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("link", LINKS)
def test_weighted_objective_matches_fp64(link):
    c = _wcase(30, 50, 9, link, [0, 1, 7, 50, 20, 33], seed=900)
    m, pr = _model_of(c), _priors_of(9, 61)
    X, y, w = c["x"].to(DEV), c["y"].to(DEV), c["w"].to(DEV)
    for klw, priors in ((1.0, None), (KLW, None), (KLW, pr)):
        kw = {} if priors is None else {"priors": priors}
        J = m.implicit_objective(X, y, w0=W0, kl_weight=klw, weights=w, **kw)
        ref = float(IWR.brute_J(c["ent"], c["bia"], c["scal"], c["x"], c["y"], c["w"], c["N"], c["M"], link, W0, klw,
                                None if priors is None else (pr.mean.cpu().double(), pr.prec.cpu().double())))
        plain = m.implicit_objective(X, y, w0=W0, w1=1.0, kl_weight=klw, **kw)
        print(f"IMPLICIT-WEIGHTS objective {link} kl {klw}: rel_err {abs(J - ref) / abs(ref):.2e}")
        assert abs(J - ref) <= 1e-5 * abs(ref), (J, ref)
        assert abs(plain - ref) > 1e-3 * abs(ref)                          # the weights are in J


def sweeps_case(link):
    return _wcase(12, 45, 5, link, [0, 1, 5, 30, 12, 21, 40, 3, 0, 17], seed=1000)


@pytest.mark.parametrize("link, learn", [("abs", False), ("softplus", False), ("softplus", True)])
def test_three_weighted_sweeps_block_by_block(link, learn):
    c = sweeps_case(link)
    N, M, d = c["N"], c["M"], c["d"]
    m = _model_of(c)
    pr = _priors_of(5, 71) if learn else None
    X, y, w = c["x"].to(DEV), c["y"].to(DEV), c["w"].to(DEV)
    args = (c["x"], c["y"], c["w"], N, M, link, W0)
    pri = lambda: None if pr is None else (pr.mean.cpu().double().clone(), pr.prec.cpu().double().clone())
    pkw = {} if pr is None else {"priors": pr}
    state = {"tab": _tables_of(m), "pri": pri(), "J": [], "whats": [], "worst": 0.0, "worst_p": 0.0, "worst_J": 0.0}
    state["J"].append(float(IWR.brute_J(*state["tab"], *args, KLW, state["pri"])))

    def on_step(sweep, what):
        before, p0 = state["tab"], state["pri"]
        now, p1 = _tables_of(m), pri()
        state["whats"].append((sweep, what))
        if what == "scalars":
            s1 = IWR.bias_block_fp64(before[0], before[1], before[2].double(), *args, KLW)
            s2 = IWR.precision_block_fp64(before[0], before[1], s1, *args)
            assert torch.equal(now[0], before[0]) and torch.equal(now[1], before[1])
            # the observed rows' moments are the fp32 kernel's: 1e-5 relative, as for the losses (the parent test's bound)
            assert torch.allclose(now[2].double(), s2, rtol=1e-5, atol=1e-7), (now[2], s2)
        elif isinstance(what, tuple):
            f = what[1]
            assert what[0] == "prior" and all(torch.equal(a, b) for a, b in zip(now, before))
            rm, rl, _ = IWR.IPR.prior_block_fp64(now[0], now[1], f, N, M, link, p0[0][f])
            ok_m, w_m = R.elementwise_ok(p1[0][f], rm.numpy(), 0.0)
            ok_l, w_l = R.elementwise_ok(p1[1][f], rl.numpy(), 0.0)
            assert ok_m and ok_l, (sweep, what, w_m, w_l)
            state["worst_p"] = max(state["worst_p"], w_m, w_l)
        else:
            lo, hi = (0, N) if what == 0 else (N, N + M)
            ids = torch.arange(lo, hi)
            sol = IWR.implicit_solve_fp64(*before, c["x"], c["y"], c["w"], what, N, M, link, W0, KLW,
                                          prior=None if p0 is None else (p0[0][what], p0[1][what]))
            assert float(sol["cond"].max()) <= 1e3
            theta, s = _written(m, ids)
            rs = IR.inv_link_t(sol["sigma"], link)
            for i in range(ids.numel()):
                rt = sol["theta"][i].numpy()
                ok_t, w_t = R.elementwise_ok(theta[i], rt, R.solve_abs_term(d, float(sol["cond"][i]), rt))
                ok_s, w_s = R.elementwise_ok(s[i], rs[i].numpy(), R.scale_abs_term(2 * (hi - lo + N + M), rs[i].numpy()))
                assert ok_t and ok_s, (sweep, what, i, w_t, w_s)
                state["worst"] = max(state["worst"], w_t, w_s)
            olo, ohi = (N, N + M) if what == 0 else (0, N)
            assert torch.equal(now[0][olo:ohi], before[0][olo:ohi]) and torch.equal(now[2], before[2])
        J = float(IWR.brute_J(*now, *args, KLW, p1))
        got = m.implicit_objective(X, y, w0=W0, kl_weight=KLW, weights=w, **pkw)
        assert abs(got - J) <= 1e-5 * abs(J), (sweep, what, got, J)
        state["worst_J"] = max(state["worst_J"], abs(got - J) / abs(J))
        assert J <= state["J"][-1] + 1e-9 * abs(state["J"][-1]), (sweep, what, J, state["J"][-1])
        state["J"].append(J)
        state["tab"], state["pri"] = now, p1

    out = m.fit_implicit(X, y, 3, w0=W0, kl_weight=KLW, split_rows=9, chunk_rows=CHUNK, on_step=on_step, weights=w,
                         update_scalars=True, learn_priors=learn, **pkw)
    blocks = (0, ("prior", 0), 1, ("prior", 1), "scalars") if learn else (0, 1, "scalars")
    assert state["whats"] == [(s, b) for s in range(3) for b in blocks]
    assert out["sweeps"] == 3 and len(out["objective"]) == 4
    for k, J in enumerate(out["objective"]):
        ref = state["J"][len(blocks) * k]
        assert abs(J - ref) <= 1e-5 * abs(ref), (k, J, ref)
    assert state["J"][-1] < state["J"][0]
    print(f"IMPLICIT-WEIGHTS sweeps {link} learn_priors={learn}: worst ratio {state['worst']:.3f}, prior blocks "
          f"{state['worst_p']:.3f}, J_imp rel_err {state['worst_J']:.2e}, J {state['J'][0]:.4f} -> {state['J'][-1]:.4f}")


# ---------------------------------------------------------------------------------------------------------------------
# guards and E = 0 through the raw op (supplied out-of-range ids only; every row list, chunk and weight read is clamped
# to [0, R) by the kernel, so nothing here reads out of bounds)
# ---------------------------------------------------------------------------------------------------------------------
def test_guards_and_an_empty_call_with_weights():
    from vae_amd import _lib
    c = _wcase(6, 40, 8, "abs", [3, 12, 0, 30], seed=1100)
    m = _model_of(c)
    o = _lib.ops()
    d, N, M, T = 8, c["N"], c["M"], c["N"] + c["M"]
    tables = m._views(m._flat)
    base = torch.empty(o.implicit_base_doubles(d), dtype=torch.float64, device=DEV)
    ws = torch.empty(o.implicit_base_workspace_bytes(M, CHUNK, d), dtype=torch.uint8, device=DEV)
    o.implicit_base(*tables, ws, base, N, M, CHUNK, 0)
    order = torch.sort(c["x"][:, 0], stable=True).indices
    xs, ys, wts = c["x"][order], c["y"][order].to(DEV), c["w"][order].contiguous().to(DEV)
    good = xs[:, 1].clone().to(DEV)
    partner = xs[:, 1].clone()
    partner[4] = T + 7                                                     # a row of entity 1: outside the table
    partner[20] = 2                                                        # a row of entity 3: inside it, outside the range
    partner = partner.to(DEV)
    ents = torch.tensor([0, 1, 2, 3, -1, T], device=DEV)
    ptr = torch.tensor([0, 3, 15, 15, 45, 45, 45], device=DEV)
    start = m._flat.clone()

    def solve(ents, row_ptr, cptr, tab, n_chunks, partner=partner, prior=None):
        loss = torch.full((ents.numel(),), 7.0, device=DEV)
        w = torch.empty(max(o.implicit_solve_workspace_bytes(ents.numel(), n_chunks, d, -1), 1), dtype=torch.uint8, device=DEV)
        o.foldin_solve_implicit_weights(ents, row_ptr, cptr, tab, ys, partner, base, *tables, w, loss, prior, wts, N, M, 0,
                                        -1, KLW, W0)
        torch.cuda.synchronize()
        return loss

    def verify(loss):
        flat = m._flat
        assert bool(torch.isnan(loss[4])) and bool(torch.isnan(loss[5]))   # ids outside the table: NaN, nothing written
        for g in (1, 3):
            row = _rows_of(m, flat, g)
            assert bool(torch.isnan(row[:2 * d]).all()) and bool(torch.isnan(row[2 * d])) and bool(torch.isnan(loss[g])), g
            assert bool(torch.isfinite(row[2 * d + 1])), g                 # s_w is a function of the weights alone
        for g in (0, 2):
            assert bool(torch.isfinite(_rows_of(m, flat, g)).all()) and bool(torch.isfinite(loss[g])), g
        assert torch.equal(flat[4 * 2 * d:N * 2 * d], start[4 * 2 * d:N * 2 * d])
        assert torch.equal(flat[N * 2 * d:T * 2 * d], start[N * 2 * d:T * 2 * d])

    verify(solve(ents, ptr, None, None, 0))                                # the row-list form
    m._flat.copy_(start)
    cptr = torch.tensor([0, 1, 2, 2, 4, 4, 4], device=DEV)                 # the chunk form; the last chunk runs past R
    tab = torch.tensor([[0, 0, 3], [1, 3, 12], [3, 15, 16], [3, 31, 1 << 40]], device=DEV)
    verify(solve(ents, None, cptr, tab, 4))
    m._flat.copy_(start)
    # E = 0: nothing is launched, nothing is written
    none = torch.zeros(0, dtype=torch.int64, device=DEV)
    loss = solve(none, torch.zeros(1, dtype=torch.int64, device=DEV), None, None, 0)
    assert loss.numel() == 0 and torch.equal(m._flat, start)
    out = m.fold_in_implicit(c["x"].to(DEV), c["y"].to(DEV), 0, w0=W0, entities=[], weights=c["w"].to(DEV))
    assert out["entities"].numel() == 0 and out["loss"].numel() == 0 and torch.equal(m._flat, start)
    # weights of another length never reach the library
    with pytest.raises(RuntimeError, match="weights"):
        o.foldin_solve_implicit_weights(ents, ptr, None, None, ys, partner, base, *tables,
                                        torch.empty(1, dtype=torch.uint8, device=DEV), torch.empty(6, device=DEV), None,
                                        wts[:-1].contiguous(), N, M, 0, -1, KLW, W0)
    # the C call with p->w1 < p->w0: accepted with weights (w1 is not read: the op's bytes), VFM_E_INVALID without
    lib = _lib.load()
    ok_ents = torch.tensor([0, 1, 2, 3], device=DEV)
    ok_ptr = torch.tensor([0, 3, 15, 15, 45], device=DEV)
    ref_loss = solve(ok_ents, ok_ptr, None, None, 0, partner=good)
    ref_flat = m._flat.clone()
    m._flat.copy_(start)
    loss = torch.full((4,), 7.0, device=DEV)
    wsb = max(lib.vfm_implicit_solve_weights_workspace_bytes(4, 0, d, -1), 1)
    wsp = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    p = _lib.ImplicitSolve()
    for k, v in dict(E=4, R=45, T=T, n_chunks=0, lo=N, n=M, d=d, flags=0, lds_dim=-1, kl_weight=KLW, w0=W0, w1=0.01,
                     entities=ok_ents.data_ptr(), row_ptr=ok_ptr.data_ptr(), y=ys.data_ptr(), partner=good.data_ptr(),
                     base=base.data_ptr(), entity_params=tables[0].data_ptr(), bias_params=tables[1].data_ptr(),
                     scalars=tables[2].data_ptr(), out_loss=loss.data_ptr(), workspace=wsp.data_ptr(),
                     workspace_bytes=wsb).items():
        setattr(p, k, v)
    E_INVALID = _lib._gen.VFM_E_INVALID
    torch.cuda.synchronize()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.vfm_foldin_solve_implicit_weights_f32(C.byref(p), None, None, stream) == E_INVALID      # the parent's w1 check
    assert b"w1" in lib.vfm_last_error() and torch.equal(m._flat, start)
    assert lib.vfm_foldin_solve_implicit_weights_f32(C.byref(p), None, C.c_void_p(wts.data_ptr()), stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(loss, ref_loss) and torch.equal(m._flat, ref_flat) and not torch.equal(ref_flat, start)
    # the parent's VFM_E_INVALID cases still return it with weights
    for bad in (dict(T=0), dict(d=0), dict(E=-1), dict(n=0), dict(flags=4), dict(lds_dim=-2), dict(kl_weight=0.0),
                dict(w0=0.0), dict(chunk_ptr=ok_ptr.data_ptr()), dict(base=None)):
        q = _lib.ImplicitSolve()
        C.memmove(C.byref(q), C.byref(p), C.sizeof(p))
        for k, v in bad.items():
            setattr(q, k, v)
        before = m._flat.clone()
        assert lib.vfm_foldin_solve_implicit_weights_f32(C.byref(q), None, C.c_void_p(wts.data_ptr()), stream) == E_INVALID, bad
        assert torch.equal(m._flat, before)
    m._flat.copy_(start)

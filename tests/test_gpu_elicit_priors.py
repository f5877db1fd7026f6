"""GPU: the exact, bound and design sessions under each field's learnt prior (include/vfm_elicit_prior.h;
elicit_field_exact / elicit_field_bound / elicit_field_design / design_scores_field with priors=).

What is asserted, and by which criterion:
  * priors=None calls the parent op; a GroupPriors at (0, 1) gives priors=None's bits (rows, scores, losses, theta,
    moments, written table), both links, reset on and off; a different prior gives different bits.
  * Under drawn priors (prior_reference.draw_priors(F, d, seed, prec_lo_for(d))) each session is bitwise the loop of
    public calls it replaces, with priors= on both halves; with reset the loop first writes foldin.prior_theta.
  * lds_dim = 0 (slab) and the default (LDS) give the same bits under a prior.
  * The reset row: round 0's moments are field_moments on a model whose respondents' rows hold foldin.prior_theta;
    prior_theta is within one fp32 ulp of the fp64 formula and has prior_s' bits at (0, 1).
  * Against fp64, independently of the shared kernels: along the rows the GPU session asked, every round's posterior
    against prior_reference.solve_fp64_prior / bound_prior_reference.bound_rounds_fp64_prior on the history plus the
    rows asked so far, by solve_reference.elementwise_ok and the loss bounds tests/test_gpu_fit_priors.py and
    tests/test_gpu_fit_bound_priors.py use (tests/test_elicit_priors_cpu.py asserts the cases' condition numbers).
  * The design scores under a prior against the fp64 restatement, by test_gpu_design.py's criterion: |got - ref| <=
    2^-23 |ref| per element."""
import numpy as np
import pytest
import torch

import bound_prior_reference as BP
import design_restatement as DR
import elicit_priors_cases as EC
import prior_reference as PR
import solve_reference as SR
from test_gpu_elicit import _same_bits, _theta_rows
from test_gpu_elicit_field import _problem, _same
from test_gpu_foldin import _model

pytestmark = pytest.mark.gpu
DEV = "cuda"
A3, C2 = (40, 90, 4), (40, 90)


def _priors(m, values=None, seed=None):
    """A GroupPriors on the device: (0, 1), the given (mean, prec), or drawn for the model's d."""
    from vae_amd import sweep
    p = sweep.GroupPriors(m.F, m.d, DEV)
    if seed is not None:
        values = PR.draw_priors(m.F, m.d, seed, PR.prec_lo_for(m.d))
    if values is not None:
        p.load_state_dict({"mean": values[0].float(), "prec": values[1].float()})
    return p


def _write_prior_rows(m, ents, priors, field):
    from vae_amd import foldin
    d = m.d
    th = foldin.prior_theta(m, priors, field).to(DEV)
    ent, bia, _ = m._views(m._flat)
    ent[ents] = th[:2 * d]
    bia[ents] = th[2 * d:]
    m.params_changed()


def _hist(hx, hy, with_hist):
    return (hx, hy) if with_hist else None


def _problem_of(m, sizes, field, strategy, with_hist, d, hist_sizes=(20, 0, 4, 11)):
    small = sizes == C2 and field == 1                       # (40 contexts in all)
    key = [f for f in range(len(sizes)) if f != field][0]    # the default key column
    return _problem(m, field, 11, [3, 9, 17, 12 if small else 30, 1], list(hist_sizes) if with_hist else [0], seed=d,
                    distinct_col=key if strategy == "random" and not small else None)


def _run(kind, m, pool, y_pool, Q, field, strategy, hist, reset, priors, n_iters=3, monkeypatch=None, **kw):
    from vae_amd import design, elicit
    if strategy == "mean" and kind == "exact":
        monkeypatch.setattr(elicit, "_check_questions", lambda model, s, n: None)
    common = dict(history=hist, kl_weight=0.8, reset=reset, priors=priors, **kw)
    if kind == "exact":
        return elicit.run_field_exact(m, pool, y_pool, Q, field, strategy, seed=21, **common)
    if kind == "bound":
        return elicit.run_field_bound(m, pool, y_pool, Q, field, strategy, seed=21, n_iters=n_iters, **common)
    return design.run_field_design(m, pool, y_pool, Q, field, **common)


# ---------------------------------------------------------------------------------------------------------------------
# 1. priors=None is the parent op; the standard prior is priors=None to the bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["exact", "bound", "design", "scores"])
def test_priors_none_calls_the_parent_op(kind, monkeypatch):
    from vae_amd import _lib
    m = _model(A3, 9, "class" if kind == "bound" else "reg", "abs", seed=3)
    pool, y_pool, hx, hy = _problem_of(m, A3, 0, "variance", True, 9)

    class Refusing:
        def __init__(self, o):
            self.o = o

        def __getattr__(self, name):
            if name.endswith("_prior"):
                raise AssertionError(f"{name} called with priors=None")
            return getattr(self.o, name)

    real = _lib.ops()
    monkeypatch.setattr(_lib, "ops", lambda: Refusing(real))
    if kind == "scores":
        out = m.design_scores_field(pool, 0, history=(hx, hy), priors=None)
        assert bool(torch.isfinite(out).all())
    else:
        out = _run(kind, m, pool, y_pool, 3, 0, "variance", (hx, hy), False, None)
        assert int((out["rows"][:, 0] >= 0).sum()) == 11


@pytest.mark.parametrize("kind,link,reset", [(k, l, r) for k in ("exact", "design", "bound")
                                              for l, r in (("abs", False), ("softplus", True), ("softplus", False),
                                                           ("abs", True))])
def test_the_standard_prior_is_priors_none_to_the_bit(kind, link, reset):
    d = 33 if link == "abs" else 9
    m = _model(A3, d, "class" if kind == "bound" else "reg", link, seed=5)
    pool, y_pool, hx, hy = _problem_of(m, A3, 0, "variance", True, d)
    start = m._flat.clone()
    outs, tables = [], []
    for priors in (None, _priors(m), _priors(m, seed=4)):
        m._flat.copy_(start)
        m.params_changed()
        outs.append(_run(kind, m, pool, y_pool, 5, 0, "variance", (hx, hy), reset, priors, write=True,
                         return_theta=True, return_moments=True))
        tables.append(m._flat.clone())
    for k in outs[0]:
        assert _same(outs[0][k], outs[1][k]), k
    assert torch.equal(tables[0], tables[1]) and not torch.equal(tables[0], start)
    assert not _same_bits(outs[0]["theta"], outs[2]["theta"]) and not torch.equal(tables[0], tables[2])


@pytest.mark.parametrize("link", ["abs", "softplus"])
def test_design_scores_at_the_standard_prior(link):
    m = _model(A3, 17, "reg", link, seed=6)
    pool, y_pool, hx, hy = _problem_of(m, A3, 0, "variance", True, 17)
    a = m.design_scores_field(pool, 0, history=(hx, hy), kl_weight=0.7)
    b = m.design_scores_field(pool, 0, history=(hx, hy), kl_weight=0.7, priors=_priors(m))
    c = m.design_scores_field(pool, 0, history=(hx, hy), kl_weight=0.7, priors=_priors(m, seed=2))
    assert _same_bits(a, b) and not _same_bits(a, c)


# ---------------------------------------------------------------------------------------------------------------------
# 2. bitwise the loop each session replaces, under drawn priors
# ---------------------------------------------------------------------------------------------------------------------
def _composed(kind, m, pool, y_pool, Q, field, strategy, hist, reset, priors, n_iters, targets=None):
    """test_gpu_elicit_exact._composed (and its bound and design siblings) with priors= on both halves (modifies m):
    with reset foldin.prior_theta is written into the respondents' rows first; per round the selection on the rows
    still unasked (design: select_next_questions_design_field(priors=) with history + asked as the history), then
    fold_in_exact(priors=) / fold_in_bound(reset=False, priors=) of the answering respondents on their history followed
    by everything they were asked so far.  Returns entities, rows, score, loss [U, Q], theta [U, Q, 2d + 2]."""
    seed, klw = 21, 0.8
    ents = torch.unique(pool[:, field])
    U, P = ents.numel(), pool.shape[0]
    if reset:
        _write_prior_rows(m, ents, priors, field)
    rows = torch.full((U, Q), -1, dtype=torch.int64, device=DEV)
    score = torch.full((U, Q), float("nan"), device=DEV)
    loss = torch.full((U, Q), float("nan"), device=DEV)
    theta = torch.empty(U, Q, 2 * m.d + 2, device=DEV)
    unasked = torch.ones(P, dtype=torch.bool, device=DEV)
    asked = torch.zeros(0, dtype=torch.int64, device=DEV)
    hx, hy = hist if hist is not None else (pool[:0], y_pool[:0])
    tg = pool if targets is None else targets
    for q in range(Q):
        idx = torch.nonzero(unasked).reshape(-1)
        if idx.numel():
            sub = pool[idx]
            if kind == "design":
                here = lambda x: torch.isin(x[:, field], sub[:, field])
                hq = torch.cat([hx[here(hx)], pool[asked][here(pool[asked])]])
                kw = dict(targets=tg[here(tg)], history=(hq, torch.zeros(hq.shape[0], device=DEV)), kl_weight=klw,
                          priors=priors)
                es, r = m.select_next_questions_design_field(sub, field, 1, **kw)
                sc = m.design_scores_field(sub, field, **kw)
            else:
                as_class = strategy == "mean" and m.output == "reg"      # (test_gpu_elicit_exact: the checks stepped over)
                if as_class:
                    m.output = "class"
                try:
                    es, r = m.select_next_questions_field(sub, field, 1, strategy, seed + q, None)
                    _, _, sc = m.field_moments(sub, field, strategy, seed + q, None)
                finally:
                    if as_class:
                        m.output = "reg"
            epos = torch.searchsorted(ents, es)
            rows[epos, q] = idx[r[:, 0]]
            score[epos, q] = sc[r[:, 0]]
            unasked[idx[r[:, 0]]] = False
            asked = torch.cat([asked, idx[r[:, 0]]])
            ha = torch.isin(hx[:, field], es)
            aa = asked[torch.isin(pool[asked, field], es)]
            X, y = torch.cat([hx[ha], pool[aa]]), torch.cat([hy[ha], y_pool[aa]])
            if kind == "bound":
                o = m.fold_in_bound(X, y, field=field, kl_weight=klw, n_iters=n_iters, reset=False, priors=priors)
            else:
                o = m.fold_in_exact(X, y, field=field, kl_weight=klw, priors=priors)
            assert torch.equal(o["entities"], es)
            loss[epos, q] = o["loss"]
        theta[:, q] = _theta_rows(m, ents)
    return ents, rows, score, loss, theta


def _against_the_composition(kind, m, pool, y_pool, Q, field, strategy, hist, reset, priors, n_iters=3,
                             monkeypatch=None, **kw):
    start = m._flat.clone()
    before = priors.state_dict()
    ents, rows, score, loss, theta = _composed(kind, m, pool, y_pool, Q, field, strategy, hist, reset, priors, n_iters)
    final = m._flat.clone()
    m._flat.copy_(start)
    m.params_changed()
    out = _run(kind, m, pool, y_pool, Q, field, strategy, hist, reset, priors, n_iters, monkeypatch, write=True,
               return_theta=True, **kw)
    assert torch.equal(out["entities"], ents)
    assert torch.equal(out["rows"], rows)
    assert _same_bits(out["score"], score)                   # (NaN where nothing was left to ask, in both)
    assert _same_bits(out["loss"], loss)
    assert _same_bits(out["theta"], theta)
    assert torch.equal(m._flat, final) and not torch.equal(final, start)
    assert bool(torch.isfinite(out["loss"][out["rows"] >= 0]).all())
    assert all(torch.equal(before[k], v) for k, v in priors.state_dict().items())
    assert out["entities"].numel() == 11 and int((out["rows"][:, 0] >= 0).sum()) == 11
    return out


# d: 1, then 9 (16, 1), 33 (64, 1), 129 (64, 4), 257 (64, 8: the primal system only in the slab).  Pools of 1 and 3 rows
# run out before Q = 6; 20 history rows: primal from round 0 at d < 20, and at d = 9 a respondent with 4 history rows
# turns from the dual to the primal system inside the session
EXACT_CASES = [  # kind, field sizes, field, link, strategy, d, history, reset
    ("exact", A3, 0, "abs", "variance", 1, True, False),
    ("exact", C2, 1, "softplus", "random", 9, True, True),
    ("exact", A3, 1, "abs", "top", 33, False, True),
    ("exact", A3, 0, "softplus", "mean", 129, True, False),
    ("exact", A3, 0, "abs", "variance", 257, True, True),
    ("design", C2, 0, "softplus", None, 1, False, True),
    ("design", A3, 1, "abs", None, 9, True, False),
    ("design", A3, 0, "softplus", None, 33, True, True),
    ("design", A3, 1, "abs", None, 129, False, False),
    ("design", A3, 0, "softplus", None, 257, True, False),
]


@pytest.mark.parametrize("kind,sizes,field,link,strategy,d,with_hist,reset", EXACT_CASES)
def test_exact_and_design_sessions_are_bitwise_the_loop(kind, sizes, field, link, strategy, d, with_hist, reset,
                                                        monkeypatch):
    m = _model(sizes, d, "reg", link, seed=d + 2, rng_seed=3)
    pool, y_pool, hx, hy = _problem_of(m, sizes, field, strategy or "variance", with_hist, d)
    out = _against_the_composition(kind, m, pool, y_pool, 6, field, strategy, _hist(hx, hy, with_hist), reset,
                                   _priors(m, seed=d + 7), monkeypatch=monkeypatch)
    assert int((out["rows"] < 0).sum()) > 0


BOUND_CASES = [  # field sizes, field, link, strategy, d, history, reset, n_iters
    (A3, 0, "abs", "variance", 1, True, False, 8),
    (C2, 0, "softplus", "top", 8, False, True, 1),
    (C2, 1, "abs", "random", 8, True, True, 8),
    (A3, 1, "softplus", "mean", 33, True, True, 1),
    (A3, 0, "abs", "mean", 33, False, False, 8),
    (A3, 1, "softplus", "variance", 129, True, False, 1),
    (A3, 0, "abs", "top", 129, True, True, 8),
    (A3, 0, "softplus", "random", 1, True, False, 1),
]


@pytest.mark.parametrize("sizes,field,link,strategy,d,with_hist,reset,n_iters", BOUND_CASES)
def test_bound_sessions_are_bitwise_the_loop(sizes, field, link, strategy, d, with_hist, reset, n_iters):
    m = _model(sizes, d, "class", link, seed=d + 2, rng_seed=3)
    pool, y_pool, hx, hy = _problem_of(m, sizes, field, strategy, with_hist, d)
    _against_the_composition("bound", m, pool, y_pool, 6, field, strategy, _hist(hx, hy, with_hist), reset,
                             _priors(m, seed=d + 9), n_iters)


# ---------------------------------------------------------------------------------------------------------------------
# 3. where the triangle lives: the LDS layout behind the prior against the slab
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["exact", "design", "bound"])
@pytest.mark.parametrize("d", [9, 33])
def test_where_the_triangle_lives_does_not_matter_under_a_prior(kind, d):
    m = _model(A3, d, "class" if kind == "bound" else "reg", "softplus", seed=8)
    pool, y_pool, hx, hy = _problem_of(m, A3, 0, "variance", True, d, hist_sizes=(40, 0, 4, 11))
    priors = _priors(m, seed=d)
    kw = dict(return_theta=True, return_moments=True)
    a = _run(kind, m, pool, y_pool, 6, 0, "variance", (hx, hy), True, priors, lds_dim=-1, **kw)
    b = _run(kind, m, pool, y_pool, 6, 0, "variance", (hx, hy), True, priors, lds_dim=0, **kw)
    for k in a:
        assert _same(a[k], b[k]), k
    assert bool(torch.isfinite(a["loss"][a["rows"] >= 0]).all())


# ---------------------------------------------------------------------------------------------------------------------
# 4. the reset row
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,link,d", [("exact", "abs", 9), ("exact", "softplus", 129), ("bound", "softplus", 9),
                                         ("design", "abs", 33)])
def test_round_zero_of_a_reset_session_is_scored_from_prior_theta(kind, link, d):
    m = _model(A3, d, "class" if kind == "bound" else "reg", link, seed=9)
    pool, y_pool, hx, hy = _problem_of(m, A3, 1, "variance", True, d)
    priors = _priors(m, seed=d + 1)
    out = _run(kind, m, pool, y_pool, 2, 1, "variance", (hx, hy), True, priors, return_moments=True)
    _write_prior_rows(m, torch.unique(pool[:, 1]), priors, 1)
    mean, var, _ = m.field_moments(pool, 1)
    assert _same_bits(out["logit_mean"][0], mean) and _same_bits(out["logit_var"][0], var)


@pytest.mark.parametrize("link", ["abs", "softplus"])
def test_prior_theta_is_the_fp64_formula_rounded(link):
    from vae_amd import foldin
    m = _model(A3, 33, "reg", link, seed=1)
    d = m.d
    std = foldin.prior_theta(m, _priors(m), 0)
    assert _same_bits(std, foldin.prior_theta(m, None, 0))
    ps = torch.tensor(foldin.prior_s(link), dtype=torch.float32)
    assert bool((std[:d] == 0).all()) and std[2 * d] == 0 and _same_bits(std[d:2 * d], ps.expand(d).contiguous())
    assert _same_bits(std[2 * d + 1:], ps.reshape(1))
    mean, prec = PR.draw_priors(m.F, d, 5, 0.25)
    got = foldin.prior_theta(m, _priors(m, (mean, prec)), 2).double()
    sg = PR.inv_link_t(torch.sqrt(1.0 / prec[2]), link)
    want = torch.cat([mean[2, 1:], sg[1:], mean[2, :1], sg[:1]])
    assert bool(((got - want).abs() <= SR.EPS32 * want.abs()).all())


# ---------------------------------------------------------------------------------------------------------------------
# 5. against fp64 along the session's own rows, independently of the shared kernels
# ---------------------------------------------------------------------------------------------------------------------
def _planted(c):
    m = _model(c["sizes"], c["d"], c["output"], c["link"], seed=1)
    m.entity_params.weight.data.copy_(c["ent"])
    m.bias_params.weight.data.copy_(c["bia"])
    m._flat[m._off_scal: m._off_scal + 3] = c["scal"].to(DEV)
    m.params_changed()
    return m, _priors(m, (c["mean"], c["prec"]))


@pytest.mark.parametrize("name", ["exact", "design"])
def test_exact_posteriors_against_fp64_along_the_sessions_rows(name):
    c = EC.case(name)
    m, priors = _planted(c)
    pool, y_pool, hx, hy = (c[k].to(DEV) for k in ("pool", "y_pool", "hist_x", "hist_y"))
    out = _run(name, m, pool, y_pool, c["Q"], c["field"], "variance", (hx, hy), True, priors, return_theta=True)
    f, d = c["field"], c["d"]
    klw = SR.f32(c["klw"])                                   # (kl_weight as the kernel receives it)
    rows, theta, loss = out["rows"].cpu(), out["theta"].cpu(), out["loss"].cpu()
    assert bool((rows >= 0).all())
    worst = 0.0
    for u, e in enumerate(out["entities"].tolist()):
        for q in range(c["Q"]):
            x, y = EC.rows_of(c, e, rows[u, :q + 1])
            ref = PR.solve_fp64_prior(c["ent"], c["bia"], c["scal"], x, y, f, c["link"], klw, c["mean"][f], c["prec"][f])
            cond, n = float(ref["cond"][0]), x.shape[0]
            assert cond <= EC.COND_EXACT
            got = theta[u, q]
            gt, gs = torch.cat([got[2 * d:2 * d + 1], got[:d]]), torch.cat([got[2 * d + 1:], got[d:2 * d]])
            rt = np.concatenate([[float(ref["mu_w"][0])], ref["mu"][0].numpy()])
            rs = np.concatenate([[float(ref["s_w"][0])], ref["s"][0].numpy()])
            ok_t, w_t = SR.elementwise_ok(gt, rt, SR.solve_abs_term(d, cond, rt))
            ok_s, w_s = SR.elementwise_ok(gs, rs, SR.scale_abs_term(n, rs))
            worst = max(worst, w_t, w_s)
            assert ok_t and ok_s, (e, q, w_t, w_s)
            th = (torch.tensor([e]), gt[None, 1:].double(), gs[None, 1:].double(), gt[:1].double(), gs[:1].double())
            want = float(PR.entity_objective_prior(c["ent"], c["bia"], c["scal"], x, y.double(), f, th, c["link"], klw,
                                                   c["mean"][f], c["prec"][f])[0])
            assert abs(float(loss[u, q]) - want) <= 1e-5 * abs(want), (e, q, float(loss[u, q]), want)
    print(f"{name}: worst elementwise ratio {worst:.3f}")


def test_bound_posteriors_against_fp64_along_the_sessions_rows():
    c = EC.case("bound")
    m, priors = _planted(c)
    pool, y_pool, hx, hy = (c[k].to(DEV) for k in ("pool", "y_pool", "hist_x", "hist_y"))
    out = _run("bound", m, pool, y_pool, c["Q"], c["field"], "variance", (hx, hy), True, priors, n_iters=c["n_iters"],
               return_theta=True)
    f, d = c["field"], c["d"]
    rows, theta, loss = out["rows"].cpu(), out["theta"].cpu(), out["loss"].cpu()
    assert bool((rows >= 0).all())
    worst = 0.0
    for u, e in enumerate(out["entities"].tolist()):
        start = EC.prior_start(c)
        for q in range(c["Q"]):
            x, y = EC.rows_of(c, e, rows[u, :q + 1])
            r = EC.bound_fold(c, x, y, e, start)
            cond = float(r["cond"].max())
            assert cond <= EC.COND_BOUND
            got = theta[u, q]
            gt, gs = torch.cat([got[2 * d:2 * d + 1], got[:d]]), torch.cat([got[2 * d + 1:], got[d:2 * d]])
            at = c["n_iters"] * SR.solve_abs_term(d, cond, r["theta"][-1])
            ok_t, w_t = SR.elementwise_ok(gt, r["theta"][-1], at)
            ok_s, w_s = SR.elementwise_ok(gs, r["s"][-1], at + SR.scale_abs_term(r["n"], r["s"][-1]))
            worst = max(worst, w_t, w_s)
            assert ok_t and ok_s, (e, q, w_t, w_s)
            want = BP.bound_objective_fp64_prior(c["ent"], c["bia"], c["scal"], x, y, f, c["link"], c["klw"], e, gt, gs,
                                                 c["mean"][f], c["prec"][f])
            assert abs(float(loss[u, q]) - want) <= 1e-5 * abs(want), (e, q, float(loss[u, q]), want)
            start = EC.start_of_row(c, gt[:1].numpy(), gt[1:].numpy(), gs[:1].numpy(), gs[1:].numpy())   # (the next fold reads the fp32 row)
    print(f"bound: worst elementwise ratio {worst:.3f}")


# ---------------------------------------------------------------------------------------------------------------------
# 6. the design score under a prior against the fp64 restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d5_abs", "d20_softplus", "d128_softplus"])
def test_design_scores_under_a_prior_against_fp64(name):
    c, ref = DR.build(name)
    m = _model(c["sizes"], c["d"], "reg", c["link"], seed=1)
    m.entity_params.weight.data.copy_(c["ent"])
    m.bias_params.weight.data.copy_(c["bia"])
    m._flat[m._off_scal: m._off_scal + 3] = c["scal"].to(DEV)
    m.params_changed()
    g = {k: (c[k].to(DEV) if c[k] is not None else None) for k in ("pool", "hist_x", "hist_y", "targets")}
    hist = (g["hist_x"], g["hist_y"]) if g["hist_x"].shape[0] else None
    f = c["field"]
    mean, prec = PR.draw_priors(len(c["sizes"]), c["d"], 3, 0.25)
    got = m.design_scores_field(g["pool"], f, targets=g["targets"], history=hist, kl_weight=c["klw"],
                                priors=_priors(m, (mean, prec))).cpu()
    pk, kl = DR.prec_kl(c["scal"], c["link"], c["klw"])
    worst = 0.0
    for e, r in ref.items():
        pm, hm = c["pool"][:, f] == e, c["hist_x"][:, f] == e
        Mp, Ap = DR.operands(c["ent"], c["bia"], c["scal"], c["pool"][pm].numpy(), f, c["link"])
        Mh, Ah = DR.operands(c["ent"], c["bia"], c["scal"], c["hist_x"][hm].numpy(), f, c["link"])
        want = EC.design_scores_prior(DR.walk_S(Mh, Ah), r["W"], int(hm.sum()), Mp, Ap, kl, pk, prec[f].numpy())
        err = np.abs(got[pm].double().numpy() - want)
        worst = max(worst, float((err / (SR.EPS32 * np.abs(want))).max()))
        assert (err <= SR.EPS32 * np.abs(want)).all(), (e, worst)
    print(f"{name}: worst |got - ref| / (2^-23 |ref|) = {worst:.3f}")


# ---------------------------------------------------------------------------------------------------------------------
# 7 / 8. write=False, the curves and the ranking curve
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["exact", "design", "bound"])
def test_write_false_leaves_the_table_and_the_priors_alone(kind):
    m = _model(A3, 9, "class" if kind == "bound" else "reg", "abs", seed=2)
    pool, y_pool, hx, hy = _problem_of(m, A3, 0, "variance", True, 9)
    priors = _priors(m, seed=1)
    start, before = m._flat.clone(), priors.state_dict()
    _run(kind, m, pool, y_pool, 4, 0, "variance", (hx, hy), True, priors, write=False)
    assert torch.equal(m._flat, start)
    assert all(torch.equal(before[k], v) for k, v in priors.state_dict().items())


def test_curves_take_priors():
    m = _model(A3, 9, "reg", "abs", seed=2)
    pool, y_pool, hx, hy = _problem_of(m, A3, 0, "variance", True, 9)
    priors = _priors(m, seed=1)
    a = m.elicitation_curve_field_exact(pool, y_pool, 3, 0, strategies=("variance", "design"), history=(hx, hy),
                                        reset=True, priors=priors)
    b = m.elicitation_curve_field_exact(pool, y_pool, 3, 0, strategies=("variance", "design"), history=(hx, hy),
                                        reset=True)
    for s in ("variance", "design"):
        assert len(a[s]) == 4 and all(np.isfinite(a[s])) and a[s] != b[s]
    mc = _model(A3, 9, "class", "abs", seed=2)
    pool, y_pool, hx, hy = _problem_of(mc, A3, 0, "variance", True, 9)
    c = mc.elicitation_curve_field_bound(pool, y_pool, 3, 0, strategies=("variance",), history=(hx, hy), reset=True,
                                         priors=_priors(mc, seed=1))
    assert len(c["variance"]) == 4


def test_ranking_curve_round_zero_is_ranked_at_prior_theta():
    from vae_amd import foldin
    m = _model(C2, 9, "reg", "abs", seed=2)
    pool, y_pool, hx, hy = _problem_of(m, C2, 0, "variance", False, 9)
    priors = _priors(m, seed=1)
    ents = torch.unique(pool[:, 0])
    idx = torch.arange(ents.numel(), device=DEV).repeat_interleave(4)
    X_test = torch.stack([ents[idx], 40 + 4 * idx + torch.arange(4, device=DEV).repeat(ents.numel())], 1)
    y_test = torch.full((X_test.shape[0],), 5.0, device=DEV)
    r = m.elicitation_ranking_curve_field(pool, y_pool, 2, 0, X_test, y_test, 1, ks=(5,), strategies=("variance",),
                                          exact=True, reset=True, priors=priors, ineligible="drop")
    queries = torch.stack([ents, torch.zeros_like(ents)], 1)
    theta = foldin.prior_theta(m, priors, 0).to(DEV).expand(ents.numel(), -1).contiguous()
    want = m.evaluate_ranking_field_posterior(queries, (idx, X_test[:, 1].contiguous()), y_test, theta, 0, 1, ks=(5,),
                                              ineligible="drop")
    compared = [k for k in r["variance"] if k in want]
    assert len(compared) >= 3, (sorted(r["variance"]), sorted(want))
    for k in compared:
        assert r["variance"][k][0] == want[k], k
    std = m.elicitation_ranking_curve_field(pool, y_pool, 2, 0, X_test, y_test, 1, ks=(5,), strategies=("variance",),
                                            exact=True, reset=True, ineligible="drop")
    assert any(std["variance"][k][0] != want[k] for k in compared)

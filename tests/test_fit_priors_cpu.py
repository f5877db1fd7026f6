"""CPU: hierarchical sweeps (VFM.fit_exact(learn_priors=True), include/vfm_prior.h) -- the fp64 restatement of
tests/prior_reference.py checked with autograd (each block is a stationary point, the clamped prior block a constrained
minimum), the monotone descent of J, the ties to the parent (standard prior, rescaling), and everything the feature
rejects before a GPU is needed: header, exports, workspace formulas, argument codes, ValueErrors, GroupPriors."""
import ctypes as C
import os
import re

import pytest
import torch

import prior_reference as P
from test_foldin_cpu import _cpu_model
from test_foldin_exact_cpu import _problem, solve_fp64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINKS = ["abs", "softplus"]


# ---------------------------------------------------------------------------------------------------------------------
# the blocks
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kl_weight", [1.0, 0.7])
@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("F", [2, 3])
def test_entity_block_is_stationary_and_its_two_forms_agree(F, link, kl_weight):
    for d in (3, 12):                                          # (more rows than d on some entities; fewer)
        ent, bia, scal, x, y, field = _problem(F, d, 20 + F + d)
        mean, prec = P.draw_priors(F, d, 5 + d)
        m, lam = mean[field], prec[field]
        sol = P.solve_fp64_prior(ent, bia, scal, x, y, field, link, kl_weight, m, lam)
        theta = [sol[k].clone().requires_grad_(True) for k in ("mu", "s", "mu_w", "s_w")]
        L = P.entity_objective_prior(ent, bia, scal, x, y, field, (sol["entities"], *theta), link, kl_weight, m, lam)
        L.sum().backward()
        for t in theta:
            assert float(t.grad.abs().max()) <= 1e-10
        dual = P.solve_fp64_prior(ent, bia, scal, x, y, field, link, kl_weight, m, lam, form="dual")
        for k in ("mu", "s", "mu_w", "s_w"):
            assert float((dual[k] - sol[k]).abs().max()) <= 1e-9, k


def _small(F, link, seed=3, d=4):
    """A planted problem on which every entity of every field occurs: (ent, bia, scal, x, y, sizes)."""
    sizes = [6, 5, 3][:F]
    g = torch.Generator().manual_seed(seed)
    T = sum(sizes)
    ent = torch.randn(T, 2 * d, generator=g, dtype=torch.float64) * 0.5
    bia = torch.randn(T, 2, generator=g, dtype=torch.float64) * 0.5
    scal = torch.tensor([1.3, 0.2, 0.4], dtype=torch.float64)
    lo = [sum(sizes[:f]) for f in range(F)]
    R = 60
    x = torch.stack([lo[f] + torch.randint(0, sizes[f], (R,), generator=g) for f in range(F)], 1)
    for f in range(F):
        x[:sizes[f], f] = lo[f] + torch.arange(sizes[f])
    y = torch.randn(R, generator=g, dtype=torch.float64) + 1.0
    return ent, bia, scal, x, y, sizes


@pytest.mark.parametrize("learn_mean", [True, False])
@pytest.mark.parametrize("link", LINKS)
def test_prior_block_is_stationary_when_unclamped(link, learn_mean):
    ent, bia, scal, x, y, sizes = _small(2, link)
    mean, prec = P.draw_priors(2, 4, 9)
    f = 1
    m, lam, raw = P.prior_block_fp64(ent, bia, x, f, link, mean[f], learn_mean)
    assert torch.equal(lam, raw)                               # (nothing clamped)
    if not learn_mean:
        assert torch.equal(m, mean[f])
    mean2, prec2 = mean.clone(), prec.clone()
    mean2[f], prec2[f] = m, lam
    mean2.requires_grad_(True)
    prec2.requires_grad_(True)
    J = P.objective_J_prior(ent, bia, scal, x, y, sizes, link, 0.7, mean2, prec2)
    J.backward()
    assert float(prec2.grad[f].abs().max()) <= 1e-10
    if learn_mean:
        assert float(mean2.grad[f].abs().max()) <= 1e-10
    assert float(J.detach()) <= float(P.objective_J_prior(ent, bia, scal, x, y, sizes, link, 0.7, mean, prec))


@pytest.mark.parametrize("side", ["max", "min"])
def test_clamped_prior_block_is_the_constrained_minimum(side):
    ent, bia, scal, x, y, sizes = _small(2, "abs")
    f, d = 0, 4
    e = torch.unique(x[:, f])
    if side == "max":                                          # the field's entities collapse onto one point
        ent[e, :d] = 0.25
        ent[e, d:] = 1e-3
        lo, hi = 1e-4, 1e4
    else:                                                      # ... or spread far apart
        ent[e, :d] = torch.arange(e.numel(), dtype=torch.float64)[:, None] * 300.0
        lo, hi = 1e-4, 1e4
    mean, prec = P.standard(2, d)
    m, lam, raw = P.prior_block_fp64(ent, bia, x, f, "abs", mean[f], True, lo, hi)
    bound = hi if side == "max" else lo
    assert bool((lam[1:] == bound).all()) and bool(((raw[1:] > hi) if side == "max" else (raw[1:] < lo)).all())

    def J_at(v):
        p2, m2 = prec.clone(), mean.clone()
        m2[f] = m
        p2[f] = lam
        p2[f, 1:] = v
        return P.objective_J_prior(ent, bia, scal, x, y, sizes, "abs", 1.0, m2, p2)

    at = float(J_at(bound))
    for v in torch.logspace(-4, 4, 41, dtype=torch.float64).tolist():          # every feasible value is no better
        assert at <= float(J_at(v)) + 1e-12 * abs(at), v
    v = torch.full((d,), bound, dtype=torch.float64, requires_grad=True)      # ... and J still falls towards the bound
    p2 = prec.clone()
    p2[f] = lam
    m2 = mean.clone()
    m2[f] = m
    Jg = P.objective_J_prior(ent, bia, scal, x, y, sizes, "abs", 1.0, m2,
                             torch.cat([p2[:f], torch.cat([p2[f, :1], v])[None], p2[f + 1:]]))
    Jg.backward()
    assert bool((v.grad < 0).all()) if side == "max" else bool((v.grad > 0).all())


def test_package_prior_block_is_the_restatement():
    from vae_amd import sweep
    ent, bia, scal, x, y, sizes = _small(2, "softplus")
    e = torch.unique(x[:, 1])
    mu = torch.cat([bia[e, :1], ent[e, :4]], 1)
    sg = torch.nn.functional.softplus(torch.cat([bia[e, 1:], ent[e, 4:]], 1))
    m_old = torch.full((5,), 0.1, dtype=torch.float64)
    for learn_mean in (True, False):
        for lo, hi in ((1e-4, 1e4), (2.0, 3.0)):
            m, lam, n = sweep.prior_block64(mu, sg, m_old, learn_mean, lo, hi)
            rm, rl, raw = P.prior_block_fp64(ent, bia, x, 1, "softplus", m_old, learn_mean, lo, hi)
            assert torch.allclose(m, rm, rtol=0, atol=1e-15) and torch.allclose(lam, rl, rtol=1e-15, atol=0)
            assert int(n) == int(((raw < lo) | (raw > hi)).sum())


# ---------------------------------------------------------------------------------------------------------------------
# the sweep
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("learn_mean", [True, False])
@pytest.mark.parametrize("kl_weight", [1.0, 0.7])
@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("F", [2, 3])
def test_J_never_increases_over_three_sweeps(F, link, kl_weight, learn_mean):
    ent, bia, scal, x, y, sizes = _small(F, link, seed=10 + F)
    mean, prec = P.standard(F, 4)
    if not learn_mean:
        mean = P.draw_priors(F, 4, 2)[0]
    J = [float(P.objective_J_prior(ent, bia, scal, x, y, sizes, link, kl_weight, mean, prec))]
    whats = []

    def after(what, e, b, s, mn, pr):
        Ja = float(P.objective_J_prior(e, b, s, x, y, sizes, link, kl_weight, mn, pr))
        assert Ja <= J[-1] + 1e-12 * abs(J[-1]), (what, Ja, J[-1])
        J.append(Ja)
        whats.append(what)

    for _ in range(3):
        ent, bia, scal, mean2, prec = P.sweep_fp64_prior(ent, bia, scal, x, y, sizes, link, kl_weight, mean, prec,
                                                         learn_mean=learn_mean, after=after)
        assert learn_mean or torch.equal(mean2, mean)
        mean = mean2
    assert whats[:2 * F + 1] == [w for f in range(F) for w in (f, ("prior", f))] + ["scalars"]
    assert J[-1] < J[0] and not torch.equal(prec, torch.ones_like(prec))


@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("F", [2, 3])
def test_standard_prior_is_the_parent_and_a_scaled_prior_rescales(F, link):
    for d in (3, 12):
        ent, bia, scal, x, y, field = _problem(F, d, 40 + F + d)
        one, zero = torch.ones(d + 1, dtype=torch.float64), torch.zeros(d + 1, dtype=torch.float64)
        ref = solve_fp64(ent, bia, scal, x, y, field, link, 0.7)
        got = P.solve_fp64_prior(ent, bia, scal, x, y, field, link, 0.7, zero, one)
        for k in ("mu", "s", "mu_w", "s_w"):
            assert float((got[k] - ref[k]).abs().max()) <= 1e-12, k
        # m = 0, lam = 2 at kl_weight 0.5: kl lam = 1, so the means of kl_weight 1 and half its variances
        ref = solve_fp64(ent, bia, scal, x, y, field, link, 1.0)
        got = P.solve_fp64_prior(ent, bia, scal, x, y, field, link, 0.5, zero, 2.0 * one)
        assert float((got["mu"] - ref["mu"]).abs().max()) <= 1e-12
        assert float((got["mu_w"] - ref["mu_w"]).abs().max()) <= 1e-12
        for ks in ("s", "s_w"):
            v_got, v_ref = P.link_t(got[ks], link) ** 2, P.link_t(ref[ks], link) ** 2
            assert float((v_got / v_ref - 0.5).abs().max()) <= 1e-12, ks


def test_an_entity_without_rows_gets_the_prior_row():
    ent, bia, scal, x, y, field = _problem(2, 3, 7)
    mean, prec = P.draw_priors(2, 3, 1)
    absent = 7 * field + 6                                     # (_problem folds ids 7 .. 10 of field 1)
    assert not bool((x[:, field] == absent).any())
    for link in LINKS:
        sol = P.solve_fp64_prior(ent, bia, scal, x, y, field, link, 0.7, mean[field], prec[field],
                                 entities=torch.tensor([absent]))
        th = torch.cat([sol["mu_w"], sol["mu"][0]])
        sg = P.link_t(torch.cat([sol["s_w"], sol["s"][0]]), link)
        assert float((th - mean[field]).abs().max()) <= 1e-15
        assert float((sg - prec[field] ** -0.5).abs().max()) <= 1e-14


# ---------------------------------------------------------------------------------------------------------------------
# the library and the package without a GPU
# ---------------------------------------------------------------------------------------------------------------------
def test_header_exports_and_workspace_formulas():
    from vae_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "vfm_prior.h")).read()
    for name in _lib.PRIOR_EXPORTS:
        getattr(lib, name)
        assert re.search(r"\b%s\(" % name, hdr), name
    assert "typedef struct" not in hdr                         # (no struct of its own, none of another header changed)
    for args in [(10, 7, 128, -1), (10, 7, 128, 4), (10_000, 7, 128, 4), (3, 5, 512, -1), (0, 0, 1, 0)]:
        assert lib.vfm_foldin_solve_prior_workspace_bytes(*args) == lib.vfm_foldin_solve_workspace_bytes(*args) >= 0
    for args in [(5, 2, 7, 8, -1), (40, 3, 9, 134, -1), (40, 3, 9, 135, -1), (1, 1, 1, 512, 0)]:
        assert lib.vfm_foldin_split_prior_workspace_bytes(*args) == lib.vfm_foldin_split_workspace_bytes(*args) > 0
    E_INVALID = _lib._gen.VFM_E_INVALID
    for bad in [(-1, 1, 8, -1), (1, -1, 8, -1), (1, 1, 0, -1), (1, 1, 513, -1), (1, 1, 8, -2)]:
        assert lib.vfm_foldin_solve_prior_workspace_bytes(*bad) == E_INVALID
    for bad in [(-1, 1, 1, 8, -1), (1, -1, 1, 8, -1), (1, 1, -1, 8, -1), (1, 1, 1, 0, -1), (1, 1, 1, 513, -1),
                (1, 1, 1, 8, -2), (1 << 41, 1, 1, 8, -1)]:
        assert lib.vfm_foldin_split_prior_workspace_bytes(*bad) == E_INVALID
    ops = open(os.path.join(ROOT, "vae_amd", "csrc_rank", "vfm_foldin_ops.cpp")).read()
    assert "foldin_solve_prior(" in ops and "foldin_solve_split_prior(" in ops


@pytest.mark.parametrize("with_prior", [True, False])
def test_argument_codes_before_any_hip_call(with_prior):
    """Everything the two prior entry points reject is rejected before any HIP call, with or without a prior."""
    from vae_amd import _lib
    lib = _lib.load()
    E_INVALID = _lib._gen.VFM_E_INVALID
    buf = (C.c_float * 18)(*([0.0] * 9 + [1.0] * 9))
    prior = C.cast(buf, C.c_void_p) if with_prior else None

    def solve(**kw):
        p = _lib.FoldinSolve()
        base = dict(E=1, R=1, T=10, n_ops=1, F=2, d=8, col=0, objective=_lib.OBJ_CLOSED_FORM, likelihood=_lib.LIK_NORMAL,
                    flags=0, lds_dim=-1, kl_weight=1.0)
        base.update(kw)
        for k, v in base.items():
            setattr(p, k, v)
        return lib.vfm_foldin_solve_prior_f32(C.byref(p), prior, None)

    def split(**kw):
        p = _lib.FoldinSplit()
        base = dict(E=1, R=1, T=10, n_ops=1, n_chunks=1, F=2, d=8, col=0, flags=0, lds_dim=-1, kl_weight=1.0)
        base.update(kw)
        for k, v in base.items():
            setattr(p, k, v)
        return lib.vfm_foldin_solve_split_prior_f32(C.byref(p), prior, None)

    assert lib.vfm_foldin_solve_prior_f32(None, prior, None) == E_INVALID
    assert lib.vfm_foldin_solve_split_prior_f32(None, prior, None) == E_INVALID
    assert solve(objective=_lib.OBJ_SAMPLED) == E_INVALID and b"closed-form" in lib.vfm_last_error()
    assert solve(likelihood=_lib.LIK_BERNOULLI) == E_INVALID and b"Normal" in lib.vfm_last_error()
    assert split(n_chunks=-1) == E_INVALID and b"n_chunks" in lib.vfm_last_error()
    for call in (solve, split):
        assert call(kl_weight=0.0) == E_INVALID and b"kl_weight" in lib.vfm_last_error()
        assert call(kl_weight=-1.0) == E_INVALID
        assert call(kl_weight=float("nan")) == E_INVALID
        assert call(T=0) == E_INVALID
        assert call(d=0) == E_INVALID
        assert call(d=513) == E_INVALID and b"d out of range" in lib.vfm_last_error()
        assert call(F=0) == E_INVALID
        assert call(F=65) == E_INVALID
        assert call(col=2) == E_INVALID
        assert call(col=-1) == E_INVALID
        assert call(E=-1) == E_INVALID
        assert call(R=-1) == E_INVALID
        assert call(n_ops=-1) == E_INVALID
        assert call(n_ops=0) == E_INVALID                       # (R > 0 needs an operand)
        assert call(flags=2) == E_INVALID and b"flags" in lib.vfm_last_error()
        assert call(lds_dim=-2) == E_INVALID
        assert call() == E_INVALID and b"null pointer" in lib.vfm_last_error()
        assert call(E=0) == 0                                   # nothing to do, nothing launched


def test_group_priors_round_trip_and_validation():
    from vae_amd import sweep
    pr = sweep.GroupPriors(3, 4)
    assert pr.mean.shape == (3, 5) and pr.prec.shape == (3, 5) and pr.mean.dtype == pr.prec.dtype == torch.float32
    assert bool((pr.mean == 0).all()) and bool((pr.prec == 1).all())
    assert pr.validate() is pr
    g = torch.Generator().manual_seed(1)
    pr.mean.copy_(torch.randn(3, 5, generator=g))
    pr.prec.copy_(torch.rand(3, 5, generator=g) + 0.5)
    state = pr.state_dict()
    assert state["mean"] is not pr.mean
    other = sweep.GroupPriors(3, 4)
    other.load_state_dict(state)
    assert torch.equal(other.mean, pr.mean) and torch.equal(other.prec, pr.prec)
    row = pr.row(2)
    assert row.shape == (2, 5) and row.is_contiguous() and torch.equal(row[0], pr.mean[2]) and torch.equal(row[1], pr.prec[2])
    with pytest.raises(ValueError, match="field"):
        pr.row(3)
    with pytest.raises(ValueError, match="field"):
        pr.row(True)
    with pytest.raises(ValueError, match=r"\[3, 5\]"):
        other.load_state_dict({"mean": torch.zeros(3, 4), "prec": torch.ones(3, 5)})
    with pytest.raises(ValueError, match="mean.*prec"):
        other.load_state_dict({"mean": torch.zeros(3, 5)})
    with pytest.raises(ValueError, match="prec must be > 0"):
        other.load_state_dict({"mean": torch.zeros(3, 5), "prec": torch.zeros(3, 5)})
    assert torch.equal(other.prec, pr.prec)                    # (a rejected state leaves it as it was)
    with pytest.raises(ValueError, match="integers >= 1"):
        sweep.GroupPriors(0, 4)
    for bad, what in ((0.0, "prec must be > 0"), (-1.0, "prec must be > 0"), (float("inf"), "finite"),
                      (float("nan"), "finite")):
        q = sweep.GroupPriors(2, 4)
        q.prec[1, 3] = bad
        with pytest.raises(ValueError, match=what):
            q.validate()
    q = sweep.GroupPriors(2, 4)
    q.mean[0, 0] = float("nan")
    with pytest.raises(ValueError, match="finite"):
        q.validate()


def test_value_errors_raise_before_a_gpu_is_needed():
    from vae_amd import sweep
    m = _cpu_model()                                           # field_sizes [6, 4], d = 4
    X = torch.tensor([[0, 6], [1, 7], [0, 9]])
    y = torch.tensor([1.0, 2.0, 3.0])
    good = sweep.GroupPriors(2, 4)
    bad_prec = sweep.GroupPriors(2, 4)
    bad_prec.prec[0, 1] = 0.0
    calls = [lambda p: m.fold_in_exact(X, y, priors=p), lambda p: m.fold_in_exact(X, y, split_rows=0, priors=p),
             lambda p: m.fold_in_objective(X, y, priors=p), lambda p: m.exact_objective(X, y, priors=p),
             lambda p: m.fit_exact(X, y, n_sweeps=1, priors=p), lambda p: m.fit_exact(X, y, priors=p, learn_priors=True)]
    for call in calls:
        with pytest.raises(ValueError, match="prec must be > 0"):
            call(bad_prec)
        with pytest.raises(ValueError, match="F = 3"):
            call(sweep.GroupPriors(3, 4))
        with pytest.raises(ValueError, match="d = 5"):
            call(sweep.GroupPriors(2, 5))
        with pytest.raises(ValueError, match="GroupPriors"):
            call((torch.zeros(2, 5), torch.ones(2, 5)))
    for kw in (dict(prec_min=0.0), dict(prec_min=-1.0), dict(prec_min=2.0, prec_max=1.0), dict(prec_max=float("inf")),
               dict(prec_min=float("nan")), dict(prec_min=1e-60), dict(prec_max=1e60)):
        with pytest.raises(ValueError, match="prec_min"):
            m.fit_exact(X, y, priors=good, learn_priors=True, **kw)
    with pytest.raises(ValueError, match="closed-form"):
        m.fold_in_objective(X, y, objective="sampled", priors=good)
    mc = _cpu_model("class")
    with pytest.raises(ValueError, match="'reg'"):
        mc.fit_exact(X, torch.tensor([1.0, 0.0, 1.0]), priors=good, learn_priors=True)
    with pytest.raises(ValueError, match="closed-form|'reg'"):
        mc.fold_in_objective(X, torch.tensor([1.0, 0.0, 1.0]), priors=good)
    # the checks of the parent come first and stay as they are
    with pytest.raises(ValueError, match="kl_weight"):
        m.fit_exact(X, y, kl_weight=0, priors=good, learn_priors=True)
    with pytest.raises(ValueError, match="field"):
        m.fold_in_exact(X, y, field=2, priors=good)


def test_cpu_model_fails_loudly_with_priors():
    from vae_amd import sweep
    from vae_amd._lib import VfmLibraryError
    m = _cpu_model()
    X, y = torch.tensor([[0, 6], [1, 7]]), torch.tensor([1.0, 2.0])
    pr = sweep.GroupPriors(2, 4)
    with pytest.raises(VfmLibraryError, match="MI355X"):
        m.fold_in_exact(X, y, priors=pr)
    with pytest.raises(VfmLibraryError, match="MI355X"):
        m.fit_exact(X, y, priors=pr, learn_priors=True)

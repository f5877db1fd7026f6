"""CPU: hierarchical bound sweeps (VFM.fit_bound(learn_priors=True), include/vfm_bound_prior.h) -- the fp64 restatement
of tests/bound_prior_reference.py: at the standard prior it is bound_reference.bound_rounds_fp64 to the bit; every round
is the exact minimiser of the quadratic bound at fixed xi (autograd, and a perturbed iterate is no better); no round, no
prior block and no bias block raises the fp64 J; the split association adds up to the round; the condition of every
matrix the GPU cases factor; and everything the feature rejects before a GPU is needed: header, exports, workspace
formulas, argument codes, ValueErrors.

Computed here (8 rounds, both starts, priors bound_prior_reference.case_priors): the largest cond of a factored matrix is
printed per d by the two condition tests; the cap asserted is the 1e3 of the bound fold-in's tests."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bound_prior_reference as BP  # noqa: E402
import bound_reference as BR  # noqa: E402
import bound_sweep_restatement as BS  # noqa: E402
import prior_reference as PR  # noqa: E402
import solve_reference as R  # noqa: E402
from test_fit_bound_cpu import _problem  # noqa: E402
from test_foldin_cpu import _cpu_model  # noqa: E402

LINKS = ["abs", "softplus"]


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reset", [False, True])
@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("F", [2, 3])
def test_standard_prior_is_bound_rounds_fp64_exactly(F, link, reset):
    c = BR.shape_case(9, link, F)
    m, lam = np.zeros(10), np.ones(10)
    for k in range(len(c["counts"])):                          # (n = 1, 8, 9: dual; 10: primal)
        a = BR.case_rounds(c, k, 4, reset)
        b = BP.case_rounds_prior(c, k, 4, reset, m, lam)
        assert a["n"] == b["n"] and a["B_start"] == b["B_start"]
        for key in ("theta", "sig2", "s", "xi", "w", "cond", "B"):
            assert np.array_equal(a[key], b[key]), (k, key)


@pytest.mark.parametrize("form", ["primal", "dual"])
@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("F", [2, 3])
def test_every_round_is_the_exact_minimiser_of_the_quadratic_bound(F, link, form):
    c = BR.bound_case((6,) + (30,) * (F - 1), 0, 5, link, [3, 5, 6, 14], seed=40 + F, kl_weight=0.7)
    mean, prec = PR.draw_priors(F, 5, 3 + F)
    m, lam = mean[0], prec[0]
    kl = R.f32(0.7)
    g = torch.Generator().manual_seed(5)
    for k in range(len(c["counts"])):
        e = int(c["ids"][k])
        for reset in (False, True):
            r = BP.bound_rounds_fp64_prior(c["ent"], c["bia"], c["scal"], c["X"], c["y"], 0, link, 0.7, e, 3, m, lam, reset,
                                           form=form)
            other = BP.bound_rounds_fp64_prior(c["ent"], c["bia"], c["scal"], c["X"], c["y"], 0, link, 0.7, e, 3, m, lam,
                                               reset, form="dual" if form == "primal" else "primal")
            assert np.abs(other["theta"] - r["theta"]).max() <= 1e-9
            o = BR.entity_operands(c["ent"], c["bia"], c["scal"], c["X"], c["y"], 0, link, e)
            if reset:                                          # the start is the prior itself
                th0, s20 = BR.table_start(c["ent"], c["bia"], link, e)
                at_table = BP.bound_rounds_fp64_prior(c["ent"], c["bia"], c["scal"], c["X"], c["y"], 0, link, 0.7, e, 1,
                                                      m, lam, False)
                assert not np.array_equal(at_table["xi"][0], r["xi"][0])
                by_hand = BP.bound_rounds_fp64_prior(c["ent"], c["bia"], c["scal"], c["X"], c["y"], 0, link, 0.7, e, 1,
                                                     m, lam, start=(m.numpy(), 1.0 / lam.numpy()), form=form)
                assert np.array_equal(by_hand["theta"][0], r["theta"][0])
            B_prev = r["B_start"]
            for it in range(3):
                xi = torch.from_numpy(r["xi"][it])
                th = torch.from_numpy(r["theta"][it]).clone().requires_grad_(True)
                sg = torch.from_numpy(np.sqrt(r["sig2"][it])).clone().requires_grad_(True)
                B = BP.bound_objective_t_prior(o, kl, th, sg, m, lam, xi)
                B.backward()
                assert float(th.grad.abs().max()) <= 1e-10 and float(sg.grad.abs().max()) <= 1e-10, (k, it)
                for _ in range(3):                             # a perturbed iterate is no better
                    dth = 1e-3 * torch.randn(6, generator=g, dtype=torch.float64)
                    dsg = 1e-3 * torch.randn(6, generator=g, dtype=torch.float64)
                    Bp = BP.bound_objective_t_prior(o, kl, th.detach() + dth, sg.detach() + dsg, m, lam, xi)
                    assert float(Bp) >= float(B.detach()) - 1e-13 * abs(float(B.detach()))
                # the collapsed bound never rises from round to round
                assert r["B"][it] <= B_prev + 1e-12 * abs(B_prev), (k, it)
                B_prev = r["B"][it]


def test_an_entity_without_rows_gets_the_prior():
    c = BR.bound_case((6, 30), 0, 5, "softplus", [3, 5], seed=41)
    mean, prec = PR.draw_priors(2, 5, 4)
    unseen = int(max(set(range(6)) - set(c["ids"].tolist())))
    r = BP.bound_rounds_fp64_prior(c["ent"], c["bia"], c["scal"], c["X"], c["y"], 0, "softplus", 1.0, unseen, 2, mean[0],
                                   prec[0], False)
    assert r["n"] == 0
    assert np.abs(r["theta"][-1] - mean[0].numpy()).max() <= 1e-15
    assert np.abs(r["sig2"][-1] - 1.0 / prec[0].numpy()).max() <= 1e-15
    assert abs(r["B"][-1]) <= 1e-14


@pytest.mark.parametrize("learn_mean", [True, False])
@pytest.mark.parametrize("n_iters", [1, 3])
@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("F", [2, 3])
def test_no_round_no_prior_block_and_no_bias_block_raises_J(F, link, n_iters, learn_mean):
    ent, bia, scal, x, y = _problem(F, 3, 40 + F)
    sizes = [5] * F
    mean, prec = PR.draw_priors(F, 3, 8 + F)
    seen = []

    def after(sweep, what, before, unrounded):
        Jb = float(BP.objective_J_prior(*before[:3], x, y, sizes, link, 0.7, *before[3:]))
        Ja = float(BP.objective_J_prior(*unrounded[:3], x, y, sizes, link, 0.7, *unrounded[3:]))
        assert Ja <= Jb + 1e-12 * abs(Jb), (sweep, what, Ja, Jb)           # (the margin covers fp64 only)
        seen.append((sweep, what, Jb, Ja))
        if isinstance(what, tuple):
            f = what[1]
            assert learn_mean or torch.equal(unrounded[3][f], before[3][f])
            other = [g for g in range(F) if g != f]
            assert torch.equal(unrounded[3][other], before[3][other]) and torch.equal(unrounded[4][other], before[4][other])

    out = BP.fit_bound_fp64_prior(ent, bia, scal, x, y, sizes, link, 0.7, mean, prec, 3, n_iters, learn_mean=learn_mean,
                                  after=after)
    whats = [w for f in range(F) for w in (f, ("prior", f))] + ["bias"]
    assert [(s, w) for s, w, _, _ in seen] == [(s, w) for s in range(3) for w in whats]
    assert seen[-1][3] < seen[0][2]
    assert not torch.equal(out[4], BS.round32(prec))
    # at the standard prior, not learnt, the loop is fit_bound_fp64's
    z, o = PR.standard(F, 3)
    a = BP.fit_bound_fp64_prior(ent, bia, scal, x, y, sizes, link, 0.7, z, o, 2, n_iters, learn_priors=False)
    b = BS.fit_bound_fp64(ent, bia, scal, x, y, link, 0.7, 2, n_iters)
    for u, v in zip(a[:3], b):
        assert torch.equal(u, v)
    J0 = float(BS.objective_J(*b, x, y, link, 0.7))
    assert abs(float(BP.objective_J_prior(*b, x, y, sizes, link, 0.7, z, o)) - J0) <= 1e-12 * abs(J0)


@pytest.mark.parametrize("link", LINKS)
def test_chunk_shares_add_up_to_the_round_under_a_prior(link):
    c = BR.bound_case((6, 30, 30), 0, 5, link, [23, 9], seed=93, kl_weight=0.7)
    mean, prec = PR.draw_priors(3, 5, 6)
    m, lam = mean[0].numpy(), prec[0].numpy()
    args = (c["ent"], c["bia"], c["scal"], c["X"], c["y"], 0, link, c["kl_weight"])
    kl = R.f32(c["kl_weight"])
    for k, n in enumerate(c["counts"]):
        e = int(c["ids"][k])
        r = BP.bound_rounds_fp64_prior(*args, e, 3, m, lam, True, form="primal")
        theta, sig2 = m, 1.0 / lam
        for it in range(3):
            for chunk in (1, 7, n):
                H, b, SB = BP.chunked_round_fp64_prior(*args, e, theta, sig2, chunk, m, lam)
                got = np.linalg.solve(H, b)
                assert np.abs(got - r["theta"][it]).max() <= 1e-10 * np.abs(r["theta"][it]).max(), (n, it, chunk)
                assert np.abs(kl / (kl * lam + SB) - r["sig2"][it]).max() <= 1e-12, (n, it, chunk)
            theta, sig2 = r["theta"][it], r["sig2"][it]


# ---------------------------------------------------------------------------------------------------------------------
# the GPU cases' condition (tests/test_gpu_fit_bound_priors.py asserts the same cap before it compares)
# ---------------------------------------------------------------------------------------------------------------------
def _worst_cond(case_of, ds, Fs=(2, 3)):
    worst = {}
    for d in ds:
        for F in Fs:
            mean, prec = BP.case_priors(F, d)
            for link in LINKS:
                c = case_of(d, link, F)
                for k in range(len(c["counts"])):
                    for reset in (False, True):
                        cond = float(BP.case_rounds_prior(c, k, 8, reset, mean[0], prec[0])["cond"].max())
                        worst[d] = max(worst.get(d, 0.0), cond)
    return worst


def test_unsplit_cases_are_well_conditioned_under_their_priors():
    worst = _worst_cond(BR.shape_case, BR.GPU_DS)
    print("largest cond of a factored matrix, unsplit cases, per d:", {d: round(v, 1) for d, v in worst.items()})
    assert max(worst.values()) <= 1e3, worst


def test_split_cases_are_well_conditioned_under_their_priors():
    worst = _worst_cond(BS.split_case, BS.SPLIT_DS)
    print("largest cond of a factored matrix, split cases, per d:", {d: round(v, 1) for d, v in worst.items()})
    assert max(worst.values()) <= 1e3, worst


def test_placement_mixed_and_fit_cases_are_well_conditioned_under_their_priors():
    for d in (R.LDS - 1, R.LDS):
        mean, prec = BP.case_priors(2, d)
        for link in LINKS:
            c = BS.placement_case(d, link)
            for k in range(2):
                assert float(BP.case_rounds_prior(c, k, 8, True, mean[0], prec[0])["cond"].max()) <= 1e3
        c = BR.bound_case((6, 300), 0, d, "abs", [d + 1], seed=211 + d)
        assert float(BP.case_rounds_prior(c, 0, 8, True, mean[0], prec[0])["cond"].max()) <= 1e3
    c = BS.mixed_case()
    mean, prec = BP.case_priors(3, 8)
    for k in (0, 1, 2, 17, 200):
        assert float(BP.case_rounds_prior(c, k, 8, False, mean[0], prec[0])["cond"].max()) <= 1e3
    for F in (2, 3):
        sizes, X, y = BS.fit_case(F)
        ent, bia, scal = R.tables(sizes, 8, seed=600 + F)
        mean, prec = PR.standard(F, 8)
        for f in range(F):
            _, _, rounds = BP.field_block_fp64_prior(BS.round32(ent), BS.round32(bia), scal.double(), X, y, f, "abs",
                                                     R.f32(0.7), 2, mean[f], prec[f])
            assert max(float(r["cond"].max()) for r in rounds.values()) <= 1e3


# ---------------------------------------------------------------------------------------------------------------------
# the library and the package without a GPU
# ---------------------------------------------------------------------------------------------------------------------
def test_header_exports_and_workspace_formulas():
    from vae_amd import _lib, build
    lib = _lib.load()
    path = os.path.join(ROOT, "include", "vfm_bound_prior.h")
    assert path in build.PUBLIC_HDRS
    hdr = open(path).read()
    for name in _lib.BOUND_PRIOR_EXPORTS:
        getattr(lib, name)
        assert re.search(r"\b%s\(" % name, hdr), name
    assert "typedef struct" not in hdr and "#define VFM_BOUND_PRIOR_H" in hdr and hdr.count("#define") == 1
    for args in [(10, 50, 7, 128, -1), (10, 50, 7, 128, 4), (10_000, 9, 7, 128, 4), (3, 0, 5, 512, -1), (0, 0, 0, 1, 0)]:
        assert lib.vfm_foldin_bound_prior_workspace_bytes(*args) == lib.vfm_foldin_bound_workspace_bytes(*args) >= 0
    for args in [(5, 2, 40, 7, 8, -1), (40, 3, 900, 9, 134, -1), (40, 3, 900, 9, 135, -1), (1, 1, 1, 1, 512, 0)]:
        assert (lib.vfm_foldin_bound_split_prior_workspace_bytes(*args) ==
                lib.vfm_foldin_bound_split_workspace_bytes(*args) > 0)
    E_INVALID = _lib._gen.VFM_E_INVALID
    for bad in [(-1, 1, 1, 8, -1), (1, -1, 1, 8, -1), (1, 1, -1, 8, -1), (1, 1, 1, 0, -1), (1, 1, 1, 513, -1),
                (1, 1, 1, 8, -2)]:
        assert lib.vfm_foldin_bound_prior_workspace_bytes(*bad) == E_INVALID
    for bad in [(-1, 1, 1, 1, 8, -1), (1, -1, 1, 1, 8, -1), (1, 1, -1, 1, 8, -1), (1, 1, 1, -1, 8, -1), (1, 1, 1, 1, 0, -1),
                (1, 1, 1, 1, 513, -1), (1, 1, 1, 1, 8, -2), (1 << 41, 1, 1, 1, 8, -1)]:
        assert lib.vfm_foldin_bound_split_prior_workspace_bytes(*bad) == E_INVALID
    ops = open(os.path.join(ROOT, "vae_amd", "csrc_rank", "vfm_foldin_ops.cpp")).read()
    assert "foldin_bound_prior(" in ops and "foldin_bound_split_prior(" in ops


@pytest.mark.parametrize("with_prior", [True, False])
def test_argument_codes_before_any_hip_call(with_prior):
    """Everything the two entry points reject is rejected before any HIP call, exactly where the parents reject it."""
    from vae_amd import _lib
    lib = _lib.load()
    E_INVALID = _lib._gen.VFM_E_INVALID
    buf = (C.c_float * 18)(*([0.0] * 9 + [1.0] * 9))
    prior = C.cast(buf, C.c_void_p) if with_prior else None

    def fill(p, base, kw):
        base.update(kw)
        for k, v in base.items():
            setattr(p, k, v)
        return p

    def bound(parent=False, **kw):
        p = fill(_lib.FoldinBound(), dict(E=1, R=1, T=10, n_ops=1, F=2, d=8, col=0, objective=_lib.OBJ_CLOSED_FORM,
                                          likelihood=_lib.LIK_BERNOULLI, flags=0, lds_dim=-1, kl_weight=1.0, n_iters=1,
                                          reset=0, mode=0), kw)
        return lib.vfm_foldin_bound_f32(C.byref(p), None) if parent else lib.vfm_foldin_bound_prior_f32(C.byref(p), prior, None)

    def split(parent=False, **kw):
        p = fill(_lib.FoldinBoundSplit(), dict(E=1, R=1, T=10, n_ops=1, n_chunks=1, F=2, d=8, col=0, flags=0, lds_dim=-1,
                                               kl_weight=1.0, n_iters=1, reset=0), kw)
        return (lib.vfm_foldin_bound_split_f32(C.byref(p), None) if parent else
                lib.vfm_foldin_bound_split_prior_f32(C.byref(p), prior, None))

    assert lib.vfm_foldin_bound_prior_f32(None, prior, None) == E_INVALID
    assert lib.vfm_foldin_bound_split_prior_f32(None, prior, None) == E_INVALID
    assert bound(objective=_lib.OBJ_SAMPLED) == E_INVALID and b"closed-form" in lib.vfm_last_error()
    assert bound(likelihood=_lib.LIK_NORMAL) == E_INVALID and b"Bernoulli" in lib.vfm_last_error()
    assert bound(mode=2) == E_INVALID and b"mode" in lib.vfm_last_error()
    assert bound(mode=1, n_iters=1) == E_INVALID and b"n_iters" in lib.vfm_last_error()
    assert split(n_chunks=-1) == E_INVALID and b"n_chunks" in lib.vfm_last_error()
    cases = [dict(kl_weight=0.0), dict(kl_weight=-1.0), dict(kl_weight=float("nan")), dict(T=0), dict(d=0), dict(d=513),
             dict(F=0), dict(F=65), dict(col=2), dict(col=-1), dict(E=-1), dict(R=-1), dict(n_ops=-1), dict(n_ops=0),
             dict(flags=2), dict(lds_dim=-2), dict(n_iters=0), dict(), dict(E=0)]
    for call in (bound, split):
        for kw in cases:
            got = call(**kw)
            msg = lib.vfm_last_error() if got else b""
            assert got == call(parent=True, **kw), kw
            assert got == (0 if kw == dict(E=0) else E_INVALID), kw
            assert not got or msg == lib.vfm_last_error(), kw
        assert call() == E_INVALID and b"null pointer" in lib.vfm_last_error()


def test_value_errors_raise_before_a_gpu_is_needed():
    from vae_amd import sweep
    m = _cpu_model("class")                                    # field_sizes [6, 4], d = 4
    X = torch.tensor([[0, 6], [1, 7], [0, 9]])
    y = torch.tensor([1.0, 0.0, 1.0])
    good = sweep.GroupPriors(2, 4)
    bad_prec = sweep.GroupPriors(2, 4)
    bad_prec.prec[0, 1] = 0.0
    neg_prec = sweep.GroupPriors(2, 4)
    neg_prec.prec[1, 0] = -2.0
    nan_mean = sweep.GroupPriors(2, 4)
    nan_mean.mean[1, 2] = float("nan")
    inf_prec = sweep.GroupPriors(2, 4)
    inf_prec.prec[0, 0] = float("inf")
    calls = [lambda p: m.fold_in_bound(X, y, priors=p), lambda p: m.fold_in_bound(X, y, split_rows=0, priors=p),
             lambda p: m.fold_in_bound_objective(X, y, priors=p), lambda p: m.bound_objective(X, y, priors=p),
             lambda p: m.fit_bound(X, y, n_sweeps=1, priors=p), lambda p: m.fit_bound(X, y, priors=p, learn_priors=True)]
    for call in calls:
        for p in (bad_prec, neg_prec):
            with pytest.raises(ValueError, match="prec must be > 0"):
                call(p)
        for p in (nan_mean, inf_prec):
            with pytest.raises(ValueError, match="finite"):
                call(p)
        with pytest.raises(ValueError, match="F = 3"):
            call(sweep.GroupPriors(3, 4))
        with pytest.raises(ValueError, match="d = 5"):
            call(sweep.GroupPriors(2, 5))
        with pytest.raises(ValueError, match="GroupPriors"):
            call((torch.zeros(2, 5), torch.ones(2, 5)))
    for kw in (dict(prec_min=0.0), dict(prec_min=-1.0), dict(prec_min=2.0, prec_max=1.0), dict(prec_max=float("inf")),
               dict(prec_min=float("nan")), dict(prec_min=1e-60), dict(prec_max=1e60)):
        with pytest.raises(ValueError, match="prec_min"):
            m.fit_bound(X, y, priors=good, learn_priors=True, **kw)
        with pytest.raises(ValueError, match="prec_min"):
            m.fit_bound(X, y, **kw)                             # (validated whether or not priors are learnt)
    mr = _cpu_model()
    with pytest.raises(ValueError, match="'class'"):
        mr.fit_bound(X, y, priors=good, learn_priors=True)
    with pytest.raises(ValueError, match="'class'"):
        mr.fold_in_bound(X, y, priors=good)
    with pytest.raises(ValueError, match="'class'"):
        mr.bound_objective(X, y, priors=good)
    # the checks of the parent come first and stay as they are
    with pytest.raises(ValueError, match="kl_weight"):
        m.fit_bound(X, y, kl_weight=0, priors=good, learn_priors=True)
    with pytest.raises(ValueError, match="n_iters"):
        m.fit_bound(X, y, n_iters=0, priors=good)
    with pytest.raises(ValueError, match="labels 0 and 1"):
        m.fold_in_bound(X, torch.tensor([1.0, 2.0, 0.0]), priors=good)
    with pytest.raises(ValueError, match="field"):
        m.fold_in_bound(X, y, field=2, priors=good)


def test_cpu_model_fails_loudly_with_priors():
    from vae_amd import sweep
    from vae_amd._lib import VfmLibraryError
    m = _cpu_model("class")
    X, y = torch.tensor([[0, 6], [1, 7]]), torch.tensor([1.0, 0.0])
    pr = sweep.GroupPriors(2, 4)
    with pytest.raises(VfmLibraryError, match="MI355X"):
        m.fold_in_bound(X, y, priors=pr)
    with pytest.raises(VfmLibraryError, match="MI355X"):
        m.fit_bound(X, y, priors=pr, learn_priors=True)
    with pytest.raises(VfmLibraryError, match="MI355X"):
        m.bound_objective(X, y, priors=pr)


def test_signatures_and_docs_name_the_feature():
    import inspect
    from vae_amd import foldin, sweep
    from vae_amd.model import VFM
    for fn in (VFM.fold_in_bound, VFM.fold_in_bound_objective, VFM.bound_objective, VFM.fit_bound, foldin.run_bound,
               sweep.run_bound_split):
        assert inspect.signature(fn).parameters["priors"].default is None, fn
    sig = inspect.signature(VFM.fit_bound).parameters
    assert (sig["learn_priors"].default, sig["learn_mean"].default, sig["prec_min"].default, sig["prec_max"].default) == \
        (False, True, 1e-4, 1e4)
    assert inspect.signature(sweep.SweepPlan.run_bound).parameters["prior"].default is None
    assert "'reg' model" not in sweep.GroupPriors.__doc__

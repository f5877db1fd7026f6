"""CPU: the sessions under learnt priors (include/vfm_elicit_prior.h) without a GPU -- the header, the exports, the
workspace functions and the argument codes against the parents'; the Python guards; foldin.prior_theta; the design score
under a prior in fp64 against the actual drop of the targets' variance between two solves; and the condition numbers of
every matrix a planted session of tests/elicit_priors_cases.py could factor, whatever order the GPU asks the rows in
(78.4 for the exact and design cases, 1e3 for the bound case: the caps tests/test_gpu_elicit_priors.py asserts again for
the order taken)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import design_restatement as DR  # noqa: E402
import elicit_priors_cases as EC  # noqa: E402
import prior_reference as PR  # noqa: E402
import solve_reference as R  # noqa: E402
from test_foldin_cpu import _cpu_model, link_t  # noqa: E402


# ---------------------------------------------------------------------------------------------------------------------
# the planted cases: every order of every respondent
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["exact", "design"])
def test_every_matrix_an_exact_case_can_factor_is_well_conditioned(name):
    c = EC.case(name)
    f, worst, forms = c["field"], 0.0, set()
    for e in torch.unique(c["pool"][:, f]).tolist():
        for order in EC.orders(c, e):
            for q in range(c["Q"]):
                x, y = EC.rows_of(c, e, order[:q + 1])
                ref = PR.solve_fp64_prior(c["ent"], c["bia"], c["scal"], x, y, f, c["link"], c["klw"], c["mean"][f],
                                          c["prec"][f])
                worst = max(worst, float(ref["cond"][0]))
                forms.add(x.shape[0] <= c["d"])
    print(f"{name}: worst cond {worst:.1f}")
    assert worst <= EC.COND_EXACT and forms == {True, False}          # (both the dual and the primal system occur)


def test_every_matrix_the_bound_case_can_factor_is_well_conditioned():
    c = EC.case("bound")
    f, worst = c["field"], 0.0
    for e in torch.unique(c["pool"][:, f]).tolist():
        for order in EC.orders(c, e):
            start = EC.prior_start(c)
            for q in range(c["Q"]):
                x, y = EC.rows_of(c, e, order[:q + 1])
                r = EC.bound_fold(c, x, y, e, start)
                worst = max(worst, float(r["cond"].max()))
                s32 = r["s"][-1].astype(np.float32).astype(np.float64)      # (the next fold reads the fp32 row)
                start = (r["theta"][-1].astype(np.float32).astype(np.float64), R._link64(s32, c["link"]) ** 2)
    print(f"bound: worst cond {worst:.1f}")
    assert worst <= EC.COND_BOUND


# ---------------------------------------------------------------------------------------------------------------------
# the design score under a prior
# ---------------------------------------------------------------------------------------------------------------------
def _variance_carried(sol, W, link):
    sg_w = link_t(sol["s_w"][0], link) ** 2
    sg = link_t(sol["s"][0], link) ** 2
    return float(sg_w + (torch.as_tensor(W) * sg).sum())


@pytest.mark.parametrize("name", ["exact", "design"])
def test_the_score_is_the_drop_of_the_targets_variance_between_two_solves(name):
    c = EC.case(name)
    f, link = c["field"], c["link"]
    m, lam = c["mean"][f], c["prec"][f]
    prec, kl = DR.prec_kl(c["scal"], link, c["klw"])
    for e in torch.unique(c["pool"][:, f]).tolist():
        pm = c["pool"][:, f] == e
        hx, hy = EC.rows_of(c, e, [])
        Mp, Ap = DR.operands(c["ent"], c["bia"], c["scal"], c["pool"][pm].numpy(), f, link)
        Mh, Ah = DR.operands(c["ent"], c["bia"], c["scal"], hx.numpy(), f, link)
        W = DR.walk_W(Mp, Ap)                                  # targets None: the respondent's own pool
        got = EC.design_scores_prior(DR.walk_S(Mh, Ah), W, hx.shape[0], Mp, Ap, kl, prec, lam.numpy())
        solve = lambda x, y: PR.solve_fp64_prior(c["ent"], c["bia"], c["scal"], x, y, f, link, kl, m, lam,
                                                 entities=[e])             # (kl: kl_weight as the kernels receive it)
        before = _variance_carried(solve(hx, hy), W, link)
        for i, p in enumerate(torch.nonzero(pm).reshape(-1).tolist()):
            x, y = EC.rows_of(c, e, [p])
            after = _variance_carried(solve(x, y), W, link)
            assert abs(got[i] - (before - after)) <= 1e-12 * before, (e, p, got[i], before - after)
            other = PR.solve_fp64_prior(c["ent"], c["bia"], c["scal"], x, y + 3.0, f, link, kl, m + 1.0, lam,
                                        entities=[e])             # neither the answers nor the prior's means are read
            assert abs(_variance_carried(other, W, link) - after) <= 1e-14


def test_a_doubled_precision_at_half_the_kl_weight_is_the_kl_weight_one_score():
    g = np.random.default_rng(0)
    S, W, Mq, Aq = g.random(7) * 5, g.random(7), g.standard_normal((4, 7)), g.random((4, 7))
    a = EC.design_scores_prior(S, W, 3, Mq, Aq, 0.5, 1.3, np.full(8, 2.0))
    b = EC.design_scores_prior(S, W, 3, Mq, Aq, 1.0, 1.3, np.ones(8))
    assert np.allclose(a, 0.5 * b, rtol=1e-15, atol=0)        # v = kl / (kl lam + prec S): the same denominators
    assert np.allclose(b, DR.scores(S, W, 3, Mq, Aq, 1.0, 1.3), rtol=1e-14, atol=0)       # (lam = 1: today's score)


# ---------------------------------------------------------------------------------------------------------------------
# the library and the package without a GPU
# ---------------------------------------------------------------------------------------------------------------------
def test_header_exports_and_workspace_functions():
    from vae_amd import _lib, build
    lib = _lib.load()
    path = os.path.join(ROOT, "include", "vfm_elicit_prior.h")
    assert path in build.PUBLIC_HDRS
    hdr = open(path).read()
    for name in _lib.ELICIT_PRIOR_EXPORTS:
        getattr(lib, name)
        assert re.search(r"\b%s\(" % name, hdr), name
    assert "typedef struct" not in hdr and "#define VFM_ELICIT_PRIOR_H" in hdr and hdr.count("#define") == 1
    E_INVALID = _lib._gen.VFM_E_INVALID
    for args in [(10, 50, 7, 128, -1), (10, 50, 7, 128, 4), (10_000, 9, 7, 128, 4), (3, 0, 5, 512, -1), (0, 0, 0, 1, 0),
                 (-1, 1, 1, 8, -1), (1, -1, 1, 8, -1), (1, 1, -1, 8, -1), (1, 1, 1, 0, -1), (1, 1, 1, 513, -1), (1, 1, 1, 8, -2)]:
        want = lib.vfm_elicit_solve_workspace_bytes(*args)
        assert lib.vfm_elicit_solve_prior_workspace_bytes(*args) == want
        assert lib.vfm_design_prior_workspace_bytes(*args) == lib.vfm_design_workspace_bytes(*args) == want
        assert (want == E_INVALID) == (min(args[:3]) < 0 or not 1 <= args[3] <= 512 or args[4] < -1)
    for args in [(10, 50, 20, 7, 128, 6, -1), (3, 0, 0, 5, 512, 0, 4), (1, 1, 1, 1, 8, 4097, -1), (1, 1, -1, 1, 8, 1, -1)]:
        assert lib.vfm_elicit_bound_prior_workspace_bytes(*args) == lib.vfm_elicit_bound_workspace_bytes(*args)
    for src, names in (("vfm_elicit_ops.cpp", ("elicit_solve_prior(", "elicit_bound_prior(")),
                       ("vfm_design_ops.cpp", ("design_scores_prior(", "design_elicit_prior("))):
        text = open(os.path.join(ROOT, "vae_amd", "csrc_rank", src)).read()
        assert all(n in text for n in names)


@pytest.mark.parametrize("with_prior", [True, False])
def test_argument_codes_are_the_parents(with_prior):
    """Everything the four entry points reject is rejected before any HIP call, exactly where the parents reject it, with
    the parents' message; prior == NULL goes the same way."""
    from vae_amd import _lib
    lib = _lib.load()
    E_INVALID = _lib._gen.VFM_E_INVALID
    buf = (C.c_float * 18)(*([0.0] * 9 + [1.0] * 9))
    prior = C.cast(buf, C.c_void_p) if with_prior else None
    base = dict(U=1, P=1, H=0, T=10, n_ops=1, F=2, d=8, field=0, n_rounds=1, flags=0, reset=0, write=0, lds_dim=-1,
                kl_weight=1.0)
    forms = [(_lib.ElicitSolve, dict(key_col=1, strategy=1), lib.vfm_elicit_solve_f32, lib.vfm_elicit_solve_prior_f32),
             (_lib.ElicitBound, dict(key_col=1, strategy=1, n_iters=1), lib.vfm_elicit_bound_f32,
              lib.vfm_elicit_bound_prior_f32),
             (_lib.ElicitDesign, dict(n_targets=0), lib.vfm_design_scores_f32, lib.vfm_design_scores_prior_f32),
             (_lib.ElicitDesign, dict(n_targets=0), lib.vfm_design_elicit_f32, lib.vfm_design_elicit_prior_f32)]
    cases = [dict(), dict(kl_weight=0.0), dict(kl_weight=float("nan")), dict(d=0), dict(d=513), dict(F=1), dict(F=65),
             dict(field=2), dict(field=-1), dict(U=-1), dict(P=-1), dict(H=-1), dict(n_ops=-1), dict(n_ops=0), dict(flags=2),
             dict(lds_dim=-2), dict(n_rounds=-1), dict(n_rounds=4097), dict(U=0), dict(struct_size=8), dict(abi_version=0)]
    for struct, own, parent, child in forms:
        assert child(None, prior, None) == parent(None, None) == E_INVALID
        for kw in cases:
            def make():
                p = struct()
                for k, v in {**base, **own, **kw}.items():
                    setattr(p, k, v)
                return p
            want = parent(C.byref(make()), None)
            msg = lib.vfm_last_error() if want else b""
            got = child(C.byref(make()), prior, None)
            assert got == want, (struct.__name__, kw)
            assert not got or msg == lib.vfm_last_error(), (struct.__name__, kw)
            assert got == (0 if kw == dict(U=0) else E_INVALID), (struct.__name__, kw)      # (dict(): null pointers)


def _bad_priors():
    from vae_amd import sweep
    zero, neg, nan, inf = (sweep.GroupPriors(2, 4) for _ in range(4))
    zero.prec[0, 1] = 0.0
    neg.prec[1, 0] = -2.0
    nan.mean[1, 2] = float("nan")
    inf.prec[0, 0] = float("inf")
    return [(zero, "prec must be > 0"), (neg, "prec must be > 0"), (nan, "finite"), (inf, "finite"),
            (sweep.GroupPriors(3, 4), "F = 3"), (sweep.GroupPriors(2, 5), "d = 5"),
            ((torch.zeros(2, 5), torch.ones(2, 5)), "GroupPriors")]


def test_value_errors_raise_before_a_gpu_is_needed():
    from vae_amd import sweep
    from vae_amd._lib import VfmLibraryError
    X = torch.tensor([[0, 6], [1, 7], [0, 9]])
    y = torch.tensor([1.0, 0.0, 1.0])
    mr, mc = _cpu_model(), _cpu_model("class")                 # field_sizes [6, 4], d = 4
    calls = [lambda p: mr.elicit_field_exact(X, y, 2, priors=p), lambda p: mr.elicit_field_design(X, y, 2, priors=p),
             lambda p: mr.design_scores_field(X, 0, priors=p), lambda p: mr.select_next_questions_design_field(X, 0, priors=p),
             lambda p: mc.elicit_field_bound(X, y, 2, priors=p),
             lambda p: mr.elicitation_curve_field_exact(X, y, 2, strategies=("variance", "design"), priors=p),
             lambda p: mc.elicitation_curve_field_bound(X, y, 2, strategies=("variance",), priors=p)]
    good = sweep.GroupPriors(2, 4)
    for call in calls:
        for p, match in _bad_priors():
            with pytest.raises(ValueError, match=match):
                call(p)
        with pytest.raises(VfmLibraryError, match="MI355X"):   # (a CPU model: the checks passed, the kernels are refused)
            call(good)
    # the parents' checks come first and stay as they are
    with pytest.raises(ValueError, match="'reg'"):
        mc.elicit_field_exact(X, y, 2, priors=good)
    with pytest.raises(ValueError, match="'class'"):
        mr.elicit_field_bound(X, y, 2, priors=good)
    with pytest.raises(ValueError, match="kl_weight"):
        mr.elicit_field_design(X, y, 2, kl_weight=0.0, priors=_bad_priors()[0][0])


@pytest.mark.parametrize("link", ["abs", "softplus"])
def test_prior_theta(link):
    from vae_amd import foldin, sweep
    from vae_amd.model import VFM
    m = VFM(field_sizes=[6, 4], embedding_size=4, output="reg", link=link, device="cpu")
    d = 4
    std = foldin.prior_theta(m, sweep.GroupPriors(2, d), 1)
    none = foldin.prior_theta(m, None, 1)
    assert std.dtype == torch.float32 and std.shape == (2 * d + 2,)
    assert torch.equal(std.view(torch.int32), none.view(torch.int32))
    ps = np.float32(foldin.prior_s(link))
    assert none.tolist() == [0.0] * d + [float(ps)] * d + [0.0, float(ps)]
    p = sweep.GroupPriors(2, d)
    mean, prec = PR.draw_priors(2, d, 3, 0.25)
    p.load_state_dict({"mean": mean.float(), "prec": prec.float()})
    got = foldin.prior_theta(m, p, 1).double()
    sg = PR.inv_link_t(torch.sqrt(1.0 / prec[1]), link)
    want = torch.cat([mean[1, 1:], sg[1:], mean[1, :1], sg[:1]])
    assert bool(((got - want).abs() <= R.EPS32 * want.abs()).all())
    assert torch.equal(got[:d].float(), mean[1, 1:].float()) and float(got[2 * d]) == float(mean[1, 0])


def test_signatures_and_docs_name_the_feature():
    import inspect
    from vae_amd import design, elicit
    from vae_amd.model import VFM
    for fn in (VFM.elicit_field_exact, VFM.elicit_field_bound, VFM.elicit_field_design, VFM.design_scores_field,
               VFM.select_next_questions_design_field, elicit.run_field_exact, elicit.run_field_bound,
               design.run_field_design, design.scores, design.select_next_questions):
        assert inspect.signature(fn).parameters["priors"].default is None, fn
    for fn in (VFM.elicit, VFM.elicit_field, VFM.fold_in, elicit.run, elicit.run_field):
        assert "priors" not in inspect.signature(fn).parameters, fn
    design_md = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "Sessions under learnt priors" in design_md
    assert "is folded in under N(0, 1) there" not in design_md

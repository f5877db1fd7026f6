"""CPU: hierarchical implicit sweeps (VFM.fit_implicit(priors=, learn_priors=True), include/vfm_implicit_prior.h) -- the
fp64 reference of tests/implicit_prior_reference.py against a brute-force J_imp over the dense grid under autograd: the
Gram form, every block's stationarity (entity blocks, each field's prior mean and precision over the field's whole id
range, the global bias, the precision; a clamped prior precision by sign), monotone J_imp over a reference sweep, the
identity with implicit_reference at the standard prior; then the header, the exports, the workspace formula, the argument
codes of the entry point and the ValueErrors of the Python surface, all before anything needs a GPU."""
import ctypes as C
import inspect
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import implicit_prior_reference as IPR  # noqa: E402
import implicit_reference as IR  # noqa: E402
import prior_reference as P  # noqa: E402
from test_foldin_cpu import _cpu_model  # noqa: E402

N, M = 7, 9
W0, W1 = 0.15, 1.25
CASES = [(d, link, klw) for d in (3, 5) for link in ("abs", "softplus") for klw in (1.0, 0.7)]


def _args(d, seed=3):
    return IR.planted(N, M, d, seed)


def _priors(d, seed=21):
    return P.draw_priors(2, d, seed + d)


@pytest.mark.parametrize("d, link, klw", CASES)
def test_gram_form_equals_brute_force(d, link, klw):
    ent, bia, scal, x, y = _args(d)
    mean, prec = _priors(d)
    J = float(IPR.brute_J_prior(ent, bia, scal, x, y, N, M, link, W0, W1, klw, mean, prec))
    G = float(IPR.gram_J_prior(ent, bia, scal, x, y, N, M, link, W0, W1, klw, mean, prec))
    assert abs(G - J) <= 1e-10 * abs(J), (G, J)
    assert abs(J - float(IR.brute_J(ent, bia, scal, x, y, N, M, link, W0, W1, klw))) > 1e-3 * abs(J)   # the priors matter
    # the KL form of the reference is prior_reference's
    mu, sg = ent[:N, :d], IR.link_t(ent[:N, d:], link)
    a, b = IPR.kl_prior(mu, sg, mean[0, 1:], prec[0, 1:]), P.kl_prior_t(mu, sg, mean[0, 1:], prec[0, 1:])
    assert torch.allclose(a, b, rtol=1e-12, atol=1e-14)
    # sum_e L_e of a field differs from J_imp by the other field's and the global bias' KL alone
    for f in (0, 1):
        lo, hi = (0, N) if f == 0 else (N, N + M)
        L = 0.0
        for e in range(lo, hi):
            theta = torch.cat([bia[e, :1], ent[e, :d]])
            sigma = IR.link_t(torch.cat([bia[e, 1:], ent[e, d:]]), link)
            L += float(IPR.entity_loss_fp64_prior(ent, bia, scal, x, y, f, N, M, link, W0, W1, klw, e, theta, sigma,
                                                  mean[f], prec[f]))
        o = 1 - f
        olo, ohi = (N, N + M) if f == 0 else (0, N)
        rest = (IPR.kl_prior(ent[olo:ohi, :d], IR.link_t(ent[olo:ohi, d:], link), mean[o, 1:], prec[o, 1:]).sum()
                + IPR.kl_prior(bia[olo:ohi, 0], IR.link_t(bia[olo:ohi, 1], link), mean[o, 0], prec[o, 0]).sum()
                + IR.kl_t(scal[1], IR.link_t(scal[2], link)))
        assert abs(L + klw * float(rest) - J) <= 1e-10 * abs(J), f


def _grads(ent, bia, scal, mean, prec, x, y, link, klw):
    e, b, s, m, p = (t.clone().requires_grad_(True) for t in (ent, bia, scal, mean, prec))
    J = IPR.brute_J_prior(e, b, s, x, y, N, M, link, W0, W1, klw, m, p)
    J.backward()
    return float(J.detach()), e.grad, b.grad, s.grad, m.grad, p.grad


@pytest.mark.parametrize("bounds", [(1e-4, 1e4), (1.5, 6.0)])
@pytest.mark.parametrize("d, link, klw", CASES)
def test_every_block_is_stationary_and_J_never_rises(d, link, klw, bounds):
    """Three reference sweeps: field 0, prior 0, field 1, prior 1, bias, precision.  bounds (1.5, 6.0) clamp some of the
    prior precisions: those are checked by the sign of the gradient (J falls towards the unclamped minimiser)."""
    ent, bia, scal, x, y = _args(d, seed=5)
    mean, prec = _priors(d)
    lo_b, hi_b = bounds
    J = [float(IPR.brute_J_prior(ent, bia, scal, x, y, N, M, link, W0, W1, klw, mean, prec))]
    seen = {"clamped": 0, "free": 0, "whats": []}

    def after(what, e, b, s, m, p):
        Jb, ge, gb, gs, gm, gp = _grads(e, b, s, m, p, x, y, link, klw)
        seen["whats"].append(what)
        if what in (0, 1):
            lo, hi = (0, N) if what == 0 else (N, N + M)                    # every entity of the field, seen or not
            assert float(ge[lo:hi].abs().max()) <= 1e-9 and float(gb[lo:hi].abs().max()) <= 1e-9, what
        elif what == "bias":
            assert float(gs[1:].abs().max()) <= 1e-9, gs
        elif what == "precision":
            assert abs(float(gs[0])) <= 1e-9, gs
        else:
            f = what[1]
            assert float(gm[f].abs().max()) <= 1e-9, (what, gm[f])
            _, _, free = IPR.prior_block_fp64(e, b, f, N, M, link, m[f])
            for c in range(d + 1):
                if float(free[c]) > hi_b:                                   # clamped from above: J still falls with lam
                    assert float(p[f, c]) == hi_b and float(gp[f, c]) <= 0.0, (what, c)
                    seen["clamped"] += 1
                elif float(free[c]) < lo_b:
                    assert float(p[f, c]) == lo_b and float(gp[f, c]) >= 0.0, (what, c)
                    seen["clamped"] += 1
                else:
                    assert abs(float(gp[f, c])) <= 1e-9, (what, c, gp[f])
                    seen["free"] += 1
        assert Jb <= J[-1] + 1e-9 * abs(J[-1]), (what, Jb, J[-1])
        J.append(Jb)

    for _ in range(3):
        ent, bia, scal, mean, prec = IPR.sweep_fp64_prior(ent, bia, scal, x, y, N, M, link, W0, W1, klw, mean, prec,
                                                          prec_min=lo_b, prec_max=hi_b, after=after)
    assert seen["whats"][:6] == [0, ("prior", 0), 1, ("prior", 1), "bias", "precision"]
    assert len(J) == 1 + 3 * 6 and J[-1] < J[0]
    assert seen["free"] > 0 and (seen["clamped"] > 0) == (bounds == (1.5, 6.0)), seen


@pytest.mark.parametrize("link", ["abs", "softplus"])
def test_learn_mean_false_keeps_the_means_and_stays_monotone(link):
    d, klw = 3, 0.7
    ent, bia, scal, x, y = _args(d, seed=7)
    mean, prec = _priors(d)
    J = [float(IPR.brute_J_prior(ent, bia, scal, x, y, N, M, link, W0, W1, klw, mean, prec))]

    def after(what, e, b, s, m, p):
        assert torch.equal(m, mean)
        Jb = float(IPR.brute_J_prior(e, b, s, x, y, N, M, link, W0, W1, klw, m, p))
        assert Jb <= J[-1] + 1e-9 * abs(J[-1]), what
        J.append(Jb)
        if isinstance(what, tuple):
            gp = _grads(e, b, s, m, p, x, y, link, klw)[5]
            assert float(gp[what[1]].abs().max()) <= 1e-9, what

    IPR.sweep_fp64_prior(ent, bia, scal, x, y, N, M, link, W0, W1, klw, mean, prec, learn_mean=False, after=after)
    assert len(J) == 7


@pytest.mark.parametrize("link", ["abs", "softplus"])
def test_entity_without_rows_gets_the_base_only_solve_under_the_prior(link):
    """Not the prior itself: its w0 rows exist."""
    d, klw = 3, 0.7
    ent, bia, scal, x, y = _args(d, seed=9)
    mean, prec = _priors(d)
    assert not bool((x[:, 0] == N - 1).any()) and not bool((x[:, 1] == N + M - 1).any())
    for f, e in ((0, N - 1), (1, N + M - 1)):
        sol = IPR.implicit_solve_fp64_prior(ent, bia, scal, x, y, f, N, M, link, W0, W1, klw, mean[f], prec[f], entities=[e])
        ids, u, A, cm, cv = IR._partners(ent, bia, scal, f, N, M, link)
        pr = IR.link_t(scal[0], link)
        H = torch.diag(klw * prec[f]) + pr * W0 * (u.T @ u + torch.diag(A.sum(0)))
        b = pr * W0 * (u.T @ (-cm)) + klw * prec[f] * mean[f]
        assert torch.allclose(sol["theta"][0], torch.linalg.solve(H, b), rtol=1e-12, atol=1e-14)
        sg2 = klw / (klw * prec[f] + pr * W0 * (A + u * u).sum(0))
        assert torch.allclose(sol["sigma"][0] ** 2, sg2, rtol=1e-12)
        assert not torch.allclose(sol["theta"][0], mean[f], atol=1e-3)
        assert bool((sol["sigma"][0] ** 2 < 1.0 / prec[f]).all())


@pytest.mark.parametrize("d, link, klw", CASES)
def test_standard_prior_is_implicit_reference_exactly(d, link, klw):
    ent, bia, scal, x, y = _args(d, seed=11)
    mean, prec = IPR.standard(d)
    args = (ent, bia, scal, x, y)
    for f in (0, 1):
        a = IPR.implicit_solve_fp64_prior(*args, f, N, M, link, W0, W1, klw, mean[f], prec[f])
        b = IR.implicit_solve_fp64(*args, f, N, M, link, W0, W1, klw)
        assert all(torch.equal(a[k], b[k]) for k in ("ids", "theta", "sigma", "cond"))
        e = int(a["ids"][2])
        Ha, ba, bd, SBa = IPR.system_fp64_prior(*args, f, N, M, link, W0, W1, klw, e, mean[f], prec[f])
        Hb, bb, SBb = IR.system_fp64(*args, f, N, M, link, W0, W1, klw, e)
        assert torch.equal(Ha, Hb) and torch.equal(ba, bb) and torch.equal(bd, bb) and torch.equal(SBa, SBb)
        La = IPR.entity_loss_fp64_prior(*args, f, N, M, link, W0, W1, klw, e, a["theta"][2], a["sigma"][2], mean[f], prec[f])
        Lb = IR.entity_loss_fp64(*args, f, N, M, link, W0, W1, klw, e, b["theta"][2], b["sigma"][2])
        assert float(La) == float(Lb)
    assert float(IPR.brute_J_prior(*args, N, M, link, W0, W1, klw, mean, prec)) == \
        float(IR.brute_J(*args, N, M, link, W0, W1, klw))
    assert float(IPR.gram_J_prior(*args, N, M, link, W0, W1, klw, mean, prec)) == \
        float(IR.gram_J(*args, N, M, link, W0, W1, klw))
    # a sweep that does not learn the priors is implicit_reference's sweep
    e1, b1, s1, _, _ = IPR.sweep_fp64_prior(*args, N, M, link, W0, W1, klw, mean, prec, learn_priors=False)
    e2, b2, s2 = ent, bia, scal
    for f in (0, 1):
        e2, b2 = IR.write_solution(e2, b2, IR.implicit_solve_fp64(e2, b2, s2, x, y, f, N, M, link, W0, W1, klw), link)
    s2 = IR.bias_block_fp64(e2, b2, s2, x, y, N, M, link, W0, W1, klw)
    s2 = IR.precision_block_fp64(e2, b2, s2, x, y, N, M, link, W0, W1)
    assert torch.equal(e1, e2) and torch.equal(b1, b2) and torch.equal(s1, s2)


# ---------------------------------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------------------------------
def test_header_exports_and_workspace_formula():
    from vae_amd import _lib, build
    path = os.path.join(ROOT, "include", "vfm_implicit_prior.h")
    assert os.path.exists(path) and path in build.PUBLIC_HDRS
    hdr = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    assert "typedef struct" not in hdr                                         # no struct of its own
    declared = sorted(set(re.findall(r"\b(vfm_\w+)\s*\(", hdr)))
    assert declared == sorted(_lib.IMPLICIT_PRIOR_EXPORTS) and len(declared) == 2
    lib = _lib.load()
    for name in _lib.IMPLICIT_PRIOR_EXPORTS:
        getattr(lib, name)
        assert name not in _lib.IMPLICIT_EXPORTS and name not in _lib.PRIOR_EXPORTS
    sws, pws = lib.vfm_implicit_solve_workspace_bytes, lib.vfm_implicit_solve_prior_workspace_bytes
    for a in [(0, 0, 8, -1), (3, 11, 1, -1), (3, 11, 128, -1), (3, 11, 128, 4), (10_000, 0, 128, 4), (5, 7, 134, -1),
              (5, 7, 135, -1), (5, 7, 512, -1)]:
        assert pws(*a) == sws(*a) and pws(*a) >= 0, a
    E_INVALID = _lib._gen.VFM_E_INVALID
    for bad in [(-1, 1, 8, -1), (1, -1, 8, -1), (1, 1, 0, -1), (1, 1, 513, -1), (1, 1, 8, -2), (1 << 41, 1, 8, -1),
                (1, 1 << 41, 8, -1)]:
        assert pws(*bad) == E_INVALID and sws(*bad) == E_INVALID, bad
    # the shim names the op
    ops_src = open(os.path.join(ROOT, "vae_amd", "csrc_rank", "vfm_foldin_ops.cpp")).read()
    assert 'm.def("foldin_solve_implicit_prior(' in ops_src and "vfm_foldin_solve_implicit_prior_f32(&p, prior_of(" in ops_src


def test_argument_codes_with_a_prior_without_a_gpu():
    """VFM_E_INVALID exactly where the parent returns it, with `prior` non-NULL: every check precedes any HIP call."""
    from vae_amd import _lib
    lib = _lib.load()
    E_INVALID = _lib._gen.VFM_E_INVALID
    buf = (C.c_char * (1 << 16))()
    addr = (C.addressof(buf) + 255) // 256 * 256
    sws = lib.vfm_implicit_solve_workspace_bytes

    def solve(**kw):
        p = _lib.ImplicitSolve()
        args = dict(E=1, R=1, T=10, n_chunks=0, lo=6, n=4, d=8, flags=0, lds_dim=-1, kl_weight=1.0, w0=0.1, w1=1.0)
        args.update(kw)
        for k, v in args.items():
            setattr(p, k, v)
        with_prior = lib.vfm_foldin_solve_implicit_prior_f32(C.byref(p), addr, None)
        msg = lib.vfm_last_error()
        assert lib.vfm_foldin_solve_implicit_prior_f32(C.byref(p), None, None) == with_prior      # NULL: the parent call
        assert lib.vfm_foldin_solve_implicit_f32(C.byref(p), None) == with_prior and lib.vfm_last_error() == msg
        return with_prior, msg

    def bad(what, **kw):
        rc, msg = solve(**kw)
        assert rc == E_INVALID and what in msg, (kw, rc, msg)

    assert lib.vfm_foldin_solve_implicit_prior_f32(None, addr, None) == E_INVALID and b"NULL" in lib.vfm_last_error()
    bad(b"T < 1", T=0)
    bad(b"d out of range", d=513)
    bad(b"d out of range", d=0)
    bad(b"E < 0", E=-1)
    bad(b"E < 0", R=-1)
    bad(b"n_chunks", n_chunks=-1)
    for rng in (dict(n=0), dict(lo=-1), dict(lo=7), dict(lo=11, n=1)):
        bad(b"partner range", **rng)
    bad(b"flags", flags=4)
    bad(b"lds_dim", lds_dim=-2)
    for klw in (0.0, -1.0, float("nan"), float("inf")):
        bad(b"kl_weight", kl_weight=klw)
    for w0 in (0.0, -0.5, float("nan"), float("inf")):
        bad(b"w0", w0=w0)
    for w1 in (0.05, float("nan"), float("inf")):
        bad(b"w1", w1=w1)
    bad(b"row_ptr")                                                            # (neither form)
    bad(b"row_ptr", row_ptr=addr, chunk_ptr=addr)
    bad(b"n_chunks", row_ptr=addr, n_chunks=2)
    bad(b"null pointer", row_ptr=addr)
    ptrs = {k: addr for k in ("entities", "y", "partner", "base", "entity_params", "bias_params", "scalars", "out_loss")}
    bad(b"null pointer", chunk_ptr=addr, n_chunks=1, **ptrs)                   # no chunks
    bad(b"workspace too small", chunk_ptr=addr, chunks=addr, n_chunks=1, **ptrs)
    bad(b"aligned", chunk_ptr=addr, chunks=addr, n_chunks=1, workspace=addr | 8, workspace_bytes=sws(1, 1, 8, -1), **ptrs)
    assert solve(E=0)[0] == 0                                                  # nothing to do, nothing launched


def test_python_surface_raises_before_a_gpu_is_needed():
    from vae_amd import sweep
    m = _cpu_model()                                                           # fields [6, 4], d = 4
    X = torch.tensor([[0, 6], [1, 7], [0, 9]])
    y = torch.tensor([1.0, 2.0, 3.0])
    calls = {"fold_in_implicit": lambda mm, X_, y_, **kw: mm.fold_in_implicit(X_, y_, 0, w0=0.1, **kw),
             "implicit_objective": lambda mm, X_, y_, **kw: mm.implicit_objective(X_, y_, w0=0.1, **kw),
             "fit_implicit": lambda mm, X_, y_, **kw: mm.fit_implicit(X_, y_, 2, w0=0.1, **kw)}

    def priors(F=2, d=4, **state):
        pr = sweep.GroupPriors(F, d)
        for k, v in state.items():
            getattr(pr, k)[0, 1] = v                                           # (past load_state_dict's own check)
        return pr

    for name, call in calls.items():
        with pytest.raises(ValueError, match="GroupPriors"):
            call(m, X, y, priors={"mean": 0})
        with pytest.raises(ValueError, match="F = 3"):
            call(m, X, y, priors=priors(F=3))
        with pytest.raises(ValueError, match="d = 5"):
            call(m, X, y, priors=priors(d=5))
        for v in (float("nan"), float("inf")):
            with pytest.raises(ValueError, match="finite"):
                call(m, X, y, priors=priors(prec=v))
        with pytest.raises(ValueError, match="finite"):
            call(m, X, y, priors=priors(mean=float("nan")))
        for v in (0.0, -2.0):
            with pytest.raises(ValueError, match="prec must be > 0"):
                call(m, X, y, priors=priors(prec=v))
        # the model's own checks come first, whatever the priors
        with pytest.raises(ValueError, match="'reg'"):
            call(_cpu_model("class"), X, torch.tensor([1.0, 0.0, 1.0]), priors=priors())
        with pytest.raises(ValueError, match="two-field"):
            call(_cpu_model(field_sizes=[3, 4, 5]), torch.tensor([[0, 3, 8]]), torch.tensor([1.0]), priors=priors(F=3))
    for kw in (dict(prec_min=2.0, prec_max=1.0), dict(prec_min=0.0), dict(prec_min=-1.0), dict(prec_max=float("inf")),
               dict(prec_min=float("nan")), dict(prec_min=1e-60), dict(prec_max=1e60)):
        with pytest.raises(ValueError, match="prec_min"):
            m.fit_implicit(X, y, 2, w0=0.1, learn_priors=True, **kw)
    with pytest.raises(ValueError, match="'reg'"):
        _cpu_model("class").fit_implicit(X, torch.tensor([1.0, 0.0, 1.0]), 2, w0=0.1, learn_priors=True)
    with pytest.raises(ValueError, match="two-field"):
        _cpu_model(field_sizes=[3, 4, 5]).fit_implicit(torch.tensor([[0, 3, 8]]), None, 2, w0=0.1, learn_priors=True)
    from vae_amd.model import STANDARD_PRIOR
    sig = inspect.signature(type(m).fit_implicit).parameters
    assert (sig["priors"].default, sig["learn_priors"].default, sig["learn_mean"].default, sig["prec_min"].default,
            sig["prec_max"].default) == (STANDARD_PRIOR, False, True, 1e-4, 1e4)
    assert inspect.signature(type(m).fold_in_implicit).parameters["priors"].default is STANDARD_PRIOR
    assert inspect.signature(type(m).implicit_objective).parameters["priors"].default is STANDARD_PRIOR
    assert inspect.signature(sweep.fit_implicit).parameters["priors"].default is None
    assert inspect.signature(sweep.run_implicit).parameters["priors"].default is None
    assert inspect.signature(sweep.implicit_objective).parameters["priors"].default is None
    for call in calls.values():                                               # a GroupPriors or nothing: not None
        with pytest.raises(TypeError, match="GroupPriors"):
            call(m, X, y, priors=None)
    assert inspect.signature(sweep.ImplicitPlan.run).parameters["prior"].default is None


def test_cpu_model_fails_loudly_under_priors():
    from vae_amd import sweep
    from vae_amd._lib import VfmLibraryError
    m = _cpu_model()
    X = torch.tensor([[0, 6], [1, 7]])
    pr = sweep.GroupPriors(2, 4)
    with pytest.raises(VfmLibraryError, match="MI355X"):
        m.fit_implicit(X, w0=0.1, learn_priors=True)
    with pytest.raises(VfmLibraryError, match="MI355X"):
        m.implicit_objective(X, None, w0=0.1, priors=pr)
    with pytest.raises(VfmLibraryError, match="MI355X"):
        m.fold_in_implicit(X, None, 1, w0=0.1, priors=pr)

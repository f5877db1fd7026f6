"""CPU: weighted implicit sweeps (VFM.fit_implicit(weights=), include/vfm_implicit_weights.h) -- the fp64 reference of
tests/implicit_weights_reference.py, written from a dense [N, M] weight matrix, against a brute-force J_imp over the
dense grid under autograd: every block's stationarity (entity blocks, the global bias, the precision, and under a mixed
prior each field's prior block) to 1e-9, monotone J_imp over three reference sweeps, the Gram form restated from
sweep.implicit_sums' formulas against brute force to 1e-10 (the two figures of tests/test_fit_implicit_cpu.py); then
hkv_weights, the header, the exports, the workspace formula, the argument codes of the entry point, the ValueErrors of
the Python surface and the route of weights=None, all before anything needs a GPU."""
import ctypes as C
import inspect
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import implicit_reference as IR  # noqa: E402
import implicit_weights_reference as IWR  # noqa: E402
import prior_reference as P  # noqa: E402
from test_foldin_cpu import _cpu_model  # noqa: E402

N, M = 7, 9
W0 = float(torch.tensor(0.15, dtype=torch.float32))
CASES = [(d, link, klw) for d in (3, 5) for link in ("abs", "softplus") for klw in (1.0, 0.7)]


def _args(d, seed=3):
    ent, bia, scal, x, y = IR.planted(N, M, d, seed)
    return ent, bia, scal, x, y, IWR.draw_weights(x.shape[0], W0, seed + 100).double()


def _priors(d, seed=21):
    return P.draw_priors(2, d, seed + d)


def _grads(ent, bia, scal, priors, x, y, wts, link, klw):
    e, b, s = (t.clone().requires_grad_(True) for t in (ent, bia, scal))
    pr = None if priors is None else tuple(t.clone().requires_grad_(True) for t in priors)
    J = IWR.brute_J(e, b, s, x, y, wts, N, M, link, W0, klw, pr)
    J.backward()
    return float(J.detach()), e.grad, b.grad, s.grad, (None, None) if pr is None else (pr[0].grad, pr[1].grad)


@pytest.mark.parametrize("mixed_prior", [False, True])
@pytest.mark.parametrize("d, link, klw", CASES)
def test_every_block_is_stationary_and_J_never_rises(d, link, klw, mixed_prior):
    """Three reference sweeps.  The gradient of brute-force J_imp at every block minimiser is <= 1e-9 and J_imp never
    increases.  mixed_prior: the same under a drawn prior per field, learnt after each field's solves."""
    ent, bia, scal, x, y, wts = _args(d, seed=5)
    assert float(wts.max()) > 8 * W0 and int((wts == W0).sum()) >= 3            # the range and the floor are there
    priors = _priors(d) if mixed_prior else None
    J = [float(IWR.brute_J(ent, bia, scal, x, y, wts, N, M, link, W0, klw, priors))]
    whats = []

    def after(what, e, b, s, pr):
        Jb, ge, gb, gs, (gm, gp) = _grads(e, b, s, pr, x, y, wts, link, klw)
        whats.append(what)
        if what in (0, 1):
            lo, hi = (0, N) if what == 0 else (N, N + M)                    # every entity of the field, seen or not
            assert float(ge[lo:hi].abs().max()) <= 1e-9 and float(gb[lo:hi].abs().max()) <= 1e-9, what
        elif what == "bias":
            assert float(gs[1:].abs().max()) <= 1e-9, gs
        elif what == "precision":
            assert abs(float(gs[0])) <= 1e-9, gs
        else:
            f = what[1]
            assert float(gm[f].abs().max()) <= 1e-9 and float(gp[f].abs().max()) <= 1e-9, (what, gm[f], gp[f])
        assert Jb <= J[-1] + 1e-9 * abs(J[-1]), (what, Jb, J[-1])
        J.append(Jb)

    for _ in range(3):
        ent, bia, scal, priors = IWR.sweep_fp64(ent, bia, scal, x, y, wts, N, M, link, W0, klw, priors,
                                                learn_priors=mixed_prior, after=after)
    per = 6 if mixed_prior else 4
    assert whats[:per] == ([0, ("prior", 0), 1, ("prior", 1)] if mixed_prior else [0, 1]) + ["bias", "precision"]
    assert len(J) == 1 + 3 * per and J[-1] < J[0]


def _gram_sums(ent, bia, scal, x, y, wts, link, w0):
    """(W, S1, S2) as vae_amd.sweep.implicit_sums forms them with weights, restated in fp64 on CPU tensors: the closed
    forms of the two fields' Grams and first moments at weight w0, corrected at the observed rows with each row's own
    weight."""
    d = ent.shape[1] // 2
    ent, bia, scal = ent.double(), bia.double(), scal.double()
    m0, s0 = scal[1], IR.link_t(scal[2], link)
    mu_u, mu_i = ent[:N, :d], ent[N:N + M, :d]
    su2, si2 = IR.link_t(ent[:N, d:], link) ** 2, IR.link_t(ent[N:N + M, d:], link) ** 2
    one = lambda n: torch.ones(n, 1, dtype=torch.float64)
    Pm = torch.cat([one(N), bia[:N, :1], mu_u], 1)
    Q = torch.cat([m0 + bia[N:N + M, :1], one(M), mu_i], 1)
    sum_m2 = ((Pm.T @ Pm) * (Q.T @ Q)).sum()
    sum_m = Pm.sum(0) @ Q.sum(0)
    sum_v = (N * M * s0 * s0 + M * (IR.link_t(bia[:N, 1], link) ** 2).sum() + N * (IR.link_t(bia[N:N + M, 1], link) ** 2).sum()
             + (mu_u * mu_u).sum(0) @ si2.sum(0) + su2.sum(0) @ (si2 + mu_i * mu_i).sum(0))
    w = wts.double()
    W = w0 * N * M + (w - w0).sum()
    u, i = x[:, 0], x[:, 1]
    m = m0 + bia[u, 0] + bia[i, 0] + (ent[u, :d] * ent[i, :d]).sum(1)
    su, si = IR.link_t(ent[u, d:], link) ** 2, IR.link_t(ent[i, d:], link) ** 2
    v = (s0 * s0 + IR.link_t(bia[u, 1], link) ** 2 + IR.link_t(bia[i, 1], link) ** 2
         + (ent[u, :d] ** 2 * si + su * si + su * ent[i, :d] ** 2).sum(1))
    yd = y.double()
    S1 = -w0 * (sum_m - N * M * m0) + (w * (yd - (m - m0)) + w0 * (m - m0)).sum()
    S2 = w0 * (sum_m2 + sum_v) + (w * ((yd - m) ** 2 + v) - w0 * (m * m + v)).sum()
    return W, S1, S2


@pytest.mark.parametrize("mixed_prior", [False, True])
@pytest.mark.parametrize("d, link, klw", CASES)
def test_gram_form_equals_brute_force(d, link, klw, mixed_prior):
    ent, bia, scal, x, y, wts = _args(d)
    priors = _priors(d) if mixed_prior else None
    J = float(IWR.brute_J(ent, bia, scal, x, y, wts, N, M, link, W0, klw, priors))
    W, S1, S2 = _gram_sums(ent, bia, scal, x, y, wts, link, W0)
    prec = IR.link_t(scal[0], link)
    G = float(0.5 * prec * S2 + W * (IR.LOG_2PI_HALF - 0.5 * torch.log(prec)) + klw * IWR._kl(ent, bia, scal, N, M, link, priors))
    assert abs(G - J) <= 1e-10 * abs(J), (G, J)
    for got, ref in zip((W, S1, S2), IWR.dense_sums(ent, bia, scal, x, y, wts, N, M, link, W0)):
        assert abs(float(got) - float(ref)) <= 1e-10 * abs(float(ref)), (got, ref)
    # the weights are in J: the binarised objective is another number
    assert abs(J - float(IWR.brute_J(ent, bia, scal, x, y, torch.ones_like(wts), N, M, link, W0, klw, priors))) > 1e-3 * abs(J)
    # sum_e L_e of a field differs from J_imp by the other field's and the global bias' KL alone
    for f in (0, 1):
        lo, hi = (0, N) if f == 0 else (N, N + M)
        pr = None if priors is None else (priors[0][f], priors[1][f])
        L = 0.0
        for e in range(lo, hi):
            theta = torch.cat([bia[e, :1], ent[e, :d]])
            sigma = IR.link_t(torch.cat([bia[e, 1:], ent[e, d:]]), link)
            L += float(IWR.entity_loss_fp64(ent, bia, scal, x, y, wts, f, N, M, link, W0, klw, e, theta, sigma, pr))
        own = 0.0
        for e in range(lo, hi):
            theta = torch.cat([bia[e, :1], ent[e, :d]])
            sigma = IR.link_t(torch.cat([bia[e, 1:], ent[e, d:]]), link)
            own += float((IR.kl_t(theta, sigma) if pr is None else IWR.IPR.kl_prior(theta, sigma, pr[0], pr[1])).sum())
        rest = float(IWR._kl(ent, bia, scal, N, M, link, priors)) - own
        assert abs(L + klw * rest - J) <= 1e-10 * abs(J), f


@pytest.mark.parametrize("link", ["abs", "softplus"])
def test_constant_weights_are_the_unweighted_reference(link):
    """weights = w1 everywhere is implicit_reference's (w0, w1) problem: the same optimum and the same J_imp."""
    d, klw, w1 = 3, 0.7, 1.25
    ent, bia, scal, x, y, _ = _args(d, seed=9)
    wts = torch.full((x.shape[0],), w1, dtype=torch.float64)
    for f in (0, 1):
        a = IWR.implicit_solve_fp64(ent, bia, scal, x, y, wts, f, N, M, link, W0, klw)
        b = IR.implicit_solve_fp64(ent, bia, scal, x, y, f, N, M, link, W0, w1, klw)
        assert torch.allclose(a["theta"], b["theta"], rtol=1e-12, atol=1e-14)
        assert torch.allclose(a["sigma"], b["sigma"], rtol=1e-12, atol=1e-14)
    Ja = float(IWR.brute_J(ent, bia, scal, x, y, wts, N, M, link, W0, klw))
    Jb = float(IR.brute_J(ent, bia, scal, x, y, N, M, link, W0, w1, klw))
    assert abs(Ja - Jb) <= 1e-13 * abs(Jb)


def test_hkv_weights_values_and_errors():
    from vae_amd import sweep
    counts = torch.tensor([0, 1, 3, 40])
    w0 = 0.15
    w0f = float(torch.tensor(w0, dtype=torch.float32))
    w = sweep.hkv_weights(counts, w0, 0.5)
    assert w.dtype == torch.float32 and w.shape == (4,)
    assert torch.equal(w, (w0f * (1.0 + 0.5 * counts.double())).float())
    assert float(w[0]) == w0f and bool((w >= w0f).all())                       # a count of 0 weighs exactly w0
    wl = sweep.hkv_weights(counts.float(), w0, 2.0, log_eps=0.5)
    assert wl.dtype == torch.float32
    assert torch.equal(wl, (w0f * (1.0 + 2.0 * torch.log1p(counts.double() / 0.5))).float())
    assert torch.equal(sweep.hkv_weights(counts, w0, 0.0), torch.full((4,), w0f))
    assert sweep.hkv_weights([2.5, 0.0], 1.0, 1.0).tolist() == [3.5, 1.0]
    assert sweep.hkv_weights(torch.zeros(0), w0, 1.0).shape == (0,)
    for bad in (torch.tensor([1.0, -1.0]), torch.tensor([float("nan")]), torch.tensor([float("inf")])):
        with pytest.raises(ValueError, match="counts"):
            sweep.hkv_weights(bad, w0, 1.0)
    for alpha in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="alpha"):
            sweep.hkv_weights(counts, w0, alpha)
    for eps in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="log_eps"):
            sweep.hkv_weights(counts, w0, 1.0, log_eps=eps)
    for w in (0.0, -1.0, float("inf")):
        with pytest.raises(ValueError, match="w0"):
            sweep.hkv_weights(counts, w, 1.0)
    assert "caller" in sweep.hkv_weights.__doc__ and "twice" in sweep.hkv_weights.__doc__     # duplicates: not aggregated


# ---------------------------------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------------------------------
def test_header_exports_and_workspace_formula():
    from vae_amd import _lib, build
    path = os.path.join(ROOT, "include", "vfm_implicit_weights.h")
    assert os.path.exists(path) and path in build.PUBLIC_HDRS
    text = open(path).read()
    assert "DOES NOT CHECK" in text and "below w0" in text                      # the header says who rejects a bad weight
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert "typedef struct" not in hdr                                         # no struct of its own
    declared = sorted(set(re.findall(r"\b(vfm_\w+)\s*\(", hdr)))
    assert declared == sorted(_lib.IMPLICIT_WEIGHTS_EXPORTS) and len(declared) == 2
    lib = _lib.load()
    for name in _lib.IMPLICIT_WEIGHTS_EXPORTS:
        getattr(lib, name)
        assert name not in _lib.IMPLICIT_EXPORTS and name not in _lib.IMPLICIT_PRIOR_EXPORTS
    sws, wws = lib.vfm_implicit_solve_workspace_bytes, lib.vfm_implicit_solve_weights_workspace_bytes
    for a in [(0, 0, 8, -1), (3, 11, 1, -1), (3, 11, 128, -1), (3, 11, 128, 4), (10_000, 0, 128, 4), (5, 7, 134, -1),
              (5, 7, 135, -1), (5, 7, 512, -1)]:
        assert wws(*a) == sws(*a) and wws(*a) >= 0, a
    E_INVALID = _lib._gen.VFM_E_INVALID
    for bad in [(-1, 1, 8, -1), (1, -1, 8, -1), (1, 1, 0, -1), (1, 1, 513, -1), (1, 1, 8, -2), (1 << 41, 1, 8, -1),
                (1, 1 << 41, 8, -1)]:
        assert wws(*bad) == E_INVALID and sws(*bad) == E_INVALID, bad
    ops_src = open(os.path.join(ROOT, "vae_amd", "csrc_rank", "vfm_foldin_ops.cpp")).read()
    assert 'm.def("foldin_solve_implicit_weights(' in ops_src and "vfm_foldin_solve_implicit_weights_f32(&p, " in ops_src
    # the kernel source keeps everything of the weights under `if constexpr`: no plain branch on the pointer
    hip = open(os.path.join(ROOT, "vae_amd", "csrc_rank", "vfm_implicit.hip")).read()
    kernels = hip[:hip.index('extern "C"')]
    assert "s.w)" not in kernels and "if (s.w" not in kernels and "template <int LINK, bool PRIOR, bool WROW>" in kernels


def test_argument_codes_with_weights_without_a_gpu():
    """VFM_E_INVALID exactly where the parent returns it, with `weights` non-NULL -- but for w1, which is then neither
    read nor checked; weights NULL is the prior call itself.  Every check precedes any HIP call."""
    from vae_amd import _lib
    lib = _lib.load()
    E_INVALID = _lib._gen.VFM_E_INVALID
    buf = (C.c_char * (1 << 16))()
    addr = (C.addressof(buf) + 255) // 256 * 256
    sws = lib.vfm_implicit_solve_workspace_bytes
    call = lib.vfm_foldin_solve_implicit_weights_f32

    def solve(**kw):
        p = _lib.ImplicitSolve()
        args = dict(E=1, R=1, T=10, n_chunks=0, lo=6, n=4, d=8, flags=0, lds_dim=-1, kl_weight=1.0, w0=0.1, w1=1.0)
        args.update(kw)
        for k, v in args.items():
            setattr(p, k, v)
        out = []
        for prior in (None, addr):
            rc = call(C.byref(p), prior, addr, None)
            msg = lib.vfm_last_error()
            assert call(C.byref(p), prior, None, None) == lib.vfm_foldin_solve_implicit_prior_f32(C.byref(p), prior, None)
            out.append((rc, msg))
        assert out[0] == out[1]
        # with a valid w1 the parent call returns the same code at the same check
        if args["w1"] >= args["w0"] and args["w1"] < float("inf"):
            assert lib.vfm_foldin_solve_implicit_f32(C.byref(p), None) == out[0][0] and lib.vfm_last_error() == out[0][1]
        return out[0]

    def bad(what, **kw):
        rc, msg = solve(**kw)
        assert rc == E_INVALID and what in msg, (kw, rc, msg)

    assert call(None, None, addr, None) == E_INVALID and b"NULL" in lib.vfm_last_error()
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
    bad(b"row_ptr")                                                            # (neither form)
    bad(b"row_ptr", row_ptr=addr, chunk_ptr=addr)
    bad(b"n_chunks", row_ptr=addr, n_chunks=2)
    bad(b"null pointer", row_ptr=addr)
    ptrs = {k: addr for k in ("entities", "y", "partner", "base", "entity_params", "bias_params", "scalars", "out_loss")}
    bad(b"null pointer", chunk_ptr=addr, n_chunks=1, **ptrs)                   # no chunks
    bad(b"workspace too small", chunk_ptr=addr, chunks=addr, n_chunks=1, **ptrs)
    bad(b"aligned", chunk_ptr=addr, chunks=addr, n_chunks=1, workspace=addr | 8, workspace_bytes=sws(1, 1, 8, -1), **ptrs)
    assert solve(E=0)[0] == 0                                                  # nothing to do, nothing launched
    # w1 is not looked at: a value the parent refuses passes (E = 0: nothing is launched), and where another check
    # fails it is that check's message, not w1's
    for w1 in (0.05, -1.0, float("nan"), float("inf")):
        p = _lib.ImplicitSolve()
        for k, v in dict(E=0, R=1, T=10, n_chunks=0, lo=6, n=4, d=8, flags=0, lds_dim=-1, kl_weight=1.0, w0=0.1, w1=w1).items():
            setattr(p, k, v)
        assert call(C.byref(p), None, addr, None) == 0
        assert call(C.byref(p), None, None, None) == E_INVALID and b"w1" in lib.vfm_last_error()
        p.E = 1
        assert call(C.byref(p), None, addr, None) == E_INVALID and b"row_ptr" in lib.vfm_last_error()


def test_python_surface_raises_before_a_gpu_is_needed():
    from vae_amd import sweep
    m = _cpu_model()                                                           # fields [6, 4], d = 4
    X = torch.tensor([[0, 6], [1, 7], [0, 9]])
    y = torch.tensor([1.0, 2.0, 3.0])
    ok = torch.tensor([0.1, 0.5, 2.0])
    calls = {"fold_in_implicit": lambda mm, X_, y_, **kw: mm.fold_in_implicit(X_, y_, 0, w0=0.1, **kw),
             "implicit_objective": lambda mm, X_, y_, **kw: mm.implicit_objective(X_, y_, w0=0.1, **kw),
             "fit_implicit": lambda mm, X_, y_, **kw: mm.fit_implicit(X_, y_, 2, w0=0.1, **kw),
             "sweep.run_implicit": lambda mm, X_, y_, **kw: sweep.run_implicit(mm, X_, y_, 0, 0.1, **kw),
             "sweep.implicit_objective": lambda mm, X_, y_, **kw: sweep.implicit_objective(mm, X_, y_, 0.1, **kw),
             "sweep.fit_implicit": lambda mm, X_, y_, **kw: sweep.fit_implicit(mm, X_, y_, 2, 0.1, **kw)}
    for name, call in calls.items():
        for w in (torch.tensor([0.1, 0.5]), torch.tensor([0.1, 0.5, 2.0, 1.0]), torch.ones(3, 1), torch.tensor(1.0),
                  torch.tensor([1, 2, 3]), torch.tensor([True, True, True])):
            with pytest.raises(ValueError, match="1-D floating"):
                call(m, X, y, weights=w)
        for v in (float("nan"), float("inf"), -float("inf")):
            with pytest.raises(ValueError, match="finite"):
                call(m, X, y, weights=torch.tensor([0.5, v, 1.0]))
        with pytest.raises(ValueError, match="finite"):
            call(m, X, y, weights=torch.tensor([0.5, 1e39, 1.0], dtype=torch.float64))       # not finite in fp32
        for v in (0.0999, 0.0, -1.0):
            with pytest.raises(ValueError, match=">= w0"):
                call(m, X, y, weights=torch.tensor([0.5, v, 1.0]))
        with pytest.raises(ValueError, match=">= w0"):                         # the fp32 value below fp32(0.1)
            call(m, X, y, weights=torch.tensor([0.5, 0.09999999, 1.0], dtype=torch.float64))
        with pytest.raises(ValueError, match="two sources"):
            call(m, X, y, weights=ok, w1=1.25)
        # the model's own checks come first, whatever the weights
        with pytest.raises(ValueError, match="'reg'"):
            call(_cpu_model("class"), X, torch.tensor([1.0, 0.0, 1.0]), weights=ok)
        with pytest.raises(ValueError, match="two-field"):
            call(_cpu_model(field_sizes=[3, 4, 5]), torch.tensor([[0, 3, 8]]), torch.tensor([1.0]), weights=ok[:1])
        with pytest.raises(ValueError, match="duplicate"):
            call(m, torch.tensor([[0, 6], [1, 7], [0, 6]]), y, weights=ok)     # repeated pairs are not added up
    # valid weights pass every check and stop where the GPU is needed; a w0 above 1 needs no w1 beside weights
    from vae_amd._lib import VfmLibraryError
    for name, call in calls.items():
        with pytest.raises(VfmLibraryError, match="MI355X"):
            call(m, X, y, weights=ok)
        with pytest.raises(VfmLibraryError, match="MI355X"):                   # 0.1 in fp64 is below fp32(0.1) and rounds to it
            call(m, X, y, weights=torch.tensor([0.1, 0.5, 2.0], dtype=torch.float64))
    x, yy, w0, w1 = sweep.check_implicit_args(m, X, y, 2.0, 1.0, 1.0, weights=torch.tensor([2.0, 3.0, 2.5]))
    assert (w0, w1) == (2.0, 1.0) and x.shape == (3, 2)
    with pytest.raises(ValueError, match="w1 must be >= w0"):
        sweep.check_implicit_args(m, X, y, 2.0, 1.0, 1.0)
    # the explicit priors=None of the methods stays a TypeError
    for name in ("fold_in_implicit", "implicit_objective", "fit_implicit"):
        with pytest.raises(TypeError, match="GroupPriors"):
            calls[name](m, X, y, priors=None, weights=ok)


def test_weights_is_the_last_keyword_and_defaults_to_none():
    from vae_amd import sweep
    from vae_amd.model import VFM
    fns = [sweep.check_implicit_args, sweep.ImplicitPlan.__init__, sweep.ImplicitPlan.run, sweep.run_implicit,
           sweep.implicit_sums, sweep.implicit_objective_terms, sweep.update_scalars_implicit, sweep.implicit_objective,
           sweep.fit_implicit, VFM.fold_in_implicit, VFM.implicit_objective, VFM.fit_implicit]
    for fn in fns:
        params = list(inspect.signature(fn).parameters.values())
        assert params[-1].name == "weights" and params[-1].default is None, fn


class _Recorder:
    """Stands in for the torch.ops shim: sizes are 1, launches are recorded."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def op(*a):
            self.calls.append((name, a))
            return 1
        return op


def test_weights_none_takes_the_parents_route(monkeypatch):
    """A plan without weights calls foldin_solve_implicit (or its _prior form) with the parent's arguments; a plan with
    weights calls foldin_solve_implicit_weights with the weights in the plan's row order and no w1."""
    from vae_amd import _lib, sweep
    m = _cpu_model()                                                           # fields [6, 4], d = 4
    X = torch.tensor([[3, 6], [1, 7], [3, 9], [0, 8], [1, 6]])
    y = torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0])
    wts = torch.tensor([0.5, 0.6, 0.7, 0.8, 0.9])
    rec = _Recorder()
    monkeypatch.setattr(_lib, "ops", lambda: rec)
    monkeypatch.setattr(type(m), "_fresh_params", lambda self: None, raising=False)
    monkeypatch.setattr(type(m), "params_changed", lambda self: None, raising=False)
    x, yy, w0, w1 = sweep.check_implicit_args(m, X, y, 0.1, 1.25, 1.0)
    plan = sweep.ImplicitPlan(m, x, yy, 0)
    assert plan.ws is None
    plan.run(m, 1.0, w0, w1)
    names = [c[0] for c in rec.calls if c[0].startswith("foldin_solve")]
    assert names and set(names) == {"foldin_solve_implicit"}
    assert all(c[1][-1] == w1 and c[1][-2] == w0 for c in rec.calls if c[0] == "foldin_solve_implicit")
    rec.calls.clear()
    prior = torch.zeros(2, 5)
    plan.run(m, 1.0, w0, w1, prior)
    assert {c[0] for c in rec.calls if c[0].startswith("foldin_solve")} == {"foldin_solve_implicit_prior"}
    with pytest.raises(ValueError, match="belong to the plan"):
        plan.run(m, 1.0, w0, w1, None, wts)
    rec.calls.clear()
    x, yy, w0, w1 = sweep.check_implicit_args(m, X, y, 0.1, 1.0, 1.0, weights=wts)
    plan = sweep.ImplicitPlan(m, x, yy, 0, weights=sweep._row_weights(m, wts))
    # the plan's rows are sorted by entity (stably): the weights follow the targets
    assert plan.ys.tolist() == [4.0, 2.0, 5.0, 1.0, 3.0]
    assert torch.allclose(plan.ws, torch.tensor([0.8, 0.6, 0.9, 0.5, 0.7]))
    for prior in (None, torch.zeros(2, 5)):
        rec.calls.clear()
        plan.run(m, 1.0, w0, w1, prior, wts)
        solves = [c for c in rec.calls if c[0].startswith("foldin_solve")]
        assert solves and {c[0] for c in solves} == {"foldin_solve_implicit_weights"}
        for _, a in solves:
            assert a[12] is prior and a[13] is plan.ws and a[-1] == w0 and len(a) == 20
    with pytest.raises(ValueError, match="belong to the plan"):
        plan.run(m, 1.0, w0, w1)
    # entities=: the weights pass the filter with their rows
    plan = sweep.ImplicitPlan(m, x, yy, 0, torch.tensor([1, 2]), weights=sweep._row_weights(m, wts))
    assert plan.ys.tolist() == [2.0, 5.0] and torch.allclose(plan.ws, torch.tensor([0.6, 0.9]))
    assert plan.empty.tolist() == [2]

"""CPU: the implicit-feedback sweeps (VFM.fit_implicit, include/vfm_implicit.h) -- the fp64 reference of
tests/implicit_reference.py against a brute-force J_imp over the dense grid under autograd: the Gram form, every
block's stationarity, monotone J_imp, the base-only solve, the identity with solve_fp64 at w0 = w1; then the header, the
exports, the struct mirrors, the workspace formulas, the argument codes of the entry points and the ValueErrors of the
Python surface, all before anything needs a GPU."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import implicit_reference as IR  # noqa: E402
from test_foldin_cpu import _cpu_model  # noqa: E402
from test_foldin_exact_cpu import solve_fp64  # noqa: E402

N, M = 7, 9
W0, W1 = 0.15, 1.25
CASES = [(d, link, klw) for d in (3, 5) for link in ("abs", "softplus") for klw in (1.0, 0.7)]


def _args(d, seed=3):
    ent, bia, scal, x, y = IR.planted(N, M, d, seed)
    return ent, bia, scal, x, y


@pytest.mark.parametrize("d, link, klw", CASES)
def test_gram_form_equals_brute_force(d, link, klw):
    ent, bia, scal, x, y = _args(d)
    J = float(IR.brute_J(ent, bia, scal, x, y, N, M, link, W0, W1, klw))
    G = float(IR.gram_J(ent, bia, scal, x, y, N, M, link, W0, W1, klw))
    assert abs(G - J) <= 1e-10 * abs(J), (G, J)
    # sum_e L_e of a field differs from J_imp by the other field's and the global bias' KL alone
    for f in (0, 1):
        lo, hi = (0, N) if f == 0 else (N, N + M)
        L = 0.0
        for e in range(lo, hi):
            theta = torch.cat([bia[e, :1], ent[e, :d]])
            sigma = IR.link_t(torch.cat([bia[e, 1:], ent[e, d:]]), link)
            L += float(IR.entity_loss_fp64(ent, bia, scal, x, y, f, N, M, link, W0, W1, klw, e, theta, sigma))
        olo, ohi = (N, N + M) if f == 0 else (0, N)
        rest = (IR.kl_t(ent[olo:ohi, :d], IR.link_t(ent[olo:ohi, d:], link)).sum()
                + IR.kl_t(bia[olo:ohi, 0], IR.link_t(bia[olo:ohi, 1], link)).sum()
                + IR.kl_t(scal[1], IR.link_t(scal[2], link)))
        assert abs(L + klw * float(rest) - J) <= 1e-10 * abs(J), f


@pytest.mark.parametrize("d, link, klw", CASES)
def test_every_block_is_stationary_and_J_never_rises(d, link, klw):
    ent, bia, scal, x, y = _args(d, seed=5)
    J = [float(IR.brute_J(ent, bia, scal, x, y, N, M, link, W0, W1, klw))]

    def grads(e, b, s):
        e, b, s = (t.clone().requires_grad_(True) for t in (e, b, s))
        Jb = IR.brute_J(e, b, s, x, y, N, M, link, W0, W1, klw)
        Jb.backward()
        return float(Jb.detach()), e.grad, b.grad, s.grad

    def step(Jb, what):
        assert Jb <= J[-1] + 1e-12 * abs(J[-1]), (what, Jb, J[-1])
        J.append(Jb)

    for _ in range(3):
        for f in (0, 1):
            sol = IR.implicit_solve_fp64(ent, bia, scal, x, y, f, N, M, link, W0, W1, klw)
            ent, bia = IR.write_solution(ent, bia, sol, link)
            Jb, ge, gb, _ = grads(ent, bia, scal)
            ids = sol["ids"]                                              # every entity of the field, seen or not
            assert ids.numel() == (N if f == 0 else M)
            assert float(ge[ids].abs().max()) <= 1e-9 and float(gb[ids].abs().max()) <= 1e-9, f
            step(Jb, f)
        scal = IR.bias_block_fp64(ent, bia, scal, x, y, N, M, link, W0, W1, klw)
        Jb, _, _, gs = grads(ent, bia, scal)
        assert float(gs[1:].abs().max()) <= 1e-9, gs
        step(Jb, "bias")
        scal = IR.precision_block_fp64(ent, bia, scal, x, y, N, M, link, W0, W1)
        Jb, _, _, gs = grads(ent, bia, scal)
        assert abs(float(gs[0])) <= 1e-9, gs
        step(Jb, "precision")
    assert len(J) == 1 + 3 * 4 and J[-1] < J[0]


@pytest.mark.parametrize("link", ["abs", "softplus"])
def test_entity_without_rows_gets_the_base_only_solve(link):
    d, klw = 3, 0.7
    ent, bia, scal, x, y = _args(d, seed=9)
    assert not bool((x[:, 0] == N - 1).any()) and not bool((x[:, 1] == N + M - 1).any())
    for f, e in ((0, N - 1), (1, N + M - 1)):
        sol = IR.implicit_solve_fp64(ent, bia, scal, x, y, f, N, M, link, W0, W1, klw, entities=[e])
        ids, u, A, cm, cv = IR._partners(ent, bia, scal, f, N, M, link)
        prec = IR.link_t(scal[0], link)
        H = klw * torch.eye(d + 1, dtype=torch.float64) + prec * W0 * (u.T @ u + torch.diag(A.sum(0)))
        b = prec * W0 * (u.T @ (-cm))
        assert torch.allclose(sol["theta"][0], torch.linalg.solve(H, b), rtol=1e-12, atol=1e-14)
        sg2 = klw / (klw + prec * W0 * (A + u * u).sum(0))
        assert torch.allclose(sol["sigma"][0] ** 2, sg2, rtol=1e-12)
        assert float(sg2[0]) == pytest.approx(klw / (klw + float(prec) * W0 * ids.numel()), rel=1e-12)


@pytest.mark.parametrize("link", ["abs", "softplus"])
@pytest.mark.parametrize("field", [0, 1])
def test_equal_weights_are_solve_fp64_on_the_dense_rows(field, link):
    """J / w is the exact objective of the dense row set (targets y or 0) at kl_weight / w."""
    d, klw, w = 3, 0.7, 0.4
    ent, bia, scal, x, y = _args(d, seed=11)
    Wgt, Y = IR.dense_targets(x, y, N, M, w, w)
    uu, ii = torch.meshgrid(torch.arange(N), torch.arange(N, N + M), indexing="ij")
    xd = torch.stack([uu.reshape(-1), ii.reshape(-1)], 1)
    yd = Y.reshape(-1)
    ref = solve_fp64(ent, bia, scal, xd, yd, field, link, klw / w)
    sol = IR.implicit_solve_fp64(ent, bia, scal, x, y, field, N, M, link, w, w, klw)
    assert torch.equal(ref["entities"], sol["ids"])
    assert torch.allclose(sol["theta"][:, 0], ref["mu_w"].double(), rtol=1e-10, atol=1e-12)
    assert torch.allclose(sol["theta"][:, 1:], ref["mu"].double(), rtol=1e-10, atol=1e-12)
    assert torch.allclose(sol["sigma"][:, 0], IR.link_t(ref["s_w"], link), rtol=1e-10)
    assert torch.allclose(sol["sigma"][:, 1:], IR.link_t(ref["s"], link), rtol=1e-10)


# ---------------------------------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------------------------------
def _header():
    return open(os.path.join(ROOT, "include", "vfm_implicit.h")).read()


def test_header_names_exports_and_struct_mirrors_match_gcc(tmp_path):
    from vae_amd import _lib, build
    assert os.path.join(ROOT, "include", "vfm_implicit.h") in build.PUBLIC_HDRS
    assert any(src == "csrc_rank/vfm_implicit.hip" and flags == build._EXACT for src, _, flags in build._UNITS)
    lib = _lib.load()
    declared = sorted(set(re.findall(r"\b(vfm_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S))))
    assert declared == sorted(_lib.IMPLICIT_EXPORTS) and len(declared) == 5
    for name in _lib.IMPLICIT_EXPORTS:
        getattr(lib, name)
        assert name not in _lib.EXPORTS and name not in _lib.SWEEP_EXPORTS
    for ctype, mirror in (("vfm_implicit_base_t", _lib.ImplicitBase), ("vfm_implicit_solve_t", _lib.ImplicitSolve)):
        fields = [n for n, _ in mirror._fields_]
        src = ('#include <stdio.h>\n#include <stddef.h>\n#include "vfm_implicit.h"\nint main(void) {\n'
               f'  printf("%zu\\n", sizeof({ctype}));\n' +
               "".join(f'  printf("%zu\\n", offsetof({ctype}, {f}));\n' for f in fields) + "  return 0;\n}\n")
        c, exe = str(tmp_path / f"{ctype}.c"), str(tmp_path / ctype)
        open(c, "w").write(src)
        subprocess.run(["gcc", "-I" + os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
        assert out[0] == C.sizeof(mirror)
        assert out[1:] == [getattr(mirror, f).offset for f in fields]
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (ctype, ctype), _header(), re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = re.findall(r"(\w+)\s*(?:,|;)", body)
        assert names == fields, ctype


def test_workspace_formulas_and_argument_codes_without_a_gpu():
    """Everything the two entry points reject is rejected before any HIP call, so these run without a device."""
    from vae_amd import _lib
    lib = _lib.load()
    E_INVALID = _lib._gen.VFM_E_INVALID
    tri = lambda m: m * (m + 1) // 2
    ru = lambda v: (v + 255) // 256 * 256
    doubles = lambda d: tri(d + 1) + 3 * (d + 1) + 1
    bd, bws, sws = lib.vfm_implicit_base_doubles, lib.vfm_implicit_base_workspace_bytes, lib.vfm_implicit_solve_workspace_bytes
    for d in (1, 5, 128, 512):
        assert bd(d) == doubles(d)
        assert bws(1, 16, d) == ru(doubles(d) * 8) and bws(16, 16, d) == ru(doubles(d) * 8)
        assert bws(17, 16, d) == ru(2 * doubles(d) * 8) and bws(26744, 2048, d) == ru(14 * doubles(d) * 8)
        assert sws(0, 0, d, -1) == 0 and sws(3, 11, d, -1) == ru(11 * doubles(d) * 8) + (3 * ru(tri(d + 1) * 8) if d + 1 > 135 else 0)
    assert sws(3, 11, 128, 4) == ru(11 * doubles(128) * 8) + 3 * ru(tri(129) * 8)
    assert sws(10_000, 0, 128, 4) == _lib.FOLDIN_SOLVE_SLABS * ru(tri(129) * 8)
    assert bd(0) == E_INVALID and bd(513) == E_INVALID
    for bad in [(0, 16, 8), (5, 0, 8), (5, 16, 0), (5, 16, 513), (1 << 41, 16, 8)]:
        assert bws(*bad) == E_INVALID, bad
    for bad in [(-1, 1, 8, -1), (1, -1, 8, -1), (1, 1, 0, -1), (1, 1, 513, -1), (1, 1, 8, -2), (1 << 41, 1, 8, -1),
                (1, 1 << 41, 8, -1)]:
        assert sws(*bad) == E_INVALID, bad

    buf = (C.c_char * (1 << 16))()
    addr = (C.addressof(buf) + 255) // 256 * 256

    def base(**kw):
        p = _lib.ImplicitBase()
        args = dict(T=10, lo=6, n=4, chunk_rows=16, d=8, flags=0)
        args.update(kw)
        for k, v in args.items():
            setattr(p, k, v)
        return lib.vfm_implicit_base_f32(C.byref(p), None)

    assert lib.vfm_implicit_base_f32(None, None) == E_INVALID and b"NULL" in lib.vfm_last_error()
    assert base(T=0) == E_INVALID and b"T < 1" in lib.vfm_last_error()
    assert base(d=0) == E_INVALID and base(d=513) == E_INVALID and b"d out of range" in lib.vfm_last_error()
    for rng in (dict(n=0), dict(lo=-1), dict(lo=7), dict(lo=11, n=1), dict(n=1 << 62)):
        assert base(**rng) == E_INVALID and b"id range" in lib.vfm_last_error(), rng
    assert base(chunk_rows=0) == E_INVALID and b"chunk_rows" in lib.vfm_last_error()
    assert base(flags=4) == E_INVALID and b"flags" in lib.vfm_last_error()
    assert base() == E_INVALID and b"null pointer" in lib.vfm_last_error()
    ptrs = {k: addr for k in ("entity_params", "bias_params", "scalars", "out_base")}
    assert base(**ptrs) == E_INVALID and b"workspace too small" in lib.vfm_last_error()
    assert base(workspace=addr | 8, workspace_bytes=bws(4, 16, 8), **ptrs) == E_INVALID and b"aligned" in lib.vfm_last_error()

    def solve(**kw):
        p = _lib.ImplicitSolve()
        args = dict(E=1, R=1, T=10, n_chunks=0, lo=6, n=4, d=8, flags=0, lds_dim=-1, kl_weight=1.0, w0=0.1, w1=1.0)
        args.update(kw)
        for k, v in args.items():
            setattr(p, k, v)
        return lib.vfm_foldin_solve_implicit_f32(C.byref(p), None)

    assert lib.vfm_foldin_solve_implicit_f32(None, None) == E_INVALID and b"NULL" in lib.vfm_last_error()
    assert solve(T=0) == E_INVALID and b"T < 1" in lib.vfm_last_error()
    assert solve(d=513) == E_INVALID and solve(d=0) == E_INVALID and b"d out of range" in lib.vfm_last_error()
    assert solve(E=-1) == E_INVALID and solve(R=-1) == E_INVALID
    assert solve(n_chunks=-1) == E_INVALID and b"n_chunks" in lib.vfm_last_error()
    for rng in (dict(n=0), dict(lo=-1), dict(lo=7), dict(lo=11, n=1)):
        assert solve(**rng) == E_INVALID and b"partner range" in lib.vfm_last_error(), rng
    assert solve(flags=4) == E_INVALID and b"flags" in lib.vfm_last_error()
    assert solve(lds_dim=-2) == E_INVALID and b"lds_dim" in lib.vfm_last_error()
    for klw in (0.0, -1.0, float("nan"), float("inf")):
        assert solve(kl_weight=klw) == E_INVALID and b"kl_weight" in lib.vfm_last_error()
    for w0 in (0.0, -0.5, float("nan"), float("inf")):
        assert solve(w0=w0) == E_INVALID and b"w0" in lib.vfm_last_error()
    for w1 in (0.05, float("nan"), float("inf")):
        assert solve(w1=w1) == E_INVALID and b"w1" in lib.vfm_last_error()
    assert solve() == E_INVALID and b"row_ptr" in lib.vfm_last_error()           # (neither form)
    assert solve(row_ptr=addr, chunk_ptr=addr) == E_INVALID and b"row_ptr" in lib.vfm_last_error()
    assert solve(row_ptr=addr, n_chunks=2) == E_INVALID and b"n_chunks" in lib.vfm_last_error()
    assert solve(row_ptr=addr) == E_INVALID and b"null pointer" in lib.vfm_last_error()
    ptrs = {k: addr for k in ("entities", "y", "partner", "base", "entity_params", "bias_params", "scalars", "out_loss")}
    assert solve(chunk_ptr=addr, n_chunks=1, **ptrs) == E_INVALID and b"null pointer" in lib.vfm_last_error()   # no chunks
    assert solve(chunk_ptr=addr, chunks=addr, n_chunks=1, **ptrs) == E_INVALID and b"workspace too small" in lib.vfm_last_error()
    need = sws(1, 1, 8, -1)
    assert solve(chunk_ptr=addr, chunks=addr, n_chunks=1, workspace=addr | 8, workspace_bytes=need, **ptrs) == E_INVALID
    assert b"aligned" in lib.vfm_last_error()
    assert solve(E=0) == 0                                                       # nothing to do, nothing launched


def test_argument_checks_raise_before_a_gpu_is_needed():
    m = _cpu_model()                                                           # fields [6, 4], d = 4
    X = torch.tensor([[0, 6], [1, 7], [0, 9]])
    y = torch.tensor([1.0, 2.0, 3.0])
    calls = {"fold_in_implicit": lambda mm, X_, y_, **kw: mm.fold_in_implicit(X_, y_, 0, **kw),
             "implicit_objective": lambda mm, X_, y_, **kw: mm.implicit_objective(X_, y_, **kw),
             "fit_implicit": lambda mm, X_, y_, **kw: mm.fit_implicit(X_, y_, 2, **kw)}
    for name, call in calls.items():
        with pytest.raises(TypeError):
            call(m, X, y)                                                      # w0 has no default
        with pytest.raises(ValueError, match="'reg'"):
            call(_cpu_model("class"), X, torch.tensor([1.0, 0.0, 1.0]), w0=0.1)
        with pytest.raises(ValueError, match="two-field"):
            call(_cpu_model(field_sizes=[3, 4, 5]), torch.tensor([[0, 3, 8]]), torch.tensor([1.0]), w0=0.1)
        for klw in (0, -1.0, float("nan")):
            with pytest.raises(ValueError, match="kl_weight"):
                call(m, X, y, w0=0.1, kl_weight=klw)
        for w0 in (float("nan"), float("inf")):
            with pytest.raises(ValueError, match="finite"):
                call(m, X, y, w0=w0)
        with pytest.raises(ValueError, match="finite"):
            call(m, X, y, w0=0.1, w1=float("inf"))
        for w0 in (0.0, -0.1):
            with pytest.raises(ValueError, match="w0 must be > 0"):
                call(m, X, y, w0=w0)
        with pytest.raises(ValueError, match="w1 must be >= w0"):
            call(m, X, y, w0=0.5, w1=0.4)
        with pytest.raises(ValueError, match="duplicate"):
            call(m, torch.tensor([[0, 6], [1, 7], [0, 6]]), y, w0=0.1)
        with pytest.raises(ValueError, match="range"):
            call(m, torch.tensor([[6, 7]]), torch.tensor([1.0]), w0=0.1)     # a field-1 id in column 0
        with pytest.raises(ValueError, match="range|lie in"):
            call(m, torch.tensor([[0, 10]]), torch.tensor([1.0]), w0=0.1)    # an id past T in column 1
        with pytest.raises(ValueError, match="range|frozen"):
            call(m, torch.tensor([[0, 3]]), torch.tensor([1.0]), w0=0.1)     # a field-0 id in column 1
        with pytest.raises(TypeError):
            call(m, X, y, w0=0.1, priors=None)                                 # priors= is not an argument
    for ents in ([6], [-1], [0, 0], [0.5]):
        with pytest.raises(ValueError, match="entities"):
            m.fold_in_implicit(X, y, 0, w0=0.1, entities=ents)
    with pytest.raises(ValueError, match="field"):
        m.fold_in_implicit(X, y, 2, w0=0.1)
    with pytest.raises(ValueError, match="n_sweeps"):
        m.fit_implicit(X, y, -1, w0=0.1)
    with pytest.raises(ValueError, match="chunk_rows"):
        m.fit_implicit(X, y, w0=0.1, chunk_rows=0)
    with pytest.raises(ValueError, match="split_rows"):
        m.fold_in_implicit(X, y, 0, w0=0.1, split_rows="big")
    with pytest.raises(ValueError, match="tol"):
        m.fit_implicit(X, y, w0=0.1, tol=-1.0)


def test_cpu_model_fails_loudly():
    from vae_amd._lib import VfmLibraryError
    m = _cpu_model()
    X = torch.tensor([[0, 6], [1, 7]])
    with pytest.raises(VfmLibraryError, match="MI355X"):
        m.fit_implicit(X, w0=0.1)                                              # y None: all ones
    with pytest.raises(VfmLibraryError, match="MI355X"):
        m.implicit_objective(X, None, w0=0.1)
    with pytest.raises(VfmLibraryError, match="MI355X"):
        m.fold_in_implicit(X, None, 1, w0=0.1)

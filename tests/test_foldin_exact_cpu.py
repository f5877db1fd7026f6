"""CPU: exact fold-in (include/vfm_foldin.h: vfm_foldin_solve_f32) -- solve_fp64, an fp64 torch restatement of the
closed-form optimum of the per-entity objective (the GPU tests compare the kernel with it): the gradient of
test_foldin_cpu.objective_fp64 vanishes at its result, its dual (n x n, Woodbury) and primal ((d + 1) x (d + 1)) forms
agree, the library exports the header's symbols with the struct laid out as gcc lays it out, and VFM.fold_in_exact
raises for what it cannot do before anything needs a GPU."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from test_foldin_cpu import _cpu_model, _tables, link_t, objective_fp64  # noqa: E402


def solve_fp64(ent, bia, scal, x, y, field, link="abs", kl_weight=1.0, form="primal"):
    """The exact minimiser of objective_fp64(..., objective="closed_form") over the folded entities' factors, in fp64.

    ent [T, 2d], bia [T, 2], scal [3]: the frozen tables; x [R, F] int64, y [R].  form "primal": H theta = b with
    H = prec (sum_r u_r u_r^T + diag(0, sum_r A_r)) + kl I;  "dual": the same theta through the n x n system of the
    Woodbury identity.  Returns dict(entities [E] ascending, mu [E, d], s [E, d], mu_w [E], s_w [E], cond [E] = cond(H)).
    """
    ent, bia, scal = ent.double(), bia.double(), scal.double()
    y = y.double()
    d = ent.shape[1] // 2
    F = x.shape[1]
    ents = torch.unique(x[:, field])
    prec = link_t(scal[0], link)
    m0, sg0 = scal[1], link_t(scal[2], link)
    kl = float(kl_weight)
    Q = [f for f in range(F) if f != field]
    mq = torch.stack([ent[x[:, q], :d] for q in Q]) if Q else torch.zeros(1, x.shape[0], d, dtype=torch.float64)
    sq2 = (torch.stack([link_t(ent[x[:, q], d:], link) for q in Q]) ** 2 if Q
           else torch.zeros(1, x.shape[0], d, dtype=torch.float64))
    M, A = mq.sum(0), sq2.sum(0)
    Cc = 2.0 * (sq2 * (M[None] - mq)).sum(0)
    pm = 0.5 * (M ** 2 - (mq ** 2).sum(0)).sum(1)
    cm = m0 + sum(bia[x[:, q], 0] for q in Q) + pm
    out = dict(entities=ents, mu=[], s=[], mu_w=[], s_w=[], cond=[])
    for e in ents.tolist():
        r = x[:, field] == e
        n = int(r.sum())
        U = torch.cat([torch.ones(n, 1, dtype=torch.float64), M[r]], 1)           # u_r = (1, M_r)
        t = y[r] - cm[r]
        D = kl + prec * torch.cat([torch.zeros(1, dtype=torch.float64), A[r].sum(0)])
        b = prec * (U.T @ t - torch.cat([torch.zeros(1, dtype=torch.float64), 0.5 * Cc[r].sum(0)]))
        H = torch.diag(D) + prec * (U.T @ U)
        if form == "primal":
            theta = torch.linalg.solve(H, b)
        else:
            v = b / D
            K = torch.eye(n, dtype=torch.float64) / prec + (U / D) @ U.T
            theta = v - (U.T @ torch.linalg.solve(K, U @ v)) / D
        sg_w = (kl / (kl + prec * n)) ** 0.5
        sg = torch.sqrt(kl / (kl + prec * (A[r] + M[r] ** 2).sum(0)))
        inv = (lambda s: s) if link == "abs" else (lambda s: torch.log(torch.expm1(s)))
        out["mu_w"].append(theta[0])
        out["mu"].append(theta[1:])
        out["s_w"].append(inv(torch.as_tensor(sg_w, dtype=torch.float64)))
        out["s"].append(inv(sg))
        out["cond"].append(torch.linalg.cond(H))
    for k in ("mu", "s", "mu_w", "s_w", "cond"):
        out[k] = torch.stack(out[k]) if out[k] else torch.zeros(0, dtype=torch.float64)
    return out


def _problem(F, d, seed, n_ent=4, R=30):
    sizes = [7] * F
    T = sum(sizes)
    ent, bia, scal = _tables(T, d, seed)
    g = torch.Generator().manual_seed(seed + 1)
    field = 1
    x = torch.stack([torch.randint(7 * f, 7 * f + 7, (R,), generator=g) for f in range(F)], 1)
    x[:, field] = 7 * field + torch.randint(0, n_ent, (R,), generator=g)
    x[-1] = x[0]                                                           # a duplicated row counts twice
    y = torch.randn(R, generator=g, dtype=torch.float64) + 1.0
    y[-1] = y[0]
    return ent, bia, scal, x, y, field


@pytest.mark.parametrize("kl_weight", [1.0, 0.7])
@pytest.mark.parametrize("link", ["abs", "softplus"])
@pytest.mark.parametrize("F", [2, 3])
def test_gradient_vanishes_and_the_two_forms_agree(F, link, kl_weight):
    # d = 3: R = 30 rows over 4 entities put more than d rows on some (the primal side of the rule); d = 12: fewer
    for d in (3, 12):
        ent, bia, scal, x, y, field = _problem(F, d, 20 + F + d)
        sol = solve_fp64(ent, bia, scal, x, y, field, link, kl_weight)
        theta = [sol[k].clone().requires_grad_(True) for k in ("mu", "s", "mu_w", "s_w")]
        L = objective_fp64(ent, bia, scal, x, y, field, (sol["entities"], *theta), link, "reg", "closed_form",
                           kl_weight=kl_weight)
        L.sum().backward()
        for t in theta:
            assert float(t.grad.abs().max()) <= 1e-10
        dual = solve_fp64(ent, bia, scal, x, y, field, link, kl_weight, form="dual")
        for k in ("mu", "s", "mu_w", "s_w"):
            assert float((dual[k] - sol[k]).abs().max()) <= 1e-9, k
        # a global optimum: no nearby point is better
        g = torch.Generator().manual_seed(3)
        with torch.no_grad():
            for _ in range(5):
                pert = [t + 1e-3 * torch.randn(t.shape, generator=g, dtype=torch.float64) for t in theta]
                Lp = objective_fp64(ent, bia, scal, x, y, field, (sol["entities"], *pert), link, "reg", "closed_form",
                                    kl_weight=kl_weight)
                assert bool((Lp >= L.detach()).all())


def test_argument_checks_raise_before_a_gpu_is_needed():
    m = _cpu_model()
    X = torch.tensor([[0, 6], [1, 7], [0, 9]])
    y = torch.tensor([1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="'reg'"):
        _cpu_model("class").fold_in_exact(X, torch.tensor([1.0, 0.0, 1.0]))
    with pytest.raises(ValueError, match="kl_weight"):
        m.fold_in_exact(X, y, kl_weight=0)
    with pytest.raises(ValueError, match="kl_weight"):
        m.fold_in_exact(X, y, kl_weight=-1.0)
    with pytest.raises(ValueError, match="kl_weight"):
        m.fold_in_exact(X, y, kl_weight=float("nan"))
    with pytest.raises(ValueError, match="field"):
        m.fold_in_exact(X, y, field=2)
    with pytest.raises(ValueError, match="range"):
        m.fold_in_exact(torch.tensor([[6, 7]]), torch.tensor([1.0]), field=0)
    with pytest.raises(ValueError, match="lie in"):
        m.fold_in_exact(torch.tensor([[0, 10]]), torch.tensor([1.0]), field=0)
    with pytest.raises(ValueError, match="length|one value"):
        m.fold_in_exact(X, y[:2])
    with pytest.raises(ValueError, match="frozen"):
        _cpu_model(field_sizes=[3, 4, 5]).fold_in_exact(torch.tensor([[0, 3, 4]]), torch.tensor([1.0]), field=1)


def test_cpu_model_fails_loudly():
    from vae_amd._lib import VfmLibraryError
    m = _cpu_model()
    with pytest.raises(VfmLibraryError, match="MI355X"):
        m.fold_in_exact(torch.tensor([[0, 6], [1, 7]]), torch.tensor([1.0, 2.0]))


def test_library_exports_and_struct_layout():
    from vae_amd import _lib
    lib = _lib.load()
    for name in _lib.FOLDIN_SOLVE_EXPORTS:
        getattr(lib, name)
    hdr = open(os.path.join(ROOT, "include", "vfm_foldin.h")).read()
    assert int(re.search(r"#define VFM_FOLDIN_SOLVE_LDS_DIM (\d+)", hdr).group(1)) == _lib.FOLDIN_SOLVE_LDS_DIM
    assert int(re.search(r"#define VFM_FOLDIN_SOLVE_SLABS (\d+)", hdr).group(1)) == _lib.FOLDIN_SOLVE_SLABS
    fields = [n for n, _ in _lib.FoldinSolve._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "vfm_foldin.h"\nint main(void) {\n'
           '  printf("%zu\\n", sizeof(vfm_foldin_solve_t));\n' +
           "".join(f'  printf("%zu\\n", offsetof(vfm_foldin_solve_t, {f}));\n' for f in fields) + "  return 0;\n}\n")
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        c, exe = os.path.join(tmp, "l.c"), os.path.join(tmp, "l")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-I" + os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == C.sizeof(_lib.FoldinSolve)
    assert out[1:] == [getattr(_lib.FoldinSolve, f).offset for f in fields]


def test_workspace_bytes_and_argument_codes_without_a_gpu():
    """Everything vfm_foldin_solve_f32 rejects is rejected before any HIP call, so these run without a device."""
    from vae_amd import _lib
    lib = _lib.load()
    wsb = lib.vfm_foldin_solve_workspace_bytes
    tri = lambda m: m * (m + 1) // 2
    ru = lambda v: (v + 255) // 256 * 256
    base = wsb(10, 7, 128, -1)
    assert base > 0 and base % 256 == 0                                   # d + 1 = 129 fits in LDS: operands only
    assert wsb(10, 7, 128, 4) == base + 10 * ru(tri(129) * 8)             # forced out: one slab per workgroup
    assert wsb(10_000, 7, 128, 4) == base + _lib.FOLDIN_SOLVE_SLABS * ru(tri(129) * 8)
    assert wsb(3, 5, 512, -1) - wsb(0, 5, 512, -1) == 3 * ru(tri(513) * 8)  # 513 > 135: slabs whatever lds_dim says
    for bad in [(-1, 1, 8, -1), (1, -1, 8, -1), (1, 1, 0, -1), (1, 1, 513, -1), (1, 1, 8, -2)]:
        assert wsb(*bad) == _lib._gen.VFM_E_INVALID

    def call(**kw):
        p = _lib.FoldinSolve()
        base = dict(E=1, R=1, T=10, n_ops=1, F=2, d=8, col=0, objective=_lib.OBJ_CLOSED_FORM, likelihood=_lib.LIK_NORMAL,
                    flags=0, lds_dim=-1, kl_weight=1.0)
        base.update(kw)
        for k, v in base.items():
            setattr(p, k, v)
        return lib.vfm_foldin_solve_f32(C.byref(p), None)

    E_INVALID = _lib._gen.VFM_E_INVALID
    assert call(kl_weight=0.0) == E_INVALID and b"kl_weight" in lib.vfm_last_error()
    assert call(kl_weight=-1.0) == E_INVALID
    assert call(objective=_lib.OBJ_SAMPLED) == E_INVALID and b"closed-form" in lib.vfm_last_error()
    assert call(likelihood=_lib.LIK_BERNOULLI) == E_INVALID and b"Normal" in lib.vfm_last_error()
    assert call(d=513) == E_INVALID and b"d out of range" in lib.vfm_last_error()
    assert call(col=2) == E_INVALID
    assert call(lds_dim=-2) == E_INVALID
    assert call() == E_INVALID and b"null pointer" in lib.vfm_last_error()     # (all pointers NULL)
    assert call(E=0) == 0                                                        # nothing to do, nothing launched

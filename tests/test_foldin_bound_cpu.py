"""CPU: bound fold-in (include/vfm_bound.h: vfm_foldin_bound_f32, VFM.fold_in_bound) -- the Jaakkola-Jordan inequality
and its small-xi series, the two block minimisers of tests/bound_reference.py (the GPU tests compare the kernel with
bound_rounds_fp64) against torch fp64 autograd, monotonicity, dual = primal, independence of the start, the header, the
exports, the struct mirror, the workspace formula and every VFM_E_INVALID code of the raw ABI (checked before any HIP
call, so they run without a device), the ValueErrors of check_args_bound, and the conditioning of the GPU tests' inputs."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bound_reference as BR  # noqa: E402
import solve_reference as R  # noqa: E402
from test_foldin_cpu import _cpu_model  # noqa: E402


# ---------------------------------------------------------------------------------------------------------------------
# the inequality and the series
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("y", [0.0, 1.0])
def test_jj_inequality_and_equality_at_xi(y):
    f = np.linspace(-8.0, 8.0, 321)
    for xi in (1e-6, 1e-3, 0.5, 3.0, 12.0):
        assert bool((BR.jj_bound(y, f, xi) >= BR.nll(y, f) - 1e-12).all()), xi
        for fe in (xi, -xi):
            assert abs(float(BR.jj_bound(y, fe, xi)) - float(BR.nll(y, fe))) <= 1e-12, (xi, fe)


def test_small_xi_series_meets_the_tanh_form():
    xi = 1e-3
    assert abs(float(0.25 - xi * xi / 48.0) - float(BR.jj_weight_tanh(xi))) <= 1e-14
    assert float(BR.jj_weight(0.0)) == 0.25 and 0.0 < float(BR.jj_weight(50.0)) <= 0.25
    # the switch itself: just below and just above 1e-3 the two branches of jj_weight agree
    assert abs(float(BR.jj_weight(np.nextafter(1e-3, 0.0))) - float(BR.jj_weight(1e-3))) <= 1e-14


# ---------------------------------------------------------------------------------------------------------------------
# the block minimisers
# ---------------------------------------------------------------------------------------------------------------------
def _problem(F, d, link, counts, seed, all_equal=()):
    sizes = (9, 30) if F == 2 else (9, 30, 11)
    return BR.bound_case(sizes, 0, d, link, counts, seed, all_equal=all_equal)


def _rounds(c, k, n_iters, kl, **kw):
    return BR.bound_rounds_fp64(c["ent"], c["bia"], c["scal"], c["X"], c["y"], c["field"], c["link"], kl,
                                int(c["ids"][k]), n_iters, **kw)


def _ops(c, k):
    return BR.entity_operands(c["ent"], c["bia"], c["scal"], c["X"], c["y"], c["field"], c["link"], int(c["ids"][k]))


@pytest.mark.parametrize("kl_weight", [1.0, 0.7])
@pytest.mark.parametrize("link", ["abs", "softplus"])
@pytest.mark.parametrize("F", [2, 3])
def test_block_minimisers(F, link, kl_weight):
    d = 6
    # n = 1, d, d + 1; 9 rows, three of them copies of the first (rows_with_counts' dup); 8 rows that all answer 1
    counts = [1, d, d + 1, 9, 8]
    c = _problem(F, d, link, counts, 300 + F + (link == "softplus"), all_equal=(4,))
    assert float(c["y"][c["X"][:, 0] == int(c["ids"][4])].min()) == 1.0
    xs = c["X"][c["X"][:, 0] == int(c["ids"][3])]
    assert xs.shape[0] - torch.unique(xs, dim=0).shape[0] >= 2                       # duplicates count as often as they occur
    kl = R.f32(kl_weight)
    for k, n in enumerate(counts):
        o = _ops(c, k)
        assert o["n"] == n
        r = _rounds(c, k, 30, kl_weight)
        # each q block is the exact minimiser of B_e(.; xi) at the xi it started from
        for it in range(30):
            th = torch.from_numpy(r["theta"][it]).requires_grad_(True)
            sg = torch.from_numpy(np.sqrt(r["sig2"][it])).requires_grad_(True)
            BR.bound_objective_t(o, kl, th, sg, torch.from_numpy(r["xi"][it])).backward()
            assert float(th.grad.abs().max()) <= 1e-10 and float(sg.grad.abs().max()) <= 1e-10, (n, it)
        # each xi block is too: d/dxi of B_e(theta, sigma; xi) vanishes at xi^2 = (E f)^2 + Var f, which is what makes
        # the collapsed form's gradient the one above once the rounds have converged
        th = torch.from_numpy(r["theta"][-1]).requires_grad_(True)
        sg = torch.from_numpy(np.sqrt(r["sig2"][-1])).requires_grad_(True)
        BR.bound_objective_t(o, kl, th, sg).backward()
        assert float(th.grad.abs().max()) <= 1e-8 and float(sg.grad.abs().max()) <= 1e-8, n
        # never up
        B = np.concatenate([[r["B_start"]], r["B"]])
        assert bool((np.diff(B) <= 1e-12 * np.abs(B[:-1])).all()), (n, B)
        # the two forms
        rd, rp = _rounds(c, k, 30, kl_weight, form="dual"), _rounds(c, k, 30, kl_weight, form="primal")
        assert float(np.abs(rd["theta"] - rp["theta"]).max()) <= 1e-9 and float(np.abs(rd["s"] - rp["s"]).max()) <= 1e-9


def test_independent_of_the_start_after_30_rounds():
    c = _problem(3, 6, "softplus", [1, 6, 7, 9], 321)
    g = np.random.default_rng(4)
    for k in range(4):
        a = _rounds(c, k, 30, 0.7, reset=True)
        b = _rounds(c, k, 30, 0.7, start=(g.standard_normal(7) * 2.0, np.exp(g.standard_normal(7))))
        assert float(np.abs(a["theta"][-1] - b["theta"][-1]).max()) <= 1e-9
        assert float(np.abs(a["s"][-1] - b["s"][-1]).max()) <= 1e-9


def test_the_bound_is_above_the_expected_nll():
    """B_e >= L_e of vfm_foldin.h: a Monte Carlo of the Bernoulli nll over Gaussian logits with the rows' moments (the
    bound holds for any law of f with those two moments; the normal one is enough to catch a sign or a factor)."""
    c = _problem(2, 6, "abs", [7], 330)
    o = _ops(c, 0)
    r = _rounds(c, 0, 8, 1.0)
    th, s2 = torch.from_numpy(r["theta"][-1]), torch.from_numpy(r["sig2"][-1])
    Ef, Vf = BR.moments_t(o, th, s2)
    g = torch.Generator().manual_seed(1)
    f = Ef[None] + torch.sqrt(Vf)[None] * torch.randn(20000, o["n"], generator=g, dtype=torch.float64)
    mc = float(torch.from_numpy(BR.nll(o["y"].numpy()[None], f.numpy())).mean(0).sum() + BR.kl_t(th, s2))
    assert r["B"][-1] >= mc - 0.05 and r["B"][-1] <= mc + 0.25 * o["n"]


# ---------------------------------------------------------------------------------------------------------------------
# the ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_header_exports_and_struct_layout():
    from vae_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vfm_bound.h")).read()
    assert '#include "vfm_foldin.h"' in hdr
    lib = _lib.load()
    for name in _lib.BOUND_EXPORTS:
        getattr(lib, name)
        assert name in hdr
    fields = [n for n, _ in _lib.FoldinBound._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "vfm_bound.h"\nint main(void) {\n'
           '  printf("%zu\\n", sizeof(vfm_foldin_bound_t));\n' +
           "".join(f'  printf("%zu\\n", offsetof(vfm_foldin_bound_t, {f}));\n' for f in fields) +
           '  printf("%d %d\\n", VFM_FOLDIN_FIT, VFM_FOLDIN_OBJECTIVE);\n  return 0;\n}\n')
    with tempfile.TemporaryDirectory() as tmp:
        cf, exe = os.path.join(tmp, "l.c"), os.path.join(tmp, "l")
        open(cf, "w").write(src)
        subprocess.run(["gcc", "-I" + os.path.join(ROOT, "include"), cf, "-o", exe], check=True)
        out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == C.sizeof(_lib.FoldinBound)
    assert out[1:-2] == [getattr(_lib.FoldinBound, f).offset for f in fields]
    from vae_amd import foldin
    assert out[-2:] == [foldin.MODE_FIT, foldin.MODE_OBJECTIVE]
    # the fields of vfm_foldin_solve_t, in its order, then the three new ones
    solve = [n for n, _ in _lib.FoldinSolve._fields_]
    assert [f for f in fields if f in solve] == solve
    assert [f for f in fields if f not in solve] == ["n_iters", "reset", "mode", "pad0"]


def test_workspace_formula():
    """operand block of the exact fold-in | n_ops doubles of c_var | R doubles of weights | the same slab rule."""
    from vae_amd import _lib
    lib = _lib.load()
    wsb, solve = lib.vfm_foldin_bound_workspace_bytes, lib.vfm_foldin_solve_workspace_bytes
    ru = lambda v: (v + 255) // 256 * 256
    for E, Rr, n_ops, d, lds_dim in [(10, 77, 7, 128, -1), (10, 77, 7, 128, 4), (10_000, 5, 3, 128, 4), (3, 0, 0, 512, -1),
                                     (3, 1000, 33, R.LDS, -1), (3, 1000, 33, R.LDS - 1, -1), (0, 0, 0, 1, -1)]:
        block = solve(0, n_ops, d, lds_dim)                                 # (E = 0: no slabs)
        slabs = solve(E, n_ops, d, lds_dim) - block
        assert slabs == (min(E, R.SLABS) * ru(R.tri(d + 1) * 8) if R.has_slabs(d, lds_dim) else 0)
        assert wsb(E, Rr, n_ops, d, lds_dim) == block + ru(n_ops * 8) + ru(Rr * 8) + slabs
    for bad in [(-1, 1, 1, 8, -1), (1, -1, 1, 8, -1), (1, 1, -1, 8, -1), (1, 1, 1, 0, -1), (1, 1, 1, 513, -1),
                (1, 1, 1, 8, -2)]:
        assert wsb(*bad) == _lib._gen.VFM_E_INVALID


def test_argument_codes_without_a_gpu():
    """Everything vfm_foldin_bound_f32 rejects is rejected before any HIP call: null device pointers, no device."""
    from vae_amd import _lib, foldin
    lib = _lib.load()

    def call(**kw):
        p = _lib.FoldinBound()
        base = dict(E=1, R=1, T=10, n_ops=1, F=2, d=8, col=0, objective=_lib.OBJ_CLOSED_FORM,
                    likelihood=_lib.LIK_BERNOULLI, flags=0, lds_dim=-1, kl_weight=1.0, n_iters=8, reset=0,
                    mode=foldin.MODE_FIT)
        base.update(kw)
        for k, v in base.items():
            setattr(p, k, v)
        return lib.vfm_foldin_bound_f32(C.byref(p), None)

    bad = _lib._gen.VFM_E_INVALID
    err = lib.vfm_last_error
    assert lib.vfm_foldin_bound_f32(None, None) == bad
    assert call(T=0) == bad
    assert call(d=0) == bad and call(d=513) == bad and b"d out of range" in err()
    assert call(F=0) == bad and call(F=65) == bad
    assert call(col=2) == bad and call(col=-1) == bad
    assert call(E=-1) == bad and call(R=-1) == bad
    assert call(objective=_lib.OBJ_SAMPLED) == bad and b"closed-form" in err()
    assert call(likelihood=_lib.LIK_NORMAL) == bad and b"Bernoulli" in err()
    assert call(n_ops=-1) == bad and call(n_ops=0) == bad                   # (R = 1 row needs an operand)
    assert call(flags=2) == bad
    assert call(lds_dim=-2) == bad
    assert call(kl_weight=0.0) == bad and b"kl_weight" in err()
    assert call(kl_weight=-1.0) == bad and call(kl_weight=float("inf")) == bad and call(kl_weight=float("nan")) == bad
    assert call(mode=2) == bad and b"mode" in err()
    assert call(n_iters=0) == bad and b"n_iters" in err()
    assert call(n_iters=-3) == bad
    assert call(mode=foldin.MODE_OBJECTIVE, n_iters=1) == bad and b"n_iters" in err()
    assert call() == bad and b"null pointer" in err()                        # (all pointers NULL)
    assert call(mode=foldin.MODE_OBJECTIVE, n_iters=0) == bad and b"null pointer" in err()
    # a short and a misaligned workspace: the pointers are never dereferenced (rejected first)
    need = lib.vfm_foldin_bound_workspace_bytes(1, 1, 1, 8, -1)
    fake = {k: 4096 for k in ("entities", "row_ptr", "y", "op_x", "row_op", "entity_params", "bias_params", "scalars",
                              "out_loss")}
    assert call(workspace=4096, workspace_bytes=need - 1, **fake) == bad and b"too small" in err()
    assert call(workspace=None, workspace_bytes=need, **fake) == bad and b"too small" in err()
    assert call(workspace=4096 + 64, workspace_bytes=need, **fake) == bad and b"aligned" in err()
    assert call(E=0) == 0                                                    # nothing to do, nothing launched


# ---------------------------------------------------------------------------------------------------------------------
# the Python layer
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("call", ["fold_in_bound", "fold_in_bound_objective"])
def test_argument_checks_raise_before_a_gpu_is_needed(call):
    m = _cpu_model("class")
    fn = getattr(m, call)
    X = torch.tensor([[0, 6], [1, 7], [0, 9]])
    y = torch.tensor([1.0, 0.0, 1.0])
    with pytest.raises(ValueError, match="'class'"):
        getattr(_cpu_model(), call)(X, y)
    for klw in (0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="kl_weight"):
            fn(X, y, kl_weight=klw)
    with pytest.raises(ValueError, match="0 and 1"):
        fn(X, torch.tensor([1.0, 0.5, 1.0]))
    with pytest.raises(ValueError, match="0 and 1"):
        fn(X, torch.tensor([1.0, 2.0, 1.0]))
    with pytest.raises(ValueError, match="field"):
        fn(X, y, field=2)
    with pytest.raises(ValueError, match="range"):
        fn(torch.tensor([[6, 7]]), torch.tensor([1.0]), field=0)
    with pytest.raises(ValueError, match="lie in"):
        fn(torch.tensor([[0, 10]]), torch.tensor([1.0]), field=0)
    with pytest.raises(ValueError, match="length|one value"):
        fn(X, y[:2])
    with pytest.raises(ValueError, match="frozen"):
        getattr(_cpu_model("class", field_sizes=[3, 4, 5]), call)(torch.tensor([[0, 3, 4]]), torch.tensor([1.0]), field=1)


def test_n_iters_and_lds_dim_checks():
    from vae_amd import foldin
    m = _cpu_model("class")
    X, y = torch.tensor([[0, 6]]), torch.tensor([1.0])
    for n in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="n_iters"):
            m.fold_in_bound(X, y, n_iters=n)
    with pytest.raises(ValueError, match="lds_dim"):
        foldin.run_bound(m, X, y, lds_dim=-2)
    foldin.check_args_bound(m, X, y, 0, 0.7, 8)


def test_cpu_model_fails_loudly():
    from vae_amd._lib import VfmLibraryError
    m = _cpu_model("class")
    X, y = torch.tensor([[0, 6], [1, 7]]), torch.tensor([1.0, 0.0])
    with pytest.raises(VfmLibraryError, match="MI355X"):
        m.fold_in_bound(X, y)
    with pytest.raises(VfmLibraryError, match="MI355X"):
        m.fold_in_bound_objective(X, y)


# ---------------------------------------------------------------------------------------------------------------------
# the inputs of the GPU tests
# ---------------------------------------------------------------------------------------------------------------------
def _worst_cond(c, which, iters=BR.GPU_ITERS):
    return max(float(BR.case_rounds(c, k, n_iters, reset)["cond"].max()) for k in which for n_iters, reset in iters)


@pytest.mark.parametrize("link", ["abs", "softplus"])
@pytest.mark.parametrize("d", BR.GPU_DS)
def test_gpu_shape_cases_are_well_conditioned(d, link):
    for F in (2, 3):
        c = BR.shape_case(d, link, F)
        assert c["counts"] == BR.shape_counts(d) and set(c["y"].tolist()) <= {0.0, 1.0}
        assert {n <= d for n in c["counts"]} == {True, False}               # both forms of the system
        worst = _worst_cond(c, range(len(c["counts"])))
        print(f"d={d} {link} F={F}: worst cond over the rounds {worst:.1f}")
        assert worst <= 1e3


def test_gpu_edge_cases_are_well_conditioned():
    c = BR.slab_case()
    assert R.storage(c["counts"][0], c["d"]) == "slab" and R.has_slabs(c["d"])
    assert _worst_cond(c, [0]) <= 1e3
    c = BR.lds_dim_case()
    assert {R.storage(n, c["d"], 3) for n in c["counts"]} == {"lds", "slab"}
    assert _worst_cond(c, range(len(c["counts"]))) <= 1e3
    c = BR.bitwise_case()
    assert len(c["counts"]) == 2 * R.SLABS + 37
    assert _worst_cond(c, R.bitwise_sample(len(c["counts"])), ((8, True),)) <= 1e3

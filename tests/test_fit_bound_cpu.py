"""CPU: coordinate-ascent training of 'class' models by bound solves (VFM.fit_bound, include/vfm_bound_sweep.h) -- the
fp64 restatement of tests/bound_sweep_restatement.py: no field block and no bias block increases J, the bias block is a
stationary point of the bound at fixed xi, the chunk-wise assembly of a round adds up to bound_rounds_fp64's system; the
condition numbers the GPU cases rely on; the header, the export tuple, the struct mirror, the workspace formula, the
argument codes of the entry point and the ValueErrors of the Python surface, all before anything needs a GPU.

Computed here: the largest cond of a factored matrix over the split cases of tests/test_gpu_fit_bound.py (every d, link,
F, n_iters up to 8 and both starts) is 78.4, at F = 3, abs, d = 128."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bound_reference as BR  # noqa: E402
import bound_sweep_restatement as BS  # noqa: E402
import solve_reference as R  # noqa: E402
from test_foldin_cpu import _cpu_model, _tables  # noqa: E402

LINKS = ["abs", "softplus"]


def _problem(F, d, seed, R_=60):
    sizes = [5] * F
    ent, bia, scal = _tables(sum(sizes), d, seed)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.stack([torch.randint(5 * f, 5 * f + 4, (R_,), generator=g) for f in range(F)], 1)   # (id 5 f + 4: unseen)
    x[-1] = x[0]                                                           # a duplicated row counts twice
    y = (torch.rand(R_, generator=g) < 0.4).float()
    y[-1] = y[0]
    return BS.round32(ent), BS.round32(bia), BS.round32(scal), x, y


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_iters", [1, 3])
@pytest.mark.parametrize("kl_weight", [1.0, 0.7])
@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("F", [2, 3])
def test_no_block_increases_J_and_the_bias_block_is_stationary(F, link, kl_weight, n_iters):
    ent, bia, scal, x, y = _problem(F, 3, 40 + F)
    ent0, bia0 = ent.clone(), bia.clone()
    seen = []

    def after(sweep, what, before, unrounded):
        Jb = float(BS.objective_J(*before, x, y, link, kl_weight))
        Ja = float(BS.objective_J(*unrounded, x, y, link, kl_weight))
        assert Ja <= Jb + 1e-12 * abs(Jb), (sweep, what, Ja, Jb)           # (the margin covers fp64 only)
        seen.append((sweep, what, Jb, Ja))
        if what == "bias":
            e, b, s = before
            _, _, xi = BS.global_bias_fp64(e, b, s, x, y, link, kl_weight)
            sg = unrounded[2].clone().requires_grad_(True)
            BS.bias_bound_t(e, b, sg, x, y, link, kl_weight, xi).backward()
            assert float(sg.grad[1:].abs().max()) <= 1e-10, sg.grad
            assert float(unrounded[2][0]) == float(s[0])                   # scalars[0] is left alone
            # at xi of the posterior the block started from, the bound is J there
            B0 = float(BS.bias_bound_t(e, b, s, x, y, link, kl_weight, xi))
            d = e.shape[1] // 2
            from test_foldin_cpu import kl_t, link_t
            o = torch.unique(x)
            rest = kl_t(e[o, :d], link_t(e[o, d:], link)).sum() + kl_t(b[o, 0], link_t(b[o, 1], link)).sum()
            assert abs(B0 + kl_weight * float(rest) - Jb) <= 1e-12 * abs(Jb)

    ent, bia, scal = BS.fit_bound_fp64(ent, bia, scal, x, y, link, kl_weight, 4, n_iters, after=after)
    assert [(s, w) for s, w, _, _ in seen] == [(s, w) for s in range(4) for w in list(range(F)) + ["bias"]]
    assert seen[-1][3] < seen[0][2]
    unseen = torch.tensor([5 * f + 4 for f in range(F)])
    assert torch.equal(ent[unseen], ent0[unseen]) and torch.equal(bia[unseen], bia0[unseen])


def test_the_weight_slope_bound_of_the_bias_terms():
    xi = np.concatenate([np.linspace(1e-3, 60.0, 600001), np.logspace(-3, 3, 20001)])
    w = BR.jj_weight_tanh(xi)
    h = 1e-6 * np.maximum(xi, 1.0)
    slope = np.abs(BR.jj_weight_tanh(xi + h) - BR.jj_weight_tanh(np.maximum(xi - h, 1e-4))) / (xi + h - np.maximum(xi - h, 1e-4))
    assert float(slope.max()) <= BS.W_SLOPE and float(w.max()) <= 0.25


@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("F", [2, 3])
def test_chunk_shares_add_up_to_the_round(F, link):
    c = BR.bound_case((6,) + (30,) * (F - 1), 0, 5, link, [23, 9], seed=90 + F, kl_weight=0.7)
    args = (c["ent"], c["bia"], c["scal"], c["X"], c["y"], 0, link, c["kl_weight"])
    for k, n in enumerate(c["counts"]):
        e = int(c["ids"][k])
        r = BR.bound_rounds_fp64(*args, e, 3, False, form="primal")
        theta, sig2 = BR.table_start(c["ent"], c["bia"], link, e)
        for it in range(3):
            for chunk in (1, 7, n):
                H, b, SB = BS.chunked_round_fp64(*args, e, theta, sig2, chunk)
                got = np.linalg.solve(H, b)
                assert np.abs(got - r["theta"][it]).max() <= 1e-10 * np.abs(r["theta"][it]).max(), (n, it, chunk)
                assert np.abs(c["kl_weight"] / (c["kl_weight"] + SB) - r["sig2"][it]).max() <= 1e-12, (n, it, chunk)
            theta, sig2 = r["theta"][it], r["sig2"][it]


# ---------------------------------------------------------------------------------------------------------------------
# the GPU cases' condition
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [2, 3])
@pytest.mark.parametrize("link", LINKS)
def test_split_cases_are_well_conditioned(link, F):
    worst = (0.0, None)
    for d in BS.SPLIT_DS:
        c = BS.split_case(d, link, F)
        assert c["counts"] == BS.split_counts(d)
        for k in range(len(c["counts"])):
            for reset in (False, True):
                cond = float(BR.case_rounds(c, k, 8, reset)["cond"].max())
                worst = max(worst, (cond, (F, link, d, c["counts"][k], reset)))
    print("largest cond of a factored matrix over the split cases:", worst)
    assert worst[0] <= 1e3, worst


def test_placement_mixed_and_fit_cases_are_well_conditioned():
    for link in LINKS:
        for d in (R.LDS - 1, R.LDS):
            c = BS.placement_case(d, link)
            assert R.has_slabs(d) == (d == R.LDS)
            for k in range(2):
                assert float(BR.case_rounds(c, k, 8, True)["cond"].max()) <= 1e3
    c = BS.mixed_case()
    for k in (0, 1, 2, 17, 200):
        assert float(BR.case_rounds(c, k, 8, False)["cond"].max()) <= 1e3
    sizes, X, y = BS.fit_case(3)
    ent, bia, scal = R.tables(sizes, 8, seed=603)
    e1, b1, rounds = BS.field_block_fp64(BS.round32(ent), BS.round32(bia), scal.double(), X, y, 1, "abs", R.f32(0.7), 2)
    assert max(float(r["cond"].max()) for r in rounds.values()) <= 1e3
    cnt = torch.bincount(X[:, 0], minlength=300)
    assert int((cnt > 40).sum()) == 2 and int(cnt[299]) == 0 and cnt[:2].tolist() == [60, 60]


# ---------------------------------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------------------------------
def _header():
    return open(os.path.join(ROOT, "include", "vfm_bound_sweep.h")).read()


def test_header_names_exports_and_struct_mirror_match_gcc(tmp_path):
    from vae_amd import _lib
    lib = _lib.load()
    declared = sorted(set(re.findall(r"\b(vfm_foldin_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S))))
    assert declared == sorted(_lib.BOUND_SWEEP_EXPORTS) and len(declared) == 2
    for name in _lib.BOUND_SWEEP_EXPORTS:
        getattr(lib, name)
        assert name not in _lib.EXPORTS and name not in _lib.SWEEP_EXPORTS and name not in _lib.BOUND_EXPORTS
    fields = [n for n, _ in _lib.FoldinBoundSplit._fields_]
    split = [n for n, _ in _lib.FoldinSplit._fields_]
    assert [f for f in fields if f not in ("n_iters", "reset")] == split             # vfm_foldin_split_t's fields plus two
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "vfm_bound_sweep.h"\nint main(void) {\n'
           '  printf("%zu\\n", sizeof(vfm_foldin_bound_split_t));\n' +
           "".join(f'  printf("%zu\\n", offsetof(vfm_foldin_bound_split_t, {f}));\n' for f in fields) + "  return 0;\n}\n")
    c, exe = str(tmp_path / "l.c"), str(tmp_path / "l")
    open(c, "w").write(src)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), c, "-o", exe], check=True)
    out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == C.sizeof(_lib.FoldinBoundSplit)
    assert out[1:] == [getattr(_lib.FoldinBoundSplit, f).offset for f in fields]
    body = re.search(r"typedef struct vfm_foldin_bound_split_t \{(.*?)\} vfm_foldin_bound_split_t;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s*(?:,|;)", body.replace("F, d", "F; d")) == fields


def test_workspace_bytes_and_argument_codes_without_a_gpu():
    """Everything vfm_foldin_bound_split_f32 rejects is rejected before any HIP call, so these run without a device."""
    from vae_amd import _lib
    lib = _lib.load()
    wsb, base = lib.vfm_foldin_bound_split_workspace_bytes, lib.vfm_foldin_solve_workspace_bytes
    tri = lambda m: m * (m + 1) // 2
    ru = lambda v: (v + 255) // 256 * 256
    part = lambda d: tri(d + 1) + 4 * d + 3
    for d, n_ops in ((128, 7), (5, 1), (1, 0)):
        ops_block = base(0, n_ops, d, -1)                                 # (no entities: the operand block alone)
        assert wsb(0, 0, 0, n_ops, d, -1) == ops_block + ru(n_ops * 8)
        assert wsb(11, 3, 100, n_ops, d, -1) == (ops_block + ru(n_ops * 8) + ru(100 * 8) + ru(3 * 2 * (d + 1) * 8) +
                                                 ru(11 * part(d) * 8) + ru(11 * 8))
    assert wsb(11, 3, 100, 7, 128, 4) - wsb(11, 3, 100, 7, 128, -1) == 3 * ru(tri(129) * 8)
    assert (wsb(11, 10_000, 9, 7, 128, 4) - wsb(11, 10_000, 9, 7, 128, -1)) == _lib.FOLDIN_SOLVE_SLABS * ru(tri(129) * 8)
    assert wsb(2, 3, 9, 5, 512, -1) - wsb(2, 3, 9, 5, 134, -1) > 3 * ru(tri(513) * 8)      # 513 > 135: triangles in the workspace
    E_INVALID = _lib._gen.VFM_E_INVALID
    for bad in [(-1, 1, 1, 1, 8, -1), (1, -1, 1, 1, 8, -1), (1, 1, -1, 1, 8, -1), (1, 1, 1, -1, 8, -1), (1, 1, 1, 1, 0, -1),
                (1, 1, 1, 1, 513, -1), (1, 1, 1, 1, 8, -2), (1 << 41, 1, 1, 1, 8, -1), (1, 1 << 41, 1, 1, 8, -1),
                (1, 1, 1 << 41, 1, 8, -1), (1, 1, 1, 1 << 41, 8, -1)]:
        assert wsb(*bad) == E_INVALID, bad

    def call(**kw):
        p = _lib.FoldinBoundSplit()
        args = dict(E=1, R=1, T=10, n_ops=1, n_chunks=1, F=2, d=8, col=0, flags=0, lds_dim=-1, kl_weight=1.0, n_iters=8,
                    reset=0)
        args.update(kw)
        for k, v in args.items():
            setattr(p, k, v)
        return lib.vfm_foldin_bound_split_f32(C.byref(p), None)

    assert lib.vfm_foldin_bound_split_f32(None, None) == E_INVALID and b"NULL" in lib.vfm_last_error()
    assert call(T=0) == E_INVALID and b"T < 1" in lib.vfm_last_error()
    assert call(d=513) == E_INVALID and b"d out of range" in lib.vfm_last_error()
    assert call(d=0) == E_INVALID
    assert call(F=0) == E_INVALID and b"F out of range" in lib.vfm_last_error()
    assert call(col=2) == E_INVALID and b"col" in lib.vfm_last_error()
    assert call(E=-1) == E_INVALID and call(R=-1) == E_INVALID
    assert call(n_chunks=-1) == E_INVALID and b"n_chunks" in lib.vfm_last_error()
    assert call(n_ops=0) == E_INVALID and b"n_ops" in lib.vfm_last_error()
    assert call(flags=4) == E_INVALID and b"flags" in lib.vfm_last_error()
    assert call(lds_dim=-2) == E_INVALID and b"lds_dim" in lib.vfm_last_error()
    assert call(kl_weight=0.0) == E_INVALID and b"kl_weight" in lib.vfm_last_error()
    assert call(kl_weight=-1.0) == E_INVALID and call(kl_weight=float("nan")) == E_INVALID
    assert call(kl_weight=float("inf")) == E_INVALID
    assert call(n_iters=0) == E_INVALID and b"n_iters" in lib.vfm_last_error()
    assert call(n_iters=-3) == E_INVALID
    assert call(n_iters=0, E=0) == E_INVALID                                     # (checked before the E = 0 return)
    assert call(n_chunks=1 << 41) == E_INVALID
    assert call() == E_INVALID and b"null pointer" in lib.vfm_last_error()     # (all pointers NULL)
    buf = (C.c_char * 4096)()
    ptrs = {k: C.addressof(buf) for k in ("entities", "chunk_ptr", "chunks", "y", "op_x", "row_op", "entity_params",
                                          "bias_params", "scalars", "out_loss")}
    assert call(**ptrs) == E_INVALID and b"workspace too small" in lib.vfm_last_error()
    need = wsb(1, 1, 1, 1, 8, -1)
    assert call(workspace=C.addressof(buf) | 8, workspace_bytes=need - 1, **ptrs) == E_INVALID
    assert b"workspace too small" in lib.vfm_last_error()
    assert call(workspace=C.addressof(buf) | 8, workspace_bytes=need, **ptrs) == E_INVALID
    assert b"aligned" in lib.vfm_last_error()
    assert call(E=0) == 0                                                        # nothing to do, nothing launched


def test_argument_checks_raise_before_a_gpu_is_needed():
    m = _cpu_model("class")
    X = torch.tensor([[0, 6], [1, 7], [0, 9]])
    y = torch.tensor([1.0, 0.0, 1.0])
    for call in ("fit_bound", "bound_objective"):
        with pytest.raises(ValueError, match="'class'.*fit_exact|fit_exact"):
            getattr(_cpu_model(), call)(X, y)
        for klw in (0, -1.0, float("nan")):
            with pytest.raises(ValueError, match="kl_weight"):
                getattr(m, call)(X, y, kl_weight=klw)
        with pytest.raises(ValueError, match="range"):
            getattr(m, call)(torch.tensor([[6, 7]]), torch.tensor([1.0]))      # a field-1 id in column 0
        with pytest.raises(ValueError, match="range|lie in"):
            getattr(m, call)(torch.tensor([[0, 10]]), torch.tensor([1.0]))     # an id past T in column 1
        with pytest.raises(ValueError, match="length|one value"):
            getattr(m, call)(X, y[:2])
        with pytest.raises(ValueError, match="labels"):
            getattr(m, call)(X, torch.tensor([1.0, 0.5, 0.0]))
    with pytest.raises(ValueError, match="n_sweeps"):
        m.fit_bound(X, y, n_sweeps=-1)
    for n_iters in (0, -2, 1.5):
        with pytest.raises(ValueError, match="n_iters"):
            m.fit_bound(X, y, n_iters=n_iters)
        with pytest.raises(ValueError, match="n_iters"):
            m.fold_in_bound(X, y, n_iters=n_iters, split_rows="auto")
    for fields in ((2,), (-1,), (0, 1.5), (True,)):
        with pytest.raises(ValueError, match="fields"):
            m.fit_bound(X, y, fields=fields)
    for cr in (0, -3, 2.5):
        with pytest.raises(ValueError, match="chunk_rows"):
            m.fit_bound(X, y, chunk_rows=cr)
        with pytest.raises(ValueError, match="chunk_rows"):
            m.fold_in_bound(X, y, split_rows=4, chunk_rows=cr)
        with pytest.raises(ValueError, match="chunk_rows"):
            m.fold_in_bound(X, y, chunk_rows=cr)
    for sr in ("big", -1, 2.5):
        with pytest.raises(ValueError, match="split_rows"):
            m.fit_bound(X, y, split_rows=sr)
        with pytest.raises(ValueError, match="split_rows"):
            m.fold_in_bound(X, y, split_rows=sr)
    with pytest.raises(ValueError, match="tol"):
        m.fit_bound(X, y, tol=-1.0)
    with pytest.raises(ValueError, match="max_workspace_bytes"):
        m.fold_in_bound(X, y, split_rows="auto", max_workspace_bytes=-1)
    with pytest.raises(ValueError, match="frozen"):
        _cpu_model("class", field_sizes=[3, 4, 5]).fit_bound(torch.tensor([[0, 3, 4]]), torch.tensor([1.0]))


def test_cpu_model_fails_loudly():
    from vae_amd._lib import VfmLibraryError
    m = _cpu_model("class")
    X, y = torch.tensor([[0, 6], [1, 7]]), torch.tensor([1.0, 0.0])
    with pytest.raises(VfmLibraryError, match="MI355X"):
        m.fit_bound(X, y)
    with pytest.raises(VfmLibraryError, match="MI355X"):
        m.bound_objective(X, y)
    with pytest.raises(VfmLibraryError, match="MI355X"):
        m.fold_in_bound(X, y, split_rows="auto")


def test_the_plan_sizes_its_groups_by_the_solve_it_is_for():
    """The bound's workspace holds the weights and the iterate besides the exact solve's parts, so at one budget its
    groups are no larger than the exact solve's."""
    from vae_amd import _lib
    lib = _lib.load()
    for args in ((40, 3, 7, 8, -1), (1, 1, 1, 128, 0)):
        exact = lib.vfm_foldin_split_workspace_bytes(*args)
        bound = lib.vfm_foldin_bound_split_workspace_bytes(args[0], args[1], 500, *args[2:])
        ru = lambda v: (v + 255) // 256 * 256
        assert bound == exact + ru(args[2] * 8) + ru(500 * 8) + ru(args[1] * 2 * (args[3] + 1) * 8)


def _former_check_fit_args(model, X, y, n_sweeps, kl_weight, fields, split_rows, chunk_rows, tol):
    """sweep.check_fit_args as it stood before the two fits shared one checker."""
    import math
    from vae_amd import foldin, sweep
    if model.output != "reg":
        raise ValueError("fit_exact needs a 'reg' model (Gaussian likelihood): the closed form its blocks solve has none "
                         "for 'class'; use fit")
    if not float(kl_weight) > 0.0 or not math.isfinite(float(kl_weight)):
        raise ValueError("kl_weight must be > 0 and finite: the prior term is what makes each system positive definite")
    if isinstance(n_sweeps, bool) or not isinstance(n_sweeps, int) or n_sweeps < 0:
        raise ValueError("n_sweeps must be an integer >= 0")
    if fields is None:
        fields = tuple(range(model.F))
    else:
        fields = tuple(fields)
        for f in fields:
            if isinstance(f, bool) or not isinstance(f, int) or not 0 <= f < model.F:
                raise ValueError(f"fields must hold ints in [0, {model.F})")
    sweep.resolve_split_rows(split_rows, model.d)
    sweep.check_chunk_rows(chunk_rows)
    if tol is not None and not float(tol) >= 0.0:
        raise ValueError("tol must be None or >= 0")
    x = yy = None
    for f in range(model.F):
        x, yy = foldin.check_args_exact(model, X, y, f, kl_weight)
    return x, yy, fields


def _former_check_fit_bound_args(model, X, y, n_sweeps, kl_weight, n_iters, fields, split_rows, chunk_rows, tol):
    """sweep.check_fit_bound_args as it stood before the two fits shared one checker."""
    from vae_amd import foldin, sweep
    if model.output != "class":
        raise ValueError("fit_bound needs a 'class' model (Bernoulli likelihood): a 'reg' model's blocks have their exact "
                         "optimum; use fit_exact")
    if isinstance(n_sweeps, bool) or not isinstance(n_sweeps, int) or n_sweeps < 0:
        raise ValueError("n_sweeps must be an integer >= 0")
    if fields is None:
        fields = tuple(range(model.F))
    else:
        fields = tuple(fields)
        for f in fields:
            if isinstance(f, bool) or not isinstance(f, int) or not 0 <= f < model.F:
                raise ValueError(f"fields must hold ints in [0, {model.F})")
    sweep.resolve_split_rows(split_rows, model.d)
    sweep.check_chunk_rows(chunk_rows)
    if tol is not None and not float(tol) >= 0.0:
        raise ValueError("tol must be None or >= 0")
    x = yy = None
    for f in range(model.F):
        x, yy = foldin.check_args_bound(model, X, y, f, kl_weight, n_iters)
    return x, yy, fields


# one case per message of the two former checkers: what differs from a valid call
_FIT_ARG_CASES = [dict(other_model=True), dict(kl_weight=0.0), dict(n_sweeps=-1), dict(fields=(2,)), dict(split_rows="big"),
                  dict(chunk_rows=0), dict(tol=-1.0), dict(X=torch.tensor([[6, 7]]), y=torch.tensor([1.0])),
                  dict(X=torch.tensor([[0, 10]]), y=torch.tensor([1.0])), dict(y=torch.tensor([1.0, 0.0])),
                  dict(X=torch.tensor([[0.5, 6.0]]), y=torch.tensor([1.0]))]


@pytest.mark.parametrize("kind", ["reg", "class"])
def test_merged_fit_checker_raises_the_former_texts(kind):
    """sweep.check_fit_args serves fit_exact and fit_bound; for each message of the two checkers it replaced, a 'reg'
    and a 'class' model raise the former text, and a valid call returns what the former one returned."""
    from vae_amd import sweep
    base = dict(X=torch.tensor([[0, 6], [1, 7], [0, 9]]), y=torch.tensor([1.0, 0.0, 1.0]), n_sweeps=3, kl_weight=0.7,
                fields=None, split_rows="auto", chunk_rows=16, tol=None)
    cases = list(_FIT_ARG_CASES)
    if kind == "class":
        cases += [dict(n_iters=0), dict(y=torch.tensor([1.0, 0.5, 0.0]))]          # the bound's own: n_iters, the labels

    def both(other_model=False, n_iters=8, **kw):
        a = dict(base, **kw)
        m = _cpu_model(("class" if kind == "reg" else "reg") if other_model else kind)
        rest = (a["fields"], a["split_rows"], a["chunk_rows"], a["tol"])
        if kind == "reg":
            return (lambda: _former_check_fit_args(m, a["X"], a["y"], a["n_sweeps"], a["kl_weight"], *rest),
                    lambda: sweep._check_fit_exact(m, a["X"], a["y"], a["n_sweeps"], a["kl_weight"], *rest))
        return (lambda: _former_check_fit_bound_args(m, a["X"], a["y"], a["n_sweeps"], a["kl_weight"], n_iters, *rest),
                lambda: sweep._check_fit_bound(m, a["X"], a["y"], a["n_sweeps"], a["kl_weight"], n_iters, *rest))

    for case in cases:
        former, merged = both(**case)
        with pytest.raises(ValueError) as want:
            former()
        with pytest.raises(ValueError) as got:
            merged()
        assert str(got.value) == str(want.value), case
    former, merged = both()
    (x0, y0, f0), (x1, y1, f1) = former(), merged()
    assert torch.equal(x0, x1) and torch.equal(y0, y1) and f0 == f1 == (0, 1)

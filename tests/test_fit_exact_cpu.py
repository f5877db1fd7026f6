"""CPU: exact coordinate-ascent training (VFM.fit_exact, include/vfm_sweep.h) -- the fp64 restatement of
tests/fit_exact_restatement.py: every block of a sweep (each field's solve_fp64, the global bias, the precision) is a
stationary point of J under autograd and J never increases; the chunk-wise assembly of the split solve adds up to
solve_fp64's system; the header, the export tuple, the struct mirror, the workspace formula, the argument codes of the
entry point and the ValueErrors of the Python surface, all before anything needs a GPU."""
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

import fit_exact_restatement as FR  # noqa: E402
import solve_reference as R  # noqa: E402
from test_foldin_cpu import _cpu_model, _tables  # noqa: E402
from test_foldin_exact_cpu import solve_fp64  # noqa: E402


def _problem(F, d, seed, R_=60):
    sizes = [5] * F
    ent, bia, scal = _tables(sum(sizes), d, seed)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.stack([torch.randint(5 * f, 5 * f + 4, (R_,), generator=g) for f in range(F)], 1)   # (id 5 f + 4: unseen)
    x[-1] = x[0]                                                           # a duplicated row counts twice
    y = torch.randn(R_, generator=g, dtype=torch.float64) + 1.0
    y[-1] = y[0]
    return ent, bia, scal, x, y


@pytest.mark.parametrize("kl_weight", [1.0, 0.7])
@pytest.mark.parametrize("link", ["abs", "softplus"])
@pytest.mark.parametrize("F", [2, 3])
def test_every_block_is_a_stationary_point_and_J_never_increases(F, link, kl_weight):
    d = 3
    ent, bia, scal, x, y = _problem(F, d, 40 + F)
    J = [float(FR.objective_J(ent, bia, scal, x, y, link, kl_weight))]
    unseen = torch.tensor([5 * f + 4 for f in range(F)])
    ent0, bia0 = ent.clone(), bia.clone()

    def after(what, e, b, s):
        e, b, s = (t.clone().requires_grad_(True) for t in (e, b, s))
        Jb = FR.objective_J(e, b, s, x, y, link, kl_weight)
        Jb.backward()
        Jb = Jb.detach()
        if what == "scalars":
            # (each a block minimiser on its own: the bias pair at the old precision was checked by value below; here
            # the precision at the new bias, and the bias pair's gradient scaled by the precision's change)
            assert abs(float(s.grad[0])) <= 1e-10, s.grad
        else:
            rows = torch.unique(x[:, what])
            assert float(e.grad[rows].abs().max()) <= 1e-10 and float(b.grad[rows].abs().max()) <= 1e-10, what
        assert float(Jb) <= J[-1] + 1e-12 * abs(J[-1]), (what, float(Jb), J[-1])
        J.append(float(Jb))

    for _ in range(5):
        ent, bia, _ = FR.sweep_fp64(ent, bia, scal, x, y, link, kl_weight, update_scalars=False, after=after)
        # the scalars, one block at a time: the global bias (jointly in mean and scale), then the precision
        s1 = scal.clone()
        s1[1], s1[2] = FR.global_bias_fp64(ent, bia, scal, x, y, link, kl_weight)
        sg = s1.clone().requires_grad_(True)
        FR.objective_J(ent, bia, sg, x, y, link, kl_weight).backward()
        assert float(sg.grad[1:].abs().max()) <= 1e-10, sg.grad
        assert float(FR.objective_J(ent, bia, s1, x, y, link, kl_weight)) <= J[-1] + 1e-12 * abs(J[-1])
        scal = FR.scalars_block_fp64(ent, bia, scal, x, y, link, kl_weight)
        assert torch.equal(scal[1:], s1[1:])
        after("scalars", ent, bia, scal)
    assert len(J) == 1 + 5 * (F + 1) and J[-1] < J[0]
    # entities that do not occur in x are not written
    assert torch.equal(ent[unseen], ent0[unseen]) and torch.equal(bia[unseen], bia0[unseen])


@pytest.mark.parametrize("link", ["abs", "softplus"])
def test_block_objective_is_J_up_to_terms_of_the_other_fields(link):
    """sum_e L_e of field f differs from J by the KL of the other fields' entities and of the global bias only, so the
    field's exact fold-in over all rows is J's block minimiser."""
    from test_foldin_cpu import kl_t, link_t, objective_fp64
    ent, bia, scal, x, y = _problem(3, 3, 7)
    d = 3
    J = float(FR.objective_J(ent, bia, scal, x, y, link, 0.7))
    for f in range(3):
        e = torch.unique(x[:, f])
        L = objective_fp64(ent, bia, scal, x, y, f, (e, ent[e, :d], ent[e, d:], bia[e, 0], bia[e, 1]), link, "reg",
                           "closed_form", None, 0.7).sum()
        o = torch.unique(torch.cat([x[:, :f], x[:, f + 1:]], 1))
        rest = kl_t(ent[o, :d], link_t(ent[o, d:], link)).sum() + kl_t(bia[o, 0], link_t(bia[o, 1], link)).sum()
        rest = rest + kl_t(scal[1], link_t(scal[2], link))
        assert abs(float(L + 0.7 * rest) - J) <= 1e-12 * abs(J), f


@pytest.mark.parametrize("link", ["abs", "softplus"])
@pytest.mark.parametrize("F", [2, 3])
def test_chunk_shares_add_up_to_the_system(F, link):
    c = R.case((6,) + (30,) * (F - 1), 0, 5, link, [23, 9], seed=90 + F, kl_weight=0.7)
    args = (c["ent"], c["bia"], c["scal"], c["X"], c["y"], 0, link, c["kl_weight"])
    sol = solve_fp64(*args)
    for k, n in enumerate(c["counts"]):
        e = int(c["ids"][k])
        H, b = FR.system_fp64(*args, e)
        theta = np.concatenate([[float(sol["mu_w"][k])], sol["mu"][k].numpy()])
        assert np.abs(np.linalg.solve(H, b) - theta).max() <= 1e-10 * np.abs(theta).max()   # solve_fp64's own system
        for chunk in (1, 7, n):
            Hc, bc = FR.chunked_system_fp64(*args, e, chunk)
            assert np.abs(Hc - H).max() <= 1e-12 * np.abs(H).max(), (n, chunk)
            assert np.abs(bc - b).max() <= 1e-12 * np.abs(b).max(), (n, chunk)


def test_chunk_table():
    from vae_amd.sweep import chunk_table
    ptr, tab = chunk_table(np.array([10, 40, 49]), np.array([30, 9, 16]), 8)
    assert ptr.tolist() == [0, 4, 6, 8]
    assert tab.tolist() == [[0, 10, 8], [0, 18, 8], [0, 26, 8], [0, 34, 6], [1, 40, 8], [1, 48, 1], [2, 49, 8], [2, 57, 8]]
    ptr, tab = chunk_table(np.zeros(0, np.int64), np.zeros(0, np.int64), 8)
    assert ptr.tolist() == [0] and tab.shape == (0, 3)


# ---------------------------------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------------------------------
def _header():
    return open(os.path.join(ROOT, "include", "vfm_sweep.h")).read()


def test_header_names_exports_and_struct_mirror_match_gcc(tmp_path):
    from vae_amd import _lib
    lib = _lib.load()
    declared = sorted(set(re.findall(r"\b(vfm_foldin_\w+)\s*\(", _header())))
    assert declared == sorted(_lib.SWEEP_EXPORTS) and len(declared) == 2
    for name in _lib.SWEEP_EXPORTS:
        getattr(lib, name)
        assert name not in _lib.EXPORTS and name not in _lib.FOLDIN_SOLVE_EXPORTS
    fields = [n for n, _ in _lib.FoldinSplit._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "vfm_sweep.h"\nint main(void) {\n'
           '  printf("%zu\\n", sizeof(vfm_foldin_split_t));\n' +
           "".join(f'  printf("%zu\\n", offsetof(vfm_foldin_split_t, {f}));\n' for f in fields) + "  return 0;\n}\n")
    c, exe = str(tmp_path / "l.c"), str(tmp_path / "l")
    open(c, "w").write(src)
    subprocess.run(["gcc", "-I" + os.path.join(ROOT, "include"), c, "-o", exe], check=True)
    out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == C.sizeof(_lib.FoldinSplit)
    assert out[1:] == [getattr(_lib.FoldinSplit, f).offset for f in fields]
    body = re.search(r"typedef struct vfm_foldin_split_t \{(.*?)\} vfm_foldin_split_t;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s*(?:,|;)", body.replace("F, d", "F; d")) == fields


def test_workspace_bytes_and_argument_codes_without_a_gpu():
    """Everything vfm_foldin_solve_split_f32 rejects is rejected before any HIP call, so these run without a device."""
    from vae_amd import _lib
    lib = _lib.load()
    wsb, base = lib.vfm_foldin_split_workspace_bytes, lib.vfm_foldin_solve_workspace_bytes
    tri = lambda m: m * (m + 1) // 2
    ru = lambda v: (v + 255) // 256 * 256
    part = lambda d: tri(d + 1) + 4 * d + 3
    for d, n_ops in ((128, 7), (5, 1), (1, 0)):
        ops_block = base(0, n_ops, d, -1)                                 # (no entities: the operand block alone)
        assert wsb(0, 0, n_ops, d, -1) == ops_block
        assert wsb(11, 3, n_ops, d, -1) == ops_block + ru(11 * part(d) * 8) + ru(11 * 8)
    ops_block = base(0, 7, 128, -1)
    assert wsb(11, 3, 7, 128, 4) == ops_block + ru(11 * part(128) * 8) + ru(11 * 8) + 3 * ru(tri(129) * 8)
    assert (wsb(11, 10_000, 7, 128, 4) - wsb(11, 0, 7, 128, 4)) == _lib.FOLDIN_SOLVE_SLABS * ru(tri(129) * 8)
    assert wsb(2, 3, 5, 512, -1) - wsb(2, 0, 5, 512, -1) == 3 * ru(tri(513) * 8)     # 513 > 135: triangles in the workspace
    E_INVALID = _lib._gen.VFM_E_INVALID
    for bad in [(-1, 1, 1, 8, -1), (1, -1, 1, 8, -1), (1, 1, -1, 8, -1), (1, 1, 1, 0, -1), (1, 1, 1, 513, -1),
                (1, 1, 1, 8, -2), (1 << 41, 1, 1, 8, -1), (1, 1 << 41, 1, 8, -1), (1, 1, 1 << 41, 8, -1)]:
        assert wsb(*bad) == E_INVALID, bad

    def call(**kw):
        p = _lib.FoldinSplit()
        args = dict(E=1, R=1, T=10, n_ops=1, n_chunks=1, F=2, d=8, col=0, flags=0, lds_dim=-1, kl_weight=1.0)
        args.update(kw)
        for k, v in args.items():
            setattr(p, k, v)
        return lib.vfm_foldin_solve_split_f32(C.byref(p), None)

    assert lib.vfm_foldin_solve_split_f32(None, None) == E_INVALID and b"NULL" in lib.vfm_last_error()
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
    assert call(n_chunks=1 << 41) == E_INVALID
    assert call() == E_INVALID and b"null pointer" in lib.vfm_last_error()     # (all pointers NULL)
    buf = (C.c_char * 4096)()
    ptrs = {k: C.addressof(buf) for k in ("entities", "chunk_ptr", "chunks", "y", "op_x", "row_op", "entity_params",
                                          "bias_params", "scalars", "out_loss")}
    assert call(**ptrs) == E_INVALID and b"workspace too small" in lib.vfm_last_error()
    need = wsb(1, 1, 1, 8, -1)
    assert call(workspace=C.addressof(buf) | 8, workspace_bytes=need, **ptrs) == E_INVALID
    assert b"aligned" in lib.vfm_last_error()
    assert call(E=0) == 0                                                        # nothing to do, nothing launched


def test_argument_checks_raise_before_a_gpu_is_needed():
    m = _cpu_model()
    X = torch.tensor([[0, 6], [1, 7], [0, 9]])
    y = torch.tensor([1.0, 2.0, 3.0])
    yc = torch.tensor([1.0, 0.0, 1.0])
    for call in ("fit_exact", "exact_objective"):
        with pytest.raises(ValueError, match="'reg'"):
            getattr(_cpu_model("class"), call)(X, yc)
        for klw in (0, -1.0, float("nan")):
            with pytest.raises(ValueError, match="kl_weight"):
                getattr(m, call)(X, y, kl_weight=klw)
        with pytest.raises(ValueError, match="range"):
            getattr(m, call)(torch.tensor([[6, 7]]), torch.tensor([1.0]))      # a field-1 id in column 0
        with pytest.raises(ValueError, match="range|lie in"):
            getattr(m, call)(torch.tensor([[0, 10]]), torch.tensor([1.0]))     # an id past T in column 1
        with pytest.raises(ValueError, match="range|frozen"):
            getattr(m, call)(torch.tensor([[0, 3]]), torch.tensor([1.0]))      # a field-0 id in column 1
        with pytest.raises(ValueError, match="length|one value"):
            getattr(m, call)(X, y[:2])
    with pytest.raises(ValueError, match="n_sweeps"):
        m.fit_exact(X, y, n_sweeps=-1)
    for fields in ((2,), (-1,), (0, 1.5), (True,)):
        with pytest.raises(ValueError, match="fields"):
            m.fit_exact(X, y, fields=fields)
    for cr in (0, -3, 2.5):
        with pytest.raises(ValueError, match="chunk_rows"):
            m.fit_exact(X, y, chunk_rows=cr)
        with pytest.raises(ValueError, match="chunk_rows"):
            m.fold_in_exact(X, y, split_rows=4, chunk_rows=cr)
    for sr in ("big", -1, 2.5):
        with pytest.raises(ValueError, match="split_rows"):
            m.fit_exact(X, y, split_rows=sr)
        with pytest.raises(ValueError, match="split_rows"):
            m.fold_in_exact(X, y, split_rows=sr)
    with pytest.raises(ValueError, match="tol"):
        m.fit_exact(X, y, tol=-1.0)
    with pytest.raises(ValueError, match="frozen"):
        _cpu_model(field_sizes=[3, 4, 5]).fit_exact(torch.tensor([[0, 3, 4]]), torch.tensor([1.0]))


def test_cpu_model_fails_loudly():
    from vae_amd._lib import VfmLibraryError
    m = _cpu_model()
    X, y = torch.tensor([[0, 6], [1, 7]]), torch.tensor([1.0, 2.0])
    with pytest.raises(VfmLibraryError, match="MI355X"):
        m.fit_exact(X, y)
    with pytest.raises(VfmLibraryError, match="MI355X"):
        m.exact_objective(X, y)
    with pytest.raises(VfmLibraryError, match="MI355X"):
        m.fold_in_exact(X, y, split_rows="auto")


def test_split_rows_rule():
    from vae_amd.sweep import resolve_split_rows
    assert resolve_split_rows(None, 8) is None and resolve_split_rows("auto", 8) == 36
    assert resolve_split_rows(0, 8) == 9 and resolve_split_rows(9, 8) == 9 and resolve_split_rows(50, 8) == 50


@pytest.mark.parametrize("link", ["abs", "softplus"])
@pytest.mark.parametrize("n, d", [(1, 1), (7, 5), (300, 20)])
def test_shared_kl_of_the_seen_rows_is_the_two_former_expressions(n, d, link):
    """sweep._add_kl64_rows, which objective_terms and bound_objective_terms now share, against the expression each of
    them held: the same two fp64 sums added in the same order, so torch.equal."""
    from vae_amd import sweep
    g = torch.Generator().manual_seed(17 * n + d)
    e = torch.randn(n, 2 * d, generator=g) * 0.7                           # fp32 table rows, as the model holds them
    b = torch.randn(n, 2, generator=g) * 0.7
    if link == "abs":
        e[:, d:] = e[:, d:].abs() + 0.05                                   # (sigma = |s| > 0)
        b[:, 1] = b[:, 1].abs() + 0.05
    kl0 = sweep._kl64(torch.randn((), generator=g).double(), torch.rand((), generator=g).double() + 0.1)

    def former_exact(kl):                                                  # objective_terms, the branch without priors
        kl = kl + sweep._kl64(e[:, :d].double(), sweep._link64(e[:, d:], link)).sum()
        kl = kl + sweep._kl64(b[:, 0].double(), sweep._link64(b[:, 1], link)).sum()
        return kl

    def former_bound(kl):                                                  # bound_objective_terms
        kl = kl + sweep._kl64(e[:, :d].double(), sweep._link64(e[:, d:], link)).sum()
        kl = kl + sweep._kl64(b[:, 0].double(), sweep._link64(b[:, 1], link)).sum()
        return kl

    got = sweep._add_kl64_rows(kl0, e, b, d, link)
    assert got.dtype == torch.float64 and bool(torch.isfinite(got))
    assert torch.equal(got, former_exact(kl0)) and torch.equal(got, former_bound(kl0))

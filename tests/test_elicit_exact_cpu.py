"""CPU: the exact field-form elicitation session (include/vfm_elicit.h: vfm_elicit_solve_f32) -- the fp64 restatement
(elicit_exact_restatement.py: elicit_field_restatement.moments + test_foldin_exact_cpu.solve_fp64): every round's theta
has a vanishing gradient of objective_fp64 on that round's rows and the asked sequence is that of a brute-force loop
over the two functions; the planted generators the GPU test uses keep the best and second-best score apart in every
round, and an fp32 numpy run asks what the fp64 run asks; the library exports the header's symbols, lays the struct out
as gcc does, sizes the workspace as documented and refuses every bad argument before any HIP call;
VFM.elicit_field_exact / elicitation_curve_field_exact raise ValueError before anything needs a GPU."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import elicit_exact_restatement as RX
import elicit_field_restatement as RF
from test_foldin_cpu import objective_fp64

HDR = os.path.join(ROOT, "include", "vfm_elicit.h")


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
def _planted_f3(kind, d, seed, n_hist, P=9):
    """A planted F = 3 model (sizes 5, 9, 4; respondents in field 1) and one respondent's pool and history."""
    g = np.random.default_rng(seed)
    sizes, field = (5, 9, 4), 1
    T = sum(sizes)
    ent = np.concatenate([g.normal(size=(T, d)) / np.sqrt(d), g.normal(size=(T, d)) * 0.3 + 0.4], 1)
    bia = np.stack([g.normal(size=T) * 0.2, g.normal(size=T) * 0.1 + 0.3], 1)
    scal = np.array([1.7, 0.2, 0.4])
    pick = g.permutation(sizes[0] * sizes[2])[:P + n_hist]
    rows = np.stack([pick // sizes[2], np.full(len(pick), 5 + 3), 14 + pick % sizes[2]], 1).astype(np.int64)
    y = g.normal(size=len(pick)) + 1.0
    return ent, bia, scal, field, 8, rows[:P], y[:P], rows[P:], y[P:]


@pytest.mark.parametrize("kind,d,n_hist,strategy,reset", [("abs", 3, 0, "variance", True), ("softplus", 3, 2, "top", False),
                                                          ("abs", 12, 4, "variance", False)])
def test_every_rounds_theta_is_the_optimum_and_the_sequence_is_brute_force(kind, d, n_hist, strategy, reset):
    ent, bia, scal, field, e, px, py, hx, hy = _planted_f3(kind, d, 3 + d, n_hist)
    Q, klw = 11, 0.7                                        # Q > P = 9: the pool runs out; d = 3: n crosses d
    s = RX.session(e, px, py, Q, strategy, ent, bia, scal, field=field, kind=kind, hist_x=hx, hist_y=hy, klw=klw,
                   reset=reset)
    assert s["rows"] == RX.brute_force(e, px, py, Q, strategy, ent, bia, scal, field, kind, hx, hy, klw, reset)
    assert sorted(r for r in s["rows"] if r >= 0) == list(range(9)) and s["rows"][9:] == [-1, -1]
    E, B, S = (torch.as_tensor(a) for a in (ent, bia, scal))
    for q in range(Q):
        if s["rows"][q] < 0:
            assert s["theta"][q] is s["theta"][q - 1]       # nothing more is folded
            continue
        X, y = torch.as_tensor(s["fold_x"][q]), torch.as_tensor(s["fold_y"][q])
        assert X.shape[0] == n_hist + q + 1
        assert np.array_equal(s["fold_x"][q][:n_hist], hx) and np.array_equal(s["fold_x"][q][-1], px[s["rows"][q]])
        mu, sp, mw, sw = s["theta"][q]
        th = [torch.tensor(v, dtype=torch.float64).reshape(shape).requires_grad_(True)
              for v, shape in ((mu, (1, d)), (sp, (1, d)), (mw, (1,)), (sw, (1,)))]
        L = objective_fp64(E, B, S, X, y, field, (torch.tensor([e]), *th), kind, "reg", "closed_form", kl_weight=klw)
        L.sum().backward()
        for t in th:
            assert float(t.grad.abs().max()) <= 1e-10       # (test_foldin_exact_cpu's tolerance)


@pytest.mark.parametrize("name", RX.PLANTED)
def test_planted_generators_keep_the_choices_apart_in_fp64_and_fp32(name):
    """The inputs of test_gpu_elicit_exact.py::test_against_the_fp64_restatement: in every round of every respondent
    the best and the second-best score differ by more than GAP_FLOOR relative -- fp32 rounding of a score is about 1e-6
    -- and a float32 numpy run of the same loop asks the same rows.  So the GPU test may require identical sequences
    for all respondents."""
    c = RF.planted_case(name)
    s64 = RX.planted_sessions(name, c)
    s32 = RX.planted_sessions(name, c, moments=RX.moments_f32, solve=RX.solve_f32)
    assert len(s64) == RF.PLANTED_RESPONDENTS
    worst = min(min(s["gap"]) for s in s64)
    cond = max(max(s["cond"]) for s in s64)
    print(f"{name}: smallest relative gap {worst:.3e}, largest cond(H) {cond:.1f}")
    assert worst > RX.GAP_FLOOR, (name, worst)
    assert cond <= 1e3, cond                                # (the bound test_gpu_foldin_exact.py asserts before comparing)
    for a, b in zip(s64, s32):
        assert a["rows"] == b["rows"] and all(r >= 0 for r in a["rows"]), a["entity"]
        assert min(b["gap"]) > 0.5 * RX.GAP_FLOOR


# ---------------------------------------------------------------------------------------------------------------------
# the library without a GPU
# ---------------------------------------------------------------------------------------------------------------------
def _header_fields():
    text = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    body = re.search(r"typedef struct vfm_elicit_solve_t \{(.*?)\} vfm_elicit_solve_t;", text, re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names = decl.split(",")
            fields.append(re.findall(r"\w+", names[0])[-1])
            fields += [re.findall(r"\w+", n)[-1] for n in names[1:]]
    return fields


def test_exports_and_struct_mirror_match_gcc(tmp_path):
    from vae_amd import _lib
    lib = _lib.load()
    for name in _lib.ELICIT_SOLVE_EXPORTS:
        getattr(lib, name)
    assert _lib.ABI_VERSION == 5                            # additions only
    fields = _header_fields()
    assert fields == [n for n, _ in _lib.ElicitSolve._fields_]           # every field, in order
    for dropped in ("n_steps", "lr", "n_samples", "t0", "lds_rows", "objective", "likelihood"):
        assert dropped not in fields
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vfm_elicit.h"', "int main(void) {",
             'printf("S %zu\\n", sizeof(vfm_elicit_solve_t));']
    lines += [f'printf("F {n} %zu\\n", offsetof(vfm_elicit_solve_t, {n}));' for n in fields]
    lines += ["return 0; }"]
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    seen = 0
    for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n"):
        t = ln.split()
        if not t:
            continue
        if t[0] == "S":
            assert C.sizeof(_lib.ElicitSolve) == int(t[1])
        else:
            assert getattr(_lib.ElicitSolve, t[1]).offset == int(t[2]), t[1]
            seen += 1
    assert seen == len(fields)
    e = _lib.ElicitSolve()
    assert (e.struct_size, e.abi_version) == (C.sizeof(_lib.ElicitSolve), _lib.ABI_VERSION)
    with pytest.raises(AttributeError):
        e.lds_rows = 1                                      # (the Adam session's field)


def test_workspace_function():
    from vae_amd import _lib
    lib = _lib.load()
    w = lib.vfm_elicit_solve_workspace_bytes
    tri = lambda m: m * (m + 1) // 2
    ru = lambda v: (v + 255) // 256 * 256
    # U = 3, P = 100, 7 contexts, d = 5 (lane shape 8 x 1): flags [P]; score operands [7, 4 d] floats and constants
    # [7, 2]; the fold-in's fp32 operands [7, 3, 8] and constants [7, 2]; its fp64 operands [7, 3, d] and c_mean [7]
    base = ru(100) + ru(7 * 20 * 4) + ru(7 * 2 * 4) + ru(7 * 24 * 4) + ru(7 * 2 * 4) + ru(7 * 15 * 8) + ru(7 * 8)
    assert w(3, 100, 7, 5, -1) == base                       # d + 1 = 6 fits in LDS: no slabs
    assert w(3, 100, 7, 5, 6) == base and w(3, 100, 7, 5, 200) == base
    assert w(3, 100, 7, 5, 0) == base + 3 * ru(tri(6) * 8)   # forced out: one slab per workgroup
    assert w(300, 100, 7, 5, 5) == base + _lib.FOLDIN_SOLVE_SLABS * ru(tri(6) * 8)       # the grid cap
    assert w(2, 0, 0, 512, -1) == ru(1) + 2 * ru(tri(513) * 8)                             # 513 > 135: slabs whatever lds_dim
    assert w(0, 0, 0, 1, -1) == 256
    # what the exact fold-in and the field session ask for, put together
    fs, ef = lib.vfm_foldin_solve_workspace_bytes, lib.vfm_elicit_field_workspace_bytes
    assert w(9, 40, 11, 128, 4) == ef(40, 11, 128, _lib.OBJ_SAMPLED) + fs(9, 11, 128, 4)
    # monotone in every argument (lds_dim: a smaller cap never needs less)
    ref = (9, 40, 11, 128, 60)
    for i, bigger in enumerate((300, 4000, 12, 129)):
        up = list(ref)
        up[i] = bigger
        assert w(*up) >= w(*ref), i
    assert w(9, 40, 11, 128, 4) >= w(9, 40, 11, 128, 60) >= w(9, 40, 11, 128, 129) == w(9, 40, 11, 128, -1)
    for bad in ((-1, 1, 1, 8, -1), (1, -1, 1, 8, -1), (1, 1, -1, 8, -1), (1, 1, 1, 0, -1), (1, 1, 1, 513, -1),
                (1, 1, 1, 8, -2)):
        assert w(*bad) == _lib._gen.VFM_E_INVALID, bad


def _valid(lib_mod):
    """A struct that passes every value check and fails only on its (missing) pointers."""
    e = lib_mod.ElicitSolve()
    e.T, e.F, e.d, e.field, e.key_col, e.U, e.P, e.H, e.n_ops = 10, 3, 4, 0, 1, 1, 2, 0, 2
    e.n_rounds, e.strategy, e.lds_dim, e.kl_weight = 3, 1, -1, 1.0
    return e


REFUSALS = [  # (field, value), .., -> a word of vfm_last_error()
    ([("F", 1)], b"F out of range"), ([("F", 65)], b"F out of range"),
    ([("field", -1)], b"field out of range"), ([("field", 3)], b"field out of range"),
    ([("key_col", -1)], b"key_col"), ([("key_col", 3)], b"key_col"), ([("key_col", 0)], b"key_col"),
    ([("d", 0)], b"d out of range"), ([("d", 513)], b"d out of range"),
    ([("U", -1)], b"U < 0"), ([("P", -1)], b"P < 0"), ([("H", -1)], b"H < 0"),
    ([("T", 0)], b"T < 1"),
    ([("n_rounds", 4097)], b"n_rounds"), ([("n_rounds", -1)], b"n_rounds"),
    ([("strategy", 4)], b"strategy"), ([("strategy", -1)], b"strategy"),
    ([("flags", 1)], b"flags"), ([("flags", 16 | 32)], b"flags"),
    ([("n_ops", 0)], b"n_ops"), ([("n_ops", -1)], b"n_ops"),
    ([("lds_dim", -2)], b"lds_dim"),
    ([("kl_weight", 0.0)], b"kl_weight"), ([("kl_weight", -1.0)], b"kl_weight"),
    ([("kl_weight", float("nan"))], b"kl_weight"), ([("kl_weight", float("inf"))], b"kl_weight"),
    ([("out_mean", 256)], b"out_mean"), ([("out_var", 256)], b"out_mean"),
]


@pytest.mark.parametrize("sets,word", REFUSALS, ids=["-".join(f"{k}={v}" for k, v in s) for s, _ in REFUSALS])
def test_library_refuses_bad_values_before_any_hip_call(sets, word):
    from vae_amd import _lib
    lib = _lib.load()
    e = _valid(_lib)
    assert lib.vfm_elicit_solve_f32(C.byref(e), None) == -1 and b"null pointer" in lib.vfm_last_error()
    for k, v in sets:
        setattr(e, k, v)
    assert lib.vfm_elicit_solve_f32(C.byref(e), None) == _lib._gen.VFM_E_INVALID
    assert word in lib.vfm_last_error(), lib.vfm_last_error()


def test_library_refuses_struct_pointers_and_workspace():
    """The pointer checks see only whether a pointer is NULL: the fake non-NULL values below are never followed, since
    every call is refused before any HIP call."""
    from vae_amd import _lib
    lib = _lib.load()
    INV = _lib._gen.VFM_E_INVALID
    f = lib.vfm_elicit_solve_f32
    assert f(None, None) == INV and b"NULL argument struct" in lib.vfm_last_error()
    e = _valid(_lib)
    e.struct_size -= 8
    assert f(C.byref(e), None) == INV and b"struct_size" in lib.vfm_last_error()
    e.struct_size += 8
    e.abi_version += 1
    assert f(C.byref(e), None) == INV and b"abi_version" in lib.vfm_last_error()
    e = _valid(_lib)
    tables = ("entities", "pool_ptr", "pool_x", "pool_y", "entity_params", "bias_params", "scalars", "out_row",
              "out_score", "out_loss")
    for name in tables:
        setattr(e, name, 4096)
    for name in tables:                                     # each one missing in turn
        setattr(e, name, None)
        assert f(C.byref(e), None) == INV and b"null pointer" in lib.vfm_last_error(), name
        setattr(e, name, 4096)
    assert f(C.byref(e), None) == INV and b"op_x" in lib.vfm_last_error()
    e.op_x = 4096
    assert f(C.byref(e), None) == INV and b"op_x" in lib.vfm_last_error()       # (pool_op)
    e.pool_op = 4096
    e.H = 1
    assert f(C.byref(e), None) == INV and b"null pointer" in lib.vfm_last_error()   # (history)
    e.hist_ptr = e.hist_x = e.hist_y = 4096
    assert f(C.byref(e), None) == INV and b"hist_op" in lib.vfm_last_error()
    e.H = 0
    need = lib.vfm_elicit_solve_workspace_bytes(e.U, e.P, e.n_ops, e.d, e.lds_dim)
    assert need > 0
    assert f(C.byref(e), None) == INV and b"workspace too small" in lib.vfm_last_error()
    e.workspace, e.workspace_bytes = 4096, need - 1
    assert f(C.byref(e), None) == INV and b"workspace too small" in lib.vfm_last_error()
    e.lds_dim = 0                                           # slabs: the same bytes no longer suffice
    e.workspace_bytes = need
    assert f(C.byref(e), None) == INV and b"workspace too small" in lib.vfm_last_error()
    e.lds_dim = -1
    e.workspace, e.workspace_bytes = 4096 + 64, need
    assert f(C.byref(e), None) == INV and b"256-byte aligned" in lib.vfm_last_error()


def test_no_respondents_is_a_no_op():
    from vae_amd import _lib
    lib = _lib.load()
    e = _valid(_lib)
    e.U = e.P = e.n_ops = 0
    assert lib.vfm_elicit_solve_f32(C.byref(e), None) == 0  # nothing to do, nothing launched


# ---------------------------------------------------------------------------------------------------------------------
# the Python entry points without a GPU
# ---------------------------------------------------------------------------------------------------------------------
def _cpu_model(output="reg", sizes=(6, 4, 3)):
    from vae_amd.model import VFM
    return VFM(field_sizes=list(sizes), embedding_size=4, output=output, device="cpu")


@pytest.mark.parametrize("call", ["elicit_field_exact", "elicitation_curve_field_exact"])
def test_argument_checks_raise_value_error(call):
    m = _cpu_model()
    fn = getattr(m, call)
    pool = torch.tensor([[0, 6, 10], [1, 7, 11], [0, 9, 12]])           # (user, item, format): T = 13
    y = torch.tensor([1.0, 2.0, 3.0])
    kw = dict(strategies=("variance",)) if call == "elicitation_curve_field_exact" else {}
    with pytest.raises(ValueError, match="'reg'"):
        getattr(_cpu_model("class"), call)(pool, torch.tensor([1.0, 0.0, 1.0]), 2, **kw)
    for bad in (0, 0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="kl_weight"):
            fn(pool, y, 2, kl_weight=bad, **kw)
    with pytest.raises(ValueError, match="at least two fields"):
        getattr(_cpu_model(sizes=(6,)), call)(torch.tensor([[0], [1]]), y[:2], 2, **kw)
    with pytest.raises(ValueError, match="hold ids of the ranked field's range"):
        fn(torch.tensor([[0, 3, 10]]), y[:1], 2, **kw)      # a respondent id in a context column: it would not be frozen
    with pytest.raises(ValueError, match="history X: context columns hold ids"):
        fn(pool, y, 2, history=(torch.tensor([[0, 2, 10]]), torch.tensor([1.0])), **kw)
    for bad in (-1, 3, 1.0, True):
        with pytest.raises(ValueError, match="field must be"):
            fn(pool, y, 2, field=bad, **kw)
    for bad in (0, 3, -1, True):
        with pytest.raises(ValueError, match="key_field"):
            fn(pool, y, 2, field=0, key_field=bad, **kw)
    for bad in (-1, 4097):
        with pytest.raises(ValueError, match="n_questions"):
            fn(pool, y, bad, **kw)
    with pytest.raises(ValueError, match=r"\[R, 3\]"):
        fn(torch.tensor([[0, 6]]), y[:1], 2, **kw)
    with pytest.raises(ValueError, match="context ids must lie"):
        fn(torch.tensor([[0, 6, 13]]), y[:1], 2, **kw)
    with pytest.raises(ValueError, match="one value"):
        fn(pool, y[:2], 2, **kw)
    with pytest.raises(ValueError, match="without a pool row"):
        fn(pool, y, 2, history=(torch.tensor([[2, 6, 10]]), torch.tensor([1.0])), **kw)
    if call == "elicit_field_exact":
        with pytest.raises(ValueError, match="strategy"):
            fn(pool, y, 2, strategy="thompson")
        with pytest.raises(ValueError, match="class"):
            fn(pool, y, 2, strategy="mean")                 # 'mean' needs a 'class' model, the exact session a 'reg' one
        with pytest.raises(TypeError):
            fn(pool, y, 2, n_steps=5)                       # nothing of Adam's is left to choose
    else:
        with pytest.raises(ValueError, match="strategy"):
            fn(pool, y, 2, strategies=("variance", "thompson"))
        with pytest.raises(ValueError, match="write"):
            fn(pool, y, 2, strategies=("variance",), write=True)


def test_cpu_model_fails_loudly():
    from vae_amd._lib import VfmLibraryError
    m = _cpu_model()
    pool, y = torch.tensor([[0, 6, 10], [1, 7, 11]]), torch.tensor([1.0, 2.0])
    with pytest.raises(VfmLibraryError, match="MI355X"):
        m.elicit_field_exact(pool, y, 2)
    with pytest.raises(VfmLibraryError, match="MI355X"):
        m.elicitation_curve_field_exact(pool, y, 2)
    with pytest.raises(VfmLibraryError, match="MI355X"):
        _cpu_model(sizes=(6, 4)).elicit_field_exact(torch.tensor([[0, 6], [1, 7]]), y, 2)     # a two-field model

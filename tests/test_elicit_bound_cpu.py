"""CPU: the bound field-form elicitation session (include/vfm_bound.h: vfm_elicit_bound_f32, VFM.elicit_field_bound) --
the ValueErrors of check_args_field_bound and of the curves, the header, the exports, the struct mirror against gcc's
layout, the workspace formula and its rejections, every VFM_E_INVALID code of the raw entry (checked before any HIP
call, so they run without a device), and the restatement tests/elicit_bound_restatement.py itself: B_e never up inside
a fold, the restated session equal to the restated composition, and the conditioning of the GPU fp64 test's inputs."""
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

import elicit_bound_restatement as RB  # noqa: E402
import solve_reference as SR  # noqa: E402
from test_foldin_cpu import _cpu_model  # noqa: E402

HDR = os.path.join(ROOT, "include", "vfm_bound.h")


# ---------------------------------------------------------------------------------------------------------------------
# the Python layer
# ---------------------------------------------------------------------------------------------------------------------
def _class_model(**kw):
    return _cpu_model("class", field_sizes=kw.pop("field_sizes", [6, 4, 3]), **kw)


POOL = torch.tensor([[0, 6, 10], [0, 7, 11], [1, 8, 12], [1, 9, 10]])
Y = torch.tensor([1.0, 0.0, 1.0, 1.0])


def test_check_args_field_bound_raises_before_a_gpu_is_needed():
    from vae_amd import elicit
    m = _class_model()
    ok = lambda **kw: elicit.check_args_field_bound(m, kw.pop("pool", POOL), kw.pop("y", Y), kw.pop("Q", 2), 0,
                                                    kw.pop("strategy", "mean"), kw.pop("history", None),
                                                    kw.pop("kl_weight", 1.0), kw.pop("n_iters", 8), None)
    x, y, hx, hy, code, field, kf = ok()
    assert x.shape == (4, 3) and hx is None and field == 0 and kf == 1
    for s in ("top", "variance", "mean", "random"):
        ok(strategy=s)
    with pytest.raises(ValueError, match="'class'"):
        elicit.check_args_field_bound(_cpu_model("reg", field_sizes=[6, 4, 3]), POOL, Y, 2, 0, "variance", None, 1.0, 8, None)
    with pytest.raises(ValueError, match="'class'"):
        _cpu_model("reg", field_sizes=[6, 4, 3]).elicit_field_bound(POOL, Y, 2)
    for klw in (0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="kl_weight"):
            ok(kl_weight=klw)
    for n in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="n_iters"):
            ok(n_iters=n)
    with pytest.raises(ValueError, match="0 and 1"):
        ok(y=torch.tensor([1.0, 0.5, 1.0, 0.0]))
    with pytest.raises(ValueError, match="0 and 1"):
        ok(history=(POOL[:2], torch.tensor([2.0, 0.0])))
    ok(history=(POOL[:2], torch.tensor([1.0, 0.0])))
    with pytest.raises(ValueError, match="two fields"):
        elicit.check_args_field_bound(_cpu_model("class", field_sizes=[6]), torch.tensor([[0]]), torch.tensor([1.0]), 1, 0,
                                      "variance", None, 1.0, 8, None)
    with pytest.raises(ValueError, match="xi"):
        ok(strategy="design")
    with pytest.raises(ValueError, match="strategy"):
        ok(strategy="best")
    with pytest.raises(ValueError, match="n_questions"):
        ok(Q=-1)
    with pytest.raises(ValueError, match="lds_dim"):
        elicit.run_field_bound(m, POOL, Y, 2, lds_dim=-2)


def test_curves_refuse_design_and_bound_with_exact():
    m = _class_model()
    with pytest.raises(ValueError, match="xi"):
        m.elicitation_curve_field_bound(POOL, Y, 2, strategies=("design",))
    with pytest.raises(ValueError, match="xi"):
        m.elicitation_ranking_curve_field(POOL, Y, 2, 0, POOL, Y, 1, strategies=("design",), bound=True)
    with pytest.raises(ValueError, match="bound=True and exact=True"):
        m.elicitation_ranking_curve_field(POOL, Y, 2, 0, POOL, Y, 1, bound=True, exact=True)
    with pytest.raises(ValueError, match="sets write"):
        m.elicitation_curve_field_bound(POOL, Y, 2, write=True)


def test_cpu_model_fails_loudly():
    from vae_amd._lib import VfmLibraryError
    with pytest.raises(VfmLibraryError, match="MI355X"):
        _class_model().elicit_field_bound(POOL, Y, 2, strategy="mean")


def test_docstrings_call_n_iters_untuned():
    from vae_amd.model import VFM
    for fn in (VFM.elicit_field_bound, VFM.elicitation_curve_field_bound, VFM.elicitation_ranking_curve_field):
        assert "untuned starting value" in " ".join(fn.__doc__.split())


# ---------------------------------------------------------------------------------------------------------------------
# the ABI
# ---------------------------------------------------------------------------------------------------------------------
def _header_fields(name):
    text = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names = decl.split(",")
            fields.append(re.findall(r"\w+", names[0])[-1])
            fields += [re.findall(r"\w+", n)[-1] for n in names[1:]]
    return fields


def test_header_exports_and_struct_mirror_match_gcc(tmp_path):
    from vae_amd import _lib
    hdr = open(HDR).read()
    assert '#include "vfm_elicit.h"' in hdr
    lib = _lib.load()
    for name in _lib.ELICIT_BOUND_EXPORTS:
        getattr(lib, name)
        assert name in hdr
    fields = _header_fields("vfm_elicit_bound_t")
    assert fields == [n for n, _ in _lib.ElicitBound._fields_]           # every field, in order
    solve = [n for n, _ in _lib.ElicitSolve._fields_]
    assert [f for f in fields if f in solve] == solve and [f for f in fields if f not in solve] == ["n_iters"]
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vfm_bound.h"', "int main(void) {",
             'printf("S %zu\\n", sizeof(vfm_elicit_bound_t));']
    lines += [f'printf("F {n} %zu\\n", offsetof(vfm_elicit_bound_t, {n}));' for n in fields]
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
            assert C.sizeof(_lib.ElicitBound) == int(t[1])
        else:
            assert getattr(_lib.ElicitBound, t[1]).offset == int(t[2]), t[1]
            seen += 1
    assert seen == len(fields)
    e = _lib.ElicitBound()
    assert (e.struct_size, e.abi_version) == (C.sizeof(_lib.ElicitBound), _lib.ABI_VERSION)
    with pytest.raises(AttributeError):
        e.n_steps = 1                                       # (the Adam session's field)


def test_workspace_formula():
    """the exact session's parts | n_ops doubles of c_var | H + U Q doubles of row weights | the slabs, each part rounded
    up to 256 bytes."""
    from vae_amd import _lib
    lib = _lib.load()
    w, solve = lib.vfm_elicit_bound_workspace_bytes, lib.vfm_elicit_solve_workspace_bytes
    ru = lambda v: (v + 255) // 256 * 256
    tri = lambda m: m * (m + 1) // 2
    # U = 3, P = 100, H = 9, 7 contexts, d = 5 (lane shape 8 x 1), Q = 6, written out
    base = ru(100) + ru(7 * 20 * 4) + ru(7 * 2 * 4) + ru(7 * 24 * 4) + ru(7 * 2 * 4) + ru(7 * 15 * 8) + ru(7 * 8)
    assert w(3, 100, 9, 7, 5, 6, -1) == base + ru(7 * 8) + ru((9 + 3 * 6) * 8)
    assert w(3, 100, 9, 7, 5, 6, 0) == base + ru(7 * 8) + ru((9 + 3 * 6) * 8) + 3 * ru(tri(6) * 8)
    for U, P, H, n_ops, d, Q, lds_dim in [(10, 77, 0, 7, 128, 20, -1), (10, 77, 31, 7, 128, 20, 4), (10_000, 5, 3, 3, 128, 1, 4),
                                          (3, 0, 0, 0, 512, 0, -1), (3, 1000, 50, 33, SR.LDS, 6, -1),
                                          (3, 1000, 50, 33, SR.LDS - 1, 6, -1), (0, 0, 0, 0, 1, 0, -1), (2, 9, 4, 3, 8, 4096, 0)]:
        parts = solve(0, P, n_ops, d, lds_dim)                              # (U = 0: no slabs)
        slabs = solve(U, P, n_ops, d, lds_dim) - parts
        assert slabs == (min(U, SR.SLABS) * ru(SR.tri(d + 1) * 8) if SR.has_slabs(d, lds_dim) else 0)
        assert w(U, P, H, n_ops, d, Q, lds_dim) == parts + ru(n_ops * 8) + ru((H + U * Q) * 8) + slabs
    for bad in [(-1, 1, 1, 1, 8, 1, -1), (1, -1, 1, 1, 8, 1, -1), (1, 1, -1, 1, 8, 1, -1), (1, 1, 1, -1, 8, 1, -1),
                (1, 1, 1, 1, 0, 1, -1), (1, 1, 1, 1, 513, 1, -1), (1, 1, 1, 1, 8, -1, -1), (1, 1, 1, 1, 8, 4097, -1),
                (1, 1, 1, 1, 8, 1, -2)]:
        assert w(*bad) == _lib._gen.VFM_E_INVALID, bad


def _valid(lib_mod):
    """A struct that passes every value check and fails only on its (missing) pointers."""
    e = lib_mod.ElicitBound()
    e.T, e.F, e.d, e.field, e.key_col, e.U, e.P, e.H, e.n_ops = 10, 3, 4, 0, 1, 1, 2, 0, 2
    e.n_rounds, e.strategy, e.lds_dim, e.kl_weight, e.n_iters = 3, 1, -1, 1.0, 8
    return e


REFUSALS = [  # (field, value), .., -> a word of vfm_last_error(): vfm_elicit_solve_f32's, and n_iters
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
    ([("n_iters", 0)], b"n_iters"), ([("n_iters", -3)], b"n_iters"),
]


@pytest.mark.parametrize("sets,word", REFUSALS, ids=["-".join(f"{k}={v}" for k, v in s) for s, _ in REFUSALS])
def test_library_refuses_bad_values_before_any_hip_call(sets, word):
    from vae_amd import _lib
    lib = _lib.load()
    e = _valid(_lib)
    assert lib.vfm_elicit_bound_f32(C.byref(e), None) == -1 and b"null pointer" in lib.vfm_last_error()
    for k, v in sets:
        setattr(e, k, v)
    assert lib.vfm_elicit_bound_f32(C.byref(e), None) == _lib._gen.VFM_E_INVALID
    assert word in lib.vfm_last_error(), lib.vfm_last_error()


def test_library_refuses_struct_pointers_and_workspace():
    """The pointer checks see only whether a pointer is NULL: the fake non-NULL values below are never followed, since
    every call is refused before any HIP call."""
    from vae_amd import _lib
    lib = _lib.load()
    INV = _lib._gen.VFM_E_INVALID
    f = lib.vfm_elicit_bound_f32
    assert f(None, None) == INV and b"NULL argument struct" in lib.vfm_last_error()
    e = _valid(_lib)
    e.struct_size -= 8
    assert f(C.byref(e), None) == INV and b"struct_size" in lib.vfm_last_error()
    e = _valid(_lib)
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
    need = lib.vfm_elicit_bound_workspace_bytes(e.U, e.P, e.H, e.n_ops, e.d, e.n_rounds, e.lds_dim)
    assert need > 0
    e.workspace, e.workspace_bytes = 4096, need - 1
    assert f(C.byref(e), None) == INV and b"too small" in lib.vfm_last_error()
    e.workspace, e.workspace_bytes = None, need
    assert f(C.byref(e), None) == INV and b"too small" in lib.vfm_last_error()
    e.workspace, e.workspace_bytes = 4096 + 64, need
    assert f(C.byref(e), None) == INV and b"aligned" in lib.vfm_last_error()
    e = _valid(_lib)
    e.U = 0
    assert f(C.byref(e), None) == 0                         # nothing to do, nothing launched


# ---------------------------------------------------------------------------------------------------------------------
# the restatement, in fp64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sessions():
    return {name: RB.case_sessions(RB.case(name)) for name in RB.CASES}


@pytest.mark.parametrize("name", sorted(RB.CASES))
def test_bound_never_up_inside_a_fold(sessions, name):
    """Inside every fold of a restated session B_e is non-increasing over the rounds, the start included: each block
    is the exact minimiser of its block.  (Between two folds a row is appended and the start is rounded to fp32: another
    objective, nothing to compare.)"""
    folds = 0
    for s in sessions[name]:
        for B in s["B"]:
            if B is None:
                continue
            assert len(B) == RB.CASES[name][7] + 1
            assert bool((np.diff(B) <= 1e-12 * np.abs(B[:-1])).all()), (name, s["entity"], B)
            folds += 1
    assert folds == RB.CASE_RESPONDENTS * RB.CASE_ROUNDS      # (8-row pools: no session runs out in 6 rounds)


@pytest.mark.parametrize("name", sorted(RB.CASES))
def test_restated_session_equals_restated_composition(sessions, name):
    c = RB.case(name)
    ent, bia, scal = (c[k].numpy() for k in ("ent", "bia", "scal"))
    pool, yp, hx, hy = (c[k].numpy() for k in ("pool", "y_pool", "hist_x", "hist_y"))
    for s in sessions[name][:3]:
        rows, thetas = RB.composition(s["entity"], pool[s["sel"]], yp[s["sel"]], RB.CASE_ROUNDS, c["strategy"], ent, bia,
                                      scal, c["field"], c["link"], hx[s["hist"]], hy[s["hist"]], c["kl_weight"],
                                      c["n_iters"], c["reset"])
        assert rows == s["rows"]
        for a, b in zip(thetas, s["theta"]):
            for u, v in zip(a, b):
                assert np.array_equal(np.asarray(u, np.float64), np.asarray(v, np.float64))


def test_a_pool_that_runs_out_and_an_empty_one():
    c = RB.case("d5")
    ent, bia, scal = (c[k].numpy() for k in ("ent", "bia", "scal"))
    pool, yp = c["pool"].numpy()[:3], c["y_pool"].numpy()[:3]
    e = int(pool[0, 0])
    s = RB.session(e, pool, yp, 5, "mean", ent, bia, scal, kind="abs", n_iters=2)
    assert sorted(s["rows"][:3]) == [0, 1, 2] and s["rows"][3:] == [-1, -1]
    assert np.isnan(s["score"][3]) and s["B"][3] is None and s["theta"][4] is s["theta"][2]
    rows, _ = RB.composition(e, pool, yp, 5, "mean", ent, bia, scal, 0, "abs", [], [], 1.0, 2, False)
    assert rows == s["rows"]
    z = RB.session(e, pool[:0], yp[:0], 2, "mean", ent, bia, scal)
    assert z["rows"] == [-1, -1]


# ---------------------------------------------------------------------------------------------------------------------
# the inputs of the GPU fp64 test
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(RB.CASES))
def test_gpu_fp64_cases_are_well_conditioned(sessions, name):
    """cond <= 1e3 of every matrix factored in every inner round of every fold: the condition test_foldin_bound_cpu.py
    puts on the bound fold-in's own cases.  The systems of a case cover both forms where its d allows."""
    c = RB.case(name)
    assert set(c["y_pool"].tolist()) <= {0.0, 1.0} and set(c["hist_y"].tolist()) <= {0.0, 1.0}
    worst = max(v for s in sessions[name] for v in s["cond"])
    forms = {n <= c["d"] for s in sessions[name] for n in s["n"]}
    print(f"{name}: worst cond over the folds' rounds {worst:.1f}; dual / primal {sorted(forms)}")
    assert worst <= 1e3
    assert forms == ({True, False} if name == "d5" else {True})

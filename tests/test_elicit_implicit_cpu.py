"""CPU: the implicit elicitation session (VFM.elicit_field_implicit, include/vfm_elicit_implicit.h) before anything needs
a GPU -- the fp64 restatement of tests/elicit_implicit_restatement.py (every round's theta is stationary for the dense
brute-force J_imp to 1e-9, implicit_reference's bound; the planted cases keep every round's choice GAP_FLOOR apart and a
float32 numpy run asks the same rows), the header and the ctypes mirror against gcc, the workspace formula, every
VFM_E_INVALID of the entry point, and the ValueErrors / TypeErrors of the Python surface."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

import elicit_implicit_restatement as EI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "vfm_elicit_implicit.h")


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted():
    out = {}
    for name in EI.PLANTED:
        case = EI.planted_case(name)
        out[name] = (case, EI.planted_sessions(name, case))
    return out


def test_planted_cases_cover_what_they_should():
    specs = list(EI.PLANTED.values())
    assert {s[4] for s in specs} == {5, 16} and {s[0] for s in specs} == {"abs", "softplus"}
    assert any(s[3] > 0 for s in specs) and any(s[5] for s in specs) and {s[2] for s in specs} == {0, 1}
    assert EI.RESPONDENTS == 8 and EI.ROUNDS == 6


@pytest.mark.parametrize("name", sorted(EI.PLANTED))
def test_every_rounds_theta_is_stationary_for_brute_force_J_imp(planted, name):
    case, sessions = planted[name]
    assert len(sessions) == EI.RESPONDENTS
    worst = 0.0
    for s in sessions:
        assert min(s["rows"]) >= 0 and len(set(s["rows"])) == EI.ROUNDS
        for q in range(EI.ROUNDS):
            assert s["fold_x"][q].shape[0] == len(s["hist"]) + q + 1          # history, then the rows asked so far
            worst = max(worst, EI.block_gradient(case, s, q))
    print(name, "worst block gradient", worst)
    assert worst <= 1e-9


@pytest.mark.parametrize("name", sorted(EI.PLANTED))
def test_planted_cases_keep_the_choices_apart_in_fp64_and_fp32(planted, name):
    case, s64 = planted[name]
    gap = min(min(s["gap"]) for s in s64)
    print(name, "smallest relative gap", gap)
    assert gap >= EI.GAP_FLOOR                               # a condition on the generator's seed, not a measurement
    s32 = EI.planted_sessions(name, case, f32=True)
    for a, b in zip(s64, s32):
        assert a["rows"] == b["rows"], a["entity"]


def test_no_answer_optimum_is_not_the_prior():
    """The base-only optimum of a respondent without rows: every partner a pair of target 0."""
    case = EI.planted_case("d5_abs")
    solve = EI.make_solve64(case["N"], case["M"], EI.W0, EI.W1)
    E, B, S = (case[k].astype("float64") for k in ("ent", "bia", "scal"))
    (mu, s, mw, sw), _ = solve(0, torch.zeros(0, 2, dtype=torch.int64).numpy(), [], E, B, S, 0, "abs", 1.0)
    assert abs(mw) > 1e-3 and float(abs(s).max()) < 1.0      # pulled towards pred = 0, scales below the prior's 1


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI without a device
# ---------------------------------------------------------------------------------------------------------------------
def test_exports_and_struct_mirror_match_gcc(tmp_path):
    from vae_amd import _lib
    lib = _lib.load()
    for name in _lib.ELICIT_IMPLICIT_EXPORTS:
        getattr(lib, name)
    assert _lib.ABI_VERSION == 5                            # additions only
    text = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    body = re.search(r"typedef struct vfm_elicit_implicit_t \{(.*?)\} vfm_elicit_implicit_t;", text, re.S).group(1)
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            fields += [re.findall(r"\w+", n)[-1] for n in decl.split(",")]
    assert fields == ["w0", "w1", "lo", "n", "base"] == [n for n, _ in _lib.ElicitImplicit._fields_]
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vfm_elicit_implicit.h"', "int main(void) {",
             'printf("S %zu\\n", sizeof(vfm_elicit_implicit_t));']
    lines += [f'printf("F {n} %zu\\n", offsetof(vfm_elicit_implicit_t, {n}));' for n in fields]
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
            assert C.sizeof(_lib.ElicitImplicit) == int(t[1])
        else:
            assert getattr(_lib.ElicitImplicit, t[1]).offset == int(t[2]), t[1]
            seen += 1
    assert seen == len(fields)
    with pytest.raises(AttributeError):
        _lib.ElicitImplicit().weights = 1                   # (no per-answer weights in a session)


def test_workspace_function():
    from vae_amd import _lib
    lib = _lib.load()
    w = lib.vfm_elicit_implicit_workspace_bytes
    tri = lambda m: m * (m + 1) // 2
    ru = lambda v: (v + 255) // 256 * 256
    # flags [P]; the score's operands [7, 4 d] floats and constants [7, 2]: no operand block of the fold
    base = ru(100) + ru(7 * 20 * 4) + ru(7 * 2 * 4)
    assert w(3, 100, 7, 5, -1) == base                       # d + 1 = 6 fits in LDS: no slabs
    assert w(3, 100, 7, 5, 6) == base and w(3, 100, 7, 5, 200) == base
    assert w(3, 100, 7, 5, 5) == base + 3 * ru(tri(6) * 8)   # m = d + 1 whatever the rows: one slab per workgroup
    assert w(300, 100, 7, 5, 0) == base + _lib.FOLDIN_SOLVE_SLABS * ru(tri(6) * 8)       # the grid cap
    assert w(2, 0, 0, 134, -1) == ru(1) and w(2, 0, 0, 135, -1) == ru(1) + 2 * ru(tri(136) * 8)     # the LDS edge
    assert w(0, 0, 0, 1, -1) == 256
    assert w(9, 40, 11, 128, -1) < lib.vfm_elicit_solve_workspace_bytes(9, 40, 11, 128, -1)
    for bad in ((-1, 1, 1, 8, -1), (1, -1, 1, 8, -1), (1, 1, -1, 8, -1), (1, 1, 1, 0, -1), (1, 1, 1, 513, -1),
                (1, 1, 1, 8, -2)):
        assert w(*bad) == _lib._gen.VFM_E_INVALID, bad


def _valid(lib_mod):
    """A struct pair that passes every value check and fails only on its (missing) pointers."""
    e = lib_mod.ElicitSolve()
    e.T, e.F, e.d, e.field, e.key_col, e.U, e.P, e.H, e.n_ops = 10, 2, 4, 0, 1, 1, 2, 0, 2
    e.n_rounds, e.strategy, e.lds_dim, e.kl_weight = 3, 1, -1, 1.0
    i = lib_mod.ElicitImplicit()
    i.w0, i.w1, i.lo, i.n, i.base = 0.1, 1.0, 6, 4, 4096   # (a fake non-NULL pointer: never followed)
    return e, i


REFUSALS = [  # ("p" / "imp", field, value) -> a word of vfm_last_error()
    (("p", "F", 1), b"F out of range"), (("p", "F", 3), b"two-field"), (("p", "F", 65), b"F out of range"),
    (("p", "field", -1), b"field out of range"), (("p", "field", 2), b"field out of range"),
    (("p", "key_col", -1), b"key_col"), (("p", "key_col", 2), b"key_col"), (("p", "key_col", 0), b"key_col"),
    (("p", "d", 0), b"d out of range"), (("p", "d", 513), b"d out of range"),
    (("p", "U", -1), b"U < 0"), (("p", "P", -1), b"P < 0"), (("p", "H", -1), b"H < 0"), (("p", "T", 0), b"T < 1"),
    (("p", "n_rounds", 4097), b"n_rounds"), (("p", "n_rounds", -1), b"n_rounds"),
    (("p", "strategy", 4), b"strategy"), (("p", "strategy", -1), b"strategy"),
    (("p", "flags", 1), b"flags"), (("p", "flags", 16 | 32), b"flags"),
    (("p", "n_ops", 0), b"n_ops"), (("p", "n_ops", -1), b"n_ops"), (("p", "lds_dim", -2), b"lds_dim"),
    (("p", "kl_weight", 0.0), b"kl_weight"), (("p", "kl_weight", -1.0), b"kl_weight"),
    (("p", "kl_weight", float("nan")), b"kl_weight"), (("p", "kl_weight", float("inf")), b"kl_weight"),
    (("p", "out_mean", 256), b"out_mean"), (("p", "out_var", 256), b"out_mean"),
    (("imp", "w0", 0.0), b"w0"), (("imp", "w0", -0.1), b"w0"), (("imp", "w0", float("nan")), b"w0"),
    (("imp", "w0", float("inf")), b"w0"), (("imp", "w1", 0.05), b"w1"), (("imp", "w1", float("nan")), b"w1"),
    (("imp", "w1", float("inf")), b"w1"),
    (("imp", "n", 0), b"partner range"), (("imp", "n", -1), b"partner range"), (("imp", "lo", -1), b"partner range"),
    (("imp", "lo", 7), b"partner range"), (("imp", "n", 5), b"partner range"), (("imp", "lo", 11), b"partner range"),
    (("imp", "base", None), b"base"),
]


@pytest.mark.parametrize("what,word", REFUSALS, ids=[f"{w[0]}.{w[1]}={w[2]}" for w, _ in REFUSALS])
def test_library_refuses_bad_values_before_any_hip_call(what, word):
    from vae_amd import _lib
    lib = _lib.load()
    e, i = _valid(_lib)
    f = lib.vfm_elicit_implicit_f32
    assert f(C.byref(e), C.byref(i), None, None) == -1 and b"null pointer" in lib.vfm_last_error()
    setattr(e if what[0] == "p" else i, what[1], what[2])
    assert f(C.byref(e), C.byref(i), None, None) == _lib._gen.VFM_E_INVALID
    assert word in lib.vfm_last_error(), lib.vfm_last_error()


def test_library_refuses_struct_pointers_and_workspace():
    """The pointer checks see only whether a pointer is NULL: the fake non-NULL values are never followed, since every
    call is refused before any HIP call."""
    from vae_amd import _lib
    lib = _lib.load()
    INV = _lib._gen.VFM_E_INVALID
    f = lib.vfm_elicit_implicit_f32
    e, i = _valid(_lib)
    assert f(None, C.byref(i), None, None) == INV and b"NULL argument struct" in lib.vfm_last_error()
    assert f(C.byref(e), None, None, None) == INV and b"NULL vfm_elicit_implicit_t" in lib.vfm_last_error()
    e.struct_size -= 8
    assert f(C.byref(e), C.byref(i), None, None) == INV and b"struct_size" in lib.vfm_last_error()
    e.struct_size += 8
    e.abi_version += 1
    assert f(C.byref(e), C.byref(i), None, None) == INV and b"abi_version" in lib.vfm_last_error()
    e, i = _valid(_lib)
    call = lambda: f(C.byref(e), C.byref(i), None, None)
    tables = ("entities", "pool_ptr", "pool_x", "pool_y", "entity_params", "bias_params", "scalars", "out_row",
              "out_score", "out_loss")
    for name in tables:
        setattr(e, name, 4096)
    for name in tables:                                     # each one missing in turn
        setattr(e, name, None)
        assert call() == INV and b"null pointer" in lib.vfm_last_error(), name
        setattr(e, name, 4096)
    assert call() == INV and b"op_x" in lib.vfm_last_error()
    e.op_x = 4096
    assert call() == INV and b"op_x" in lib.vfm_last_error()             # (pool_op)
    e.pool_op = 4096
    e.H = 1
    assert call() == INV and b"null pointer" in lib.vfm_last_error()     # (history)
    e.hist_ptr = e.hist_x = e.hist_y = 4096
    assert call() == INV and b"hist_op" in lib.vfm_last_error()
    e.H = 0
    need = lib.vfm_elicit_implicit_workspace_bytes(e.U, e.P, e.n_ops, e.d, e.lds_dim)
    assert need > 0
    assert call() == INV and b"workspace too small" in lib.vfm_last_error()
    e.workspace, e.workspace_bytes = 4096, need - 1
    assert call() == INV and b"workspace too small" in lib.vfm_last_error()
    e.lds_dim = 0                                           # slabs: the same bytes no longer suffice
    e.workspace_bytes = need
    assert call() == INV and b"workspace too small" in lib.vfm_last_error()
    e.lds_dim = -1
    e.workspace, e.workspace_bytes = 4096 + 64, need
    assert call() == INV and b"256-byte aligned" in lib.vfm_last_error()


def test_no_respondents_is_a_no_op():
    from vae_amd import _lib
    lib = _lib.load()
    e, i = _valid(_lib)
    e.U = e.P = e.n_ops = 0
    assert lib.vfm_elicit_implicit_f32(C.byref(e), C.byref(i), None, None) == 0    # nothing to do, nothing launched


# ---------------------------------------------------------------------------------------------------------------------
# the Python entry points without a GPU
# ---------------------------------------------------------------------------------------------------------------------
def _cpu_model(output="reg", sizes=(6, 4)):
    from vae_amd.model import VFM
    return VFM(field_sizes=list(sizes), embedding_size=4, output=output, device="cpu")


def test_argument_checks_raise_before_a_gpu_is_needed():
    from vae_amd import elicit, sweep
    m = _cpu_model()
    fn = m.elicit_field_implicit
    pool = torch.tensor([[0, 6], [1, 7], [0, 9]])           # (user, item): T = 10
    y = torch.tensor([1.0, 1.0, 1.0])
    with pytest.raises(TypeError):
        fn(pool, y, 2)                                      # w0 has no default
    with pytest.raises(TypeError):
        fn(pool, y, 2, 0, 0.1)                              # ... and is keyword-only
    with pytest.raises(TypeError, match="GroupPriors"):
        fn(pool, y, 2, w0=0.1, priors=None)
    with pytest.raises(ValueError, match="GroupPriors"):
        fn(pool, y, 2, w0=0.1, priors=(0, 1))
    with pytest.raises(ValueError, match="priors are for"):
        fn(pool, y, 2, w0=0.1, priors=sweep.GroupPriors(2, 5))
    with pytest.raises(ValueError, match="'reg'"):
        _cpu_model("class").elicit_field_implicit(pool, y, 2, w0=0.1)
    with pytest.raises(ValueError, match="two-field"):
        _cpu_model(sizes=(6, 4, 3)).elicit_field_implicit(torch.tensor([[0, 6, 10]]), y[:1], 2, w0=0.1)
    for bad in (0, 0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="kl_weight"):
            fn(pool, y, 2, w0=0.1, kl_weight=bad)
    for bad in (0.0, -0.1, 1e-50):                          # (1e-50 rounds to 0 in fp32)
        with pytest.raises(ValueError, match="w0 must be > 0"):
            fn(pool, y, 2, w0=bad)
    with pytest.raises(ValueError, match="w1 must be >= w0"):
        fn(pool, y, 2, w0=0.5, w1=0.25)
    for kw in (dict(w0=float("nan")), dict(w0=float("inf")), dict(w0=0.1, w1=float("nan")), dict(w0=0.1, w1=1e39)):
        with pytest.raises(ValueError, match="finite"):
            fn(pool, y, 2, **kw)
    with pytest.raises(ValueError, match="hold ids of the ranked field's range"):
        fn(torch.tensor([[0, 3]]), y[:1], 2, w0=0.1)        # a respondent id in the partner column
    with pytest.raises(ValueError, match="context ids must lie"):
        fn(torch.tensor([[0, 10]]), y[:1], 2, w0=0.1)
    with pytest.raises(ValueError):
        fn(torch.tensor([[7, 6]]), y[:1], 2, w0=0.1)        # a respondent outside its field
    with pytest.raises(ValueError, match="duplicate"):
        fn(torch.tensor([[0, 6], [0, 6]]), y[:2], 2, w0=0.1)
    with pytest.raises(ValueError, match="duplicate"):      # ... pool and history together
        fn(pool, y, 2, w0=0.1, history=(torch.tensor([[0, 9]]), torch.tensor([1.0])))
    with pytest.raises(ValueError, match="without a pool row"):
        fn(pool, y, 2, w0=0.1, history=(torch.tensor([[2, 6]]), torch.tensor([1.0])))
    with pytest.raises(ValueError, match="class"):
        fn(pool, y, 2, w0=0.1, strategy="mean")
    with pytest.raises(ValueError, match="design"):
        fn(pool, y, 2, w0=0.1, strategy="design")
    with pytest.raises(ValueError, match="strategy"):
        fn(pool, y, 2, w0=0.1, strategy="thompson")
    for bad in (-1, 2, 1.0, True):
        with pytest.raises(ValueError, match="field must be"):
            fn(pool, y, 2, field=bad, w0=0.1)
    for bad in (-1, 4097):
        with pytest.raises(ValueError, match="n_questions"):
            fn(pool, y, bad, w0=0.1)
    with pytest.raises(ValueError, match="chunk_rows"):
        fn(pool, y, 2, w0=0.1, chunk_rows=0)
    with pytest.raises(ValueError, match="lds_dim"):
        fn(pool, y, 2, w0=0.1, lds_dim=-2)
    with pytest.raises(TypeError):
        fn(pool, y, 2, w0=0.1, weights=torch.ones(3))       # per-answer weights are not built
    assert elicit.SESSION_KINDS["implicit"]["runner"] == "run_field_implicit"
    assert elicit._kind_of(elicit.run_field_implicit) == "implicit"


def test_ranking_curve_argument_checks():
    m = _cpu_model()
    pool, y = torch.tensor([[0, 6], [1, 7], [0, 9]]), torch.tensor([1.0, 1.0, 1.0])
    X, yt = torch.tensor([[0, 8], [1, 8]]), torch.tensor([5.0, 5.0])
    fn = lambda **kw: m.elicitation_ranking_curve_field(pool, y, 2, 0, X, yt, 1, **kw)
    with pytest.raises(ValueError, match="excludes"):
        fn(implicit=True, exact=True, w0=0.1)
    with pytest.raises(ValueError, match="excludes"):
        fn(implicit=True, bound=True, w0=0.1)
    with pytest.raises(ValueError, match="needs w0"):
        fn(implicit=True)
    with pytest.raises(ValueError, match="implicit=True"):
        fn(exact=True, w0=0.1)
    with pytest.raises(ValueError, match="design"):
        fn(implicit=True, w0=0.1, strategies=("design",))
    with pytest.raises(TypeError, match="GroupPriors"):
        fn(implicit=True, w0=0.1, priors=None)
    with pytest.raises(ValueError, match="w0 must be > 0"):
        fn(implicit=True, w0=-1.0, strategies=("variance",))


def test_cpu_model_fails_loudly():
    from vae_amd._lib import VfmLibraryError
    m = _cpu_model()
    with pytest.raises(VfmLibraryError, match="MI355X"):
        m.elicit_field_implicit(torch.tensor([[0, 6], [1, 7]]), torch.tensor([1.0, 1.0]), 2, w0=0.1)

"""CPU: elicitation sessions in the field form (include/vfm_elicit.h: vfm_elicit_field_f32) -- the library checks every
argument before any HIP call and says which one; the ctypes mirror of vfm_elicit_field_t is laid out as gcc lays out the
header; VFM.elicit_field / elicitation_curve_field / select_next_questions_field raise ValueError before anything needs a
GPU; the two-field entry points keep refusing models with more fields; the fp64 restatement of the field form
(elicit_field_restatement.py) agrees with the two-field restatement on a two-field model and with a brute-force
evaluation of the closed form of vfm_rank.h."""
import ctypes as C
import math
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

import elicit_field_restatement as RF
import elicit_restatement as R

HDR = os.path.join(ROOT, "include", "vfm_elicit.h")


def _header_fields():
    text = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    body = re.search(r"typedef struct vfm_elicit_field_t \{(.*?)\} vfm_elicit_field_t;", text, re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names = decl.split(",")
            fields.append(re.findall(r"\w+", names[0])[-1])
            fields += [re.findall(r"\w+", n)[-1] for n in names[1:]]
    return fields


def test_struct_mirror_matches_gcc(tmp_path):
    from vae_amd import _lib
    fields = _header_fields()
    assert fields == [n for n, _ in _lib.ElicitField._fields_]          # every field, in order
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vfm_elicit.h"', "int main(void) {",
             'printf("S %zu\\n", sizeof(vfm_elicit_field_t));']
    lines += [f'printf("F {n} %zu\\n", offsetof(vfm_elicit_field_t, {n}));' for n in fields]
    lines += ["return 0; }"]
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    seen = 0
    for ln in got:
        t = ln.split()
        if not t:
            continue
        if t[0] == "S":
            assert C.sizeof(_lib.ElicitField) == int(t[1])
        else:
            assert getattr(_lib.ElicitField, t[1]).offset == int(t[2]), t[1]
            seen += 1
    assert seen == len(fields)
    e = _lib.ElicitField()
    assert (e.struct_size, e.abi_version) == (C.sizeof(_lib.ElicitField), _lib.ABI_VERSION)
    with pytest.raises(AttributeError):
        e.key_column = 1                                    # a misspelt field


def test_workspace_function():
    from vae_amd import _lib
    lib = _lib.load()
    w = lib.vfm_elicit_field_workspace_bytes
    # flags [P] -> 256; score operands [7, 4 * 5] floats = 560 -> 768; their constants [7, 2] -> 256
    assert w(100, 7, 5, _lib.OBJ_SAMPLED) == 256 + 768 + 256
    # closed form: plus the fold-in's operands [7, 3, 8] floats = 672 -> 768 and constants -> 256
    assert w(100, 7, 5, _lib.OBJ_CLOSED_FORM) == 256 + 768 + 256 + 768 + 256
    assert w(0, 0, 1, _lib.OBJ_SAMPLED) == 256
    for bad in ((-1, 7, 5, 0), (100, -1, 5, 0), (100, 7, 0, 0), (100, 7, 513, 0), (100, 7, 5, 2)):
        assert w(*bad) < 0, bad


def _valid(lib_mod):
    """A struct that passes every value check and fails only on its (missing) pointers."""
    e = lib_mod.ElicitField()
    e.T, e.F, e.d, e.field, e.key_col, e.U, e.P, e.H, e.n_ops = 10, 3, 4, 0, 1, 1, 2, 0, 2
    e.n_rounds, e.strategy, e.objective, e.likelihood, e.n_steps, e.n_samples = 3, 1, lib_mod.OBJ_SAMPLED, 0, 5, 1
    e.lr, e.kl_weight = 0.05, 1.0
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
    ([("objective", 2)], b"objective"), ([("likelihood", 2)], b"likelihood"),
    ([("objective", 1), ("likelihood", 1)], b"Normal"),
    ([("n_samples", 5)], b"n_samples"), ([("n_samples", 0)], b"n_samples"),
    ([("flags", 1)], b"flags"), ([("flags", 16 | 32)], b"flags"),
    ([("n_steps", -1)], b"n_steps"),
    ([("t0", -1)], b"t0"), ([("t0", 1 << 59)], b"t0"),
    ([("n_ops", 0)], b"n_ops"), ([("n_ops", -1)], b"n_ops"),
    ([("lr", -0.5)], b"lr"), ([("kl_weight", float("nan"))], b"kl_weight"),
    ([("out_mean", 256)], b"out_mean"), ([("out_var", 256)], b"out_mean"),
]


@pytest.mark.parametrize("sets,word", REFUSALS, ids=["-".join(f"{k}={v}" for k, v in s) for s, _ in REFUSALS])
def test_library_refuses_bad_values_before_any_hip_call(sets, word):
    from vae_amd import _lib
    lib = _lib.load()
    e = _valid(_lib)
    assert lib.vfm_elicit_field_f32(C.byref(e), None) == -1 and b"null pointer" in lib.vfm_last_error()
    for k, v in sets:
        setattr(e, k, v)
    assert lib.vfm_elicit_field_f32(C.byref(e), None) == _lib._gen.VFM_E_INVALID
    assert word in lib.vfm_last_error(), lib.vfm_last_error()


def test_library_refuses_struct_pointers_and_workspace():
    """The pointer checks see only whether a pointer is NULL: the fake non-NULL values below are never followed, since
    every call is refused before any HIP call."""
    from vae_amd import _lib
    lib = _lib.load()
    INV = _lib._gen.VFM_E_INVALID
    assert lib.vfm_elicit_field_f32(None, None) == INV and b"NULL argument struct" in lib.vfm_last_error()
    e = _valid(_lib)
    e.struct_size -= 8
    assert lib.vfm_elicit_field_f32(C.byref(e), None) == INV and b"struct_size" in lib.vfm_last_error()
    e.struct_size += 8
    e.abi_version += 1
    assert lib.vfm_elicit_field_f32(C.byref(e), None) == INV and b"abi_version" in lib.vfm_last_error()
    e = _valid(_lib)
    tables = ("entities", "pool_ptr", "pool_x", "pool_y", "entity_params", "bias_params", "scalars", "out_row",
              "out_score", "out_loss")
    for name in tables:
        setattr(e, name, 4096)
    for name in tables:                                     # each one missing in turn
        setattr(e, name, None)
        assert lib.vfm_elicit_field_f32(C.byref(e), None) == INV and b"null pointer" in lib.vfm_last_error(), name
        setattr(e, name, 4096)
    assert lib.vfm_elicit_field_f32(C.byref(e), None) == INV and b"op_x" in lib.vfm_last_error()
    e.op_x = 4096
    assert lib.vfm_elicit_field_f32(C.byref(e), None) == INV and b"op_x" in lib.vfm_last_error()     # (pool_op)
    e.pool_op = 4096
    e.H = 1
    assert lib.vfm_elicit_field_f32(C.byref(e), None) == INV and b"null pointer" in lib.vfm_last_error()   # (history)
    e.hist_ptr = e.hist_x = e.hist_y = 4096
    assert lib.vfm_elicit_field_f32(C.byref(e), None) == INV and b"hist_op" in lib.vfm_last_error()
    e.H = 0
    need = lib.vfm_elicit_field_workspace_bytes(e.P, e.n_ops, e.d, e.objective)
    assert need > 0
    assert lib.vfm_elicit_field_f32(C.byref(e), None) == INV and b"workspace too small" in lib.vfm_last_error()
    e.workspace, e.workspace_bytes = 4096, need - 1
    assert lib.vfm_elicit_field_f32(C.byref(e), None) == INV and b"workspace too small" in lib.vfm_last_error()
    e.workspace, e.workspace_bytes = 4096 + 64, need
    assert lib.vfm_elicit_field_f32(C.byref(e), None) == INV and b"256-byte aligned" in lib.vfm_last_error()


def test_no_respondents_is_a_no_op():
    from vae_amd import _lib
    lib = _lib.load()
    e = _valid(_lib)
    e.U = e.P = e.n_ops = 0
    assert lib.vfm_elicit_field_f32(C.byref(e), None) == 0  # nothing to do, nothing launched


def _cpu_model(output="reg", sizes=(6, 4, 3)):
    from vae_amd.model import VFM
    return VFM(field_sizes=list(sizes), embedding_size=4, output=output, device="cpu")


@pytest.mark.parametrize("call", ["elicit_field", "elicitation_curve_field"])
def test_argument_checks_raise_value_error(call):
    m = _cpu_model()
    fn = getattr(m, call)
    pool = torch.tensor([[0, 6, 10], [1, 7, 11], [0, 9, 12]])           # (user, item, format): T = 13
    y = torch.tensor([1.0, 2.0, 3.0])
    kw = dict(strategies=("variance",)) if call == "elicitation_curve_field" else {}
    for bad in (-1, 3, 1.0, True):
        with pytest.raises(ValueError, match="field must be"):
            fn(pool, y, 2, field=bad, **kw)
    for bad in (0, 3, -1, True):                            # (0 is the folded field itself)
        with pytest.raises(ValueError, match="key_field"):
            fn(pool, y, 2, field=0, key_field=bad, **kw)
    with pytest.raises(ValueError, match="n_questions"):
        fn(pool, y, -1, **kw)
    with pytest.raises(ValueError, match="n_questions"):
        fn(pool, y, 4097, **kw)
    with pytest.raises(ValueError, match=r"\[R, 3\]"):
        fn(torch.tensor([[0, 6]]), y[:1], 2, **kw)          # a two-column pool on a three-field model
    with pytest.raises(ValueError, match="integer ids"):
        fn(pool.float(), y, 2, **kw)
    with pytest.raises(ValueError, match="column 0 must lie"):
        fn(torch.tensor([[6, 7, 10]]), y[:1], 2, **kw)      # an item id in the respondents' column
    with pytest.raises(ValueError, match="context ids must lie"):
        fn(torch.tensor([[0, 6, 13]]), y[:1], 2, **kw)      # a context id past T
    with pytest.raises(ValueError, match="hold ids of the ranked field's range"):
        fn(torch.tensor([[0, 3, 10]]), y[:1], 2, **kw)      # a respondent id in a context column: it would not be frozen
    with pytest.raises(ValueError, match="column 1 must lie"):
        fn(torch.tensor([[0, 0, 10]]), y[:1], 2, field=1, **kw)  # a user id in the items' column
    with pytest.raises(ValueError, match="one value"):
        fn(pool, y[:2], 2, **kw)
    with pytest.raises(ValueError, match="n_samples"):
        fn(pool, y, 2, objective="sampled", n_samples=5, **kw)
    with pytest.raises(ValueError, match="objective"):
        fn(pool, y, 2, objective="exact", **kw)
    with pytest.raises(ValueError, match="n_steps"):
        fn(pool, y, 2, n_steps=-1, **kw)
    with pytest.raises(ValueError, match="lr"):
        fn(pool, y, 2, lr=-0.1, **kw)
    with pytest.raises(ValueError, match="history"):
        fn(pool, y, 2, history=torch.tensor([[0, 6, 10]]), **kw)
    with pytest.raises(ValueError, match=r"history X must be \[R, 3\]"):
        fn(pool, y, 2, history=(torch.tensor([[0, 6]]), torch.tensor([1.0])), **kw)
    with pytest.raises(ValueError, match="history X: context columns hold ids"):
        fn(pool, y, 2, history=(torch.tensor([[0, 2, 10]]), torch.tensor([1.0])), **kw)
    with pytest.raises(ValueError, match="without a pool row"):
        fn(pool, y, 2, history=(torch.tensor([[2, 6, 10]]), torch.tensor([1.0])), **kw)
    with pytest.raises(ValueError, match="one value"):
        fn(pool, y, 2, history=(torch.tensor([[0, 8, 11]]), torch.tensor([1.0, 2.0])), **kw)
    if call == "elicit_field":
        with pytest.raises(ValueError, match="strategy"):
            fn(pool, y, 2, strategy="thompson")
        with pytest.raises(ValueError, match="class"):
            fn(pool, y, 2, strategy="mean")                 # 'mean' on a 'reg' model
    else:
        with pytest.raises(ValueError, match="strategy"):
            fn(pool, y, 2, strategies=("variance", "thompson"))
        with pytest.raises(ValueError, match="class"):
            fn(pool, y, 2)                                  # the default strategies hold 'mean'
        with pytest.raises(ValueError, match="write"):
            fn(pool, y, 2, strategies=("variance",), write=True)
    with pytest.raises(ValueError, match="closed-form"):
        getattr(_cpu_model("class"), call)(pool, torch.tensor([1.0, 0.0, 1.0]), 2, objective="closed_form", **kw)


def test_select_next_questions_field_argument_checks():
    m = _cpu_model()
    pool = torch.tensor([[0, 6, 10], [1, 7, 11]])
    with pytest.raises(ValueError, match="field must be"):
        m.select_next_questions_field(pool, 3)
    with pytest.raises(ValueError, match="key_field"):
        m.select_next_questions_field(pool, 0, key_field=0)
    with pytest.raises(ValueError, match="strategy"):
        m.select_next_questions_field(pool, 0, strategy="thompson")
    with pytest.raises(ValueError, match="class"):
        m.select_next_questions_field(pool, 0, strategy="mean")
    with pytest.raises(ValueError, match="n must be"):
        m.select_next_questions_field(pool, 0, n=0)
    with pytest.raises(ValueError, match="hold ids of the ranked field's range"):
        m.select_next_questions_field(torch.tensor([[0, 3, 10]]), 0)
    with pytest.raises(ValueError, match="column 2 must lie"):
        m.select_next_questions_field(torch.tensor([[0, 6, 9]]), 2)


def test_cpu_model_fails_loudly():
    from vae_amd._lib import VfmLibraryError
    m = _cpu_model()
    pool, y = torch.tensor([[0, 6, 10], [1, 7, 11]]), torch.tensor([1.0, 2.0])
    with pytest.raises(VfmLibraryError, match="MI355X"):
        m.elicit_field(pool, y, 2)
    with pytest.raises(VfmLibraryError, match="MI355X"):
        m.elicitation_curve_field(pool, y, 2, strategies=("variance",))
    with pytest.raises(VfmLibraryError, match="MI355X"):
        m.select_next_questions_field(pool, 0)


def test_two_field_entry_points_still_refuse_three_fields(monkeypatch):
    from vae_amd import ops
    m = _cpu_model()
    # (select_next_questions asks for a GPU model before it looks at F: that check is stepped over here, and the call is
    # refused before anything would touch a device; test_gpu_elicit_field.py makes the same call on a GPU model)
    monkeypatch.setattr(ops, "_need_cuda", lambda t, name: None)
    pool, y = torch.tensor([[0, 6, 10]]), torch.tensor([1.0])
    with pytest.raises(ValueError, match="two-field"):
        m.elicit(pool, y, 2)
    with pytest.raises(ValueError, match="two-field"):
        m.elicitation_curve(pool, y, 2, strategies=("variance",))
    with pytest.raises(ValueError, match="two-field"):
        m.select_next_questions(pool)
    from vae_amd import _lib
    lib = _lib.load()
    e = _lib.Elicit()
    e.T, e.F, e.d, e.U, e.n_samples = 13, 3, 4, 1, 1
    assert lib.vfm_elicit_f32(C.byref(e), None) == -1 and b"two-field" in lib.vfm_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# the fp64 restatement of the field form
# ---------------------------------------------------------------------------------------------------------------------
def _tables(T, d, seed):
    g = np.random.default_rng(seed)
    return g.normal(size=(T, 2 * d)) * 0.6, g.normal(size=(T, 2)) * 0.5, np.array([1.3, 0.2, 0.4])


def _eps(T, d, seed):
    def f(t):
        g = np.random.default_rng([seed, t])
        return g.normal(size=(T, d)), g.normal(size=T), g.normal()
    return f


@pytest.mark.parametrize("kind", ["abs", "softplus"])
def test_field_moments_are_the_closed_form_of_the_header(kind):
    """RF.moments (context operands M, A, C, c_mean, c_var) against the closed form of vfm_rank.h evaluated pair by
    pair over all fields, and against a Monte-Carlo-free check of its structure: permuting the columns of a row together
    with `field` changes nothing."""
    d, T = 3, 14
    ent, bia, scal = _tables(T, d, 4)
    g = np.random.default_rng(0)
    X = np.stack([g.integers(0, 4, 9), 4 + g.integers(0, 5, 9), 9 + g.integers(0, 3, 9), 12 + g.integers(0, 2, 9)], 1)
    for field in range(4):
        for r in X:
            theta = R.table_theta(ent, bia, r[field])
            mean, var = RF.moments(theta, ent, bia, scal, r[None, :], field, kind)
            m = ent[r, :d]
            s2 = R.link(ent[r, d:], kind) ** 2
            want_m = scal[1] + bia[r, 0].sum()
            want_v = float(R.link(scal[2], kind)) ** 2 + (R.link(bia[r, 1], kind) ** 2).sum()
            for a in range(4):
                want_v += (s2[a] * (m.sum(0) - m[a]) ** 2).sum()
                for b in range(a + 1, 4):
                    want_m += (m[a] * m[b]).sum()
                    want_v += (s2[a] * s2[b]).sum()
            assert abs(mean[0] - want_m) < 1e-12 * max(1.0, abs(want_m))
            assert abs(var[0] - want_v) < 1e-12 * max(1.0, abs(want_v))


@pytest.mark.parametrize("strategy,output,objective,kind,reset,n_hist", [
    ("variance", "reg", "closed_form", "abs", False, 3), ("top", "reg", "closed_form", "softplus", True, 0),
    ("mean", "class", "sampled", "softplus", False, 2), ("variance", "class", "sampled", "abs", True, 0)])
def test_two_fields_through_the_field_form_is_the_two_field_session(strategy, output, objective, kind, reset, n_hist):
    d, N, M, P, Q = 3, 4, 12, 5, 7                                       # Q > P: the pool runs out
    ent, bia, scal = _tables(N + M, d, 7)
    g = np.random.default_rng(1)
    u = 2
    items = N + g.permutation(M)
    pool_items, hist_items = items[:P], items[P:P + n_hist]
    yv = (lambda n: g.normal(size=n) + 1.0) if output == "reg" else (lambda n: (g.random(n) < 0.5).astype(np.float64))
    pool_y, hist_y = yv(P), yv(n_hist)
    kw = dict(kind=kind, output=output, objective=objective, n_steps=6, lr=0.05, klw=0.8, reset=reset,
              eps=_eps(N + M, d, 5), t0=3)
    a = R.session(u, pool_items, pool_y, Q, strategy, ent, bia, scal, hist_items=hist_items, hist_y=hist_y, **kw)
    rows = lambda it: np.stack([np.full(len(it), u), it], 1).astype(np.int64)
    b = RF.session(u, rows(pool_items), pool_y, Q, strategy, ent, bia, scal, field=0, hist_x=rows(hist_items),
                   hist_y=hist_y, **kw)
    assert a["rows"] == b["rows"] and sorted(r for r in b["rows"] if r >= 0) == list(range(P))
    for q in range(Q):
        if a["rows"][q] < 0:
            assert math.isnan(b["loss"][q]) and math.isnan(b["score"][q])
            continue
        assert abs(a["loss"][q] - b["loss"][q]) <= 1e-10 * abs(a["loss"][q])
        assert abs(a["score"][q] - b["score"][q]) <= 1e-10 * abs(a["score"][q])
        for x, z in zip(a["theta"][q], b["theta"][q]):
            np.testing.assert_allclose(z, x, rtol=1e-9, atol=1e-12)


def test_restatement_gradients_match_finite_differences():
    d = 3
    ent, bia, scal = _tables(14, d, 2)
    X = np.array([[1, 5, 9, 12], [1, 7, 10, 13], [1, 4, 11, 12]])
    y = np.array([1.0, 0.0, 1.0])
    for field, e in ((0, 1), (2, 9)):
        Xf = X.copy()
        Xf[:, field] = e
        for objective, output in (("closed_form", "reg"), ("sampled", "class"), ("sampled", "reg")):
            th = R.table_theta(ent, bia, e)
            args = (Xf, y, ent, bia, scal, field, "softplus", output, objective)
            f = lambda t: RF.fold(t, e, *args, 0, 0.0, 0.7, _eps(14, d, 1), 2)[1]
            # one Adam step of size lr moves every parameter by -lr sign(g): recover the signs from finite differences
            stepped, _ = RF.fold(th, e, *args, 1, 1e-3, 0.7, _eps(14, d, 1), 2)
            flat = lambda t: np.concatenate([t[0], t[1], [t[2], t[3]]])
            unflat = lambda p: (p[:d], p[d:2 * d], p[2 * d], p[2 * d + 1])
            p0 = flat(th)
            for k in range(2 * d + 2):
                h = np.zeros(2 * d + 2)
                h[k] = 1e-6
                fd = (f(unflat(p0 + h)) - f(unflat(p0 - h))) / 2e-6
                assert np.sign(fd) == -np.sign(flat(stepped)[k] - p0[k]), (field, objective, k)


def test_planted_seeds_keep_the_choices_apart():
    """The inputs of test_gpu_elicit_field.py::test_against_the_fp64_restatement_on_a_planted_model (RF.planted_case):
    in the restatement the best and the second-best score of every respondent and round differ by more than 1e-3
    relative, so fp32 rounding (1e-6) cannot change a choice and the GPU test allows no exception."""
    for name in RF.PLANTED:
        c = RF.planted_case(name)
        worst = min(min(s["gap"]) for s in RF.planted_sessions(name, c, RF.numpy_eps(c)))
        assert worst > 1e-3, (name, worst)

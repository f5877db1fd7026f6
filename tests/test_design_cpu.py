"""CPU: target-aware elicitation (include/vfm_design.h, vae_amd/design.py) -- the properties of the fp64 restatement
(tests/design_restatement.py: the score is non-negative, blind to the answers and to the respondent's table row, greedy
optimal against a brute-force fold of every candidate, and equal to the realised drop), the header against the
library's exports and the ctypes mirror against gcc, every argument error of the three methods and both C entries
without a GPU, the "design" name in the curves, and the GPU cases themselves: every round of every respondent keeps a
gap of 2^-20 of the best between its two best scores."""
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

import design_restatement as DR  # noqa: E402
import solve_reference as SR  # noqa: E402
from test_foldin_cpu import _cpu_model  # noqa: E402

HDR = os.path.join(ROOT, "include", "vfm_design.h")


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
def _small(link, seed, n_hist=6, n_pool=12, n_tgt=9, d=7, F=3):
    sizes = (5, 30, 6)[:F] if F == 3 else (5, 60)
    ent, bia, scal = SR.tables(sizes, d, seed)
    g = torch.Generator().manual_seed(seed + 7)
    lo = [sum(sizes[:f]) for f in range(F)]
    rows = DR._rows(g, sizes, lo, 0, 2, n_hist + n_pool + n_tgt)
    y = (torch.randn(n_hist + n_pool, generator=g) + 1.0).numpy()
    return dict(ent=ent, bia=bia, scal=scal, hist=rows[:n_hist].numpy(), pool=rows[n_hist:n_hist + n_pool].numpy(),
                tgt=rows[n_hist + n_pool:].numpy(), y_hist=y[:n_hist], y_pool=y[n_hist:], link=link)


@pytest.mark.parametrize("link", ["abs", "softplus"])
@pytest.mark.parametrize("n_hist", [0, 6, 11])
def test_score_is_the_realised_drop_and_greedy_optimal(link, n_hist):
    klw = 0.8
    c = _small(link, 3 + n_hist, n_hist=n_hist)
    prec, kl = DR.prec_kl(c["scal"], link, klw)
    Mp, Ap = DR.operands(c["ent"], c["bia"], c["scal"], c["pool"], 0, link)
    Mh, Ah = DR.operands(c["ent"], c["bia"], c["scal"], c["hist"], 0, link)
    Mt, At = DR.operands(c["ent"], c["bia"], c["scal"], c["tgt"], 0, link)
    W = DR.walk_W(Mt, At)
    sc = DR.scores(DR.walk_S(Mh, Ah), W, n_hist, Mp, Ap, kl, prec)
    assert (sc >= 0).all() and (W >= 0).all()
    before = DR.objective_after(c["ent"], c["bia"], c["scal"], c["hist"], c["y_hist"], 0, link, klw, W)
    after = np.array([DR.objective_after(c["ent"], c["bia"], c["scal"], np.concatenate([c["hist"], c["pool"][q:q + 1]]),
                                         np.concatenate([c["y_hist"], c["y_pool"][q:q + 1]]), 0, link, klw, W)
                      for q in range(len(sc))])
    assert int(np.argmax(sc)) == int(np.argmin(after))      # greedy optimal, by brute force
    assert (np.abs((before - after) - sc) <= 1e-12 * np.abs(sc)).all(), np.abs((before - after) - sc) / sc


def test_restated_session_is_blind_to_answers_and_to_the_table_row():
    c = _small("abs", 5)
    args = lambda ent, y: (ent, c["bia"], c["scal"], c["pool"], y, c["hist"], c["y_hist"], c["tgt"], 0, "abs", 0.8, 5)
    a = DR.session(*args(c["ent"], c["y_pool"]))
    b = DR.session(*args(c["ent"], -3.0 * c["y_pool"] + 1.0))
    ent2 = c["ent"].clone()
    ent2[2] = 9.0                                            # the respondent's own row
    r = DR.session(*args(ent2, c["y_pool"]))
    assert a["rows"] == b["rows"] == r["rows"] and a["score"] == b["score"] == r["score"]
    assert not np.allclose(a["theta"][-1]["mu"], b["theta"][-1]["mu"])       # (the answers do move the means)
    e = DR.session(c["ent"], c["bia"], c["scal"], c["pool"], c["y_pool"], c["hist"], c["y_hist"], c["tgt"][:0], 0, "abs",
                   0.8, 3)
    assert e["rows"] == [0, 1, 2] and (e["W"] == 0).all()    # empty targets: the bias term alone, position decides


# ---------------------------------------------------------------------------------------------------------------------
# header, exports, struct mirror
# ---------------------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)


def _header_fields():
    body = re.search(r"typedef struct vfm_design_t \{(.*?)\} vfm_design_t;", _header(), re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names = decl.split(",")
            fields.append(re.findall(r"\w+", names[0])[-1])
            fields += [re.findall(r"\w+", n)[-1] for n in names[1:]]
    return fields


def test_header_names_exports_and_struct_mirror_match_gcc(tmp_path):
    from vae_amd import _lib
    lib = _lib.load()
    declared = sorted(set(re.findall(r"\b(vfm_design_\w+)\s*\(", _header())))
    assert declared == sorted(_lib.DESIGN_EXPORTS) and len(declared) == 3
    for name in _lib.DESIGN_EXPORTS:
        getattr(lib, name)
        assert name not in _lib.EXPORTS and name not in _lib.ELICIT_EXPORTS
    assert _lib.ABI_VERSION == 5                            # additions only
    fields = _header_fields()
    assert fields == [n for n, _ in _lib.ElicitDesign._fields_]
    solve = [n for n, _ in _lib.ElicitSolve._fields_]
    assert [f for f in solve if f not in fields] == ["key_col", "strategy", "seed"]
    assert [f for f in fields if f not in solve] == ["n_targets", "tgt_ptr", "tgt_op", "out_pool_score"]
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vfm_design.h"', "int main(void) {",
             'printf("S %zu\\n", sizeof(vfm_design_t));']
    lines += [f'printf("F {n} %zu\\n", offsetof(vfm_design_t, {n}));' for n in fields]
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
            assert C.sizeof(_lib.ElicitDesign) == int(t[1])
        else:
            assert getattr(_lib.ElicitDesign, t[1]).offset == int(t[2]), t[1]
            seen += 1
    assert seen == len(fields)
    with pytest.raises(AttributeError):
        _lib.ElicitDesign().strategy = 1


def test_workspace_function():
    from vae_amd import _lib
    lib = _lib.load()
    w, ws = lib.vfm_design_workspace_bytes, lib.vfm_elicit_solve_workspace_bytes
    for a in ((3, 100, 7, 5, -1), (3, 100, 7, 5, 0), (300, 100, 7, 5, 5), (2, 0, 0, 512, -1), (9, 40, 11, 128, 4)):
        assert w(*a) == ws(*a) > 0
    for bad in ((-1, 1, 1, 8, -1), (1, -1, 1, 8, -1), (1, 1, -1, 8, -1), (1, 1, 1, 0, -1), (1, 1, 1, 513, -1),
                (1, 1, 1, 8, -2)):
        assert w(*bad) == _lib._gen.VFM_E_INVALID, bad


def _valid(lib_mod):
    """A struct that passes every value check and fails only on its (missing) pointers."""
    e = lib_mod.ElicitDesign()
    e.T, e.F, e.d, e.field, e.U, e.P, e.H, e.n_ops, e.n_targets = 10, 3, 4, 0, 1, 2, 0, 2, 2
    e.n_rounds, e.lds_dim, e.kl_weight = 3, -1, 1.0
    return e


REFUSALS = [  # (field, value), -> a word of vfm_last_error(), sessions only?
    ("F", 1, b"F out of range", False), ("F", 65, b"F out of range", False),
    ("field", -1, b"field out of range", False), ("field", 3, b"field out of range", False),
    ("d", 0, b"d out of range", False), ("d", 513, b"d out of range", False),
    ("U", -1, b"U < 0", False), ("P", -1, b"P < 0", False), ("H", -1, b"H < 0", False),
    ("n_targets", -1, b"n_targets < 0", False), ("T", 0, b"T < 1", False),
    ("n_rounds", 4097, b"n_rounds", True), ("n_rounds", -1, b"n_rounds", True),
    ("flags", 1, b"flags", False), ("n_ops", 0, b"n_ops", False), ("n_ops", -1, b"n_ops", False),
    ("lds_dim", -2, b"lds_dim", False),
    ("kl_weight", 0.0, b"kl_weight", False), ("kl_weight", -1.0, b"kl_weight", False),
    ("kl_weight", float("nan"), b"kl_weight", False), ("kl_weight", float("inf"), b"kl_weight", False),
    ("out_mean", 256, b"out_mean", True), ("out_var", 256, b"out_mean", True),
]


@pytest.mark.parametrize("entry", ["vfm_design_scores_f32", "vfm_design_elicit_f32"])
@pytest.mark.parametrize("key,value,word,session_only", REFUSALS, ids=[f"{k}={v}" for k, v, _, _ in REFUSALS])
def test_library_refuses_bad_values_before_any_hip_call(entry, key, value, word, session_only):
    from vae_amd import _lib
    lib = _lib.load()
    fn = getattr(lib, entry)
    e = _valid(_lib)
    assert fn(C.byref(e), None) == -1 and b"null pointer" in lib.vfm_last_error()
    setattr(e, key, value)
    rc = fn(C.byref(e), None)
    assert rc == _lib._gen.VFM_E_INVALID
    if session_only and entry == "vfm_design_scores_f32":
        assert b"null pointer" in lib.vfm_last_error()       # (n_rounds and the moments are the sessions')
    else:
        assert word in lib.vfm_last_error(), lib.vfm_last_error()


@pytest.mark.parametrize("entry", ["vfm_design_scores_f32", "vfm_design_elicit_f32"])
def test_library_refuses_struct_pointers_and_workspace(entry):
    """The pointer checks see only whether a pointer is NULL: the fake non-NULL values below are never followed, since
    every call is refused before any HIP call."""
    from vae_amd import _lib
    lib = _lib.load()
    fn = getattr(lib, entry)
    INV = _lib._gen.VFM_E_INVALID
    assert fn(None, None) == INV and b"NULL argument struct" in lib.vfm_last_error()
    e = _valid(_lib)
    e.struct_size -= 8                                       # a shorter struct of another build
    assert fn(C.byref(e), None) == INV and b"struct_size" in lib.vfm_last_error()
    e = _valid(_lib)
    e.abi_version += 1
    assert fn(C.byref(e), None) == INV and b"abi_version" in lib.vfm_last_error()
    e = _valid(_lib)
    e.U = 0
    assert fn(C.byref(e), None) == 0                         # nothing to do, nothing launched
    e = _valid(_lib)
    ptrs = ["entities", "pool_ptr", "pool_x", "tgt_ptr", "tgt_op", "entity_params", "bias_params", "scalars"]
    ptrs += ["pool_y", "out_row", "out_score", "out_loss"] if entry.endswith("elicit_f32") else ["out_pool_score"]
    for k in ptrs:
        setattr(e, k, 256)
    for k in ptrs:                                           # each one missing in turn
        setattr(e, k, None)
        assert fn(C.byref(e), None) == INV and b"null pointer" in lib.vfm_last_error(), k
        setattr(e, k, 256)
    assert fn(C.byref(e), None) == INV and b"op_x, pool_op" in lib.vfm_last_error()
    e.op_x = e.pool_op = 256
    assert fn(C.byref(e), None) == INV and b"workspace too small" in lib.vfm_last_error()
    e.workspace, e.workspace_bytes = 256 + 8, 1 << 30
    assert fn(C.byref(e), None) == INV and b"aligned" in lib.vfm_last_error()
    e.H = 1                                                  # a history needs its lists
    assert fn(C.byref(e), None) == INV and b"null pointer" in lib.vfm_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# the Python entry points: every argument error, before a GPU is needed
# ---------------------------------------------------------------------------------------------------------------------
POOL = torch.tensor([[0, 6], [1, 7], [0, 9]])
Y = torch.tensor([1.0, 2.0, 3.0])


def _calls(m):
    return {"scores": lambda pool=POOL, field=0, **k: m.design_scores_field(pool, field, **k),
            "select": lambda pool=POOL, field=0, **k: m.select_next_questions_design_field(pool, field, **k),
            "session": lambda pool=POOL, field=0, y=Y, Q=2, **k: m.elicit_field_design(pool, y, Q, field, **k)}


@pytest.mark.parametrize("which", ["scores", "select", "session"])
def test_argument_checks_raise_before_a_gpu_is_needed(which):
    call = _calls(_cpu_model())[which]
    with pytest.raises(ValueError, match="'reg'"):
        _calls(_cpu_model("class"))[which]()
    for bad in (0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="kl_weight"):
            call(kl_weight=bad)
    with pytest.raises(ValueError, match="field"):
        call(field=2)
    with pytest.raises(ValueError, match="field"):
        call(field=True)
    with pytest.raises(ValueError, match="pool must be"):
        call(pool=torch.tensor([0, 6]))
    with pytest.raises(ValueError, match="integer ids"):
        call(pool=POOL.float())
    with pytest.raises(ValueError, match="lie in"):
        call(pool=torch.tensor([[0, 10]]), **({"y": Y[:1]} if which == "session" else {}))
    with pytest.raises(ValueError, match="range"):
        call(pool=torch.tensor([[6, 7]]), **({"y": Y[:1]} if which == "session" else {}))
    with pytest.raises(ValueError, match="history"):
        call(history=(POOL, Y, Y))
    with pytest.raises(ValueError, match="history must be a pair"):
        call(history=POOL)                                   # (X alone: the pair of the sessions is asked for)
    with pytest.raises(ValueError, match="history X"):
        call(history=(torch.tensor([0, 6]), Y[:1]))
    with pytest.raises(ValueError, match="without a pool row"):
        call(history=(torch.tensor([[2, 6]]), Y[:1]))
    with pytest.raises(ValueError, match="targets must be"):
        call(targets=torch.tensor([0, 6]))
    with pytest.raises(ValueError, match="targets: context ids"):
        call(targets=torch.tensor([[0, 10]]))
    with pytest.raises(ValueError, match="targets: column 0"):
        call(targets=torch.tensor([[6, 7]]))
    with pytest.raises(ValueError, match="targets hold respondents without a pool row"):
        call(targets=torch.tensor([[2, 7]]))
    if which == "select":
        for bad in (0, -2, True):
            with pytest.raises(ValueError, match="n must be"):
                call(n=bad)
    if which == "session":
        with pytest.raises(ValueError, match="one value per row"):
            call(y=Y[:2])
        for bad in (-1, 4097, 1.5, True):
            with pytest.raises(ValueError, match="n_questions"):
                call(Q=bad)
        with pytest.raises(ValueError, match="lds_dim"):
            call(lds_dim=-2)
    with pytest.raises(ValueError, match="frozen|ranked field"):
        _calls(_cpu_model(field_sizes=[3, 4, 5]))[which](pool=torch.tensor([[0, 1, 8]]), field=0,
                                                         **({"y": Y[:1]} if which == "session" else {}))


@pytest.mark.parametrize("which", ["scores", "select", "session"])
def test_cpu_model_fails_loudly(which):
    from vae_amd._lib import VfmLibraryError
    with pytest.raises(VfmLibraryError, match="MI355X"):
        _calls(_cpu_model())[which]()


# ---------------------------------------------------------------------------------------------------------------------
# the name "design" in the curves
# ---------------------------------------------------------------------------------------------------------------------
def test_design_is_a_name_of_the_exact_curves_only(monkeypatch):
    from vae_amd import design, elicit, rank
    assert rank.STRATEGIES == {"top": 0, "variance": 1, "mean": 2, "random": 3}
    m = _cpu_model()
    X, yt = torch.tensor([[0, 7]]), torch.tensor([5.0])
    unknown = "strategy must be one of"
    for name in ("design", "nonsense"):
        with pytest.raises(ValueError, match=unknown):
            m.elicitation_curve(POOL, Y, 2, strategies=[name])
        with pytest.raises(ValueError, match=unknown):
            m.elicitation_curve_field(POOL, Y, 2, 0, strategies=[name])
        with pytest.raises(ValueError, match=unknown):
            m.elicitation_ranking_curve_field(POOL, Y, 2, 0, X, yt, 1, strategies=[name])
        with pytest.raises(ValueError, match=unknown):
            m.elicit_field_exact(POOL, Y, 2, 0, strategy=name)
        with pytest.raises(ValueError, match=unknown):
            m.select_next_questions_field(POOL, 0, 1, name)
    with pytest.raises(ValueError, match=unknown):
        m.elicitation_curve_field_exact(POOL, Y, 2, 0, strategies=["design", "nonsense"])
    with pytest.raises(ValueError, match=unknown):
        m.elicitation_ranking_curve_field(POOL, Y, 2, 0, X, yt, 1, strategies=["nonsense"], exact=True)

    # routing: "design" goes to run_field_design with `targets` and without seed / key_field; the others to the
    # exact session without `targets`
    seen = []
    monkeypatch.setattr(design, "run_field_design", lambda *a, **k: seen.append(("design", a[1:], k)) or 1 / 0)
    monkeypatch.setattr(elicit, "run_field_exact", lambda *a, **k: seen.append(("exact", a[1:], k)) or 1 / 0)
    tg = torch.tensor([[0, 8]])
    for strategies in (["design"], ["variance"]):
        with pytest.raises(ZeroDivisionError):
            m.elicitation_curve_field_exact(POOL, Y, 2, 0, strategies=strategies, targets=tg, seed=4, kl_weight=0.5)
        with pytest.raises(ZeroDivisionError):
            m.elicitation_ranking_curve_field(POOL, Y, 2, 0, X, yt, 1, strategies=strategies, exact=True, targets=tg,
                                              seed=4, kl_weight=0.5)
    kinds = [s[0] for s in seen]
    assert kinds == ["design", "design", "exact", "exact"]
    for kind, a, k in seen:
        assert (a[3] if len(a) > 3 else k["field"]) == 0     # the field, by position or by name
        assert k["kl_weight"] == 0.5 and k["write"] is False
        if kind == "design":
            assert k["targets"] is tg and "seed" not in k and "key_field" not in k and "strategy" not in k
        else:
            assert "targets" not in k and k["seed"] == 4
    with pytest.raises(ValueError, match=unknown):           # not exact: the name is unknown, whatever else is passed
        m.elicitation_ranking_curve_field(POOL, Y, 2, 0, X, yt, 1, strategies=["design"], exact=False, targets=tg)


# ---------------------------------------------------------------------------------------------------------------------
# the GPU cases
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(DR.CASES))
def test_gpu_cases_keep_the_gap(name):
    c, ref = DR.build(name)
    spec = DR.CASES[name]
    assert sorted(ref) == c["ents"].tolist() and len(ref) == spec["n_resp"]
    for e, r in ref.items():
        assert len(r["gaps"]) == spec["Q"]
        for q, gap in enumerate(r["gaps"]):
            assert gap >= DR.GAP, (name, e, q, gap)          # (duplicates of a context and empty targets: inf)
    c2 = DR.generate(name, c["seed"])                        # the same draw wherever it is built
    assert torch.equal(c2["pool"], c["pool"]) and torch.equal(c2["ent"], c["ent"])
    # what the case is there for
    counts = torch.bincount(torch.searchsorted(c["ents"], c["pool"][:, spec["field"]].contiguous()))
    assert sorted(set(counts.tolist())) == sorted(set(spec["pools"][i % len(spec["pools"])] for i in range(spec["n_resp"])))
    assert any(-1 in r["rows"] for r in ref.values()) == (min(spec["pools"]) < spec["Q"])
    if spec["targets"] == "given":
        assert sum((r["W"] == 0).all() for r in ref.values()) == 1       # one respondent without targets
    if name == "d200_slab":
        n = max(spec["hists"])
        assert SR.storage(n + 1, spec["d"]) == "slab" and SR.storage(1, spec["d"]) == "lds"
    if name == "d5_past_cap":
        assert spec["n_resp"] > SR.SLABS and SR.has_slabs(spec["d"], 0)

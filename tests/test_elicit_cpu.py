"""CPU: elicitation sessions (include/vfm_elicit.h) -- the library exports the header's functions and lays out
vfm_elicit_t as the ctypes mirror does; the argument checks of VFM.elicit / elicitation_curve raise before anything needs
a GPU; the list helpers keep the pool's order and map rows back to the caller's indices; the fp64 restatement of the
session (elicit_restatement.py) agrees with a literal loop over its single-round pieces."""
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

import elicit_restatement as R

HDR = os.path.join(ROOT, "include", "vfm_elicit.h")


def test_library_exports_every_declared_function():
    from vae_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(vfm_elicit\w*)\s*\(", text)))
    assert declared == sorted(_lib.ELICIT_EXPORTS)
    lib = _lib.load()
    for name in declared:
        getattr(lib, name)                                  # AttributeError: not exported
    assert lib.vfm_elicit_workspace_bytes(100, 7, 5, _lib.OBJ_SAMPLED) == 256
    assert lib.vfm_elicit_workspace_bytes(100, 7, 5, _lib.OBJ_CLOSED_FORM) == 256 + 768 + 256
    assert lib.vfm_elicit_workspace_bytes(100, 7, 513, _lib.OBJ_SAMPLED) < 0


def test_struct_mirror_matches_gcc(tmp_path):
    from vae_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    body = re.search(r"typedef struct vfm_elicit_t \{(.*?)\} vfm_elicit_t;", text, re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names = decl.split(",")
            fields.append(re.findall(r"\w+", names[0])[-1])
            fields += [re.findall(r"\w+", n)[-1] for n in names[1:]]
    assert fields == [n for n, _ in _lib.Elicit._fields_]  # every field, in order
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vfm_elicit.h"', "int main(void) {",
             'printf("S %zu\\n", sizeof(vfm_elicit_t));']
    lines += [f'printf("F {n} %zu\\n", offsetof(vfm_elicit_t, {n}));' for n in fields]
    lines += [f'printf("M {n} %d\\n", (int){n});' for n in ("VFM_ELICIT_MAX_ROUNDS", "VFM_ABI_VERSION")]
    lines += ["return 0; }"]
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    for ln in got:
        t = ln.split()
        if not t:
            continue
        if t[0] == "S":
            assert C.sizeof(_lib.Elicit) == int(t[1])
        elif t[0] == "F":
            assert getattr(_lib.Elicit, t[1]).offset == int(t[2]), t[1]
        elif t[1] == "VFM_ELICIT_MAX_ROUNDS":
            assert _lib.ELICIT_MAX_ROUNDS == int(t[2])
        else:
            assert _lib.ABI_VERSION == int(t[2])
    e = _lib.Elicit()
    assert (e.struct_size, e.abi_version) == (C.sizeof(_lib.Elicit), _lib.ABI_VERSION)
    with pytest.raises(AttributeError):
        e.n_round = 3                                       # a misspelt field


def test_library_checks_arguments_before_any_hip_call():
    from vae_amd import _lib
    lib = _lib.load()
    e = _lib.Elicit()
    e.T, e.F, e.d, e.U, e.n_samples = 10, 3, 4, 1, 1
    assert lib.vfm_elicit_f32(C.byref(e), None) == -1 and b"two-field" in lib.vfm_last_error()
    e.F = 2
    e.struct_size -= 8
    assert lib.vfm_elicit_f32(C.byref(e), None) == -1 and b"struct_size" in lib.vfm_last_error()
    e.struct_size += 8
    e.strategy = 4
    assert lib.vfm_elicit_f32(C.byref(e), None) == -1 and b"strategy" in lib.vfm_last_error()
    e.strategy, e.objective, e.likelihood = 1, _lib.OBJ_CLOSED_FORM, _lib.LIK_BERNOULLI
    assert lib.vfm_elicit_f32(C.byref(e), None) == -1 and b"Normal" in lib.vfm_last_error()
    e.objective, e.n_rounds = _lib.OBJ_SAMPLED, 5000
    assert lib.vfm_elicit_f32(C.byref(e), None) == -1 and b"n_rounds" in lib.vfm_last_error()
    e.n_rounds = 3
    assert lib.vfm_elicit_f32(C.byref(e), None) == -1 and b"null pointer" in lib.vfm_last_error()
    e.U = 0
    assert lib.vfm_elicit_f32(C.byref(e), None) == 0        # nothing to do, nothing launched


def _cpu_model(output="reg", sizes=(6, 4)):
    from vae_amd.model import VFM
    return VFM(field_sizes=list(sizes), embedding_size=4, output=output, device="cpu")


@pytest.mark.parametrize("call", ["elicit", "elicitation_curve"])
def test_argument_checks_raise_value_error(call):
    m = _cpu_model()
    fn = getattr(m, call)
    pool = torch.tensor([[0, 6], [1, 7], [0, 9]])
    y = torch.tensor([1.0, 2.0, 3.0])
    kw = dict(strategies=("variance",)) if call == "elicitation_curve" else {}
    with pytest.raises(ValueError, match="n_questions"):
        fn(pool, y, -1, **kw)
    with pytest.raises(ValueError, match="n_questions"):
        fn(pool, y, 4097, **kw)
    with pytest.raises(ValueError, match=r"\[P, 2\]"):
        fn(torch.tensor([0, 1]), y[:2], 2, **kw)
    with pytest.raises(ValueError, match="range"):
        fn(torch.tensor([[6, 7]]), y[:1], 2, **kw)          # an item id in the user column
    with pytest.raises(ValueError, match="lie in"):
        fn(torch.tensor([[0, 10]]), y[:1], 2, **kw)         # item id past T
    with pytest.raises(ValueError, match="frozen"):
        fn(torch.tensor([[0, 3]]), y[:1], 2, **kw)          # a user id as the item: it would not be frozen
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
        fn(pool, y, 2, history=torch.tensor([[0, 6]]), **kw)
    with pytest.raises(ValueError, match="without a pool row"):
        fn(pool, y, 2, history=(torch.tensor([[2, 6]]), torch.tensor([1.0])), **kw)
    with pytest.raises(ValueError, match="one value"):
        fn(pool, y, 2, history=(torch.tensor([[0, 8]]), torch.tensor([1.0, 2.0])), **kw)
    if call == "elicit":
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
    with pytest.raises(ValueError, match="two-field"):
        getattr(_cpu_model(sizes=(3, 4, 5)), call)(torch.tensor([[0, 3, 8]]), y[:1], 2, **kw)


def test_cpu_model_fails_loudly():
    from vae_amd._lib import VfmLibraryError
    m = _cpu_model()
    pool, y = torch.tensor([[0, 6], [1, 7]]), torch.tensor([1.0, 2.0])
    with pytest.raises(VfmLibraryError, match="MI355X"):
        m.elicit(pool, y, 2)
    with pytest.raises(VfmLibraryError, match="MI355X"):
        m.elicitation_curve(pool, y, 2, strategies=("variance",))


def test_list_helpers_keep_pool_order_and_map_rows_back():
    from vae_amd import elicit as E
    g = torch.Generator().manual_seed(3)
    users = torch.tensor([5, 2, 9, 2, 5, 5, 0, 9, 2, 5])
    pool = torch.stack([users, 20 + torch.randperm(10, generator=g)], 1)
    order, us, ptr = E.pool_lists(pool)
    assert us.tolist() == [0, 2, 5, 9] and ptr.tolist() == [0, 1, 4, 8, 10]
    for i, u in enumerate(us.tolist()):
        seg = order[ptr[i]:ptr[i + 1]].tolist()
        assert seg == [r for r in range(10) if int(users[r]) == u]       # the caller's order kept within a user
    # sorted-pool positions back to caller indices, -1 kept
    out_row = torch.tensor([[0, -1, -1], [3, 1, 2], [7, 4, 5], [9, 8, -1]])
    rows = E.rows_to_caller(out_row, order)
    assert rows.tolist() == [[6, -1, -1], [8, 1, 3], [9, 0, 4], [7, 2, -1]]
    assert all(int(pool[r, 0]) == u for u, rr in zip(us.tolist(), rows.tolist()) for r in rr if r >= 0)
    v = torch.arange(20.0).reshape(2, 10)
    back = E.to_caller_order(v, order)
    assert torch.equal(back[:, order], v)
    when = E.asked_round(rows, 10)
    assert when.tolist() == [1, 1, 1, 2, 2, 3, 0, 0, 0, 0]               # 3 = never asked (Q)
    hx = torch.tensor([[5, 30], [0, 31], [5, 32], [9, 33]])
    horder, hptr = E.history_lists(us, hx)
    assert hptr.tolist() == [0, 1, 1, 3, 4] and horder.tolist() == [1, 0, 2, 3]
    # a shuffled pool with the same rows: each user's asked row maps to the same (user, item) pair
    perm = torch.randperm(10, generator=g)
    o2, u2, p2 = E.pool_lists(pool[perm])
    assert torch.equal(u2, us) and torch.equal(p2, ptr)


def _lists_restated(E, x, y, hx, hy, field, targets):
    """field_lists from its primitives, as the four sessions spelt it out before they shared it: run_field's text for
    targets "absent", design's for targets None (own pool rows) or given."""
    order, ents, ptr = E.pool_lists(x, field)
    px, ys = x[order].contiguous(), y[order].contiguous()
    P = px.shape[0]
    hptr = hxs = hys = hist_op = None
    if hx is not None and hx.shape[0]:
        horder, hptr = E.history_lists(ents, hx, field)
        hxs, hys = hx[horder].contiguous(), hy[horder].contiguous()
    if isinstance(targets, str):
        ctx = (px if hxs is None else torch.cat([px, hxs])).clone()
        ctx[:, field] = 0
        op_x, inv = torch.unique(ctx, dim=0, return_inverse=True)
        inv = inv.reshape(-1)
        op_x, pool_op = op_x.contiguous(), inv[:P].contiguous()
        if hxs is not None:
            hist_op = inv[P:].contiguous()
        return dict(order=order, ents=ents, ptr=ptr, px=px, ys=ys, hptr=hptr, hxs=hxs, hys=hys, tptr=None, op_x=op_x,
                    pool_op=pool_op, hist_op=hist_op, tgt_op=None)
    H = 0 if hxs is None else hxs.shape[0]
    if targets is None:
        txs, tptr = None, ptr
    else:
        torder, tptr = E.history_lists(ents, targets, field)
        txs = targets[torder]
    parts = [px] + ([hxs] if hxs is not None else []) + ([txs] if txs is not None else [])
    ctx = torch.cat(parts).clone()
    ctx[:, field] = 0
    op_x, inv = torch.unique(ctx, dim=0, return_inverse=True)
    inv = inv.reshape(-1)
    pool_op = inv[:P].contiguous()
    if hxs is not None:
        hist_op = inv[P:P + H].contiguous()
    tgt_op = pool_op if txs is None else inv[P + H:].contiguous()
    return dict(order=order, ents=ents, ptr=ptr, px=px, ys=ys, hptr=hptr, hxs=hxs, hys=hys, tptr=tptr,
                op_x=op_x.contiguous(), pool_op=pool_op, hist_op=hist_op, tgt_op=tgt_op)


@pytest.mark.parametrize("targets", ["absent", "own", "given"])
@pytest.mark.parametrize("history", ["none", "empty", "some"])
@pytest.mark.parametrize("F,field", [(2, 0), (2, 1), (3, 0), (3, 2)])
def test_field_lists_are_the_restated_lists(F, field, history, targets):
    from vae_amd import elicit as E
    shared = [20, 30][:F - 1]                               # the context that pool, history and targets all hold

    def rows(resp, ctxs):                                   # [n, F]: respondent ids in column `field`, contexts beside
        out = torch.tensor([c[:F - 1] for c in ctxs])
        return torch.cat([out[:, :field], torch.tensor(resp)[:, None], out[:, field:]], 1)

    # respondents 4, 1, 7 in shuffled order; contexts repeat within and across respondents
    x = rows([4, 1, 7, 1, 4, 4, 7, 1, 4, 1],
             [shared, [21, 30], [22, 31], [21, 30], [21, 31], shared, [23, 30], [20, 31], [22, 31], [24, 32]])
    y = torch.arange(10.0)
    hx, hy = {"none": (None, None), "empty": (x[:0], y[:0]),
              "some": (rows([4, 1, 4], [[21, 30], shared, [25, 33]]), torch.tensor([7.0, 8.0, 9.0]))}[history]
    tx = {"absent": "absent", "own": None,                  # given: respondent 1 has none, one context is the targets' own
          "given": rows([7, 4, 7, 4], [[26, 34], [21, 30], shared, [24, 32]])}[targets]
    want = _lists_restated(E, x, y, hx, hy, field, tx)
    got = E.field_lists(x, y, hx, hy, field) if targets == "absent" else E.field_lists(x, y, hx, hy, field, tx)
    assert sorted(got) == sorted(want)
    for key, w in want.items():
        if w is None:
            assert got[key] is None, key
        else:
            assert got[key].dtype == w.dtype and torch.equal(got[key], w), key
    assert got["ents"].tolist() == [1, 4, 7] and got["px"].shape == (10, F)
    n_hist = 3 if history == "some" else 0
    assert (got["hist_op"] is None) == (n_hist == 0) and (n_hist == 0 or got["hist_op"].shape == (n_hist,))
    zeroed = lambda t: torch.cat([t[:, :field], torch.zeros_like(t[:, :1]), t[:, field + 1:]], 1)
    if targets == "absent":                                 # nothing of the targets: the operands of pool and history alone
        assert got["tptr"] is None and got["tgt_op"] is None
        both = x if n_hist == 0 else torch.cat([x, hx])
        assert torch.equal(got["op_x"], torch.unique(zeroed(both), dim=0))
    elif targets == "own":
        assert got["tgt_op"] is got["pool_op"] and got["tptr"] is got["ptr"]
    else:
        assert got["tptr"].tolist() == [0, 0, 2, 4] and got["tgt_op"].shape == (4,)
    # the shared context is one operand wherever it occurs, and every index points at its own row's context
    c0 = zeroed(rows([0], [shared]))[0]
    hit = (got["op_x"] == c0).all(1).nonzero().reshape(-1)
    assert hit.numel() == 1
    assert torch.equal(got["op_x"][got["pool_op"]], zeroed(got["px"])) and int(hit) in got["pool_op"].tolist()
    if n_hist:
        assert torch.equal(got["op_x"][got["hist_op"]], zeroed(got["hxs"])) and int(hit) in got["hist_op"].tolist()
    if targets == "given":
        assert int(hit) in got["tgt_op"].tolist() and got["op_x"][got["tgt_op"]][:, field].eq(0).all()


def test_metric_helpers():
    from vae_amd import elicit as E
    y = torch.tensor([1.0, 0.0, 1.0, 0.0, 1.0])
    s = torch.tensor([0.9, 0.1, 0.4, 0.4, 0.8])
    assert abs(E.auc(s, y) - (2 + 2 + 1 + 0.5) / 6) < 1e-12              # the tie counts 1/2
    assert math.isnan(E.auc(s, torch.ones(5)))
    mean, var = torch.tensor([1.0, 2.0, float("nan")]), torch.tensor([0.5, 0.5, 0.5])
    assert abs(E.metric("reg", mean, var, torch.tensor([2.0, 2.0, 9.0])) - math.sqrt(0.5)) < 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# the fp64 restatement: the session against a literal loop over the single-round pieces
# ---------------------------------------------------------------------------------------------------------------------
def _tables(T, d, seed):
    g = np.random.default_rng(seed)
    return g.normal(size=(T, 2 * d)) * 0.6, g.normal(size=(T, 2)) * 0.5, np.array([1.3, 0.2, 0.4])


def _uniform(seed):
    return lambda q, item: float(np.random.default_rng([seed, q, item]).random())


def _eps(T, d, seed):
    def f(t):
        g = np.random.default_rng([seed, t])
        return g.normal(size=(T, d)), g.normal(size=T), g.normal()
    return f


@pytest.mark.parametrize("strategy,output,objective,kind,reset,n_hist", [
    ("variance", "reg", "closed_form", "abs", False, 3), ("top", "reg", "closed_form", "softplus", True, 0),
    ("random", "reg", "sampled", "abs", False, 2), ("mean", "class", "sampled", "softplus", False, 0),
    ("variance", "class", "sampled", "abs", True, 4)])
def test_session_equals_loop_over_single_rounds(strategy, output, objective, kind, reset, n_hist):
    d, N, M, P, Q = 3, 4, 12, 5, 7                                       # Q > P: the pool runs out
    ent, bia, scal = _tables(N + M, d, 7)
    g = np.random.default_rng(1)
    u = 2
    items = N + g.permutation(M)
    pool_items, hist_items = items[:P], items[P:P + n_hist]
    yv = (lambda n: g.normal(size=n) + 1.0) if output == "reg" else (lambda n: (g.random(n) < 0.5).astype(np.float64))
    pool_y, hist_y = yv(P), yv(n_hist)
    kw = dict(kind=kind, output=output, objective=objective, n_steps=6, lr=0.05, klw=0.8)
    s = R.session(u, pool_items, pool_y, Q, strategy, ent, bia, scal, hist_items=hist_items, hist_y=hist_y, reset=reset,
                  eps=_eps(N + M, d, 5), t0=3, uniform=_uniform(9), **kw)
    theta = R.prior_theta(d, kind) if reset else R.table_theta(ent, bia, u)
    asked = np.zeros(P, dtype=bool)
    f_items, f_y = list(hist_items), list(hist_y)
    for q in range(Q):
        mean, var = R.moments(theta, ent, bia, scal, pool_items, kind)
        np.testing.assert_allclose(s["mean"][q], mean, rtol=1e-12)
        np.testing.assert_allclose(s["var"][q], var, rtol=1e-12)
        best, _ = R.choose(R.score(strategy, mean, var, q, pool_items, _uniform(9)), asked)
        assert s["rows"][q] == best
        if best < 0:
            assert q >= P and math.isnan(s["loss"][q]) and math.isnan(s["score"][q])
            continue
        asked[best] = True
        f_items.append(pool_items[best])
        f_y.append(pool_y[best])
        theta, loss = R.fold(theta, u, f_items, f_y, ent, bia, scal, kind, output, objective, 6, 0.05, 0.8,
                             _eps(N + M, d, 5), 3 + q * 7)
        assert abs(s["loss"][q] - loss) <= 1e-10 * abs(loss)
        for a, b in zip(s["theta"][q], theta):
            np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-12)
    assert sorted(r for r in s["rows"] if r >= 0) == list(range(P)) and s["rows"][P:] == [-1] * (Q - P)


def test_restatement_gradients_match_finite_differences():
    d, N, M = 3, 2, 6
    ent, bia, scal = _tables(N + M, d, 2)
    items, y = np.array([3, 5, 4]), np.array([1.0, 0.0, 1.0])
    for objective, output in (("closed_form", "reg"), ("sampled", "class"), ("sampled", "reg")):
        th = R.table_theta(ent, bia, 1)
        f = lambda t: R.fold(t, 1, items, y, ent, bia, scal, "softplus", output, objective, 0, 0.0, 0.7,
                             _eps(N + M, d, 1), 2)[1]
        # one Adam step of size lr moves every parameter by -lr sign(g): recover the signs from finite differences
        stepped, _ = R.fold(th, 1, items, y, ent, bia, scal, "softplus", output, objective, 1, 1e-3, 0.7,
                            _eps(N + M, d, 1), 2)
        flat = lambda t: np.concatenate([t[0], t[1], [t[2], t[3]]])
        p0 = flat(th)
        for k in range(2 * d + 2):
            e = np.zeros(2 * d + 2)
            e[k] = 1e-6
            unflat = lambda p: (p[:d], p[d:2 * d], p[2 * d], p[2 * d + 1])
            fd = (f(unflat(p0 + e)) - f(unflat(p0 - e))) / 2e-6
            assert np.sign(fd) == -np.sign(flat(stepped)[k] - p0[k]), (objective, k)


def test_planted_generator_is_well_conditioned_in_fp32():
    """The inputs of test_gpu_elicit.py::test_against_the_fp64_restatement_on_a_planted_model (its generator): at lr = 0.01 a numpy fp32 transcription of the folds stays 10x inside the 1e-4 tolerance of the fp64
    thetas, at lr = 0.05 fp32 rounding alone breaks it -- the reason the GPU test runs at lr = 0.01."""
    N, M, d, Q, n_steps = 32, 300, 8, 8, 20
    g = torch.Generator().manual_seed(2)
    mu = torch.randn(N + M, d, generator=g)
    ent = torch.cat([mu, torch.full((N + M, d), 0.05)], 1)
    bia = torch.stack([torch.randn(N + M, generator=g) * 0.1, torch.full((N + M,), 0.05)], 1)
    pool = torch.stack([torch.arange(N).repeat_interleave(40),
                        torch.cat([N + torch.randperm(M, generator=g)[:40] for _ in range(N)])], 1)
    truth = (mu[pool[:, 0]] * mu[pool[:, 1]]).sum(1) + bia[pool[:, 0], 0] + bia[pool[:, 1], 0]
    y_pool = truth + 0.5 * torch.randn(pool.shape[0], generator=g)
    E, B = ent.numpy().astype(np.float64), bia.numpy().astype(np.float64)
    S = np.array([4.0, 0.0, 0.05], dtype=np.float32).astype(np.float64)
    worst = {0.01: 0.0, 0.05: 0.0}
    for lr in worst:
        for u in range(N):
            sel = (pool[:, 0] == u).nonzero().reshape(-1)
            items, ys = pool[sel, 1].numpy(), y_pool[sel].numpy()
            s = R.session(u, items, ys, Q, "variance", E, B, S, n_steps=n_steps, lr=lr, reset=True)
            assert min(s["gap"]) > 1e-5
            for th, t32 in zip(s["theta"], R.closed_form_thetas_fp32(s["rows"], items, ys, E, B, S, n_steps, lr)):
                for a, b in ((t32[0], th[0]), (t32[1], th[1]), (t32[2], np.array(th[2:]))):
                    worst[lr] = max(worst[lr], float(np.abs(a - b).max() / np.abs(b).max()))
    assert worst[0.01] < 1e-5, worst
    assert worst[0.05] > 1e-4, worst


def test_per_round_generators_are_well_conditioned_in_fp32():
    """The inputs of test_gpu_elicit_shapes.py::test_rounds_against_the_fp64_restatement (R.FP64_CASES, built by
    R.planted_case: 16 users, 30-row pools, 5 rounds of 20 Adam steps at lr = 0.01, one draw per iteration).  The GPU test
    compares every round on its own -- R.fold from the theta the round starts from, on the history followed by the rows
    asked so far -- with the 1e-4 of test_trajectory_matches_fp64_adam, which bounds fp32 rounding and so means
    something only where a plain fp32 run of the same fold stays well inside it.  Here: the fp64 session's selections
    and starting thetas (rounded to fp32, as the kernel's are), each round folded by R.fold in fp32 and in fp64; the
    condition is 1e-5, 10x inside the tolerance.  The draws are numpy normals keyed on the iteration (the kernel's Philox
    stream needs a GPU; the condition is one on the inputs, not on the stream).  Largest distance over users, rounds
    and theta parts (max |fp32 - fp64| / max |fp64|), and of the loss:
      sampled, class, softplus, 12 history rows, 'mean', d = 33:      theta 7.3e-7, loss 1.8e-7
      sampled, reg, |.|, cold start (reset), 'variance', d = 300:     theta 5.4e-7, loss 7.6e-7
      closed form, reg, softplus, 12 history rows, 'top', d = 129:    theta 1.1e-6, loss 2.3e-7
    None of the three needed a change (item means of norm 1 at every d keep a one-row cold-start fold from
    overshooting)."""
    def eps_of(T, d):
        cache = {}

        def f(t):
            if t not in cache:
                g = np.random.default_rng([7, t])
                cache[t] = (g.normal(size=(T, d)).astype(np.float32), g.normal(size=T).astype(np.float32),
                            np.float32(g.normal()))
            return cache[t]
        return f

    f32 = lambda th: (th[0].astype(np.float32).astype(np.float64), th[1].astype(np.float32).astype(np.float64),
                      float(np.float32(th[2])), float(np.float32(th[3])))
    for name, (output, objective, kind, strategy, reset, n_hist, d) in R.FP64_CASES.items():
        c = R.planted_case(name)
        E, B, S = (c[k].astype(np.float64) for k in ("ent", "bia", "scal"))
        eps = eps_of(E.shape[0], d)
        worst, worst_loss, n_rounds = 0.0, 0.0, 0
        for u in range(R.FP64_USERS):
            sel, hs = np.nonzero(c["pool"][:, 0] == u)[0], np.nonzero(c["hist_x"][:, 0] == u)[0]
            assert len(sel) == R.FP64_POOL and len(hs) == n_hist
            s = R.session(u, c["pool"][sel, 1], c["y_pool"][sel], R.FP64_ROUNDS, strategy, E, B, S, kind=kind,
                          output=output, objective=objective, hist_items=c["hist_x"][hs, 1], hist_y=c["hist_y"][hs],
                          n_steps=R.FP64_STEPS, lr=R.FP64_LR, reset=reset, eps=eps)
            start = R.prior_theta(d, kind) if reset else R.table_theta(E, B, u)
            before = lambda q: f32(start if q == 0 else s["theta"][q - 1])
            r64 = R.rounds_along(name, c, u, s["rows"], before, eps)
            r32 = R.rounds_along(name, c, u, s["rows"], before, eps, dtype=np.float32)
            for a, b in zip(r64, r32):
                assert b[5][0].dtype == np.float32 and b[5][1].dtype == np.float32   # (nothing was promoted on the way)
                for x, y in ((b[5][0], a[5][0]), (b[5][1], a[5][1]), (np.array(b[5][2:]), np.array(a[5][2:]))):
                    worst = max(worst, float(np.abs(x - y).max() / np.abs(y).max()))
                worst_loss = max(worst_loss, abs(b[6] - a[6]) / abs(a[6]))
                n_rounds += 1
        assert n_rounds == R.FP64_USERS * R.FP64_ROUNDS
        assert worst < 1e-5 and worst_loss < 1e-5, (name, worst, worst_loss)


def test_fold_dtype_argument_leaves_fp64_callers_alone():
    """R.fold with no dtype, with dtype=float64 and as session's own round give the same numbers."""
    d, N, M = 3, 2, 6
    ent, bia, scal = _tables(N + M, d, 2)
    items, y = np.array([3, 5, 4]), np.array([1.0, 0.0, 1.0])
    for objective, output, kind in (("closed_form", "reg", "abs"), ("sampled", "class", "softplus")):
        args = (R.table_theta(ent, bia, 1), 1, items, y, ent, bia, scal, kind, output, objective, 5, 0.05, 0.7,
                _eps(N + M, d, 1), 2)
        (a, la), (b, lb) = R.fold(*args), R.fold(*args, dtype=np.float64)
        assert la == lb and all(np.array_equal(x, z) for x, z in zip(a, b))
        (c, lc) = R.fold(*args, dtype=np.float32)
        assert c[0].dtype == np.float32 and abs(lc - la) < 1e-4 * abs(la) and lc != la

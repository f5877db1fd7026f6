"""GPU: exact fold-in (VFM.fold_in_exact, include/vfm_foldin.h: vfm_foldin_solve_f32) -- the written rows against the
fp64 closed-form optimum solve_fp64 of test_foldin_exact_cpu.py and the returned loss against objective_fp64 at the
written rows, at every lane shape of the loss pass, at the edges of the dual / primal rule, with the triangle in LDS and
in the workspace; optimality against fold_in's Adam; independence of the start; frozen means frozen; determinism and
independence of the other entities; the lazy / look-ahead step forms; a 5,000-row entity; the empty call; the raw ABI.

Bounds: rel_err <= 1e-4 for the rows and <= 1e-5 for the loss, the two bounds test_gpu_foldin.py uses for trajectories
and for the objective; every comparison asserts cond(H) <= 1e3 of the oracle first, so that the bound tests the kernel
(fp64 operands, sums and factorisation, fp32 results: about 6e-8) and not the conditioning.  That holds for the primal
form: an entity with n <= d rows is solved in the dual form, whose conditioning is that of K = I / prec + U D^-1 U^T, not
of H; test_gpu_solve_edges.py asserts cond(K) for those and tests the dual path where cond(K) is large."""
import ctypes as C
import functools

import pytest
import torch

import test_gpu_foldin as G
from golden_util import rel_err
from test_foldin_exact_cpu import solve_fp64

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [  # link, field sizes, folded field, d, kl_weight: the closed-form CASES of test_gpu_foldin.py and d = 512
    ("abs", (40, 30), 0, 5, 1.0),
    ("softplus", (20, 30, 25), 1, 8, 0.7),
    ("abs", (20, 30, 25), 2, 128, 0.7),
    ("softplus", (40, 30), 1, 20, 1.0),
    ("abs", (20, 30, 25), 2, 512, 1.0),
]


def _tables(m):
    return m.entity_params.weight.detach().cpu(), m.bias_params.weight.detach().cpu(), m._scalars().cpu()


def _solve(m, X, y, field, kl_weight):
    """solve_fp64 on the model's current tables (the folded rows in them are not read)."""
    sol = solve_fp64(*_tables(m), X.cpu(), y.cpu(), field, m.link, kl_weight)
    assert float(sol["cond"].max()) <= 1e3, sol["cond"]
    return sol


def _check(m, X, y, field, kl_weight, out, sol, what=""):
    """The written rows against sol, the returned loss against objective_fp64 at the written rows."""
    ents = out["entities"]
    assert torch.equal(ents.cpu(), sol["entities"])
    e, d = ents.cpu(), m.d
    ent, bia = m.entity_params.weight.detach().cpu(), m.bias_params.weight.detach().cpu()
    errs = (rel_err(ent[e, :d].numpy(), sol["mu"].numpy()), rel_err(ent[e, d:].numpy(), sol["s"].numpy()),
            rel_err(bia[e].numpy(), torch.stack([sol["mu_w"], sol["s_w"]], 1).numpy()))
    th = G._theta(m, ents, grad=False)
    L = G._oracle(m, X, y, field, "closed_form", th, ents, kl_weight=kl_weight)
    el = rel_err(out["loss"].cpu().numpy(), L.numpy())
    print(f"{what} d={d} rows mu/s/bias {errs[0]:.2e} {errs[1]:.2e} {errs[2]:.2e} loss {el:.2e} "
          f"cond {float(sol['cond'].max()):.1f}")
    assert max(errs) <= 1e-4, errs
    assert el <= 1e-5, el
    assert out["rows"].tolist() == [int((X[:, field] == int(v)).sum()) for v in e]


@functools.lru_cache(maxsize=None)
def _case(i):
    """Shape i: the model's starting parameters, the rows and the oracle, computed once and left unchanged."""
    link, sizes, field, d, klw = SHAPES[i]
    m = G._model(sizes, d, "reg", link, seed=d + field)
    X, y = G._rows(m, field, 7, 60, seed=d)
    return m, m._flat.clone(), X, y, _solve(m, X, y, field, klw)


@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_rows_and_loss_match_fp64(i):
    field, klw = SHAPES[i][2], SHAPES[i][4]
    m, start, X, y, sol = _case(i)
    m._flat.copy_(start)
    out = m.fold_in_exact(X, y, field=field, kl_weight=klw)
    _check(m, X, y, field, klw, out, sol, "shape")


@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_no_worse_than_adam(i):
    """A global optimum: L_exact <= L_adam (1 + 1e-5), the 1e-5 at which the two fp32 loss evaluations agree with fp64."""
    field, klw = SHAPES[i][2], SHAPES[i][4]
    m, start, X, y, _ = _case(i)
    m._flat.copy_(start)
    exact = m.fold_in_exact(X, y, field=field, kl_weight=klw)["loss"].double()
    for n_steps, lr in ((200, 0.05), (2000, 0.01)):
        m._flat.copy_(start)
        adam = m.fold_in(X, y, field=field, n_steps=n_steps, lr=lr, kl_weight=klw)["loss"].double()
        gap = ((adam - exact) / exact).cpu()
        print(f"d={m.d} n_steps={n_steps} lr={lr}: (L_adam - L_exact) / L_exact in [{float(gap.min()):.2e}, {float(gap.max()):.2e}]")
        assert bool((exact <= adam * (1 + 1e-5)).all()), (exact, adam)
    m._flat.copy_(start)


@functools.lru_cache(maxsize=None)
def _edges():
    """d = 8, F = 3: entities with n = 1, 7, 8 (= d, the last dual), 9 (= d + 1, the first primal) and 40 rows, some
    rows duplicated, all rows shuffled so that the entities interleave in X."""
    m = G._model((20, 30, 25), 8, "reg", "softplus", seed=11)
    g = torch.Generator().manual_seed(5)
    rows = []
    for k, n in enumerate((1, 7, 8, 9, 40)):
        x = torch.stack([torch.randint(0, 20, (n,), generator=g), torch.full((n,), 20 + 3 * k + 1),
                         50 + torch.randint(0, 25, (n,), generator=g)], 1)
        if n >= 7:
            x[-1] = x[0]                    # duplicates count twice
            x[-2] = x[0]
        rows.append(x)
    X = torch.cat(rows)
    X = X[torch.randperm(X.shape[0], generator=g)]
    y = torch.randn(X.shape[0], generator=g) + 3.0
    X, y = X.to(DEV), y.to(DEV)
    return m, m._flat.clone(), X, y, _solve(m, X, y, 1, 0.7)


def test_system_form_edges():
    m, start, X, y, sol = _edges()
    m._flat.copy_(start)
    out = m.fold_in_exact(X, y, field=1, kl_weight=0.7)
    assert out["rows"].tolist() == [1, 7, 8, 9, 40]
    _check(m, X, y, 1, 0.7, out, sol, "edges")


def test_workspace_path():
    from vae_amd import foldin
    m, start, X, y, sol = _edges()
    m._flat.copy_(start)
    lds = m.fold_in_exact(X, y, field=1, kl_weight=0.7)
    lds_flat = m._flat.clone()
    m._flat.copy_(start)
    ents, loss, rows = foldin.run_exact(m, X, y, 1, 0.7, lds_dim=4)          # n = 7, 8, 9 (primal), 40 (primal): workspace
    _check(m, X, y, 1, 0.7, dict(entities=ents, loss=loss, rows=rows), sol, "lds_dim=4")
    assert rel_err(m._flat.cpu().numpy(), lds_flat.cpu().numpy()) <= 1e-6
    assert rel_err(loss.cpu().numpy(), lds["loss"].cpu().numpy()) <= 1e-6
    m._flat.copy_(start)
    # d = 512, one entity of 600 rows: the primal 513 x 513 system, 1 MB, never in LDS
    m = G._model((20, 30, 25), 512, "reg", "abs", seed=2)
    X, y = G._rows(m, 2, 1, 600, seed=3)
    sol = _solve(m, X, y, 2, 1.0)
    out = m.fold_in_exact(X, y, field=2)
    assert out["rows"].tolist() == [600]
    _check(m, X, y, 2, 1.0, out, sol, "513x513")


def test_independent_of_the_start():
    field, klw = SHAPES[1][2], SHAPES[1][4]
    m, start, X, y, _ = _case(1)
    m._flat.copy_(start)
    a = m.fold_in_exact(X, y, field=field, kl_weight=klw)
    flat_a = m._flat.clone()
    m._flat.copy_(start)
    ents = a["entities"]
    g = torch.Generator().manual_seed(9)
    m.entity_params.weight.data[ents] = (torch.randn(ents.numel(), 2 * m.d, generator=g) * 3).to(DEV)
    m.bias_params.weight.data[ents] = (torch.randn(ents.numel(), 2, generator=g) * 3).to(DEV)
    b = m.fold_in_exact(X, y, field=field, kl_weight=klw)
    assert torch.equal(a["loss"], b["loss"]) and torch.equal(m._flat, flat_a)
    m._flat.copy_(start)


def test_frozen_means_frozen():
    m, _ = G._trained()
    m.save_weights()
    before = {k: getattr(m, k).clone() for k in ("_flat", "_adam_m", "_adam_v", "_last_flat", "_mean_flat")}
    t_before = m._adam_t
    X, y = G._fold_rows(m)
    out = m.fold_in_exact(X, y)
    changed = torch.zeros(m._n_flat, dtype=torch.bool, device=DEV)
    for e in out["entities"].tolist():
        changed[e * 2 * m.d:(e + 1) * 2 * m.d] = True
        changed[m._off_bias + 2 * e: m._off_bias + 2 * e + 2] = True
    assert torch.equal(m._flat[~changed], before["_flat"][~changed])
    assert not torch.equal(m._flat[changed], before["_flat"][changed])
    for k in ("_adam_m", "_adam_v", "_last_flat", "_mean_flat"):
        assert torch.equal(getattr(m, k), before[k]), k
    assert m._adam_t == t_before
    assert torch.isfinite(out["loss"]).all()


def test_deterministic_and_independent_of_the_other_entities():
    m, _ = G._trained()
    X, y = G._fold_rows(m, n_ent=7)
    start = m._flat.clone()
    outs = []
    for _ in range(2):
        m._flat.copy_(start)
        outs.append((m.fold_in_exact(X, y), m._flat.clone()))
    assert torch.equal(outs[0][0]["loss"], outs[1][0]["loss"]) and torch.equal(outs[0][1], outs[1][1])
    together = outs[0][1]
    alone = start.clone()
    assert outs[0][0]["entities"].numel() == 7
    for i, e in enumerate(outs[0][0]["entities"].tolist()):              # each alone = each among six others
        m._flat.copy_(start)
        sel = X[:, 0] == e
        o = m.fold_in_exact(X[sel], y[sel])
        assert torch.equal(o["loss"], outs[0][0]["loss"][i:i + 1])
        rows = slice(e * 2 * m.d, (e + 1) * 2 * m.d)
        alone[rows] = m._flat[rows]
        alone[m._off_bias + 2 * e: m._off_bias + 2 * e + 2] = m._flat[m._off_bias + 2 * e: m._off_bias + 2 * e + 2]
    assert torch.equal(alone, together)


@pytest.mark.parametrize("form", ["lazy", "lookahead"])
def test_step_forms_rows_that_lag(form):
    """test_step_forms of test_gpu_foldin.py with fold_in_exact in fold_in's place: folding into rows that lag behind the
    last step = folding into the synced model, and the next train_steps = those after a direct write of the same rows +
    params_changed(), all bit for bit."""
    kw = dict(lazy=True) if form == "lazy" else dict(lookahead=True)
    a, pa = G._trained(**kw)
    b, _ = G._trained(**kw)
    c, pc = G._trained(**kw)
    assert a._lazy_dirty and b._lazy_dirty                 # rows lag behind the last step
    X, y = G._fold_rows(a)
    oa = a.fold_in_exact(X, y)
    b.sync_lazy()
    ob = b.fold_in_exact(X, y)
    assert torch.equal(a._flat, b._flat) and torch.equal(oa["loss"], ob["loss"])
    c.sync_lazy()
    ents = oa["entities"]
    c.entity_params.weight.data[ents] = a.entity_params.weight.data[ents]
    c.bias_params.weight.data[ents] = a.bias_params.weight.data[ents]
    c.params_changed()
    _steps_equal(form, a, pa, c, pc)


def _steps_equal(form, a, pa, c, pc):
    assert torch.equal(a._flat, c._flat)
    for s in range(3):
        la, _ = a.train_step(pa[(12 + s) % 30], next_plan=pa[(13 + s) % 30] if form == "lookahead" else None)
        lc, _ = c.train_step(pc[(12 + s) % 30], next_plan=pc[(13 + s) % 30] if form == "lookahead" else None)
        assert torch.equal(la, lc)
    a.sync_lazy()
    c.sync_lazy()
    assert torch.equal(a._flat, c._flat) and torch.equal(a._adam_m, c._adam_m) and torch.equal(a._adam_v, c._adam_v)


@pytest.mark.parametrize("form", ["lazy", "lookahead"])
def test_step_forms(form):
    """After a few train_steps in the lazy / look-ahead form, fold_in_exact followed by train_steps equals writing
    solve_fp64's rows (rounded to fp32) directly and then stepping, at the tolerance of test_gpu_foldin.py's
    test_step_forms: equality.

    Equality holds because the kernel solves in fp64 from fp64 row operands (k_foldin_solve_prep), as solve_fp64
    does: the two optima differ by about 1e-15 cond(H), far below the last fp32 bit of the rows.  (From the fp32 operand
    table of k_foldin_prep 39 of the 204 values differed in that bit.)"""
    kw = dict(lazy=True) if form == "lazy" else dict(lookahead=True)
    a, pa = G._trained(**kw)
    c, pc = G._trained(**kw)
    X, y = G._fold_rows(a)
    oa = a.fold_in_exact(X, y)
    c.sync_lazy()
    sol = _solve(c, X, y, 0, 1.0)
    _check(a, X, y, 0, 1.0, oa, sol, form)
    ents = oa["entities"]
    ref_e = torch.cat([sol["mu"], sol["s"]], 1).float().to(DEV)
    ref_b = torch.stack([sol["mu_w"], sol["s_w"]], 1).float().to(DEV)
    got_e, got_b = a.entity_params.weight.data[ents], a.bias_params.weight.data[ents]
    print(f"{form}: {int((ref_e != got_e).sum()) + int((ref_b != got_b).sum())} of {ref_e.numel() + ref_b.numel()} "
          f"fp32 values of solve_fp64 differ from the kernel's, by at most "
          f"{float(((ref_e - got_e).abs() / ref_e.abs().clamp_min(1e-30)).max()):.2e} relative")
    c.entity_params.weight.data[ents] = ref_e
    c.bias_params.weight.data[ents] = ref_b
    c.params_changed()
    _steps_equal(form, a, pa, c, pc)


def test_heavy_entity():
    """One entity of 5,000 rows (primal 129 x 129) among 200 of 20 rows (dual 20 x 20), d = 128."""
    m = G._model((400, 300), 128, "reg", "abs", seed=4)
    g = torch.Generator().manual_seed(6)
    users = torch.randperm(400, generator=g)[:201]
    n = torch.full((201,), 20, dtype=torch.int64)
    n[7] = 5000
    u = torch.repeat_interleave(users, n)
    X = torch.stack([u, 400 + torch.randint(0, 300, (u.numel(),), generator=g)], 1).to(DEV)
    y = (torch.randn(u.numel(), generator=g) + 3.0).to(DEV)
    out = m.fold_in_exact(X, y)
    assert out["entities"].numel() == 201 and int(out["rows"].max()) == 5000
    pick = torch.unique(torch.cat([users[7:8], users[torch.randperm(201, generator=g)[:12]]])).to(DEV)
    sel = torch.isin(X[:, 0], pick)
    sol = _solve(m, X[sel], y[sel], 0, 1.0)
    pos = torch.searchsorted(out["entities"], pick)
    sub = dict(entities=out["entities"][pos], loss=out["loss"][pos], rows=out["rows"][pos])
    _check(m, X[sel], y[sel], 0, 1.0, sub, sol, "heavy")


def test_empty_fold_in_exact_does_nothing():
    m = G._model((10, 12), 8)
    before = m._flat.clone()
    out = m.fold_in_exact(torch.zeros(0, 2, dtype=torch.int64), torch.zeros(0))
    assert out["entities"].numel() == 0 and out["loss"].numel() == 0 and out["rows"].numel() == 0
    assert torch.equal(m._flat, before)


def test_raw_abi_rejects_before_launching():
    """vfm_foldin_solve_f32 on live device pointers: VFM_E_INVALID, and nothing written, for kl_weight = 0, the sampled
    objective, Bernoulli, d > 512 and a short workspace; the same struct with nothing wrong runs."""
    from vae_amd import _lib, foldin
    lib = _lib.load()
    m = G._model((40, 30), 5, "reg", "abs", seed=1)
    X, y = G._rows(m, 0, 4, 30, seed=2)
    xs, ys, ents, ptr, _ = foldin.row_lists(X, y, 0)
    op_x, row_op = foldin.partner_tuples(xs, 0)
    E, d = ents.numel(), m.d
    need = lib.vfm_foldin_solve_workspace_bytes(E, op_x.shape[0], d, 0)      # (lds_dim = 0: slabs included)
    assert need > lib.vfm_foldin_solve_workspace_bytes(E, op_x.shape[0], d, -1) > 0
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    loss = torch.full((E,), -7.0, device=DEV)
    ent, bia, scal = m._views(m._flat)
    before = m._flat.clone()

    def call(**kw):
        p = _lib.FoldinSolve()
        args = dict(E=E, R=ys.numel(), T=m.T, n_ops=op_x.shape[0], F=2, d=d, col=0, objective=_lib.OBJ_CLOSED_FORM,
                    likelihood=_lib.LIK_NORMAL, flags=0, lds_dim=0, kl_weight=1.0, entities=ents.data_ptr(),
                    row_ptr=ptr.data_ptr(), y=ys.data_ptr(), op_x=op_x.data_ptr(), row_op=row_op.data_ptr(),
                    entity_params=ent.data_ptr(), bias_params=bia.data_ptr(), scalars=scal.data_ptr(),
                    out_loss=loss.data_ptr(), workspace=ws.data_ptr(), workspace_bytes=need)
        args.update(kw)
        for k, v in args.items():
            setattr(p, k, v)
        rc = lib.vfm_foldin_solve_f32(C.byref(p), C.c_void_p(_lib.raw_stream(torch.device(DEV))))
        torch.cuda.synchronize()
        return rc

    bad = _lib._gen.VFM_E_INVALID
    for kw in (dict(kl_weight=0.0), dict(objective=_lib.OBJ_SAMPLED), dict(likelihood=_lib.LIK_BERNOULLI), dict(d=513),
               dict(workspace_bytes=need - 1)):
        assert call(**kw) == bad, kw
        assert lib.vfm_last_error()
        assert torch.equal(m._flat, before) and bool((loss == -7.0).all()) and not bool(ws.any()), kw
    assert call() == 0
    assert torch.isfinite(loss).all() and not torch.equal(m._flat, before)
    sol = _solve_from(before, m, X, y)
    e = ents.cpu()
    assert rel_err(m.entity_params.weight.detach().cpu()[e, :d].numpy(), sol["mu"].numpy()) <= 1e-4


def _solve_from(flat, m, X, y):
    now = m._flat.clone()
    m._flat.copy_(flat)
    sol = _solve(m, X, y, 0, 1.0)
    m._flat.copy_(now)
    return sol

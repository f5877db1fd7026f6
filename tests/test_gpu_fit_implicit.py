"""GPU: the implicit-feedback solves (include/vfm_implicit.h: VFM.fold_in_implicit, implicit_objective, fit_implicit)
against the fp64 reference of tests/implicit_reference.py, which solves every entity from its dense row set.

Bounds.  Rows written by a solve: per element |got - ref| <= 2^-23 |ref| + 4 (d + 1) 2^-52 cond(H) max|ref|
(solve_reference.elementwise_ok / solve_abs_term), after asserting cond(H) <= 1e3 on the reference's own matrix; the
scales with solve_reference.scale_abs_term over the dense row count.  The tables are planted (implicit_reference.planted:
means of size 0.3, scales in [0.2, 0.6], so that cond(H) stays below about 1 / (0.3^2 + 0.2^2)).  Losses and J_imp: the
1e-5 relative of test_gpu_fit_exact.py.  J_imp after a block: J_after <= J_before + 1e-9 |J_before|, as there.  The C ABI
takes w0, w1 and kl_weight as floats, so the tests use fp32-representable values for them.

Measured on an MI355X: worst elementwise ratio of the solve 0.498 (1 = at the bound; the reference itself rounded to fp32
gives at most 0.5), of the field blocks of fit_implicit 0.493; losses within 6.2e-8 and J_imp within 5.1e-9 relative."""
import functools

import numpy as np
import pytest
import torch

import implicit_reference as IR
import solve_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
LINKS = ["abs", "softplus"]
CHUNK = 16
W0, W1, KLW = R.f32(0.15), 1.25, R.f32(0.7)            # (the C ABI takes the weights and kl_weight as floats)


def _case(n_folded, n_partner, d, link, counts, seed, field=0):
    """fp32 planted tables and observed rows in which entity k of the folded field has counts[k] distinct partners
    (entities past len(counts) have none)."""
    N, M = (n_folded, n_partner) if field == 0 else (n_partner, n_folded)
    ent, bia, scal, _, _ = IR.planted(N, M, d, seed, dtype=torch.float32)
    g = torch.Generator().manual_seed(seed + 1)
    flo, plo = (0, N) if field == 0 else (N, 0)
    rows = []
    for k, n in enumerate(counts):
        assert n <= n_partner
        j = torch.randperm(n_partner, generator=g)[:n] + plo
        e = torch.full((n,), flo + k, dtype=torch.int64)
        rows.append(torch.stack([e, j] if field == 0 else [j, e], 1))
    x = torch.cat(rows) if rows else torch.zeros(0, 2, dtype=torch.int64)
    x = x[torch.randperm(x.shape[0], generator=g)]
    y = (torch.randn(x.shape[0], generator=g) * 0.5 + 1.0).float()
    return dict(N=N, M=M, d=d, link=link, field=field, ent=ent, bia=bia, scal=scal, x=x, y=y, counts=list(counts),
                sizes=(N, M))


def _model_of(c):
    from vae_amd.model import VFM
    torch.manual_seed(0)
    m = VFM(field_sizes=list(c["sizes"]), embedding_size=c["d"], output="reg", link=c["link"], device=DEV)
    m.entity_params.weight.data.copy_(c["ent"])
    m.bias_params.weight.data.copy_(c["bia"])
    m._flat[m._off_scal: m._off_scal + 3] = c["scal"].to(DEV)
    return m


def _tables_of(m):
    ent, bia, scal = m._views(m._flat)
    return ent.detach().cpu().clone(), bia.detach().cpu().clone(), scal.detach().cpu().clone()


def _written(m, ids):
    d = m.d
    ent = m.entity_params.weight.detach()[ids.to(DEV)].cpu()
    bia = m.bias_params.weight.detach()[ids.to(DEV)].cpu()
    return torch.cat([bia[:, :1], ent[:, :d]], 1), torch.cat([bia[:, 1:], ent[:, d:]], 1)


def _fold(c, m, field=None, w0=W0, w1=W1, klw=KLW, **kw):
    kw.setdefault("chunk_rows", CHUNK)
    return m.fold_in_implicit(c["x"].to(DEV), c["y"].to(DEV), c["field"] if field is None else field, w0=w0, w1=w1,
                              kl_weight=klw, **kw)


def _check(tab, c, m, out, what, field=None, w0=W0, w1=W1, klw=KLW, factor=1.0):
    """The rows of out["entities"] written into m against implicit_solve_fp64 from the tables `tab` per element, and
    out["loss"] against entity_loss_fp64 at the written rows.  Returns (worst elementwise ratio, worst loss error)."""
    field = c["field"] if field is None else field
    ent, bia, scal = tab
    N, M, d, link = c["N"], c["M"], c["d"], c["link"]
    ids = out["entities"].cpu()
    sol = IR.implicit_solve_fp64(ent, bia, scal, c["x"], c["y"], field, N, M, link, w0, w1, klw, entities=ids)
    assert float(sol["cond"].max()) <= 1e3, sol["cond"]
    theta, s = _written(m, ids)
    n_dense = M if field == 0 else N
    rs = IR.inv_link_t(sol["sigma"], link)
    worst, worst_l = 0.0, 0.0
    for i, e in enumerate(ids.tolist()):
        rt = sol["theta"][i].numpy()
        ok_t, w_t = R.elementwise_ok(theta[i], rt, factor * R.solve_abs_term(d, float(sol["cond"][i]), rt))
        ok_s, w_s = R.elementwise_ok(s[i], rs[i].numpy(), factor * R.scale_abs_term(2 * n_dense, rs[i].numpy()))
        assert ok_t and ok_s, (what, e, int(out["rows"][i]), w_t, w_s)
        worst = max(worst, w_t, w_s)
        L = float(IR.entity_loss_fp64(ent, bia, scal, c["x"], c["y"], field, N, M, link, w0, w1, klw, e,
                                      theta[i], IR.link_t(s[i], link)))
        err = abs(float(out["loss"][i]) - L) / abs(L)
        assert err <= 1e-5, (what, e, float(out["loss"][i]), L)
        worst_l = max(worst_l, err)
    print(f"IMPLICIT {what} {link} d={d} field={field}: worst ratio {worst:.3f}, loss rel_err {worst_l:.2e}")
    return worst, worst_l


def _counts(d, split):
    k = split // CHUNK + 2
    return [0, 1, d, d + 1, split, split + 1, CHUNK * k - 1, CHUNK * k, CHUNK * k + 1, CHUNK * 40]


# ---------------------------------------------------------------------------------------------------------------------
# the solve against implicit_solve_fp64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("d", [1, 8, 9, 33, 128])
def test_solve_matches_fp64(d, link, field):
    from vae_amd import sweep
    split = sweep.resolve_split_rows(20, d)                                # (max(20, d + 1))
    counts = _counts(d, split)
    c = _case(len(counts) + 1, CHUNK * 40 + 5, d, link, counts, seed=500 + d, field=field)
    m = _model_of(c)
    tab = _tables_of(m)
    out = _fold(c, m, split_rows=20)
    assert out["rows"].tolist() == counts + [0] and out["entities"].numel() == len(counts) + 1
    _check(tab, c, m, out, "solve")


@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("d", [R.LDS - 1, R.LDS])
def test_triangle_in_lds_and_in_the_slab(d, link):
    counts = [0, d + 2, CHUNK * (d // CHUNK + 2) + 1]
    c = _case(4, 200, d, link, counts, seed=600 + d)
    m = _model_of(c)
    tab = _tables_of(m)
    assert R.has_slabs(d) == (d == R.LDS)
    out = _fold(c, m, split_rows=d + 3)                                    # the second in its workgroup, the third in chunks
    _check(tab, c, m, out, "lds/slab")


@pytest.mark.parametrize("n_partner", [1, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5])
def test_catalog_sizes(n_partner):
    d = 8
    counts = sorted({0, 1, min(n_partner, d + 1), n_partner})
    for link, field in (("abs", 0), ("softplus", 1)):
        c = _case(len(counts), n_partner, d, link, counts, seed=700 + n_partner, field=field)
        m = _model_of(c)
        tab = _tables_of(m)
        out = _fold(c, m, split_rows=0)
        _check(tab, c, m, out, f"catalog {n_partner}")


# ---------------------------------------------------------------------------------------------------------------------
# identity with the exact fold-in at w0 = w1, the objective, bits, the existing paths
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("field", [0, 1])
def test_equal_weights_are_the_exact_fold_in_of_the_dense_rows(field, link):
    w, d = 0.5, 8                                                          # (KLW / w is exact in fp32)
    c = _case(6, 40, d, link, [0, 3, 12, 40, 25], seed=800 + field, field=field)
    N, M = c["N"], c["M"]
    m, m2 = _model_of(c), _model_of(c)
    tab = _tables_of(m)
    out = _fold(c, m, w0=w, w1=w, split_rows=0)
    _, Y = IR.dense_targets(c["x"], c["y"], N, M, w, w)
    uu, ii = torch.meshgrid(torch.arange(N), torch.arange(N, N + M), indexing="ij")
    xd = torch.stack([uu.reshape(-1), ii.reshape(-1)], 1)
    ex = m2.fold_in_exact(xd.to(DEV), Y.reshape(-1).float().to(DEV), field=field, kl_weight=KLW / w)
    assert torch.equal(ex["entities"], out["entities"])
    # each lies within one bound of the same optimum: the implicit rows within 1 x (checked), the pair within 2 x
    _check(tab, c, m, out, "w0 = w1", w0=w, w1=w)
    ids = out["entities"].cpu()
    sol = IR.implicit_solve_fp64(*tab, c["x"], c["y"], field, N, M, link, w, w, KLW, entities=ids)
    ta, sa = _written(m, ids)
    tb, sb = _written(m2, ids)
    n_dense = M if field == 0 else N
    for i in range(ids.numel()):
        rt = sol["theta"][i].numpy()
        bound_t = R.EPS32 * np.abs(rt) + R.solve_abs_term(d, float(sol["cond"][i]), rt)
        assert (np.abs(ta[i].double().numpy() - tb[i].double().numpy()) <= 2 * bound_t).all(), i
        rs = IR.inv_link_t(sol["sigma"][i], link).numpy()
        bound_s = R.EPS32 * np.abs(rs) + R.scale_abs_term(2 * n_dense, rs)
        assert (np.abs(sa[i].double().numpy() - sb[i].double().numpy()) <= 2 * bound_s).all(), i


@pytest.mark.parametrize("link", LINKS)
def test_implicit_objective_matches_fp64(link):
    c = _case(30, 50, 9, link, [0, 1, 7, 50, 20, 33], seed=900)
    m = _model_of(c)
    for klw in (1.0, KLW):
        J = m.implicit_objective(c["x"].to(DEV), c["y"].to(DEV), w0=W0, w1=W1, kl_weight=klw)
        ref = float(IR.brute_J(c["ent"], c["bia"], c["scal"], c["x"], c["y"], c["N"], c["M"], link, W0, W1, klw))
        print(f"IMPLICIT objective {link} kl {klw}: rel_err {abs(J - ref) / abs(ref):.2e}")
        assert abs(J - ref) <= 1e-5 * abs(ref), (J, ref)
    ones = m.implicit_objective(c["x"].to(DEV), None, w0=W0)
    ref = float(IR.brute_J(c["ent"], c["bia"], c["scal"], c["x"], torch.ones(c["x"].shape[0]), c["N"], c["M"], link,
                           W0, 1.0, 1.0))
    assert abs(ones - ref) <= 1e-5 * abs(ref)


def _rows_of(m, flat, e):
    d = m.d
    return torch.cat([flat[e * 2 * d:(e + 1) * 2 * d], flat[m._off_bias + 2 * e: m._off_bias + 2 * e + 2]])


@functools.lru_cache(maxsize=None)
def _mixed():
    """60 entities of 0 .. 11 observed rows and three heavy ones (100, 61 and 47 rows), d = 8, softplus."""
    counts = [g % 12 for g in range(60)]
    counts[17], counts[40], counts[41] = 100, 61, 47
    c = _case(60, 130, 8, "softplus", counts, seed=55)
    m = _model_of(c)
    return c, m, m._flat.clone()


def test_bits_do_not_depend_on_the_call():
    c, m, start = _mixed()
    kw = dict(split_rows=20)
    out = _fold(c, m, **kw)
    flat = m._flat.clone()
    assert out["rows"].tolist() == c["counts"]
    m._flat.copy_(start)
    again = _fold(c, m, **kw)                                              # repeated calls
    assert torch.equal(m._flat, flat) and torch.equal(again["loss"], out["loss"])
    # groups: a workspace cap that holds one heavy entity's chunks at a time
    from vae_amd import _lib, foldin, sweep
    one = _lib.load().vfm_implicit_solve_workspace_bytes(1, 6, 8, -1)     # (7, 4 and 3 chunks: no two fit together)
    x, y, _, _ = sweep.check_implicit_args(m, c["x"].to(DEV), c["y"].to(DEV), W0, W1, KLW)
    plan = sweep.ImplicitPlan(m, x, y, 0, None, 20, CHUNK, one)
    assert len(plan.obs.groups) == 3 and plan.obs.n_light == 52 and plan.empty.numel() == 5
    m._flat.copy_(start)
    grouped = _fold(c, m, max_workspace_bytes=one, **kw)
    assert torch.equal(m._flat, flat) and torch.equal(grouped["loss"], out["loss"])
    # alone: a heavy entity, a light one, one without rows
    for e in (17, 40, 5, 0, 59):
        m._flat.copy_(start)
        alone = _fold(c, m, entities=[e], **kw)
        assert alone["entities"].tolist() == [e] and alone["rows"].tolist() == [c["counts"][e]]
        assert torch.equal(alone["loss"], out["loss"][e:e + 1]), e
        assert torch.equal(_rows_of(m, m._flat, e), _rows_of(m, flat, e)), e
        other = (e + 1) % 60
        assert torch.equal(_rows_of(m, m._flat, other), _rows_of(m, start, other))       # nothing else is written
    m._flat.copy_(start)


def test_existing_exact_paths_keep_their_bits():
    c = _case(12, 60, 8, "abs", [3, 9, 10, 40, 25, 1], seed=77)
    X, y = c["x"].to(DEV), c["y"].to(DEV)

    def exact(m):
        a = m.fold_in_exact(X, y, field=0, kl_weight=KLW)
        b = m.fold_in_exact(X, y, field=1, kl_weight=KLW, split_rows=0, chunk_rows=4)
        f = m.fit_exact(X, y, n_sweeps=2, kl_weight=KLW, split_rows=9, chunk_rows=4)
        return a["loss"].clone(), b["loss"].clone(), m._flat.clone(), f["objective"]

    before = exact(_model_of(c))
    _fold(c, _model_of(c), split_rows=0)                                   # the implicit kernels run on a clone
    _model_of(c).fit_implicit(X, None, 1, w0=W0, chunk_rows=CHUNK)
    after = exact(_model_of(c))
    assert all(torch.equal(p, q) for p, q in zip(before[:3], after[:3])) and before[3] == after[3]


# ---------------------------------------------------------------------------------------------------------------------
# the sweeps
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("link", LINKS)
def test_three_sweeps_block_by_block(link):
    counts = [0, 1, 5, 30, 12, 21, 40, 3, 0, 17]
    c = _case(12, 45, 5, link, counts, seed=1000)
    N, M = c["N"], c["M"]
    m = _model_of(c)
    g = torch.Generator().manual_seed(3)
    m._ensure_opt_state()
    m._adam_m.copy_(torch.randn(m._adam_m.shape, generator=g).to(DEV))
    m._adam_v.copy_(torch.rand(m._adam_v.shape, generator=g).to(DEV))
    adam = (m._adam_m.clone(), m._adam_v.clone())
    X, y = c["x"].to(DEV), c["y"].to(DEV)
    args = (c["x"], c["y"], N, M, link, W0, W1)
    state = {"tab": _tables_of(m), "J": [], "whats": [], "worst": 0.0}
    state["J"].append(float(IR.gram_J(*state["tab"][:3], *args, KLW)))

    def on_step(sweep, what):
        before = state["tab"]
        now = _tables_of(m)
        state["whats"].append((sweep, what))
        if what == "scalars":
            s1 = IR.bias_block_fp64(before[0], before[1], before[2].double(), *args, KLW)
            s2 = IR.precision_block_fp64(before[0], before[1], s1, *args)
            assert torch.equal(now[0], before[0]) and torch.equal(now[1], before[1])
            # the observed rows' moments are the fp32 kernel's: 1e-5 relative, as for the losses
            assert torch.allclose(now[2].double(), s2, rtol=1e-5, atol=1e-7), (now[2], s2)
        else:
            lo, hi = (0, N) if what == 0 else (N, N + M)
            ids = torch.arange(lo, hi)
            sol = IR.implicit_solve_fp64(*before, c["x"], c["y"], what, N, M, link, W0, W1, KLW)
            assert float(sol["cond"].max()) <= 1e3
            theta, s = _written(m, ids)
            rs = IR.inv_link_t(sol["sigma"], link)
            for i in range(ids.numel()):
                rt = sol["theta"][i].numpy()
                ok_t, w_t = R.elementwise_ok(theta[i], rt, R.solve_abs_term(c["d"], float(sol["cond"][i]), rt))
                ok_s, w_s = R.elementwise_ok(s[i], rs[i].numpy(), R.scale_abs_term(2 * (hi - lo + N + M), rs[i].numpy()))
                assert ok_t and ok_s, (sweep, what, i, w_t, w_s)
                state["worst"] = max(state["worst"], w_t, w_s)
            olo, ohi = (N, N + M) if what == 0 else (0, N)
            assert torch.equal(now[0][olo:ohi], before[0][olo:ohi]) and torch.equal(now[2], before[2])
        J = float(IR.gram_J(*now, *args, KLW))
        got = m.implicit_objective(X, y, w0=W0, w1=W1, kl_weight=KLW)
        assert abs(got - J) <= 1e-5 * abs(J), (sweep, what, got, J)
        assert J <= state["J"][-1] + 1e-9 * abs(state["J"][-1]), (sweep, what, J, state["J"][-1])
        state["J"].append(J)
        state["tab"] = now

    out = m.fit_implicit(X, y, 3, w0=W0, w1=W1, kl_weight=KLW, split_rows=9, chunk_rows=CHUNK, on_step=on_step)
    assert state["whats"] == [(s, w) for s in range(3) for w in (0, 1, "scalars")]
    assert out["sweeps"] == 3 and len(out["objective"]) == 4 and len(out["ms"]) == 3
    for k, J in enumerate(out["objective"]):
        ref = state["J"][3 * k]
        assert abs(J - ref) <= 1e-5 * abs(ref), (k, J, ref)
    assert state["J"][-1] < state["J"][0]
    print(f"IMPLICIT sweeps {link}: worst ratio {state['worst']:.3f}, J {state['J'][0]:.4f} -> {state['J'][-1]:.4f}")
    assert torch.equal(m._adam_m, adam[0]) and torch.equal(m._adam_v, adam[1])


# ---------------------------------------------------------------------------------------------------------------------
# guards and E = 0 (supplied out-of-range ids only)
# ---------------------------------------------------------------------------------------------------------------------
def test_guards_and_an_empty_call():
    from vae_amd import _lib, foldin
    c = _case(6, 40, 8, "abs", [3, 12, 0, 30], seed=1100)
    m = _model_of(c)
    o = _lib.ops()
    d, N, M, T = 8, c["N"], c["M"], c["N"] + c["M"]
    tables = m._views(m._flat)
    base = torch.empty(o.implicit_base_doubles(d), dtype=torch.float64, device=DEV)
    ws = torch.empty(o.implicit_base_workspace_bytes(M, CHUNK, d), dtype=torch.uint8, device=DEV)
    o.implicit_base(*tables, ws, base, N, M, CHUNK, 0)
    order = torch.sort(c["x"][:, 0], stable=True).indices
    xs, ys = c["x"][order], c["y"][order].to(DEV)
    partner = xs[:, 1].clone()
    partner[4] = T + 7                                                     # a row of entity 1: outside the table
    partner[20] = 2                                                        # a row of entity 3: inside it, outside the range
    ents = torch.tensor([0, 1, 2, 3, -1, T], device=DEV)
    ptr = torch.tensor([0, 3, 15, 15, 45, 45, 45], device=DEV)
    start = m._flat.clone()

    def solve(ents, row_ptr, cptr, tab, n_chunks):
        loss = torch.full((ents.numel(),), 7.0, device=DEV)
        w = torch.empty(max(o.implicit_solve_workspace_bytes(ents.numel(), n_chunks, d, -1), 1), dtype=torch.uint8, device=DEV)
        o.foldin_solve_implicit(ents, row_ptr, cptr, tab, ys, partner.to(DEV), base, *tables, w, loss, N, M, 0, -1, KLW, W0, W1)
        torch.cuda.synchronize()
        return loss

    def verify(loss):
        flat = m._flat
        assert bool(torch.isnan(loss[4])) and bool(torch.isnan(loss[5]))   # ids outside the table: NaN, nothing written
        for g in (1, 3):
            row = _rows_of(m, flat, g)
            assert bool(torch.isnan(row[:2 * d]).all()) and bool(torch.isnan(row[2 * d])) and bool(torch.isnan(loss[g])), g
            assert bool(torch.isfinite(row[2 * d + 1])), g                 # s_w is a function of the counts
        for g in (0, 2):
            assert bool(torch.isfinite(_rows_of(m, flat, g)).all()) and bool(torch.isfinite(loss[g])), g
        assert torch.equal(flat[4 * 2 * d:N * 2 * d], start[4 * 2 * d:N * 2 * d])
        assert torch.equal(flat[N * 2 * d:T * 2 * d], start[N * 2 * d:T * 2 * d])

    verify(solve(ents, ptr, None, None, 0))                                # the row-list form
    m._flat.copy_(start)
    cptr = torch.tensor([0, 1, 2, 2, 4, 4, 4], device=DEV)                 # the chunk form; the last chunk runs past R
    tab = torch.tensor([[0, 0, 3], [1, 3, 12], [3, 15, 16], [3, 31, 1 << 40]], device=DEV)
    verify(solve(ents, None, cptr, tab, 4))
    m._flat.copy_(start)
    # E = 0: nothing is launched, nothing is written
    none = torch.zeros(0, dtype=torch.int64, device=DEV)
    loss = solve(none, torch.zeros(1, dtype=torch.int64, device=DEV), None, None, 0)
    assert loss.numel() == 0 and torch.equal(m._flat, start)
    out = m.fold_in_implicit(c["x"].to(DEV), c["y"].to(DEV), 0, w0=W0, entities=[])
    assert out["entities"].numel() == 0 and out["loss"].numel() == 0 and torch.equal(m._flat, start)

"""GPU: the split exact solve (include/vfm_sweep.h, VFM.fold_in_exact(split_rows=...)), VFM.exact_objective and
VFM.fit_exact against the fp64 restatements of tests/fit_exact_restatement.py and solve_fp64.

Bounds.  Rows written by a solve: per element |got - ref| <= 2^-23 |ref| + 4 (d + 1) 2^-52 cond max|ref| against
solve_fp64 (solve_reference.elementwise_ok / solve_abs_term), after asserting cond <= 1e3 of the matrix that is factored;
all tables are planted (solve_reference.tables).  Losses and J: the 1e-5 relative of test_gpu_foldin_exact.py.  Scalars:
elementwise_ok with the absolute terms of fit_exact_restatement.scalar_abs_terms, a running-error bound of the fp32
moments kernel the update reads.  J after a block: J_after <= J_before + 1e-9 |J_before|: each block is written as the
fp32 rounding of an exact minimiser, so the excess over the minimum is second order in 2^-24 (the gradient vanishes
there), about 1e-14 relative, far below the margin.

Measured on an MI355X: worst elementwise ratio of the split solve 0.496 (1 = at the bound; the reference itself rounded
to fp32 gives at most 0.5), of the field blocks of fit_exact 0.497; losses within 6.5e-8 and J within 9e-9 relative of
the restatement."""
import functools

import numpy as np
import pytest
import torch

import fit_exact_restatement as FR
import solve_reference as R
from test_gpu_solve_edges import _check, _model_of
from test_foldin_exact_cpu import solve_fp64

pytestmark = pytest.mark.gpu
DEV = "cuda"
LINKS = ["abs", "softplus"]
CHUNK = 8


def split_counts(d):
    """d + 1 (at the threshold: not split), d + 2, around a chunk edge, one chunk (where d allows) and 40 chunks."""
    k = d // CHUNK + 2
    c = [d + 1, d + 2, CHUNK * k - 1, CHUNK * k, CHUNK * k + 1, CHUNK * 40]
    return c + [CHUNK - 1] if d + 2 <= CHUNK - 1 else c


def _sizes(F, n_ent):
    return (n_ent + 3, 60) if F == 2 else (n_ent + 3, 40, 7)


def _fold(c, m, X=None, y=None, **kw):
    X, y = (c["X"], c["y"]) if X is None else (X, y)
    return m.fold_in_exact(X.to(DEV), y.to(DEV), field=c["field"], kl_weight=c["kl_weight"], **kw)


def _plan(c, m, **kw):
    from vae_amd import foldin, sweep
    x, y = foldin.check_args_exact(m, c["X"].to(DEV), c["y"].to(DEV), c["field"], c["kl_weight"])
    return sweep.SweepPlan(m, x, y, c["field"], **kw)


# ---------------------------------------------------------------------------------------------------------------------
# the split solve against solve_fp64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [2, 3])
@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("d", [1, 8, 9, 33, 128])
def test_split_solve_matches_fp64(d, link, F):
    counts = split_counts(d)
    c = R.case(_sizes(F, len(counts)), 0, d, link, counts, seed=300 + d + F, kl_weight=0.7 if F == 3 else 1.0)
    m = _model_of(c)
    plan = _plan(c, m, split_rows=0, chunk_rows=CHUNK)
    assert plan.threshold == d + 1 and plan.E - plan.n_light == len(counts) - 1      # (only n = d + 1 is not split)
    out = _fold(c, m, split_rows=0, chunk_rows=CHUNK)
    assert torch.equal(out["entities"].cpu(), c["ids"]) and out["rows"].tolist() == counts
    _check(c, m, out["loss"], f"split F={F}")


@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("d", [R.LDS - 1, R.LDS])
def test_split_solve_triangle_in_lds_and_in_the_slab(d, link):
    counts = [d + 2, CHUNK * (d // CHUNK + 2) + 1]
    c = R.case((6, 300), 0, d, link, counts, seed=400 + d)
    m = _model_of(c)
    assert R.has_slabs(d) == (d == R.LDS)
    out = _fold(c, m, split_rows=0, chunk_rows=CHUNK)
    assert out["rows"].tolist() == counts
    _check(c, m, out["loss"], "split lds/slab")


def test_split_rows_at_n_is_not_split_and_below_it_is():
    d, n = 8, 30
    c = R.case((6, 60), 0, d, "abs", [n, 12], seed=77)
    m = _model_of(c)
    start = m._flat.clone()
    assert _plan(c, m, split_rows=n, chunk_rows=CHUNK).n_light == 2
    p = _plan(c, m, split_rows=n - 1, chunk_rows=CHUNK)
    assert p.n_light == 1 and len(p.groups) == 1 and p.groups[0][3].shape[0] == 4
    plain = _fold(c, m)
    flat_plain = m._flat.clone()
    m._flat.copy_(start)
    at_n = _fold(c, m, split_rows=n, chunk_rows=CHUNK)
    assert torch.equal(m._flat, flat_plain) and torch.equal(at_n["loss"], plain["loss"])
    m._flat.copy_(start)
    below = _fold(c, m, split_rows=n - 1, chunk_rows=CHUNK)
    _check(c, m, below["loss"], "split_rows = n - 1")


# ---------------------------------------------------------------------------------------------------------------------
# bits
# ---------------------------------------------------------------------------------------------------------------------
def _rows_of(m, flat, e):
    d = m.d
    return torch.cat([flat[e * 2 * d:(e + 1) * 2 * d], flat[m._off_bias + 2 * e: m._off_bias + 2 * e + 2]])


@functools.lru_cache(maxsize=None)
def _mixed():
    """300 light entities of 3 .. 14 rows and two heavy ones (100 and 61 rows), d = 8, F = 3, softplus."""
    counts = [3 + g % 12 for g in range(300)]
    counts[17], counts[200] = 100, 61
    c = R.case((320, 40, 7), 0, 8, "softplus", counts, seed=55, kl_weight=0.7)
    m = _model_of(c)
    return c, m, m._flat.clone()


def test_bits_of_light_and_heavy_entities_do_not_depend_on_the_call():
    c, m, start = _mixed()
    heavy = [17, 200]
    kw = dict(split_rows=20, chunk_rows=CHUNK)
    m._flat.copy_(start)
    out = _fold(c, m, **kw)
    flat = m._flat.clone()
    assert out["rows"].tolist() == c["counts"]
    # two consecutive calls
    m._flat.copy_(start)
    again = _fold(c, m, **kw)
    assert torch.equal(m._flat, flat) and torch.equal(again["loss"], out["loss"])
    # the light entities: a plain fold_in_exact of those alone
    sel = ~torch.isin(c["X"][:, 0], c["ids"][heavy])
    m._flat.copy_(start)
    light = _fold(c, m, c["X"][sel], c["y"][sel])
    keep = [g for g in range(300) if g not in heavy]
    assert torch.equal(light["loss"], out["loss"][keep])
    for g in keep:
        e = int(c["ids"][g])
        assert torch.equal(_rows_of(m, m._flat, e), _rows_of(m, flat, e)), g
    # a heavy entity alone = among 300 others
    for g in heavy:
        e = int(c["ids"][g])
        sel = c["X"][:, 0] == e
        m._flat.copy_(start)
        alone = _fold(c, m, c["X"][sel], c["y"][sel], **kw)
        assert torch.equal(alone["loss"], out["loss"][g:g + 1])
        assert torch.equal(_rows_of(m, m._flat, e), _rows_of(m, flat, e)), g
    # groups of one = one group
    p1 = _plan(c, m, max_workspace_bytes=0, **kw)
    assert len(p1.groups) == 2 and len(_plan(c, m, **kw).groups) == 1
    m._flat.copy_(start)
    grouped = _fold(c, m, max_workspace_bytes=0, **kw)
    assert torch.equal(m._flat, flat) and torch.equal(grouped["loss"], out["loss"])
    m._flat.copy_(start)
    _fold(c, m, **kw)
    _check(c, m, out["loss"], "mixed", which=[0, 1, 2] + heavy)


def test_split_rows_none_is_the_parent_path():
    from vae_amd import foldin
    c, m, start = _mixed()
    m._flat.copy_(start)
    out = _fold(c, m)
    flat = m._flat.clone()
    m._flat.copy_(start)
    ents, loss, rows = foldin.run_exact(m, c["X"].to(DEV), c["y"].to(DEV), 0, c["kl_weight"])
    assert torch.equal(m._flat, flat) and torch.equal(loss, out["loss"]) and torch.equal(ents, out["entities"])
    assert torch.equal(rows, out["rows"])
    m._flat.copy_(start)


def test_duplicated_rows_of_a_heavy_entity_count_twice():
    c = R.case((6, 60), 0, 8, "abs", [40], seed=88, dup=False)
    c2 = dict(c, X=torch.cat([c["X"], c["X"]]), y=torch.cat([c["y"], c["y"]]), counts=[80])
    m, m2 = _model_of(c), _model_of(c2)
    o = _fold(c, m, split_rows=0, chunk_rows=CHUNK)
    o2 = _fold(c2, m2, split_rows=0, chunk_rows=CHUNK)
    _check(c, m, o["loss"], "once")
    _check(c2, m2, o2["loss"], "twice")                       # (solve_fp64 counts every row)
    assert not torch.equal(m._flat, m2._flat)


# ---------------------------------------------------------------------------------------------------------------------
# the objective
# ---------------------------------------------------------------------------------------------------------------------
def _tables(m):
    return m.entity_params.weight.detach().cpu().clone(), m.bias_params.weight.detach().cpu().clone(), m._scalars().cpu().clone()


@pytest.mark.parametrize("F", [2, 3])
@pytest.mark.parametrize("link", LINKS)
def test_exact_objective_matches_the_restatement(link, F):
    c = R.case(_sizes(F, 20), 0, 8, link, [5 + g for g in range(20)], seed=500 + F, kl_weight=0.7)
    m = _model_of(c)
    J = m.exact_objective(c["X"].to(DEV), c["y"].to(DEV), kl_weight=0.7)
    ref = float(FR.objective_J(*_tables(m), c["X"], c["y"].double(), link, R.f32(0.7)))
    print(f"J {link} F={F}: {J:.9g} against {ref:.9g}, rel {abs(J - ref) / abs(ref):.2e}")
    assert abs(J - ref) <= 1e-5 * abs(ref)


# ---------------------------------------------------------------------------------------------------------------------
# fit_exact, block by block
# ---------------------------------------------------------------------------------------------------------------------
KLW = R.f32(0.7)


@functools.lru_cache(maxsize=None)
def _fit_run(F, link):
    """3 sweeps on 12 users x 9 items (x 3 formats), d = 8; item 0 has 12 rows (split at split_rows = 9, chunk_rows =
    4), the others 9; user 12, item 9 and format 3 never occur.  Returns the model, its start, the
    rows, and per block (what, tables before, tables after)."""
    sizes = (13, 10) if F == 2 else (13, 10, 4)
    ent, bia, scal = R.tables(sizes, 8, seed=600 + F)
    g = torch.Generator().manual_seed(9)
    rows = [(u, i) for i in range(9) for u in range(12) if i == 0 or (u + i) % 4 != 0]
    X = torch.tensor(rows)
    X[:, 1] += 13
    if F == 3:
        X = torch.cat([X, 23 + torch.randint(0, 3, (X.shape[0], 1), generator=g)], 1)
    X = X[torch.randperm(X.shape[0], generator=g)]
    y = torch.randn(X.shape[0], generator=g) + 3.0
    c = dict(sizes=sizes, d=8, link=link, ent=ent, bia=bia, scal=scal)
    m = _model_of(c)
    m._ensure_opt_state()
    m._adam_m.copy_(torch.randn(m._adam_m.shape, generator=g).to(DEV))
    m._adam_v.copy_(torch.rand(m._adam_v.shape, generator=g).to(DEV))
    start = dict(flat=m._flat.clone(), adam_m=m._adam_m.clone(), adam_v=m._adam_v.clone())
    blocks, prev = [], [_tables(m)]

    def on_step(sweep, what):
        now = _tables(m)
        blocks.append((sweep, what, prev[0], now))
        prev[0] = now

    out = m.fit_exact(X.to(DEV), y.to(DEV), n_sweeps=3, kl_weight=KLW, split_rows=9, chunk_rows=4, on_step=on_step)
    return m, start, X, y, blocks, out


@pytest.mark.parametrize("F", [2, 3])
@pytest.mark.parametrize("link", LINKS)
def test_fit_exact_every_block_is_the_exact_minimiser(link, F):
    from vae_amd import foldin, sweep
    m, start, X, y, blocks, out = _fit_run(F, link)
    d = 8
    assert [(s, w) for s, w, _, _ in blocks] == [(s, w) for s in range(3) for w in list(range(F)) + ["scalars"]]
    x1, y1 = foldin.check_args_exact(m, X.to(DEV), y.to(DEV), 1, KLW)
    p = sweep.SweepPlan(m, x1, y1, 1, 9, 4)
    assert p.E - p.n_light == 1 and int(p.ents[-1]) == 13     # (item 0 is split, into 3 chunks)
    assert p.groups[0][3].shape[0] == 3
    worst = 0.0
    for sweep_i, what, (e0, b0, s0), (e1, b1, s1) in blocks:
        if what == "scalars":
            assert torch.equal(e0, e1) and torch.equal(b0, b1)
            m0, sg0 = FR.global_bias_fp64(e0, b0, s0, X, y, link, KLW)
            t_m0, _ = FR.scalar_abs_terms(e0, b0, s0, X, y, link)
            ok, w = R.elementwise_ok(s1[1:2], [float(m0)], t_m0)
            assert ok, ("m0", w)
            ok, w = R.elementwise_ok(s1[2:3], [float(sg0)], R.scale_abs_term(1, [float(sg0)]))
            assert ok, ("s0", w)
            at = torch.stack([s0[0], s1[1], s1[2]])             # (the precision's block: at the bias as written)
            _, t_a = FR.scalar_abs_terms(e0, b0, at, X, y, link)
            ok, w = R.elementwise_ok(s1[0:1], [float(FR.precision_fp64(e0, b0, at, X, y, link))], t_a)
            assert ok, ("alpha", w)
            continue
        assert torch.equal(s0, s1)
        sol = solve_fp64(e0, b0, s0, X, y, what, link, KLW)
        ids = sol["entities"]
        other = torch.ones(e0.shape[0], dtype=torch.bool)
        other[ids] = False
        assert torch.equal(e0[other], e1[other]) and torch.equal(b0[other], b1[other])
        for i, e in enumerate(ids.tolist()):
            cond = R.cond_of_the_factored(e0, b0, s0, X, y, what, link, KLW, e)
            assert cond <= 1e3, cond
            n = int((X[:, what] == e).sum())
            rt = np.concatenate([[float(sol["mu_w"][i])], sol["mu"][i].numpy()])
            rs = np.concatenate([[float(sol["s_w"][i])], sol["s"][i].numpy()])
            ok_t, w_t = R.elementwise_ok(torch.cat([b1[e, :1], e1[e, :d]]), rt, R.solve_abs_term(d, cond, rt))
            ok_s, w_s = R.elementwise_ok(torch.cat([b1[e, 1:], e1[e, d:]]), rs, R.scale_abs_term(n, rs))
            assert ok_t and ok_s, (sweep_i, what, e, w_t, w_s)
            worst = max(worst, w_t, w_s)
    print(f"FIT {link} F={F}: worst elementwise ratio of the field blocks {worst:.3f}")


@pytest.mark.parametrize("F", [2, 3])
@pytest.mark.parametrize("link", LINKS)
def test_fit_exact_J_never_increases_and_unseen_rows_stay(link, F):
    m, start, X, y, blocks, out = _fit_run(F, link)
    yd = y.double()
    J = [float(FR.objective_J(*blocks[0][2], X, yd, link, KLW))]
    for sweep_i, what, _, now in blocks:
        Ja = float(FR.objective_J(*now, X, yd, link, KLW))
        assert Ja <= J[-1] + 1e-9 * abs(J[-1]), (sweep_i, what, Ja, J[-1])
        J.append(Ja)
    per_sweep = [J[0]] + J[F + 1::F + 1]
    assert out["sweeps"] == 3 and len(out["ms"]) == 3 and all(t > 0 for t in out["ms"])
    assert len(out["objective"]) == 4
    for got, ref in zip(out["objective"], per_sweep):
        assert abs(got - ref) <= 1e-5 * abs(ref), (got, ref)
    print(f"FIT {link} F={F}: J per sweep {out['objective']}")
    seen = torch.unique(X)
    unseen = torch.ones(m.T, dtype=torch.bool)
    unseen[seen] = False
    assert int(unseen.sum()) >= 2
    e0, b0, _ = blocks[0][2]
    e1, b1, _ = blocks[-1][3]
    assert torch.equal(e0[unseen], e1[unseen]) and torch.equal(b0[unseen], b1[unseen])
    assert not torch.equal(e0[~unseen], e1[~unseen])
    assert torch.equal(m._adam_m, start["adam_m"]) and torch.equal(m._adam_v, start["adam_v"])


def test_fit_exact_one_field_without_scalars_changes_only_that_fields_seen_rows():
    m, start, X, y, _, _ = _fit_run(2, "abs")
    now = m._flat.clone()
    m._flat.copy_(start["flat"])
    whats = []
    out = m.fit_exact(X.to(DEV), y.to(DEV), n_sweeps=1, kl_weight=KLW, fields=(1,), update_scalars=False, split_rows=9,
                      chunk_rows=4, on_step=lambda s, w: whats.append((s, w)))
    assert whats == [(0, 1)] and out["sweeps"] == 1
    changed = m._flat != start["flat"]
    own = torch.zeros_like(changed)
    for e in torch.unique(X[:, 1]).tolist():
        own[e * 2 * m.d:(e + 1) * 2 * m.d] = True
        own[m._off_bias + 2 * e: m._off_bias + 2 * e + 2] = True
    assert bool(changed.any()) and not bool((changed & ~own).any())
    m._flat.copy_(now)


def test_fit_exact_tol_stops_and_zero_sweeps_do_nothing():
    m, start, X, y, _, _ = _fit_run(2, "abs")
    now = m._flat.clone()
    m._flat.copy_(start["flat"])
    out = m.fit_exact(X.to(DEV), y.to(DEV), n_sweeps=0, kl_weight=KLW)
    assert out["sweeps"] == 0 and len(out["objective"]) == 1 and out["ms"] == [] and torch.equal(m._flat, start["flat"])
    out = m.fit_exact(X.to(DEV), y.to(DEV), n_sweeps=50, kl_weight=KLW, tol=1e-3)
    assert 1 <= out["sweeps"] < 50 and len(out["objective"]) == out["sweeps"] + 1
    m._flat.copy_(now)


# ---------------------------------------------------------------------------------------------------------------------
# the guards of the split entry: they return, they do not fault
# ---------------------------------------------------------------------------------------------------------------------
class _Raw:
    """The operands of one split call on the heavy entities of a small case, through torch.ops.vfm_hip."""

    def __init__(self, link):
        from vae_amd import _lib, ops
        self.softplus = ops.FLAG_LINK_SOFTPLUS
        self.c = c = R.case((8, 60), 0, 8, link, [30, 41, 12, 25], seed=700, kl_weight=0.7)
        self.m = m = _model_of(c)
        self.start = m._flat.clone()
        p = _plan(c, m, split_rows=0, chunk_rows=CHUNK)
        assert p.n_light == 0 and len(p.groups) == 1
        self.p, self.o = p, _lib.ops()
        _, _, self.cptr, self.tab = p.groups[0]

    def __call__(self, ents=None, cptr=None, tab=None, op_x=None, row_op=None):
        p, m = self.p, self.m
        ents = p.ents if ents is None else ents
        cptr, tab = self.cptr if cptr is None else cptr, self.tab if tab is None else tab
        op_x, row_op = p.op_x if op_x is None else op_x, p.row_op if row_op is None else row_op
        m._flat.copy_(self.start)
        ent, bia, scal = m._views(m._flat)
        ws = torch.zeros(max(self.o.foldin_split_workspace_bytes(tab.shape[0], ents.numel(), op_x.shape[0], m.d, -1), 1),
                         dtype=torch.uint8, device=DEV)
        loss = torch.full((max(ents.numel(), 1),), -7.0, device=DEV)
        self.o.foldin_solve_split(ents, cptr, tab, p.ys, op_x, row_op, ent, bia, scal, ws, loss, 0,
                                  self.softplus if m.link == "softplus" else 0, -1, 0.7)
        torch.cuda.synchronize()
        return m._flat.clone(), loss, ws


@pytest.mark.parametrize("link", LINKS)
def test_guards_of_the_split_entry(link):
    r = _Raw(link)
    m, p, d = r.m, r.p, r.m.d
    flat0, loss0, _ = r()
    assert torch.isfinite(loss0).all() and not torch.equal(flat0, r.start)
    _check(r.c, m, loss0[p.asc], "raw")
    E = p.E
    # entity ids outside the table, with chunks of their own: NaN loss, nothing written, the others bit for bit
    ents = torch.cat([torch.tensor([-3], device=DEV), p.ents, torch.tensor([m.T + 2], device=DEV)])
    nch = r.tab.shape[0]
    tab = torch.cat([r.tab[:1], r.tab, r.tab[:2]]).clone()
    tab[1:1 + nch, 0] += 1
    tab[0, 0], tab[-2:, 0] = 0, E + 1
    cptr = torch.cat([torch.tensor([0], device=DEV), r.cptr + 1, torch.tensor([nch + 3], device=DEV)])
    flat, loss, _ = r(ents=ents, cptr=cptr, tab=tab)
    assert bool(torch.isnan(loss[0])) and bool(torch.isnan(loss[-1])) and torch.equal(loss[1:-1], loss0[:E])
    assert torch.equal(flat, flat0)
    # a chunk whose entity number is outside [0, E) and rows outside [0, R): clamped and skipped, no fault
    tab = r.tab.clone()
    tab = torch.cat([tab, torch.tensor([[E + 5, -4, 1 << 40], [-1, 1 << 40, 5]], device=DEV)])
    flat, loss, _ = r(tab=tab)
    assert torch.equal(flat, flat0) and torch.equal(loss, loss0)
    # partner ids outside the table on one row of entities 1 and 3: NaN row and loss, a finite s_w; the others bit for bit
    n_ops = p.op_x.shape[0]
    op_x = torch.cat([p.op_x, torch.tensor([[0, m.T + 5], [0, -2]], device=DEV)])
    row_op = p.row_op.clone()
    hit = (1, 3)
    row_op[int(p.ptr[1]) + 2] = n_ops
    row_op[int(p.ptr[3])] = n_ops + 1
    flat, loss, _ = r(op_x=op_x, row_op=row_op)
    for g, e in enumerate(p.ents.tolist()):
        row = _rows_of(m, flat, e)
        if g in hit:
            assert bool(torch.isnan(row[:2 * d]).all()) and bool(torch.isnan(row[2 * d])) and bool(torch.isnan(loss[g])), g
            assert bool(torch.isfinite(row[2 * d + 1])), g
        else:
            assert torch.equal(row, _rows_of(m, flat0, e)) and torch.equal(loss[g], loss0[g]), g
    # a row operand outside [0, n_ops): the same outcome
    row_op = p.row_op.clone()
    row_op[int(p.ptr[2]) + 1] = n_ops + 9
    flat, loss, _ = r(row_op=row_op)
    assert bool(torch.isnan(_rows_of(m, flat, int(p.ents[2]))[:2 * d]).all()) and bool(torch.isnan(loss[2]))
    assert torch.equal(loss[[0, 1, 3]], loss0[[0, 1, 3]])
    # an empty chunk table: every entity at the prior, loss = its KL there
    flat, loss, _ = r(cptr=torch.zeros(E + 1, dtype=torch.int64, device=DEV),
                      tab=torch.zeros(0, 3, dtype=torch.int64, device=DEV))
    prior = 1.0 if link == "abs" else float(np.log(np.expm1(1.0)))
    for e in p.ents.tolist():
        row = _rows_of(m, flat, e)
        assert bool((row[:d] == 0).all()) and float(row[2 * d]) == 0.0
        assert R.elementwise_ok(torch.cat([row[d:2 * d], row[2 * d + 1:]]).cpu(), np.full(d + 1, prior), 0.0)[0]
    assert float(loss[:E].abs().max()) <= (d + 1) * 4 * R.EPS32
    # E = 0: nothing written
    flat, loss, ws = r(ents=p.ents[:0], cptr=r.cptr[:1], tab=r.tab)
    assert torch.equal(flat, r.start) and bool((loss == -7.0).all()) and not bool(ws.any())

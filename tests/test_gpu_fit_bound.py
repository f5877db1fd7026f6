"""GPU: the split bound rounds (include/vfm_bound_sweep.h, VFM.fold_in_bound(split_rows=...)), VFM.bound_objective and
VFM.fit_bound against the fp64 references of tests/bound_reference.py and tests/bound_sweep_restatement.py.

Bounds: those of test_gpu_foldin_bound.py (its _check is used as it stands).  Rows rel_err <= 1e-4, loss <= 1e-5 against
the fp64 B_e at the written rows; per element |got - ref| <= 2^-23 |ref| + n_iters solve_abs_term(d, cond_max, ref) for
the means and the same plus scale_abs_term for the scales, after asserting cond <= 1e3 of every round's factored matrix
(tests/test_fit_bound_cpu.py asserts it for the split cases on the CPU: at most 78.4).  J and bound_objective: the 1e-5
relative of a loss summed from fp32 moments.  J after a block: J_after <= J_before + 1e-5 |J_before|, both from fp32
moments; the rounds of a block do not end at a stationary point, so no second-order margin applies.  The bias block:
elementwise with the absolute terms of bound_sweep_restatement.bias_abs_terms.

Measured on an MI355X (the printed BOUND and FITB lines): worst elementwise ratio of the split rounds 0.498 (1 = at the
bound; the reference itself rounded to fp32 gives at most 0.5), rows within 5.7e-8 and losses within 7.0e-8 relative;
bound_objective within 1.3e-8 of the restatement; the field blocks of fit_bound 0.498, its bias blocks 0.041; the
largest relative step of J over a block -2.2e-8 (none rose)."""
import functools

import numpy as np
import pytest
import torch

import bound_reference as BR
import bound_sweep_restatement as BS
import solve_reference as R
from test_gpu_foldin_bound import _check, _model_of

pytestmark = pytest.mark.gpu
DEV = "cuda"
LINKS = ["abs", "softplus"]
CHUNK = BS.CHUNK


def _fold(c, m, n_iters=8, reset=False, X=None, y=None, **kw):
    X, y = (c["X"], c["y"]) if X is None else (X, y)
    return m.fold_in_bound(X.to(DEV), y.to(DEV), field=c["field"], kl_weight=c["kl_weight"], n_iters=n_iters, reset=reset,
                           **kw)


def _fold_lds(c, m, lds_dim, n_iters=8, reset=False, **kw):
    from vae_amd import sweep
    ents, loss, rows = sweep.run_bound_split(m, c["X"].to(DEV), c["y"].to(DEV), c["field"], c["kl_weight"], n_iters, reset,
                                             lds_dim=lds_dim, **kw)
    return {"entities": ents, "loss": loss, "rows": rows}


def _plan(c, m, **kw):
    from vae_amd import foldin, sweep
    x, y = foldin.check_args_bound(m, c["X"].to(DEV), c["y"].to(DEV), c["field"], c["kl_weight"], 8)
    return sweep.SweepPlan(m, x, y, c["field"], bound=True, **kw)


def _rows_of(m, flat, e):
    d = m.d
    return torch.cat([flat[e * 2 * d:(e + 1) * 2 * d], flat[m._off_bias + 2 * e: m._off_bias + 2 * e + 2]])


# ---------------------------------------------------------------------------------------------------------------------
# the split rounds against fp64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [2, 3])
@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("d", BS.SPLIT_DS)
def test_split_rounds_match_fp64(d, link, F):
    c = BS.split_case(d, link, F)
    counts = c["counts"]
    m = _model_of(c)
    start = m._flat.clone()
    plan = _plan(c, m, split_rows=0, chunk_rows=CHUNK)
    assert plan.threshold == d + 1 and plan.E - plan.n_light == len(counts) - 1      # (only n = d + 1 is not split)
    worst = 0.0
    for n_iters, reset in BS.ITERS:
        m._flat.copy_(start)
        out = _fold(c, m, n_iters, reset, split_rows=0, chunk_rows=CHUNK)
        assert torch.equal(out["entities"].cpu(), c["ids"]) and out["rows"].tolist() == counts
        worst = max(worst, _check(c, m, out["loss"], n_iters, reset, f"split F={F}"))
    print(f"BOUND split worst d={d} {link} F={F}: {worst:.3f}")


@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("d", [R.LDS - 1, R.LDS])
def test_split_rounds_triangle_in_lds_and_in_the_slab(d, link):
    c = BS.placement_case(d, link)
    m = _model_of(c)
    assert R.has_slabs(d) == (d == R.LDS)
    out = _fold(c, m, 8, True, split_rows=0, chunk_rows=CHUNK)
    assert out["rows"].tolist() == c["counts"]
    _check(c, m, out["loss"], 8, True, "split lds/slab")


def test_split_rows_at_n_is_not_split_and_below_it_is():
    d, n = 8, 30
    c = BR.bound_case((6, 60), 0, d, "abs", [n, 12], seed=77)
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
    _check(c, m, below["loss"], 8, False, "split_rows = n - 1")
    e = int(c["ids"][1])                                      # the light entity: the bits of the plain call
    assert torch.equal(_rows_of(m, m._flat, e), _rows_of(m, flat_plain, e)) and torch.equal(below["loss"][1], plain["loss"][1])


# ---------------------------------------------------------------------------------------------------------------------
# bits
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mixed():
    c = BS.mixed_case()
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
    # on a repeat
    m._flat.copy_(start)
    again = _fold(c, m, **kw)
    assert torch.equal(m._flat, flat) and torch.equal(again["loss"], out["loss"])
    # the light entities: a plain fold_in_bound of those alone
    sel = ~torch.isin(c["X"][:, 0], c["ids"][heavy])
    m._flat.copy_(start)
    light = _fold(c, m, X=c["X"][sel], y=c["y"][sel])
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
        alone = _fold(c, m, X=c["X"][sel], y=c["y"][sel], **kw)
        assert torch.equal(alone["loss"], out["loss"][g:g + 1])
        assert torch.equal(_rows_of(m, m._flat, e), _rows_of(m, flat, e)), g
    # wherever the triangle lives
    for lds_dim in (-1, 0, 3):
        m._flat.copy_(start)
        o2 = _fold_lds(c, m, lds_dim, **kw)
        assert torch.equal(m._flat, flat) and torch.equal(o2["loss"], out["loss"]), lds_dim
    # groups of one = one group
    p1 = _plan(c, m, max_workspace_bytes=0, **kw)
    assert len(p1.groups) == 2 and len(_plan(c, m, **kw).groups) == 1
    m._flat.copy_(start)
    grouped = _fold(c, m, max_workspace_bytes=0, **kw)
    assert torch.equal(m._flat, flat) and torch.equal(grouped["loss"], out["loss"])
    _check(c, m, out["loss"], 8, False, "mixed", which=[0, 1, 2] + heavy)
    # another chunk length may change the bits of the heavy entities, not the bounds; the light ones keep theirs
    m._flat.copy_(start)
    other = _fold(c, m, split_rows=20, chunk_rows=3 * CHUNK)
    _check(c, m, other["loss"], 8, False, "mixed chunk_rows=24", which=[0, 1, 2] + heavy)
    assert torch.equal(other["loss"][keep], out["loss"][keep])
    m._flat.copy_(start)


def test_split_rows_none_is_the_parent_path():
    from vae_amd import foldin
    c, m, start = _mixed()
    m._flat.copy_(start)
    out = _fold(c, m)
    flat = m._flat.clone()
    m._flat.copy_(start)
    ents, loss, rows = foldin.run_bound(m, c["X"].to(DEV), c["y"].to(DEV), 0, c["kl_weight"], 8, False)
    assert torch.equal(m._flat, flat) and torch.equal(loss, out["loss"]) and torch.equal(ents, out["entities"])
    assert torch.equal(rows, out["rows"])
    m._flat.copy_(start)


# ---------------------------------------------------------------------------------------------------------------------
# monotone, frozen
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reset", [False, True])
def test_monotone_in_n_iters_and_frozen_rows(reset):
    c, m, start = _mixed()
    heavy = [17, 200]
    prev = None
    for n_iters in (1, 2, 4, 8):
        m._flat.copy_(start)
        out = _fold(c, m, n_iters, reset, split_rows=20, chunk_rows=CHUNK)
        B = out["loss"].double().cpu()
        assert bool(torch.isfinite(B).all())
        if prev is not None:
            print(f"BOUND split monotone reset={int(reset)} n_iters={n_iters}: heavy B - B_prev = {(B - prev)[heavy].tolist()}")
            assert bool((B <= prev + 1e-5 * prev.abs()).all()), (n_iters, B[heavy], prev[heavy])
        prev = B
    changed = torch.zeros(m._n_flat, dtype=torch.bool, device=DEV)
    for e in out["entities"].tolist():
        changed[e * 2 * m.d:(e + 1) * 2 * m.d] = True
        changed[m._off_bias + 2 * e: m._off_bias + 2 * e + 2] = True
    assert torch.equal(m._flat[~changed], start[~changed]) and int((~changed).sum()) > 0
    assert not torch.equal(m._flat[changed], start[changed])
    m._flat.copy_(start)


# ---------------------------------------------------------------------------------------------------------------------
# the guards of the split entry: they return, they do not fault
# ---------------------------------------------------------------------------------------------------------------------
class _Raw:
    """The operands of one split call on the heavy entities of a small case, through torch.ops.vfm_hip."""

    def __init__(self, link):
        from vae_amd import _lib, ops
        self.softplus = ops.FLAG_LINK_SOFTPLUS
        self.c = c = BR.bound_case((8, 60), 0, 8, link, [30, 41, 12, 25], seed=700, kl_weight=0.7)
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
        need = self.o.foldin_bound_split_workspace_bytes(tab.shape[0], ents.numel(), p.ys.numel(), op_x.shape[0], m.d, -1)
        ws = torch.zeros(max(need, 1), dtype=torch.uint8, device=DEV)
        loss = torch.full((max(ents.numel(), 1),), -7.0, device=DEV)
        self.o.foldin_bound_split(ents, cptr, tab, p.ys, op_x, row_op, ent, bia, scal, ws, loss, 0,
                                  self.softplus if m.link == "softplus" else 0, -1, 0.7, 8, 0)
        torch.cuda.synchronize()
        return m._flat.clone(), loss, ws


@pytest.mark.parametrize("link", LINKS)
def test_guards_of_the_split_entry(link):
    r = _Raw(link)
    m, p, d = r.m, r.p, r.m.d
    flat0, loss0, _ = r()
    assert torch.isfinite(loss0).all() and not torch.equal(flat0, r.start)
    m._flat.copy_(flat0)
    _check(r.c, m, loss0[p.asc], 8, False, "raw")
    E = p.E
    # entity ids outside the table, with chunks of their own: NaN loss, nothing written, the others bit for bit
    ents = torch.cat([torch.tensor([-3], device=DEV), p.ents, torch.tensor([m.T + 2], device=DEV)])
    nch = r.tab.shape[0]
    tab = torch.cat([r.tab[:1], r.tab, r.tab[:2]]).clone()
    tab[1:1 + nch, 0] += 1
    tab[0, 0], tab[-2:, 0] = 0, E + 1
    # (the chunks of the two bad entities take rows of other entities: give them rows of their own weights by pointing
    # them at an empty range, so that no row's weight has two writers)
    tab[0, 2], tab[-2:, 2] = 0, 0
    cptr = torch.cat([torch.tensor([0], device=DEV), r.cptr + 1, torch.tensor([nch + 3], device=DEV)])
    flat, loss, _ = r(ents=ents, cptr=cptr, tab=tab)
    assert bool(torch.isnan(loss[0])) and bool(torch.isnan(loss[-1])) and torch.equal(loss[1:-1], loss0[:E])
    assert torch.equal(flat, flat0)
    # a chunk whose entity number is outside [0, E) and rows outside [0, R): clamped and skipped, no fault
    tab = torch.cat([r.tab, torch.tensor([[E + 5, -4, 1 << 40], [-1, 1 << 40, 5]], device=DEV)])
    flat, loss, _ = r(tab=tab)
    assert torch.equal(flat, flat0) and torch.equal(loss, loss0)
    # partner ids outside the table on one row of entities 1 and 3: NaN row and loss; the others bit for bit
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
            assert bool(torch.isnan(row).all()) and bool(torch.isnan(loss[g])), g
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


# ---------------------------------------------------------------------------------------------------------------------
# the objective
# ---------------------------------------------------------------------------------------------------------------------
def _tables(m):
    return m.entity_params.weight.detach().cpu().clone(), m.bias_params.weight.detach().cpu().clone(), m._scalars().cpu().clone()


@pytest.mark.parametrize("F", [2, 3])
@pytest.mark.parametrize("link", LINKS)
def test_bound_objective_matches_the_restatement(link, F):
    c = BR.bound_case(BS.split_sizes(F, 20), 0, 8, link, [5 + g for g in range(20)], seed=500 + F, kl_weight=0.7)
    m = _model_of(c)
    before = m._flat.clone()
    J = m.bound_objective(c["X"].to(DEV), c["y"].to(DEV), kl_weight=0.7)
    ref = float(BS.objective_J(*_tables(m), c["X"], c["y"], link, R.f32(0.7)))
    print(f"FITB J {link} F={F}: {J:.9g} against {ref:.9g}, rel {abs(J - ref) / abs(ref):.2e}")
    assert abs(J - ref) <= 1e-5 * abs(ref)
    assert torch.equal(m._flat, before)


# ---------------------------------------------------------------------------------------------------------------------
# fit_bound, block by block
# ---------------------------------------------------------------------------------------------------------------------
KLW = R.f32(0.7)
N_ITERS = 2
FIT_KW = dict(kl_weight=KLW, n_iters=N_ITERS, split_rows=40, chunk_rows=16)


@functools.lru_cache(maxsize=None)
def _fit_run(F, link):
    """3 sweeps on bound_sweep_restatement.fit_case, d = 8.  Returns the model, its start, the rows, per block (sweep,
    what, tables before, tables after, J before, J after) and fit_bound's result."""
    sizes, X, y = BS.fit_case(F)
    ent, bia, scal = R.tables(sizes, 8, seed=600 + F)
    c = dict(sizes=sizes, d=8, link=link, ent=ent, bia=bia, scal=scal)
    m = _model_of(c)
    g = torch.Generator().manual_seed(9)
    m._ensure_opt_state()
    m._adam_m.copy_(torch.randn(m._adam_m.shape, generator=g).to(DEV))
    m._adam_v.copy_(torch.rand(m._adam_v.shape, generator=g).to(DEV))
    start = dict(flat=m._flat.clone(), adam_m=m._adam_m.clone(), adam_v=m._adam_v.clone())
    Xd, yd = X.to(DEV), y.to(DEV)
    blocks, prev = [], [_tables(m), m.bound_objective(Xd, yd, kl_weight=KLW)]

    def on_step(sweep, what):
        now, J = _tables(m), m.bound_objective(Xd, yd, kl_weight=KLW)
        blocks.append((sweep, what, prev[0], now, prev[1], J))
        prev[0], prev[1] = now, J

    out = m.fit_bound(Xd, yd, n_sweeps=3, on_step=on_step, **FIT_KW)
    return m, start, X, y, blocks, out


@pytest.mark.parametrize("F", [2, 3])
@pytest.mark.parametrize("link", LINKS)
def test_fit_bound_every_block_is_the_restatement_s(link, F):
    from vae_amd import foldin, sweep
    m, start, X, y, blocks, out = _fit_run(F, link)
    d = 8
    assert [(b[0], b[1]) for b in blocks] == [(s, w) for s in range(3) for w in list(range(F)) + ["bias"]]
    x0, y0 = foldin.check_args_bound(m, X.to(DEV), y.to(DEV), 0, KLW, N_ITERS)
    p = sweep.SweepPlan(m, x0, y0, 0, 40, 16, bound=True)
    assert p.E == 299 and p.E - p.n_light == 2 and sorted(p.ents[-2:].tolist()) == [0, 1]     # (users 0 and 1 are split)
    assert p.groups[0][3].shape[0] == 8                                                       # (60 rows: 4 chunks each)
    worst = worst_b = 0.0
    for sweep_i, what, (e0, b0, s0), (e1, b1, s1), _, _ in blocks:
        if what == "bias":
            assert torch.equal(e0, e1) and torch.equal(b0, b1) and torch.equal(s0[0], s1[0])
            m0, sg0, _ = BS.global_bias_fp64(e0, b0, s0, X, y, link, KLW)
            t_m0, t_s0 = BS.bias_abs_terms(e0, b0, s0, X, y, link, KLW)
            ok, w1 = R.elementwise_ok(s1[1:2], [float(m0)], t_m0)
            assert ok, ("m0", w1)
            ok, w2 = R.elementwise_ok(s1[2:3], [float(sg0)], t_s0 + R.scale_abs_term(1, [float(sg0)]))
            assert ok, ("s0", w2)
            worst_b = max(worst_b, w1, w2)
            continue
        assert torch.equal(s0, s1)
        ids = torch.unique(X[:, what])
        other = torch.ones(e0.shape[0], dtype=torch.bool)
        other[ids] = False
        assert torch.equal(e0[other], e1[other]) and torch.equal(b0[other], b1[other])
        for e in ids.tolist():
            r = BR.bound_rounds_fp64(e0, b0, s0, X, y, what, link, KLW, e, N_ITERS, False)
            cond = float(r["cond"].max())
            assert cond <= 1e3, cond
            rt, rs = r["theta"][-1], r["s"][-1]
            at = N_ITERS * R.solve_abs_term(d, cond, rt)
            ok_t, w_t = R.elementwise_ok(torch.cat([b1[e, :1], e1[e, :d]]), rt, at)
            ok_s, w_s = R.elementwise_ok(torch.cat([b1[e, 1:], e1[e, d:]]), rs, at + R.scale_abs_term(r["n"], rs))
            assert ok_t and ok_s, (sweep_i, what, e, w_t, w_s)
            worst = max(worst, w_t, w_s)
    print(f"FITB {link} F={F}: worst elementwise ratio of the field blocks {worst:.3f}, of the bias blocks {worst_b:.3f}")


@pytest.mark.parametrize("F", [2, 3])
@pytest.mark.parametrize("link", LINKS)
def test_fit_bound_J_never_increases_and_unseen_rows_stay(link, F):
    m, start, X, y, blocks, out = _fit_run(F, link)
    worst = -1e30
    for sweep_i, what, _, _, Jb, Ja in blocks:
        worst = max(worst, (Ja - Jb) / abs(Jb))
        assert Ja <= Jb + 1e-5 * abs(Jb), (sweep_i, what, Ja, Jb)
    assert out["sweeps"] == 3 and len(out["ms"]) == 3 and all(t > 0 for t in out["ms"])
    assert len(out["objective"]) == 4 and out["objective"][-1] < out["objective"][0]
    per_sweep = [blocks[0][4]] + [b[5] for b in blocks if b[1] == "bias"]
    assert out["objective"] == per_sweep                      # (the same kernel on the same tables)
    ref = float(BS.objective_J(*blocks[-1][3], X, y, link, KLW))
    assert abs(out["objective"][-1] - ref) <= 1e-5 * abs(ref)
    print(f"FITB {link} F={F}: J per sweep {out['objective']}, largest relative step of a block {worst:.2e}")
    seen = torch.unique(X)
    unseen = torch.ones(m.T, dtype=torch.bool)
    unseen[seen] = False
    assert int(unseen.sum()) >= 2
    e0, b0, _ = blocks[0][2]
    e1, b1, _ = blocks[-1][3]
    assert torch.equal(e0[unseen], e1[unseen]) and torch.equal(b0[unseen], b1[unseen])
    assert not torch.equal(e0[~unseen], e1[~unseen])
    assert torch.equal(m._adam_m, start["adam_m"]) and torch.equal(m._adam_v, start["adam_v"])


def test_fit_bound_one_field_without_the_bias_changes_only_that_fields_seen_rows():
    m, start, X, y, _, _ = _fit_run(2, "abs")
    now = m._flat.clone()
    m._flat.copy_(start["flat"])
    whats = []
    out = m.fit_bound(X.to(DEV), y.to(DEV), n_sweeps=1, fields=(1,), update_bias=False,
                      on_step=lambda s, w: whats.append((s, w)), **FIT_KW)
    assert whats == [(0, 1)] and out["sweeps"] == 1
    changed = m._flat != start["flat"]
    own = torch.zeros_like(changed)
    for e in torch.unique(X[:, 1]).tolist():
        own[e * 2 * m.d:(e + 1) * 2 * m.d] = True
        own[m._off_bias + 2 * e: m._off_bias + 2 * e + 2] = True
    assert bool(changed.any()) and not bool((changed & ~own).any())
    m._flat.copy_(now)


def test_fit_bound_tol_stops_and_zero_sweeps_do_nothing():
    m, start, X, y, _, _ = _fit_run(2, "abs")
    now = m._flat.clone()
    m._flat.copy_(start["flat"])
    out = m.fit_bound(X.to(DEV), y.to(DEV), n_sweeps=0, **FIT_KW)
    assert out["sweeps"] == 0 and len(out["objective"]) == 1 and out["ms"] == [] and torch.equal(m._flat, start["flat"])
    out = m.fit_bound(X.to(DEV), y.to(DEV), n_sweeps=50, tol=1e-3, **FIT_KW)
    assert 1 <= out["sweeps"] < 50 and len(out["objective"]) == out["sweeps"] + 1
    m._flat.copy_(now)

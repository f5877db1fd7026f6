"""GPU: bound fold-in (VFM.fold_in_bound, include/vfm_bound.h: vfm_foldin_bound_f32) -- the written rows against
bound_rounds_fp64 of tests/bound_reference.py at the same n_iters and start, and the returned loss against the fp64
B_e at the written rows: both links, two and three fields, n_iters 1 and 8, from the rows and from the prior, at every
lane shape of the loss pass (d = 1, 8, 9, 33, 128) and around the dual / primal rule (n = 1, d - 1, d, d + 1), with the
triangle in LDS and in a slab; monotone in n_iters; the objective mode; bitwise repeatability and independence of the
other entities, of the grid and of lds_dim; frozen means frozen; the guards of the raw entry.

Bounds: rel_err <= 1e-4 for the rows and <= 1e-5 for the loss, the project's bounds in test_gpu_foldin_exact.py.
tests/test_foldin_bound_cpu.py asserts cond <= 1e3 of every round's factored matrix for the cases used here.  Per
element: |got - ref| <= 2^-23 |ref| + n_iters solve_abs_term(d, cond_max, ref) for the means (the fp64 iterate is never
rounded between rounds, so each round adds at most one solve's error), and the same plus scale_abs_term for the scales,
whose sums hold the weights of the last iterate.

Measured on an MI355X: see DESIGN.md §4 "Bound fold-in" (the printed BOUND lines)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import bound_reference as BR
import solve_reference as R
from golden_util import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
LINKS = ["abs", "softplus"]


def _model_of(c):
    """A 'class' model holding the tables of a case."""
    from vae_amd.model import VFM
    torch.manual_seed(0)
    m = VFM(field_sizes=list(c["sizes"]), embedding_size=c["d"], output="class", link=c["link"], device=DEV)
    m.entity_params.weight.data.copy_(c["ent"])
    m.bias_params.weight.data.copy_(c["bia"])
    m._flat[m._off_scal: m._off_scal + 3] = c["scal"].to(DEV)
    return m


def _written(m, ids):
    """(theta [E, d + 1] = (mu_w, mu), s [E, d + 1] = (s_w, s)) of the rows ids, fp32 on the CPU."""
    d = m.d
    ent = m.entity_params.weight.detach()[ids.to(DEV)].cpu()
    bia = m.bias_params.weight.detach()[ids.to(DEV)].cpu()
    return torch.cat([bia[:, :1], ent[:, :d]], 1), torch.cat([bia[:, 1:], ent[:, d:]], 1)


def _fit(c, m, n_iters, reset, lds_dim=-1, X=None, y=None):
    from vae_amd import foldin
    X, y = (c["X"], c["y"]) if X is None else (X, y)
    return foldin.run_bound(m, X.to(DEV), y.to(DEV), c["field"], c["kl_weight"], n_iters, reset, lds_dim)


def _check(c, m, loss, n_iters, reset, what, which=None):
    """The written rows of the entities number `which` of case c against bound_rounds_fp64 (relative and per element),
    the loss against the fp64 B_e at the written rows.  Returns the worst elementwise ratio."""
    which = list(range(len(c["counts"]))) if which is None else list(which)
    ids, d = c["ids"][which], c["d"]
    theta, s = _written(m, ids)
    worst, Bref, rt, rs = 0.0, [], [], []
    for i, k in enumerate(which):
        r = BR.case_rounds(c, k, n_iters, reset)
        assert r["n"] == c["counts"][k] and float(r["cond"].max()) <= 1e3
        rt.append(r["theta"][-1])
        rs.append(r["s"][-1])
        at = n_iters * R.solve_abs_term(d, float(r["cond"].max()), r["theta"][-1])
        ok_t, w_t = R.elementwise_ok(theta[i], r["theta"][-1], at)
        ok_s, w_s = R.elementwise_ok(s[i], r["s"][-1], at + R.scale_abs_term(r["n"], r["s"][-1]))
        worst = max(worst, w_t, w_s)
        assert ok_t and ok_s, (what, r["n"], w_t, w_s)
        Bref.append(BR.bound_objective_fp64(c["ent"], c["bia"], c["scal"], c["X"], c["y"], c["field"], c["link"],
                                            c["kl_weight"], int(ids[i]), theta[i], s[i]))
    e_rows = max(rel_err(theta.numpy(), np.array(rt)), rel_err(s.numpy(), np.array(rs)))
    e_loss = rel_err(loss.cpu()[which].numpy(), np.array(Bref))
    print(f"BOUND {what} {c['link']} F={len(c['sizes'])} d={d} n_iters={n_iters} reset={int(reset)}: rows {e_rows:.2e} "
          f"loss {e_loss:.2e} worst elementwise ratio {worst:.3f}")
    assert e_rows <= 1e-4, e_rows
    assert e_loss <= 1e-5, e_loss
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# against fp64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [2, 3])
@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("d", BR.GPU_DS)
def test_rows_and_loss_match_fp64(d, link, F):
    c = BR.shape_case(d, link, F)
    m = _model_of(c)
    start = m._flat.clone()
    for n_iters, reset in BR.GPU_ITERS:
        m._flat.copy_(start)
        ents, loss, rows = _fit(c, m, n_iters, reset)
        assert torch.equal(ents.cpu(), c["ids"]) and rows.tolist() == c["counts"]
        _check(c, m, loss, n_iters, reset, "shape")


def test_slab_storage():
    """d = VFM_FOLDIN_SOLVE_LDS_DIM, n = d + 1: the primal system lives in the workgroup's slab."""
    c = BR.slab_case()
    m = _model_of(c)
    ents, loss, rows = _fit(c, m, 8, True)
    assert rows.tolist() == [R.LDS + 1] and R.storage(R.LDS + 1, R.LDS) == "slab"
    _check(c, m, loss, 8, True, "slab")


@pytest.mark.parametrize("lds_dim", [0, 3])
def test_lds_dim(lds_dim):
    c = BR.lds_dim_case()
    m = _model_of(c)
    ents, loss, rows = _fit(c, m, 8, False, lds_dim)
    _check(c, m, loss, 8, False, f"lds_dim={lds_dim}")


# ---------------------------------------------------------------------------------------------------------------------
# monotone, and the objective mode
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reset", [False, True])
def test_monotone_in_n_iters_and_objective_mode(reset):
    c = BR.shape_case(9, "softplus", 3)
    m = _model_of(c)
    start = m._flat.clone()
    X, y = c["X"].to(DEV), c["y"].to(DEV)
    prev = None
    for n_iters in (1, 2, 4, 8):
        m._flat.copy_(start)
        out = m.fold_in_bound(X, y, field=c["field"], kl_weight=c["kl_weight"], n_iters=n_iters, reset=reset)
        B = out["loss"].double().cpu()
        assert bool(torch.isfinite(B).all())
        if prev is not None:
            print(f"BOUND monotone reset={int(reset)} n_iters={n_iters}: B - B_prev in "
                  f"[{float((B - prev).min()):.3e}, {float((B - prev).max()):.3e}]")
            assert bool((B <= prev + 1e-5 * prev.abs()).all()), (n_iters, B, prev)
        prev = B
        before = m._flat.clone()
        obj = m.fold_in_bound_objective(X, y, field=c["field"], kl_weight=c["kl_weight"])
        assert torch.equal(obj["loss"], out["loss"]) and torch.equal(obj["entities"], out["entities"])
        assert torch.equal(m._flat, before)                                  # OBJECTIVE mode writes nothing


# ---------------------------------------------------------------------------------------------------------------------
# bitwise
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bitwise():
    c = BR.bitwise_case()
    m = _model_of(c)
    start = m._flat.clone()
    runs = {}
    for lds_dim in BR.LDS_DIMS:
        m._flat.copy_(start)
        _, loss, _ = _fit(c, m, 8, True, lds_dim)
        runs[lds_dim] = (loss.clone(), m._flat.clone())
    return c, m, start, runs


def test_bitwise_repeatable_and_independent_of_lds_dim():
    c, m, start, runs = _bitwise()
    m._flat.copy_(start)
    _, loss, _ = _fit(c, m, 8, True)
    assert torch.equal(loss, runs[-1][0]) and torch.equal(m._flat, runs[-1][1])          # two runs
    for lds_dim in (0, 3):
        assert torch.equal(runs[lds_dim][0], runs[-1][0]) and torch.equal(runs[lds_dim][1], runs[-1][1]), lds_dim
    assert bool(torch.isfinite(runs[-1][0]).all())
    m._flat.copy_(runs[-1][1])
    _check(c, m, runs[-1][0], 8, True, "bitwise sample", R.bitwise_sample(len(c["counts"])))


def test_an_entity_alone_equals_the_same_entity_among_the_others():
    c, m, start, runs = _bitwise()
    loss_all, flat_all = runs[0]                                             # (lds_dim = 0: slabs, the grid capped)
    d = c["d"]
    for k in (0, R.SLABS, 2 * R.SLABS, 2 * R.SLABS + 36):                    # block 0's three trips and the last entity
        e = int(c["ids"][k])
        sel = c["X"][:, c["field"]] == e
        m._flat.copy_(start)
        _, loss, _ = _fit(c, m, 8, True, 0, c["X"][sel], c["y"][sel])
        assert torch.equal(loss, loss_all[k:k + 1]), k
        assert torch.equal(m._flat[e * 2 * d:(e + 1) * 2 * d], flat_all[e * 2 * d:(e + 1) * 2 * d]), k
        assert torch.equal(m._flat[m._off_bias + 2 * e: m._off_bias + 2 * e + 2],
                           flat_all[m._off_bias + 2 * e: m._off_bias + 2 * e + 2]), k


# ---------------------------------------------------------------------------------------------------------------------
# frozen means frozen
# ---------------------------------------------------------------------------------------------------------------------
def test_frozen_means_frozen():
    c = BR.shape_case(8, "abs", 3)
    m = _model_of(c)
    X, y = c["X"].to(DEV), c["y"].to(DEV)
    m.pipeline = False                                                       # a few training steps: a live Adam state
    m.set_training_data(X)
    m.lr = 0.05
    plan = m.plan(X, y)
    for _ in range(3):
        m.train_step(plan)
    m.save_weights()
    keys = ("_flat", "_adam_m", "_adam_v", "_last_flat", "_mean_flat")
    before = {k: getattr(m, k).clone() for k in keys}
    t_before = m._adam_t
    assert bool(before["_adam_v"].any())
    obj = m.fold_in_bound_objective(X, y, field=c["field"], kl_weight=c["kl_weight"])
    for k in keys:
        assert torch.equal(getattr(m, k), before[k]), k                      # OBJECTIVE mode writes nothing
    out = m.fold_in_bound(X, y, field=c["field"], kl_weight=c["kl_weight"])
    changed = torch.zeros(m._n_flat, dtype=torch.bool, device=DEV)
    for e in out["entities"].tolist():
        changed[e * 2 * m.d:(e + 1) * 2 * m.d] = True
        changed[m._off_bias + 2 * e: m._off_bias + 2 * e + 2] = True
    assert torch.equal(m._flat[~changed], before["_flat"][~changed])
    assert not torch.equal(m._flat[changed], before["_flat"][changed])
    for k in keys[1:]:
        assert torch.equal(getattr(m, k), before[k]), k
    assert m._adam_t == t_before
    assert bool((out["loss"] <= obj["loss"] * (1 + 1e-5)).all())             # the fit did not raise the bound


def test_empty_call_does_nothing():
    c = BR.shape_case(8, "abs", 2)
    m = _model_of(c)
    before = m._flat.clone()
    out = m.fold_in_bound(torch.zeros(0, 2, dtype=torch.int64), torch.zeros(0))
    assert out["entities"].numel() == 0 and out["loss"].numel() == 0 and out["rows"].numel() == 0
    assert torch.equal(m._flat, before)


# ---------------------------------------------------------------------------------------------------------------------
# the guards of the raw entry: ids that are valid integers outside the table, which the kernels check before any access
# ---------------------------------------------------------------------------------------------------------------------
def test_raw_abi_guards():
    from vae_amd import _lib, foldin
    lib = _lib.load()
    c = BR.shape_case(8, "softplus", 2)
    m = _model_of(c)
    X, y = c["X"].to(DEV), c["y"].to(DEV)
    xs, ys, ents, ptr, _ = foldin.row_lists(X, y, 0)
    op_x, row_op = foldin.partner_tuples(xs, 0)
    E, d, T = ents.numel(), m.d, m.T
    assert E == 4
    need = lib.vfm_foldin_bound_workspace_bytes(E, ys.numel(), op_x.shape[0], d, 0)
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    loss = torch.full((E,), -7.0, device=DEV)
    ent, bia, scal = m._views(m._flat)
    start = m._flat.clone()

    def call(**kw):
        p = _lib.FoldinBound()
        args = dict(E=E, R=ys.numel(), T=T, n_ops=op_x.shape[0], F=2, d=d, col=0, objective=_lib.OBJ_CLOSED_FORM,
                    likelihood=_lib.LIK_BERNOULLI, flags=_lib._gen.VFM_FLAG_LINK_SOFTPLUS, lds_dim=0, kl_weight=1.0,
                    n_iters=8, reset=0, mode=foldin.MODE_FIT, entities=ents.data_ptr(), row_ptr=ptr.data_ptr(),
                    y=ys.data_ptr(), op_x=op_x.data_ptr(), row_op=row_op.data_ptr(), entity_params=ent.data_ptr(),
                    bias_params=bia.data_ptr(), scalars=scal.data_ptr(), out_loss=loss.data_ptr(),
                    workspace=ws.data_ptr(), workspace_bytes=need)
        args.update(kw)
        for k, v in args.items():
            setattr(p, k, v)
        rc = lib.vfm_foldin_bound_f32(C.byref(p), C.c_void_p(_lib.raw_stream(torch.device(DEV))))
        torch.cuda.synchronize()
        return rc

    # rejected before anything is launched: nothing written
    bad = _lib._gen.VFM_E_INVALID
    for kw in (dict(kl_weight=0.0), dict(likelihood=_lib.LIK_NORMAL), dict(n_iters=0), dict(workspace_bytes=need - 1),
               dict(mode=foldin.MODE_OBJECTIVE)):
        assert call(**kw) == bad, kw
        assert torch.equal(m._flat, start) and bool((loss == -7.0).all()) and not bool(ws.any()), kw
    assert call(E=0) == 0 and bool((loss == -7.0).all())                     # E = 0 launches nothing

    # the plain call
    assert call() == 0
    good_loss, good_flat = loss.clone(), m._flat.clone()
    assert bool(torch.isfinite(good_loss).all()) and not torch.equal(good_flat, start)

    # an entity id outside [0, T): a NaN loss and no write; the others as before
    m._flat.copy_(start)
    ents_bad = ents.clone()
    ents_bad[1] = T + 5
    assert call(entities=ents_bad.data_ptr()) == 0
    assert bool(torch.isnan(loss[1])) and torch.equal(loss[[0, 2, 3]], good_loss[[0, 2, 3]])
    e1 = int(ents[1])
    keep = torch.ones(m._n_flat, dtype=torch.bool, device=DEV)
    keep[e1 * 2 * d:(e1 + 1) * 2 * d] = False
    keep[m._off_bias + 2 * e1: m._off_bias + 2 * e1 + 2] = False
    assert torch.equal(m._flat[keep], good_flat[keep]) and torch.equal(m._flat[~keep], start[~keep])
    ents_bad[1] = -3
    m._flat.copy_(start)
    assert call(entities=ents_bad.data_ptr()) == 0
    assert bool(torch.isnan(loss[1])) and torch.equal(m._flat[~keep], start[~keep])

    # a partner id outside [0, T): the rows of the entities that use that operand and their losses are NaN
    m._flat.copy_(start)
    op_bad = op_x.clone()
    o_bad = int(row_op[int(ptr[2])])                                         # the operand of entity 2's first row
    op_bad[o_bad, 1] = T + 9
    assert call(op_x=op_bad.data_ptr()) == 0
    hit = [g for g in range(E) if bool((row_op[int(ptr[g]):int(ptr[g + 1])] == o_bad).any())]
    assert 2 in hit
    for g in range(E):
        e = int(ents[g])
        row = m._flat[e * 2 * d:(e + 1) * 2 * d]
        if g in hit:
            assert bool(torch.isnan(loss[g])) and bool(torch.isnan(row).all())
        else:
            assert torch.equal(loss[g], good_loss[g]) and torch.equal(row, good_flat[e * 2 * d:(e + 1) * 2 * d])

    # an empty range: the prior (mu = 0, s = link^-1(1)) and loss 0
    m._flat.copy_(start)
    ptr_e = ptr.clone()
    ptr_e[2] = ptr[1]                                                        # entity 1: [ptr[1], ptr[1]) is empty
    assert call(row_ptr=ptr_e.data_ptr()) == 0
    assert float(loss[1]) == 0.0
    theta, s = _written(m, ents[1:2].cpu())
    assert bool((theta == 0).all()) and float((s - foldin.prior_s("softplus")).abs().max()) <= 1e-7
    assert torch.equal(loss[0], good_loss[0])

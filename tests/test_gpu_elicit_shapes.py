"""GPU: elicitation sessions (include/vfm_elicit.h) at every compiled lane-group shape of k_elicit and at the edges of
its pool, stage and guards -- bitwise against the composition of select_next_questions and fold_in at every <W, CPL>,
both links, both objectives; ties through the butterfly; the documented guards through the raw op; the refusals; and a
per-round fp64 check (no feedback between rounds) that covers the sampled objective, softplus, 'class' and history."""
# k_elicit <W, CPL, LINK, SAMPLED>: 7 shapes x 2 links x {closed form, sampled} = 28 instances (vfm_elicit.hip).
#   shape_of (vfm_foldin_body.hpp): W = 8 / 16 / 32 / 64 lanes for d <= 8 / 16 / 32 / above; CPL = ceil(d / W) rounded up
#     to 1, 2, 4, 8.  for_shape switches on W * 16 + CPL; its default case is <64, 8>.
#   lds_cap (closed form; the sampled form stages nothing): FB = 256 threads, LDS_BYTES = 48 KiB = 12288 floats per
#     block, GPB = 256 / W groups per block, DP = W * CPL; per group 12288 / GPB floats hold theta_u's copy (2 DP + 2)
#     and cap rows of DP + 1:  cap = (12288 / GPB - (2 DP + 2)) / (DP + 1), rounded down.
#
#     d              (W, CPL)  GPB  per group   cap                     lanes / coordinates filled
#     1, 8           (8, 1)    32     384   (384 - 18) / 9     = 40     1 of 8; all
#     9              (16, 1)   16     768   (768 - 34) / 17    = 43     9 of 16
#     17, 32         (32, 1)    8    1536   (1536 - 66) / 33   = 44     17 of 32; all
#     33, 64         (64, 1)    4    3072   (3072 - 130) / 65  = 45     33 of 64; all
#     65             (64, 2)    4    3072   (3072 - 258) / 129 = 21     65 of 128
#     129, 256       (64, 4)    4    3072   (3072 - 514) / 257 =  9     129 of 256; all
#     257, 300, 512  (64, 8)    4    3072   (3072 - 1026) / 513 = 3     257, 300 of 512; all
#
# Every d below runs the four VARIANTS: both SAMPLED values and both links at each shape, 28 of 28 instances.
import numpy as np
import pytest
import torch

import elicit_restatement as R
from golden_util import rel_err
from test_gpu_elicit import _composed, _problem, _same_bits, _theta_rows
from test_gpu_foldin import _model

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPE = {1: (8, 1, 40), 8: (8, 1, 40), 9: (16, 1, 43), 17: (32, 1, 44), 32: (32, 1, 44), 33: (64, 1, 45),
         64: (64, 1, 45), 65: (64, 2, 21), 129: (64, 4, 9), 256: (64, 4, 9), 257: (64, 8, 3), 300: (64, 8, 3),
         512: (64, 8, 3)}                                    # d -> (W, CPL, lds_cap): the table above
SHAPE_D = list(SHAPE)
VARIANTS = [("closed_form", "reg", "abs"), ("closed_form", "reg", "softplus"), ("sampled", "class", "abs"),
            ("sampled", "class", "softplus")]
VARIANT_IDS = ["-".join(v) for v in VARIANTS]


def _rotation(d, vi):
    """(strategy, reset, with history, n_samples, kl_weight) of a case, rotated over its index ('mean' needs 'class')."""
    di = SHAPE_D.index(d)
    names = ("variance", "top", "random") if VARIANTS[vi][1] == "reg" else ("mean", "variance", "random", "top")
    strategy = names[(di + vi) % len(names)]
    S = 1 + (di + vi) % 3 if VARIANTS[vi][0] == "sampled" else 1
    return strategy, (di + vi) % 2 == 1, (di + 2 * vi) % 4 != 3, S, (0.8, 1.0, 1.3)[(4 * di + vi) % 3]


def _where(a, b):
    """The (user, round) pairs at which two [U, Q, ..] results differ in bits: the message of a failed comparison."""
    ne = a.contiguous().view(torch.int32) != b.contiguous().view(torch.int32) if a.dtype == torch.float32 else a != b
    ne = ne.reshape(ne.shape[0], ne.shape[1], -1).any(2)
    return [tuple(t) for t in torch.nonzero(ne).tolist()][:12]


def _assert_same_session(a, b, keys, note):
    for k in keys:
        same = _same_bits(a[k], b[k]) if a[k].dtype == torch.float32 else torch.equal(a[k], b[k])
        assert same, (note, k, "differs at (user, round)", _where(a[k], b[k]))


def test_the_rotation_reaches_every_instance_strategy_and_edge():
    """The table above against the parameter list: every <W, CPL> runs both objectives and both links; every strategy
    and both reset values occur at W = 64 and below it; the closed form (the only form with a stage) runs with a
    history at every shape; kl_weight != 1 and 1 to 3 samples occur."""
    assert sorted({v[:2] for v in SHAPE.values()}) == [(8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 4), (64, 8)]
    for d, (W, CPL, cap) in SHAPE.items():
        w = 8 if d <= 8 else 16 if d <= 16 else 32 if d <= 32 else 64
        c = -(-d // w)
        assert (W, CPL) == (w, 1 if c <= 1 else 2 if c <= 2 else 4 if c <= 4 else 8)
        assert cap == (12288 // (256 // W) - (2 * W * CPL + 2)) // (W * CPL + 1) and cap - 2 >= 1
    seen = {True: set(), False: set()}
    staged = set()
    for d in SHAPE_D:
        for vi in range(4):
            strategy, reset, with_hist, S, klw = _rotation(d, vi)
            seen[SHAPE[d][0] == 64] |= {strategy, ("reset", reset), ("S", S), ("klw", klw != 1.0)}
            if vi < 2 and with_hist:
                staged.add(SHAPE[d][:2])
    for wide in (True, False):
        assert {"top", "variance", "mean", "random", ("reset", True), ("reset", False), ("S", 1), ("S", 2), ("S", 3),
                ("klw", True)} <= seen[wide]
    assert len(staged) == 7


# ------------------------------------------------------------------------------------------------ 1. every shape
@pytest.mark.parametrize("vi", range(4), ids=VARIANT_IDS)
@pytest.mark.parametrize("d", SHAPE_D)
def test_every_shape_bitwise_against_the_composition(d, vi):
    """37 users: more than one block and a partial last block at every W (GPB = 32, 16, 8, 4: 32 + 5, 2 x 16 + 5,
    4 x 8 + 5, 9 x 4 + 1).  Pools of 1, W - 1, W, W + 1, 2 W + 3 rows: lanes that score no row, one row and several;
    the one-row pool runs out before Q.  Histories of 60 rows (past every cap), 0, cap - 2 (the appended rows cross
    i < cap in round 2 of 6: the single-row append's branch and fold_run's mixed staged / streamed read) and 2.  Then
    the same sessions with every row streamed (lds_rows = 0) and write=False."""
    from vae_amd import elicit
    objective, output, link = VARIANTS[vi]
    W, CPL, cap = SHAPE[d]
    strategy, reset, with_hist, S, klw = _rotation(d, vi)
    Q, n_steps = 6, 9
    m = _model((40, 200), d, output, link, seed=d + vi, rng_seed=3)
    pool, y_pool, hx, hy = _problem(m, 37, [1, W - 1, W, W + 1, 2 * W + 3], [60, 0, cap - 2, 2] if with_hist else [0],
                                    seed=d)
    hist = (hx, hy) if with_hist else None
    note = dict(d=d, shape=(W, CPL), cap=cap, strategy=strategy, reset=reset, history=with_hist, S=S, klw=klw)
    start = m._flat.clone()
    users, rows, score, loss, theta = _composed(m, pool, y_pool, Q, strategy, hist, n_steps, 0.05, objective, S, 21,
                                                klw, reset)
    want = dict(users=users, rows=rows, score=score, loss=loss, theta=theta)
    final = m._flat.clone()
    m._flat.copy_(start)
    m.params_changed()
    kw = dict(history=hist, n_steps=n_steps, lr=0.05, objective=objective, n_samples=S, seed=21, kl_weight=klw,
              reset=reset, return_theta=True)
    out = m.elicit(pool, y_pool, Q, strategy, write=True, **kw)
    assert users.numel() == 37 and torch.equal(out["users"], users)
    _assert_same_session(out, want, ("rows", "score", "loss", "theta"), note)     # (NaNs included)
    assert torch.equal(m._flat, final), note
    assert not torch.equal(final, start)
    assert int((rows < 0).sum()) > 0 and int((rows[:, 0] >= 0).sum()) == 37
    # every row streamed from the operand table == rows staged up to the cap; write=False leaves the model alone
    m._flat.copy_(start)
    m.params_changed()
    streamed = elicit.run(m, pool, y_pool, Q, strategy, write=False, lds_rows=0, **kw)
    assert torch.equal(m._flat, start), note
    assert torch.equal(streamed["users"], users)
    _assert_same_session(streamed, out, ("rows", "score", "loss", "theta"), dict(note, lds_rows=0))


# ------------------------------------------------------------------------------------------------ 2. ties
TIE_K = 37          # the copies' distance: 37 % 64 and 37 % 16 != 0, and position 40's copy (77) sits on a LOWER lane


def _twin_pool(m, d):
    """A pool in which every (user, item) row appears twice, TIE_K positions apart in the user's own order (blocks of
    TIE_K items followed by the same items again: 74 or 148 rows per user, more than W), the users' rows interleaved
    at random with each user's order kept.  Returns (pool, y_pool, twin [P]: the caller index of each row's copy)."""
    g = torch.Generator().manual_seed(d)
    N, M = m.field_sizes
    users = torch.randperm(N, generator=g)[:9]
    blocks, ys = [], []
    for i, u in enumerate(users.tolist()):
        nb = 1 + i % 2
        it = N + torch.randperm(M, generator=g)[:TIE_K * nb]
        y = torch.randn(TIE_K * nb, generator=g) + 1.0
        blocks.append(torch.stack([torch.full((2 * TIE_K * nb,), u),
                                   torch.cat([it[b * TIE_K:(b + 1) * TIE_K].repeat(2) for b in range(nb)])], 1))
        ys.append(torch.cat([y[b * TIE_K:(b + 1) * TIE_K].repeat(2) for b in range(nb)]))
    by_user, y_by_user = torch.cat(blocks), torch.cat(ys)
    P = by_user.shape[0]
    slot_user = by_user[torch.randperm(P, generator=g), 0]           # which user's row each caller index holds
    pool, y_pool = torch.empty_like(by_user), torch.empty_like(y_by_user)
    twin = torch.empty(P, dtype=torch.int64)
    for u in users.tolist():
        idx = torch.nonzero(slot_user == u).reshape(-1)              # ascending: the user's own order
        pool[idx], y_pool[idx] = by_user[by_user[:, 0] == u], y_by_user[by_user[:, 0] == u]
        p = torch.arange(idx.numel())
        twin[idx] = idx[torch.where(p % (2 * TIE_K) < TIE_K, p + TIE_K, p - TIE_K)]
    assert torch.equal(pool[twin], pool) and torch.equal(y_pool[twin], y_pool) and bool((twin != torch.arange(P)).all())
    return pool.to(DEV), y_pool.to(DEV), twin


@pytest.mark.parametrize("strategy", ["top", "variance", "random"])
@pytest.mark.parametrize("d", [33, 9])
def test_ties_go_to_the_lower_pool_position(d, strategy):
    """Two copies of a row have the same score to the bit under the same posterior, on different lanes of the group
    (W = 64 at d = 33, W = 16 at d = 9): the butterfly has to pick the lower position, as select_next_questions' stable
    sort does.  Round 0 ties in every user whatever the strategy.  'random' is keyed on (seed + q, user, item), so its
    copies tie as well, in every round in which both are left; it does not depend on the posterior, which separates
    the pool's construction from the scoring."""
    Q, n_steps = 8, 9
    m = _model((40, 200), d, "reg", "abs", seed=d + len(strategy), rng_seed=3)
    pool, y_pool, twin = _twin_pool(m, d)
    start = m._flat.clone()
    users, rows, score, loss, theta = _composed(m, pool, y_pool, Q, strategy, None, n_steps, 0.05, "closed_form", 1, 13,
                                                1.0, False)
    want = dict(rows=rows, score=score, loss=loss, theta=theta)
    m._flat.copy_(start)
    m.params_changed()
    out = m.elicit(pool, y_pool, Q, strategy, n_steps=n_steps, lr=0.05, seed=13, return_theta=True)
    assert torch.equal(out["users"], users)
    _assert_same_session(out, want, ("rows", "score", "loss", "theta"), (d, strategy))
    both = 0
    for u, asked in enumerate(out["rows"].cpu().tolist()):
        seen = set()
        for q, r in enumerate(asked):
            assert r >= 0
            t = int(twin[r])
            assert r < t or t in seen, (u, q, r, t)          # the higher copy only after the lower one
            both += t in seen
            seen.add(r)
    print(f"d = {d}, {strategy}: both copies of a row asked {both} times")


# ------------------------------------------------------------------------------------------------ 3. the guards
GUARD_CASES = [(17, "closed_form", "reg", "abs"), (17, "sampled", "class", "softplus"),
               (300, "closed_form", "reg", "softplus"), (300, "sampled", "class", "abs")]
GUARD_IDS = [f"{c[0]}-{c[1]}" for c in GUARD_CASES]


def _raw(m, users, ptr, items, ys, Q, strategy, objective, write=0, moments=False, n_steps=5, seed=3):
    """torch.ops.vfm_hip.elicit on hand-built lists (the argument order of vae_amd/elicit.py::run), no Python-side
    validation.  The outputs start from sentinels (-7, 7.0) so that what the kernel left alone shows."""
    from vae_amd import _lib, foldin, ops
    from vae_amd.rank import strategy_code
    i64 = dict(dtype=torch.int64, device=DEV)
    f32 = dict(dtype=torch.float32, device=DEV)
    users, ptr, items = (torch.tensor(v, **i64) for v in (users, ptr, items))
    ys = torch.as_tensor(ys).to(**f32).contiguous()
    U, P, d = users.numel(), items.numel(), m.d
    o = _lib.ops()
    obj = foldin.OBJECTIVES[objective]
    op_x = pool_op = None
    n_ops = 0
    if objective == "closed_form":
        uq, inv = torch.unique(items, return_inverse=True)
        op_x = torch.zeros(uq.numel(), 2, **i64)
        op_x[:, 1] = uq
        pool_op, n_ops = inv.contiguous(), uq.numel()
    res = dict(rows=torch.full((U, Q), -7, **i64), score=torch.full((U, Q), 7.0, **f32),
               loss=torch.full((U, Q), 7.0, **f32), theta=torch.full((U, Q, 2 * d + 2), 7.0, **f32))
    if moments:
        res["mean"], res["var"] = torch.full((Q + 1, P), 7.0, **f32), torch.full((Q + 1, P), 7.0, **f32)
    ws = torch.empty(max(o.elicit_workspace_bytes(P, n_ops, d, obj), 1), dtype=torch.uint8, device=DEV)
    m._fresh_params()
    ent, bia, scal = m._views(m._flat)
    lik = _lib.LIK_NORMAL if m.output == "reg" else _lib.LIK_BERNOULLI
    o.elicit(users, ptr, items, ys, None, None, None, op_x, pool_op, None, ent, bia, scal, ws, res["rows"],
             res["score"], res["loss"], res["theta"], res.get("mean"), res.get("var"), Q, strategy_code(strategy), obj,
             lik, ops.FLAG_LINK_SOFTPLUS if m.link == "softplus" else 0, n_steps, 1, 0, int(write), -1, 0.05, 1.0, seed, 0)
    if write:
        m.params_changed()
    return res


def _guard_problem(d, objective, output, link, sizes=(12, 5, 9)):
    """Three users (ascending) with pools of distinct items, as lists."""
    m = _model((40, 200), d, output, link, seed=d + 1, rng_seed=3)
    g = torch.Generator().manual_seed(d)
    users = sorted(torch.randperm(40, generator=g)[:3].tolist())
    items = [(40 + torch.randperm(200, generator=g)[:n]).tolist() for n in sizes]
    n = sum(sizes)
    ys = torch.randn(n, generator=g) + 1.0 if output == "reg" else (torch.rand(n, generator=g) < 0.5).float()
    return m, users, items, ys


def _lists(items):
    ptr = [0]
    for it in items:
        ptr.append(ptr[-1] + len(it))
    return ptr, [i for it in items for i in it]


def _user_rows_mask(m, users):
    mask = torch.zeros(m._n_flat, dtype=torch.bool, device=DEV)
    for e in users:
        mask[e * 2 * m.d:(e + 1) * 2 * m.d] = True
        mask[m._off_bias + 2 * e: m._off_bias + 2 * e + 2] = True
    return mask


@pytest.mark.parametrize("d,objective,output,link", GUARD_CASES, ids=GUARD_IDS)
def test_guard_a_user_id_outside_the_table_asks_nothing(d, objective, output, link):
    m, users, items, ys = _guard_problem(d, objective, output, link)
    ptr, flat = _lists(items)
    start = m._flat.clone()
    Q = 4
    for bad, b in ((-4, 0), (m.T + 5, 2)):                   # (in place of the first / the last user: ids stay ascending)
        m._flat.copy_(start)
        m.params_changed()
        us = users[:]
        us[b] = bad
        out = _raw(m, us, ptr, flat, ys, Q, "variance", objective, write=1)
        assert out["rows"][b].tolist() == [-1] * Q
        assert bool(torch.isnan(out["score"][b]).all()) and bool(torch.isnan(out["loss"][b]).all())
        ok = [i for i in range(3) if i != b]
        mask = _user_rows_mask(m, [users[i] for i in ok])
        assert torch.equal(m._flat[~mask], start[~mask])     # no table row but the valid users'
        assert not torch.equal(m._flat[mask], start[mask])
        after = m._flat.clone()
        # the valid users are what they are in a launch without the bad one
        m._flat.copy_(start)
        m.params_changed()
        rptr, rflat = _lists([items[i] for i in ok])
        ref = _raw(m, [users[i] for i in ok], rptr, rflat, torch.cat([ys[ptr[i]:ptr[i + 1]] for i in ok]), Q,
                   "variance", objective, write=1)
        assert torch.equal(m._flat, after)
        assert bool((ref["rows"] >= 0).all())
        for j, i in enumerate(ok):
            assert torch.equal(out["rows"][i] - ptr[i], ref["rows"][j] - rptr[j])
        for k in ("score", "loss", "theta"):
            assert _same_bits(out[k][ok].contiguous(), ref[k]), k


@pytest.mark.parametrize("d,objective,output,link", GUARD_CASES, ids=GUARD_IDS)
def test_guard_a_pool_item_outside_the_table_is_never_asked(d, objective, output, link):
    m, users, items, ys = _guard_problem(d, objective, output, link)
    ptr, _ = _lists(items)
    start = m._flat.clone()
    Q, at = 6, 2                                             # user 1 has 5 rows: 4 askable, then nothing is left
    bad = m.T + 9 if d == 17 else -1
    its = [items[0], items[1][:at] + [bad] + items[1][at + 1:], items[2]]
    out = _raw(m, users, *_lists(its), ys, Q, "variance", objective, moments=True)
    assert torch.equal(m._flat, start)
    p_bad = ptr[1] + at
    assert bool(torch.isnan(out["mean"][:, p_bad]).all()) and bool(torch.isnan(out["var"][:, p_bad]).all())
    others = [p for p in range(ptr[3]) if p != p_bad]
    assert bool(torch.isfinite(out["mean"][:, others]).all()) and bool(torch.isfinite(out["var"][:, others]).all())
    assert not bool((out["rows"] == p_bad).any())
    assert sorted(out["rows"][1, :4].tolist()) == [p for p in range(ptr[1], ptr[2]) if p != p_bad]
    assert out["rows"][1, 4:].tolist() == [-1, -1]
    # the same user without that row: the same questions in the same order, the same thetas
    keep = [p for p in range(ptr[3]) if p != p_bad]
    ref = _raw(m, users, *_lists([items[0], items[1][:at] + items[1][at + 1:], items[2]]), ys[keep], Q, "variance",
               objective)
    back = torch.tensor(keep + [-1], device=DEV)             # reference position -> position in the main call
    assert torch.equal(back[ref["rows"]], out["rows"])
    for k in ("score", "loss", "theta"):
        assert _same_bits(ref[k], out[k]), k


@pytest.mark.parametrize("d,objective,output,link", GUARD_CASES, ids=GUARD_IDS)
def test_guard_an_empty_pool_slice_between_two_users(d, objective, output, link):
    m, users, items, ys = _guard_problem(d, objective, output, link, sizes=(12, 0, 9))
    start = m._flat.clone()
    Q = 4
    out = _raw(m, users, *_lists(items), ys, Q, "variance", objective)
    assert torch.equal(m._flat, start)
    assert out["rows"][1].tolist() == [-1] * Q
    assert bool(torch.isnan(out["score"][1]).all()) and bool(torch.isnan(out["loss"][1]).all())
    ref = _raw(m, [users[0], users[2]], *_lists([items[0], items[2]]), ys, Q, "variance", objective)
    assert bool((ref["rows"] >= 0).all())
    for k in ("rows", "score", "loss", "theta"):
        same = torch.equal if k == "rows" else _same_bits
        assert same(out[k][[0, 2]].contiguous(), ref[k]), k


@pytest.mark.parametrize("d,objective,output,link", GUARD_CASES, ids=GUARD_IDS)
def test_guard_no_rounds_with_moments_is_predictive_moments(d, objective, output, link):
    m, users, items, ys = _guard_problem(d, objective, output, link)
    ptr, flat = _lists(items)
    start = m._flat.clone()
    out = _raw(m, users, ptr, flat, ys, 0, "variance", objective, write=1, moments=True)
    assert torch.equal(m._flat, start)                       # (write with no round: the rows as they were, bit for bit)
    pool = torch.tensor([[u, i] for u, it in zip(users, items) for i in it], device=DEV)
    mean, var = m.predictive_moments(pool)
    assert _same_bits(out["mean"][0], mean) and _same_bits(out["var"][0], var)
    assert out["rows"].numel() == 0


# ------------------------------------------------------------------------------------------------ 4. refusals, n_steps = 0
def test_d_above_512_is_refused_before_any_launch():
    m = _model((40, 200), 513, "reg", "abs", seed=1)
    pool, y_pool, hx, hy = _problem(m, 4, [5], [2], seed=1)
    before = m._flat.clone()
    with pytest.raises(ValueError, match="512"):
        m.elicit(pool, y_pool, 3, "variance", history=(hx, hy), n_steps=2, write=True)
    with pytest.raises(ValueError, match="512"):
        m.elicitation_curve(pool, y_pool, 3, strategies=("variance",), n_steps=2)
    assert torch.equal(m._flat, before)


@pytest.mark.parametrize("d,objective,output,link,strategy", [(17, "closed_form", "reg", "softplus", "top"),
                                                              (65, "sampled", "class", "abs", "mean")])
def test_no_adam_steps_equals_the_composed_loop(d, objective, output, link, strategy):
    """n_steps = 0: the thetas never move, loss is the objective at the starting theta (fold_in_objective on the
    history followed by the rows asked so far, draw key q), the selections are those of repeated
    select_next_questions on the rows left."""
    Q = 5
    m = _model((40, 200), d, output, link, seed=d, rng_seed=3)
    pool, y_pool, hx, hy = _problem(m, 9, [3, 8, 20], [4, 0], seed=d)
    start = m._flat.clone()
    users, rows, score, loss, theta = _composed(m, pool, y_pool, Q, strategy, (hx, hy), 0, 0.05, objective, 2, 6, 0.9,
                                                False)
    assert torch.equal(m._flat, start)
    out = m.elicit(pool, y_pool, Q, strategy, history=(hx, hy), n_steps=0, objective=objective, n_samples=2, seed=6,
                   kl_weight=0.9, write=True, return_theta=True)
    assert torch.equal(m._flat, start)
    _assert_same_session(out, dict(rows=rows, score=score, loss=loss, theta=theta), ("rows", "score", "loss", "theta"), d)
    at_start = _theta_rows(m, users)
    for q in range(Q):
        assert torch.equal(out["theta"][:, q], at_start)
    # by hand: the selections with the model as it is, and the objective of the rows so far
    left = torch.ones(pool.shape[0], dtype=torch.bool, device=DEV)
    asked = torch.zeros(0, dtype=torch.int64, device=DEV)
    for q in range(Q):
        idx = torch.nonzero(left).reshape(-1)
        us, r = m.select_next_questions(pool[idx], 1, strategy, 6 + q)
        pos = torch.searchsorted(users, us)
        assert torch.equal(out["rows"][pos, q], idx[r[:, 0]])
        assert bool((out["rows"][:, q] >= 0).sum() == us.numel())
        left[idx[r[:, 0]]] = False
        asked = torch.cat([asked, idx[r[:, 0]]])
        sel = asked[torch.isin(pool[asked, 0], us)]
        hs = torch.isin(hx[:, 0], us)
        l, g = m.fold_in_objective(torch.cat([hx[hs], pool[sel]]), torch.cat([hy[hs], y_pool[sel]]), objective=objective,
                                   n_samples=2, seed=6, step=q, kl_weight=0.9)
        assert torch.equal(g["entities"], us) and _same_bits(out["loss"][pos, q], l)
    assert int((out["rows"] < 0).sum()) > 0


# ------------------------------------------------------------------------------------------------ 5. per-round fp64
def _planted_model(name):
    from vae_amd.model import VFM
    output, objective, kind, strategy, reset, n_hist, d = R.FP64_CASES[name]
    c = R.planted_case(name)
    torch.manual_seed(0)
    m = VFM(field_sizes=[R.FP64_USERS, R.FP64_ITEMS], embedding_size=d, output=output, link=kind, device=DEV)
    m.entity_params.weight.data.copy_(torch.tensor(c["ent"]))
    m.bias_params.weight.data.copy_(torch.tensor(c["bia"]))
    m._flat[m._off_scal: m._off_scal + 3] = torch.tensor(c["scal"], device=DEV)
    return m, c


@pytest.mark.parametrize("name", list(R.FP64_CASES))
def test_rounds_against_the_fp64_restatement(name):
    """Every round of every user on its own, given the kernel's theta before the round and the kernel's selections so
    far -- no feedback, so no gap condition, and any objective, link, output and history can be checked.
    Selection: with R.moments / R.score from theta[q - 1] in fp64, score_fp64[chosen] >= best - tau |best| over the
    unasked rows; tau = 4 x the largest relative difference between the kernel's and R's scores of round 0
    (test_against_the_fp64_restatement_on_a_planted_model's definition).  Fold: R.fold from theta[q - 1] on the history
    followed by the asked rows, t0 = q (n_steps + 1), the kernel's own draws (ops.philox_eps), reproduces theta[q] and
    loss[q] within the 1e-4 of test_trajectory_matches_fp64_adam.  Inputs: R.planted_case (16 users, 30-row pools,
    Q = 5, 20 steps at lr = 0.01, one draw per iteration), shown well conditioned in fp32 by
    test_elicit_cpu.py::test_per_round_generators_are_well_conditioned_in_fp32.
    Measured on an MI355X (tau; worst theta rel_err; worst relative error of the loss; every one of the 80 choices of a
    case was the fp64 arg-max itself):
      sampled, class, softplus, history, 'mean', d = 33:     tau 5.9e-4 (scores near 0: -|mean| ..); 6.7e-7; 2.5e-7
      sampled, reg, |.|, reset, 'variance', d = 300:         tau 1.6e-6; 4.9e-7; 5.8e-7
      closed form, reg, softplus, history, 'top', d = 129:   tau 1.5e-5; 9.1e-7; 2.2e-7"""
    from test_gpu_shape_buckets import _eps_any_d
    from vae_amd import rank
    output, objective, kind, strategy, reset, n_hist, d = R.FP64_CASES[name]
    Q, n_steps, seed = R.FP64_ROUNDS, R.FP64_STEPS, 4
    m, c = _planted_model(name)
    pool, y_pool = torch.tensor(c["pool"], device=DEV), torch.tensor(c["y_pool"], device=DEV)
    hist = (torch.tensor(c["hist_x"], device=DEV), torch.tensor(c["hist_y"], device=DEV)) if n_hist else None
    out = m.elicit(pool, y_pool, Q, strategy, history=hist, n_steps=n_steps, lr=R.FP64_LR, objective=objective,
                   n_samples=1, seed=seed, reset=reset, return_theta=True, return_moments=True)
    assert out["users"].tolist() == list(range(R.FP64_USERS)) and bool((out["rows"] >= 0).all())
    # the kernel's scores of round 0, every pool row
    if strategy == "mean":
        assert not reset
        ent, bia, scal = m._views(m._flat)
        score0 = rank.predictive_moments(pool, ent, bia, scal, m.link, strategy, seed)[2]
    else:
        score0 = out["logit_var" if strategy == "variance" else "logit_mean"][0]
    score0 = score0.cpu().numpy().astype(np.float64)
    rows, theta, loss = out["rows"].cpu().numpy(), out["theta"].cpu().numpy().astype(np.float64), out["loss"].cpu().numpy()
    draws = {}

    def eps(t):
        if t not in draws:
            ee, eb, eg = _eps_any_d(m, seed, t, 1)[0]
            draws[t] = (ee.numpy(), eb.numpy(), float(eg.reshape(-1)[0]))
        return draws[t]

    E, B = c["ent"].astype(np.float64), c["bia"].astype(np.float64)
    tup = lambda v: (v[:d], v[d:2 * d], float(v[2 * d]), float(v[2 * d + 1]))
    prior = tup(np.concatenate([np.zeros(d), np.full(d, np.float32(R.prior_theta(d, kind)[3])), [0.0],
                                [np.float32(R.prior_theta(d, kind)[3])]]).astype(np.float64))
    per_user, tau = [], 0.0
    for u in range(R.FP64_USERS):
        sel = np.nonzero(c["pool"][:, 0] == u)[0]
        first = prior if reset else R.table_theta(E, B, u)
        before = lambda q: first if q == 0 else tup(theta[u, q - 1])
        local = [int(np.nonzero(sel == r)[0][0]) for r in rows[u]]
        rr = R.rounds_along(name, c, u, local, before, eps if objective == "sampled" else None)
        assert len(rr) == Q
        per_user.append((local, rr))
        tau = max(tau, float(np.max(np.abs(score0[sel] - rr[0][3]) / np.abs(rr[0][3]))))
    tau *= 4.0
    worst, worst_loss, not_argmax = 0.0, 0.0, 0
    for u, (local, rr) in enumerate(per_user):
        for q, mean, var, sc, mask, th, ls in rr:
            best = float(np.max(sc[mask]))
            assert mask[local[q]] and sc[local[q]] >= best - tau * abs(best), (u, q, sc[local[q]], best, tau)
            not_argmax += sc[local[q]] != best
            for a, b in ((theta[u, q, :d], th[0]), (theta[u, q, d:2 * d], th[1]), (theta[u, q, 2 * d:], np.array(th[2:]))):
                worst = max(worst, rel_err(a, b))
            worst_loss = max(worst_loss, abs(float(loss[u, q]) - ls) / abs(ls))
    print(f"{name}: tau = {tau:.3e}; worst theta rel_err {worst:.3e}; worst loss relative error {worst_loss:.3e}; "
          f"{not_argmax} of {R.FP64_USERS * Q} choices are not the fp64 arg-max")
    assert worst <= 1e-4                                     # test_trajectory_matches_fp64_adam's tolerance
    assert worst_loss <= 1e-4

"""GPU: the bound field-form elicitation session (VFM.elicit_field_bound, include/vfm_bound.h: vfm_elicit_bound_f32) --
bitwise against the composition of select_next_questions_field and fold_in_bound(reset=False) it replaces (both links,
all four strategies, F = 2 and F = 3 with the first and a middle field, history, reset, n_iters 1 and 3, exhausted
pools, one d per lane shape of the loss pass), the dual system turning primal inside a session, the triangle in LDS
against the workspace (past the slab grid cap), independence of the other respondents, write=False, the per-round
moments, ties and the guards, the fp64 restatement along the session's own rows, and the curve.

Bounds of the fp64 test: those of test_gpu_foldin_bound.py at the same n_iters, since a round's fold is that kernel's
per-entity work from an fp32 start both sides share -- rel_err <= 1e-4 for the parameters; per element
|got - ref| <= 2^-23 |ref| + n_iters solve_abs_term(d, cond_max, ref) for the means and the same plus scale_abs_term for
the scales; <= 1e-5 for the loss against the fp64 B_e at the returned parameters; cond <= 1e3 asserted first
(tests/test_elicit_bound_cpu.py asserts it for the restatement's own choices).  The restatement asks the rows the
session asked and starts each fold at the fp32 posterior the session returned for the round before, so a near-tie in
the argmax cannot fail the test.

Measured on an MI355X: see DESIGN.md §4 "Bound sessions" (the printed BOUND lines)."""
import numpy as np
import pytest
import torch

import bound_reference as BR
import elicit_bound_restatement as RB
import solve_reference as SR
from golden_util import rel_err
from test_gpu_elicit import _same_bits, _set_prior, _theta_rows
from test_gpu_elicit_field import _problem, _same
from test_gpu_foldin import _model

pytestmark = pytest.mark.gpu
DEV = "cuda"
A3, C2 = (40, 90, 4), (40, 90)


def _composed(m, pool, y_pool, Q, field, strategy, hist, seed, klw, n_iters, reset, key_field=None):
    """The loop the session replaces, on the public pieces (modifies m): with reset the prior is written first; per round
    select_next_questions_field with seed + q on the rows still unasked, then fold_in_bound(reset=False) of the answering
    respondents on their history followed by everything they were asked so far.  Returns entities, rows, score, loss
    [U, Q], theta [U, Q, 2d + 2]."""
    ents = torch.unique(pool[:, field])
    U, P = ents.numel(), pool.shape[0]
    if reset:
        _set_prior(m, ents)
    rows = torch.full((U, Q), -1, dtype=torch.int64, device=DEV)
    score = torch.full((U, Q), float("nan"), device=DEV)
    loss = torch.full((U, Q), float("nan"), device=DEV)
    theta = torch.empty(U, Q, 2 * m.d + 2, device=DEV)
    unasked = torch.ones(P, dtype=torch.bool, device=DEV)
    asked = torch.zeros(0, dtype=torch.int64, device=DEV)              # caller indices in the order asked
    hx, hy = hist if hist is not None else (pool[:0], y_pool[:0])
    for q in range(Q):
        idx = torch.nonzero(unasked).reshape(-1)
        if idx.numel():
            sub = pool[idx]
            es, r = m.select_next_questions_field(sub, field, 1, strategy, seed + q, key_field)
            _, _, sc = m.field_moments(sub, field, strategy, seed + q, key_field)
            epos = torch.searchsorted(ents, es)
            rows[epos, q] = idx[r[:, 0]]
            score[epos, q] = sc[r[:, 0]]
            unasked[idx[r[:, 0]]] = False
            asked = torch.cat([asked, idx[r[:, 0]]])
            ha = torch.isin(hx[:, field], es)
            aa = asked[torch.isin(pool[asked, field], es)]
            X, y = torch.cat([hx[ha], pool[aa]]), torch.cat([hy[ha], y_pool[aa]])
            o = m.fold_in_bound(X, y, field=field, kl_weight=klw, n_iters=n_iters, reset=False)
            assert torch.equal(o["entities"], es)
            loss[epos, q] = o["loss"]
        theta[:, q] = _theta_rows(m, ents)
    return ents, rows, score, loss, theta


def _against_the_composition(m, pool, y_pool, Q, field, strategy, hist, reset, n_iters, key_field=None, lds_dim=-1,
                             klw=0.8, seed=21):
    from vae_amd import elicit
    start = m._flat.clone()
    ents, rows, score, loss, theta = _composed(m, pool, y_pool, Q, field, strategy, hist, seed, klw, n_iters, reset,
                                               key_field)
    final = m._flat.clone()
    m._flat.copy_(start)
    m.params_changed()
    out = elicit.run_field_bound(m, pool, y_pool, Q, field, strategy, history=hist, seed=seed, kl_weight=klw,
                                 n_iters=n_iters, reset=reset, write=True, return_theta=True, key_field=key_field,
                                 lds_dim=lds_dim)
    assert torch.equal(out["entities"], ents)
    assert torch.equal(out["rows"], rows)
    assert _same_bits(out["score"], score)                   # (NaN where nothing was left to ask, in both)
    assert _same_bits(out["loss"], loss)
    assert _same_bits(out["theta"], theta)
    assert torch.equal(m._flat, final)                       # write=True: the composition's table
    assert not torch.equal(final, start)
    assert bool(torch.isfinite(out["loss"][out["rows"] >= 0]).all())
    return out


# d: 1; then one per (W, CPL) shape of the loss pass -- 8 (8, 1), 9 (16, 1), 17 (32, 1), 33 (64, 1), 65 (64, 2), 129
# (64, 4), 257 (64, 8).  Pools of 1 and 3 rows run out before Q = 6; 20 history rows: primal from round 0 at d < 20
CASES = [  # field sizes, field, link, strategy, d, history, reset, n_iters
    (A3, 0, "abs", "variance", 1, True, False, 3),
    (C2, 0, "softplus", "top", 8, False, True, 1),
    (C2, 1, "abs", "random", 9, True, False, 3),
    (A3, 1, "softplus", "mean", 17, True, True, 1),
    (A3, 0, "abs", "top", 33, True, False, 3),
    (A3, 0, "softplus", "random", 65, False, False, 1),
    (A3, 1, "abs", "mean", 129, True, False, 3),
    (A3, 0, "softplus", "variance", 257, True, True, 1),
]


@pytest.mark.parametrize("sizes,field,link,strategy,d,with_hist,reset,n_iters", CASES)
def test_bitwise_against_the_composition(sizes, field, link, strategy, d, with_hist, reset, n_iters):
    m = _model(sizes, d, "class", link, seed=d + len(strategy), rng_seed=3)
    small = sizes == C2 and field == 1                       # (40 contexts in all)
    key = [f for f in range(len(sizes)) if f != field][0]    # the default key column
    pool, y_pool, hx, hy = _problem(m, field, 11, [3, 9, 17, 12 if small else 30, 1], [20, 0, 4, 11] if with_hist else [0],
                                    seed=d, distinct_col=key if strategy == "random" and not small else None)
    assert set(y_pool.tolist()) <= {0.0, 1.0}
    out = _against_the_composition(m, pool, y_pool, 6, field, strategy, (hx, hy) if with_hist else None, reset, n_iters)
    rows = out["rows"]
    assert out["entities"].numel() == 11
    assert int((rows < 0).sum()) > 0 and int((rows[:, 0] >= 0).sum()) == 11


@pytest.mark.parametrize("d,n_hist,Q", [(5, 3, 6), (8, 0, 10)])
def test_the_dual_system_turns_primal_inside_a_session(d, n_hist, Q):
    """n = history + rounds so far crosses d: d = 5 with 3 history rows in round 2, d = 8 without history in round 8."""
    m = _model(A3, d, "class", "softplus", seed=7)
    pool, y_pool, hx, hy = _problem(m, 0, 6, [14, 11], [n_hist], seed=3)
    out = _against_the_composition(m, pool, y_pool, Q, 0, "mean", (hx, hy) if n_hist else None, False, 3)
    assert int((out["rows"] < 0).sum()) == 0                 # every round folded: n ran from n_hist + 1 to n_hist + Q > d


def _storages(m, pool, y_pool, Q, hist, lds_dims):
    from vae_amd import elicit
    kw = dict(history=hist, seed=3, kl_weight=0.9, n_iters=3, return_theta=True, return_moments=True)
    runs = [elicit.run_field_bound(m, pool, y_pool, Q, 0, "variance", lds_dim=ld, **kw) for ld in lds_dims]
    for b in runs[1:]:
        for k in runs[0]:
            assert _same(runs[0][k], b[k]), k
    return runs[0]


def test_where_the_triangle_lives_does_not_matter():
    # d = 5: every system in LDS (-1), every system in the slabs (0), the dual ones up to 3 rows in LDS (3)
    m = _model(A3, 5, "class", "softplus", seed=8)
    pool, y_pool, hx, hy = _problem(m, 0, 11, [9, 14, 3], [0, 2, 7], seed=12)
    a = _storages(m, pool, y_pool, 6, (hx, hy), (-1, 0, 3))
    assert bool(torch.isfinite(a["loss"][a["rows"] >= 0]).all()) and int((a["rows"] < 0).sum()) > 0
    # SLABS + 5 respondents with every system in the slabs: more than the grid cap, so blocks take a second respondent
    # and rebuild their slab, their LDS and their row weights for it
    n = SR.SLABS + 5
    m = _model((n + 20, 30, 4), 5, "class", "abs", seed=8)
    pool, y_pool, hx, hy = _problem(m, 0, n, [5, 8, 3], [0, 2, 7], seed=12)
    a = _storages(m, pool, y_pool, 4, (hx, hy), (-1, 0))
    assert a["entities"].numel() == n and bool(torch.isfinite(a["loss"][a["rows"] >= 0]).all())


def test_independent_of_the_other_respondents_and_of_their_pools_order():
    m = _model(A3, 16, "class", "softplus", seed=6)
    pool, y_pool, hx, hy = _problem(m, 0, 10, [14, 6, 2, 30], [5, 0, 12], seed=8)
    kw = dict(history=(hx, hy), seed=4, n_iters=3, return_theta=True)
    Q = 5
    full = m.elicit_field_bound(pool, y_pool, Q, 0, "mean", **kw)
    row_of = lambda o, p: torch.where((o["rows"] >= 0)[..., None], p[o["rows"].clamp(min=0)], -1)
    ents = full["entities"].tolist()
    for i, e in enumerate(ents):
        sel = pool[:, 0] == e
        hs = hx[:, 0] == e
        one = m.elicit_field_bound(pool[sel], y_pool[sel], Q, 0, "mean", **dict(kw, history=(hx[hs], hy[hs])))
        assert torch.equal(row_of(one, pool[sel]), row_of(full, pool)[i:i + 1])
        for k in ("score", "loss", "theta"):
            assert _same_bits(one[k], full[k][i:i + 1]), (e, k)
    # the OTHER respondents' pools permuted, the first respondent's rows where they were
    mine = torch.nonzero(pool[:, 0] == ents[0]).reshape(-1)
    others = torch.nonzero(pool[:, 0] != ents[0]).reshape(-1)
    perm = torch.arange(pool.shape[0], device=DEV)
    perm[others] = others[torch.randperm(others.numel(), generator=torch.Generator().manual_seed(1)).to(DEV)]
    shuf = m.elicit_field_bound(pool[perm], y_pool[perm], Q, 0, "mean", **kw)
    assert torch.equal(shuf["rows"][0], full["rows"][0]) and bool((perm[mine] == mine).all())
    assert torch.equal(row_of(full, pool), row_of(shuf, pool[perm]))
    for k in ("score", "loss", "theta"):
        assert _same_bits(full[k], shuf[k]), k


def test_write_false_leaves_the_model_alone():
    m = _model(A3, 16, "class", "abs", seed=5)
    pool, y_pool, hx, hy = _problem(m, 0, 9, [10, 4, 25], [3, 0], seed=1)
    before = m._flat.clone()
    kw = dict(history=(hx, hy), return_theta=True, return_moments=True)
    a = m.elicit_field_bound(pool, y_pool, 5, 0, "variance", **kw)
    assert torch.equal(m._flat, before)
    b = m.elicit_field_bound(pool, y_pool, 5, 0, "variance", **kw)
    assert torch.equal(m._flat, before)
    for k in a:
        assert _same(a[k], b[k]), k
    assert bool(torch.isfinite(a["loss"][a["rows"] >= 0]).all())


@pytest.mark.parametrize("link,d", [("abs", 5), ("softplus", 128)])
def test_round_moments_are_field_moments_of_that_rounds_posterior(link, d):
    m = _model(A3, d, "class", link, seed=9)
    pool, y_pool, _, _ = _problem(m, 0, 8, [11, 3, 20], [0], seed=2)
    Q = 4
    out = m.elicit_field_bound(pool, y_pool, Q, 0, "mean", n_iters=2, return_theta=True, return_moments=True)
    ents = out["entities"]
    ent, bia, _ = m._views(m._flat)
    for q in range(Q + 1):
        if q > 0:
            ent[ents] = out["theta"][:, q - 1, :2 * d]
            bia[ents] = out["theta"][:, q - 1, 2 * d:]
            m.params_changed()
        mean, var, _ = m.field_moments(pool, 0)
        assert _same_bits(out["logit_mean"][q], mean) and _same_bits(out["logit_var"][q], var), q


@pytest.mark.parametrize("strategy,reset", [("mean", False), ("variance", True)])
def test_equal_contexts_tie_and_the_lower_pool_row_is_asked_first(strategy, reset):
    """One respondent, 300 pool rows: 150 distinct contexts, every context twice, the second copy at least a wave away
    and with the other answer.  Two rows of one context have the same operand, hence the same score in every round: the
    lower position of each pair is asked before the higher."""
    m = _model(A3, 16, "class", "abs", seed=11)
    pool, y_pool, _, _ = _problem(m, 0, 1, [150], [0], seed=5)
    perm = torch.randperm(150, generator=torch.Generator().manual_seed(2)).to(DEV)
    pool2, y2 = torch.cat([pool, pool[perm]]), torch.cat([y_pool, 1.0 - y_pool[perm]])
    Q = 40
    out = m.elicit_field_bound(pool2, y2, Q, 0, strategy, n_iters=2, reset=reset)
    order = out["rows"][0].tolist()
    assert len(set(order)) == Q and min(order) >= 0
    when = {r: q for q, r in enumerate(order)}
    pos = {int(j): 150 + i for i, j in enumerate(perm.tolist())}         # context j's second copy
    seen = 0
    for r in order:
        if r >= 150:                                        # a second copy: its first copy was asked before it
            j = int(perm[r - 150])
            assert j in when and when[j] < when[r], r
            seen += 1
        else:
            assert pos[r] not in when or when[pos[r]] > when[r]
    print(f"{strategy}: {seen} second copies among the {Q} rows asked")


def test_guards_an_invalid_context_a_respondent_outside_the_table_no_rounds_and_no_respondents():
    """A context id >= T and a negative one, planted through the torch op past the Python checks: NaN moments in every
    round, never asked, the respondent's other rows asked as if the bad rows were not there.  A respondent id >= T asks
    nothing.  Q = 0 returns empty results and, with return_moments, the one scoring pass.  U = 0 launches nothing."""
    from vae_amd import _lib, elicit
    m = _model(A3, 16, "class", "softplus", seed=13)
    pool, y_pool, _, _ = _problem(m, 0, 3, [6, 4], [0], seed=6)
    Q, n_iters = 8, 3
    good = m.elicit_field_bound(pool, y_pool, Q, 0, "variance", n_iters=n_iters, return_theta=True)
    bad = pool[:2].clone()
    bad[0, 1], bad[1, 2] = m.T + 5, -3
    ghost = pool[:3].clone()
    ghost[:, 0] = m.T + 2                                    # a respondent outside the table, sorted last
    x, y = torch.cat([bad, pool, ghost]), torch.cat([y_pool[:2], y_pool, y_pool[:3]])
    order, ents, ptr = elicit.pool_lists(x, 0)
    px, ys = x[order].contiguous(), y[order].contiguous()
    ctx = px.clone()
    ctx[:, 0] = 0
    op_x, inv = torch.unique(ctx, dim=0, return_inverse=True)
    U, P, d = ents.numel(), px.shape[0], m.d
    assert U == 4
    o = _lib.ops()
    out_row = torch.full((U, Q), -7, dtype=torch.int64, device=DEV)
    score, loss = torch.zeros(U, Q, device=DEV), torch.zeros(U, Q, device=DEV)
    theta = torch.zeros(U, Q, 2 * d + 2, device=DEV)
    mean, var = torch.zeros(Q + 1, P, device=DEV), torch.zeros(Q + 1, P, device=DEV)
    ws = torch.empty(o.elicit_bound_workspace_bytes(U, P, 0, op_x.shape[0], d, Q, -1), dtype=torch.uint8, device=DEV)
    ent, bia, scal = m._views(m._flat)
    before = m._flat.clone()
    o.elicit_bound(ents, ptr, px, ys, None, None, None, op_x.contiguous(), inv.reshape(-1).contiguous(), None, ent, bia,
                   scal, ws, out_row, score, loss, theta, mean, var, 0, 1, Q, 1, 16, 0, 1, -1, 1.0, 0, n_iters)
    rows = elicit.rows_to_caller(out_row, order)
    assert not bool(((rows == 0) | (rows == 1)).any())                  # the planted rows: never asked
    assert torch.equal(torch.where(rows[:3] >= 0, rows[:3] - 2, rows[:3]), good["rows"])
    assert _same_bits(score[:3], good["score"]) and _same_bits(loss[:3], good["loss"])
    assert _same_bits(theta[:3], good["theta"])
    assert bool((rows[3] == -1).all()) and bool(torch.isnan(score[3]).all()) and bool(torch.isnan(loss[3]).all())
    mean, var = elicit.to_caller_order(mean, order), elicit.to_caller_order(var, order)
    n = pool.shape[0]
    assert bool(torch.isnan(mean[:, :2]).all()) and bool(torch.isnan(var[:, :2]).all())
    assert bool(torch.isfinite(mean[:, 2:2 + n]).all()) and bool(torch.isnan(mean[:, 2 + n:]).all())
    # write = 1 wrote the three real respondents' rows and nothing else
    changed = m._flat != before
    allowed = torch.zeros_like(changed)
    for e in ents[:3].tolist():
        allowed[e * 2 * d:(e + 1) * 2 * d] = True
        allowed[m._off_bias + 2 * e: m._off_bias + 2 * e + 2] = True
    assert bool(changed.any()) and not bool((changed & ~allowed).any())
    m._flat.copy_(before)
    m.params_changed()
    z = m.elicit_field_bound(pool, y_pool, 0, 0, "variance", return_moments=True, return_theta=True, write=True)
    assert z["rows"].shape == (3, 0) and z["loss"].shape == (3, 0) and z["theta"].shape == (3, 0, 2 * d + 2)
    m0, v0, _ = m.field_moments(pool, 0)
    assert _same_bits(z["logit_mean"][0], m0) and _same_bits(z["logit_var"][0], v0)
    assert torch.equal(m._flat, before)                      # (write with no round: the rows written are the rows read)
    z = m.elicit_field_bound(pool[:0], y_pool[:0], 3, 0, "variance", return_theta=True, write=True)
    assert z["entities"].numel() == 0 and z["rows"].shape == (0, 3) and z["theta"].shape == (0, 3, 2 * d + 2)
    assert torch.equal(m._flat, before)


def _model_of(c):
    """A 'class' model holding the tables of a case of the restatement."""
    from vae_amd.model import VFM
    torch.manual_seed(0)
    m = VFM(field_sizes=list(c["sizes"]), embedding_size=c["d"], output="class", link=c["link"], device=DEV)
    m.entity_params.weight.data.copy_(c["ent"])
    m.bias_params.weight.data.copy_(c["bia"])
    m._flat[m._off_scal: m._off_scal + 3] = c["scal"].to(DEV)
    return m


def _tuple_of(t, d):
    """A row [mu | s | mu_w | s_w] of return_theta as the restatement's (mu, s, mu_w, s_w), fp64."""
    t = t.double().numpy()
    return t[:d], t[d:2 * d], float(t[2 * d]), float(t[2 * d + 1])


@pytest.mark.parametrize("name", sorted(RB.CASES))
def test_against_the_fp64_restatement_along_the_sessions_own_rows(name):
    c = RB.case(name)
    m = _model_of(c)
    d, f, Q, n_iters = c["d"], c["field"], RB.CASE_ROUNDS, c["n_iters"]
    hist = (c["hist_x"].to(DEV), c["hist_y"].to(DEV)) if c["hist_x"].shape[0] else None
    before = m._flat.clone()
    out = m.elicit_field_bound(c["pool"].to(DEV), c["y_pool"].to(DEV), Q, f, c["strategy"], history=hist,
                               kl_weight=c["kl_weight"], n_iters=n_iters, reset=c["reset"], return_theta=True)
    assert torch.equal(m._flat, before)
    rows, theta, loss = out["rows"].cpu().numpy(), out["theta"].cpu(), out["loss"].cpu().numpy()
    U = rows.shape[0]
    assert U == RB.CASE_RESPONDENTS and int((rows < 0).sum()) == 0
    # each round's fold starts from the fp32 posterior the session returned for the round before (round 0: the
    # restatement's own start, the table row or the prior row)
    start = [[None if q == 0 else _tuple_of(theta[u, q - 1], d) for q in range(Q)] for u in range(U)]
    for u, e in enumerate(out["entities"].tolist()):
        start[u][0] = (RB.prior_theta32(d, c["link"]) if c["reset"] else
                       RB.R.table_theta(c["ent"].numpy().astype(np.float64), c["bia"].numpy().astype(np.float64), e))
    ref = RB.case_sessions(c, along=rows, start=start)
    assert out["entities"].tolist() == [s["entity"] for s in ref]
    worst, got_t, ref_t, got_s, ref_s, got_l, ref_l, cond_max, agree = 0.0, [], [], [], [], [], [], 0.0, 0
    own = RB.case_sessions(c)
    for u, s in enumerate(ref):
        agree += int([int(s["sel"][r]) for r in own[u]["rows"]] == rows[u].tolist())
        for q in range(Q):
            cond = s["cond"][q]
            assert cond <= 1e3, (name, u, q, cond)           # (the condition on the inputs, on the rows actually asked)
            cond_max = max(cond_max, cond)
            rt, rs = s["unrounded"][q]
            th = theta[u, q]
            gt = torch.cat([th[2 * d:2 * d + 1], th[:d]])
            gs = torch.cat([th[2 * d + 1:], th[d:2 * d]])
            at = n_iters * SR.solve_abs_term(d, cond, rt)
            ok_t, w_t = SR.elementwise_ok(gt, rt, at)
            ok_s, w_s = SR.elementwise_ok(gs, rs, at + SR.scale_abs_term(s["n"][q], rs))
            worst = max(worst, w_t, w_s)
            assert ok_t and ok_s, (name, u, q, s["n"][q], w_t, w_s)
            got_t.append(gt.numpy()); ref_t.append(rt); got_s.append(gs.numpy()); ref_s.append(rs)
            X = torch.from_numpy(s["fold_x"][q])
            got_l.append(float(loss[u, q]))
            ref_l.append(BR.bound_objective_fp64(c["ent"], c["bia"], c["scal"], X, torch.from_numpy(s["fold_y"][q]).float(),
                                                 f, c["link"], c["kl_weight"], s["entity"], gt, gs))
    e_rows = max(rel_err(np.array(got_t), np.array(ref_t)), rel_err(np.array(got_s), np.array(ref_s)))
    e_loss = rel_err(np.array(got_l), np.array(ref_l))       # (that file's measure: against the largest B_e of the case)
    e_each = float(np.max(np.abs(np.array(got_l) - np.array(ref_l)) / np.abs(np.array(ref_l))))
    print(f"BOUND session {name} {c['link']} F={len(c['sizes'])} d={d} n_iters={n_iters} reset={int(c['reset'])}: rows "
          f"{e_rows:.2e} loss {e_loss:.2e} (each fold's own: {e_each:.2e}) worst elementwise ratio {worst:.3f} cond {cond_max:.1f}; {agree} of {U} "
          f"respondents ask the fp64 session's own rows")
    assert e_rows <= 1e-4, e_rows
    assert e_loss <= 1e-5, e_loss


def test_a_reg_model_is_refused():
    m = _model(A3, 8, "reg", "abs", seed=1)
    pool, y_pool, _, _ = _problem(m, 0, 3, [4], [0], seed=1)
    with pytest.raises(ValueError, match="'class'"):
        m.elicit_field_bound(pool, (y_pool > 1.0).float(), 2, 0, "variance")


def test_curve_returns_finite_aucs_and_counts_the_rows_left():
    from vae_amd import elicit
    m = _model(A3, 16, "class", "abs", seed=12)
    pool, y_pool, _, _ = _problem(m, 0, 12, [9, 15, 2], [0], seed=3, distinct_col=1)
    Q = 4
    start = m._flat.clone()
    c = m.elicitation_curve_field_bound(pool, y_pool, Q, 0, strategies=("mean", "random", "variance"), seed=5, n_iters=3)
    assert torch.equal(m._flat, start)
    sizes = torch.unique(pool[:, 0], return_counts=True)[1]
    for s in ("mean", "random", "variance"):
        assert len(c[s]) == Q + 1 and all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in c[s])
        left = c["n_unasked"][s]
        assert left[0] == pool.shape[0]
        for q in range(Q):                                   # one row fewer per respondent that still had one
            assert left[q] - left[q + 1] == int((sizes > q).sum()), (s, q)
    r = m.elicit_field_bound(pool, y_pool, Q, 0, "random", seed=5, n_iters=3, return_moments=True)
    keep = elicit.asked_round(r["rows"], pool.shape[0]) >= 2
    assert c["random"][2] == elicit.metric("class", r["logit_mean"][2][keep], r["logit_var"][2][keep], y_pool[keep])

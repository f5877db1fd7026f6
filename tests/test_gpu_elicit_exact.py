"""GPU: the exact field-form elicitation session (VFM.elicit_field_exact, include/vfm_elicit.h: vfm_elicit_solve_f32) --
bitwise against the composition of select_next_questions_field and fold_in_exact it replaces (both links, all four
strategies, F = 2 and F = 3 with the first and a middle field, history, reset, exhausted pools, one d per lane shape of
the loss pass and d = 1 and 512), ragged pools over more than one wave, the dual system turning primal inside a
session, the triangle in LDS against the workspace (past the slab grid cap, and a 301 x 301 system), independence of the
other respondents, write=False, the per-round moments, ties and the guards, the fp64 restatement on planted models, and
the curve.

Bounds of the restatement test: those of test_gpu_foldin_exact.py for fold_in_exact against solve_fp64 (rel_err <= 1e-4
for the parameters, <= 1e-5 for the loss against objective_fp64 at the returned parameters, cond(H) <= 1e3 asserted
first): the arithmetic is the same.  The cond(H) assertion separates the kernel from the conditioning for the primal
form only: the dual form (n <= d rows) factors K = I / prec + U D^-1 U^T, whose conditioning is cond(K);
test_gpu_solve_edges.py asserts that one and runs sessions across the solver's storage and width edges."""
import contextlib

import numpy as np
import pytest
import torch

import elicit_exact_restatement as RX
import elicit_field_restatement as RF
from golden_util import rel_err
from test_foldin_cpu import objective_fp64
from test_gpu_elicit import _same_bits, _set_prior, _theta_rows
from test_gpu_elicit_field import _problem, _same
from test_gpu_foldin import _model

pytestmark = pytest.mark.gpu
DEV = "cuda"
A3, C2 = (40, 90, 4), (40, 90)


@contextlib.contextmanager
def _scores_of_a_class_model(m, strategy):
    """'mean' (closest to p = 0.5) is refused for 'reg' models by the Python checks of both halves; the kernels score
    it from the moments alone.  For that strategy the checks are stepped over: the model calls itself 'class' while the
    composition selects, and the session is entered below its strategy check."""
    if strategy != "mean":
        yield
        return
    m.output = "class"
    try:
        yield
    finally:
        m.output = "reg"


def _session(m, pool, y_pool, Q, field, strategy, monkeypatch=None, **kw):
    from vae_amd import elicit
    if strategy == "mean":
        monkeypatch.setattr(elicit, "_check_questions", lambda model, s, n: None)
    return elicit.run_field_exact(m, pool, y_pool, Q, field, strategy, **kw)


def _composed(m, pool, y_pool, Q, field, strategy, hist, seed, klw, reset, key_field=None):
    """The loop the session replaces, on the public pieces (modifies m): per round select_next_questions_field with
    seed + q on the rows still unasked, then fold_in_exact of the answering respondents on their history followed by
    everything they were asked so far.  Returns entities, rows, score, loss [U, Q], theta [U, Q, 2d + 2]."""
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
            with _scores_of_a_class_model(m, strategy):
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
            o = m.fold_in_exact(X, y, field=field, kl_weight=klw)
            assert torch.equal(o["entities"], es)
            loss[epos, q] = o["loss"]
        theta[:, q] = _theta_rows(m, ents)
    return ents, rows, score, loss, theta


def _against_the_composition(m, pool, y_pool, Q, field, strategy, hist, reset, key_field=None, monkeypatch=None,
                             lds_dim=-1, klw=0.8, seed=21):
    start = m._flat.clone()
    ents, rows, score, loss, theta = _composed(m, pool, y_pool, Q, field, strategy, hist, seed, klw, reset, key_field)
    final = m._flat.clone()
    m._flat.copy_(start)
    m.params_changed()
    out = _session(m, pool, y_pool, Q, field, strategy, monkeypatch, history=hist, seed=seed, kl_weight=klw, reset=reset,
                   write=True, return_theta=True, key_field=key_field, lds_dim=lds_dim)
    assert torch.equal(out["entities"], ents)
    assert torch.equal(out["rows"], rows)
    assert _same_bits(out["score"], score)                   # (NaN where nothing was left to ask, in both)
    assert _same_bits(out["loss"], loss)
    assert _same_bits(out["theta"], theta)
    assert torch.equal(m._flat, final)                       # write=True: the composition's table
    assert not torch.equal(final, start)
    return out


# d: 1; then one per (W, CPL) shape of the loss pass -- 8 (8, 1), 9 (16, 1), 17 (32, 1), 33 (64, 1), 65 (64, 2), 129
# (64, 4), 257 and 512 (64, 8); 257 and 512: the primal system only in the slab.  Pools of 1 and 3 rows run out before
# Q = 6; 60 history rows: primal from round 0 at d < 60, dual throughout above
CASES = [  # field sizes, field, link, strategy, d, history, reset
    (A3, 0, "abs", "variance", 1, True, False),
    (C2, 0, "softplus", "top", 8, False, True),
    (C2, 1, "abs", "random", 9, True, False),
    (A3, 1, "softplus", "variance", 17, True, True),
    (A3, 0, "abs", "top", 33, True, False),
    (A3, 0, "softplus", "random", 65, False, False),
    (A3, 1, "abs", "variance", 129, True, False),
    (A3, 0, "softplus", "top", 257, True, True),
    (A3, 0, "abs", "variance", 512, True, False),
    (C2, 0, "abs", "variance", 16, True, False),
    (A3, 0, "abs", "mean", 9, True, False),
    (A3, 1, "softplus", "mean", 33, False, True),
]


@pytest.mark.parametrize("sizes,field,link,strategy,d,with_hist,reset", CASES)
def test_bitwise_against_the_composition(sizes, field, link, strategy, d, with_hist, reset, monkeypatch):
    m = _model(sizes, d, "reg", link, seed=d + len(strategy), rng_seed=3)
    small = sizes == C2 and field == 1                       # (40 contexts in all)
    key = [f for f in range(len(sizes)) if f != field][0]    # the default key column
    pool, y_pool, hx, hy = _problem(m, field, 11, [3, 9, 17, 12 if small else 30, 1],
                                    ([20, 0, 4, 11] if small else [60, 0, 4, 11]) if with_hist else [0], seed=d,
                                    distinct_col=key if strategy == "random" and not small else None)
    out = _against_the_composition(m, pool, y_pool, 6, field, strategy, (hx, hy) if with_hist else None, reset,
                                   monkeypatch=monkeypatch)
    rows = out["rows"]
    assert out["entities"].numel() == 11
    assert int((rows < 0).sum()) > 0 and int((rows[:, 0] >= 0).sum()) == 11


def test_ragged_pools_over_the_waves():
    """37 respondents with pools of 1 / 63 / 64 / 65 / 259 rows: the scoring loop with and without a second trip, the
    waves of the reduction empty, partly and wholly filled."""
    m = _model(A3, 9, "reg", "abs", seed=4)
    pool, y_pool, hx, hy = _problem(m, 0, 37, [1, 63, 64, 65, 259], [0, 5], seed=9)
    _against_the_composition(m, pool, y_pool, 4, 0, "variance", (hx, hy), False)
    m = _model(A3, 9, "reg", "softplus", seed=4)
    pool, y_pool, hx, hy = _problem(m, 0, 37, [1, 63, 64, 65, 259], [0, 5], seed=10)
    _against_the_composition(m, pool, y_pool, 3, 0, "top", (hx, hy), True)


@pytest.mark.parametrize("d,n_hist,Q", [(5, 3, 6), (8, 0, 10)])
def test_the_dual_system_turns_primal_inside_a_session(d, n_hist, Q):
    """n = history + rounds so far crosses d: d = 5 with 3 history rows in round 2, d = 8 without history in round 8."""
    m = _model(A3, d, "reg", "softplus", seed=7)
    pool, y_pool, hx, hy = _problem(m, 0, 6, [14, 11], [n_hist], seed=3)
    out = _against_the_composition(m, pool, y_pool, Q, 0, "variance", (hx, hy) if n_hist else None, False)
    assert int((out["rows"] < 0).sum()) == 0                 # every round folded: n ran from n_hist + 1 to n_hist + Q > d


def _both_storages(m, pool, y_pool, Q, hist):
    from vae_amd import elicit
    kw = dict(history=hist, seed=3, kl_weight=0.9, return_theta=True, return_moments=True)
    a = elicit.run_field_exact(m, pool, y_pool, Q, 0, "variance", lds_dim=-1, **kw)
    b = elicit.run_field_exact(m, pool, y_pool, Q, 0, "variance", lds_dim=0, **kw)
    for k in a:
        assert _same(a[k], b[k]), k
    return a


def test_where_the_triangle_lives_does_not_matter():
    # 300 respondents at d = 5 with every system in the slabs: more than the 256-block grid cap, so blocks take a
    # second respondent and rebuild their slab and LDS for it
    m = _model((320, 30, 4), 5, "reg", "abs", seed=8)
    pool, y_pool, hx, hy = _problem(m, 0, 300, [5, 8, 3], [0, 2, 7], seed=12)
    a = _both_storages(m, pool, y_pool, 4, (hx, hy))
    assert a["entities"].numel() == 300 and bool(torch.isfinite(a["loss"][a["rows"] >= 0]).all())
    # one respondent at d = 300 with 305 history rows: the primal 301 x 301 system, in the slab whatever lds_dim says
    m = _model(A3, 300, "reg", "softplus", seed=8)
    pool, y_pool, hx, hy = _problem(m, 0, 1, [10], [305], seed=13)
    a = _both_storages(m, pool, y_pool, 2, (hx, hy))
    assert bool(torch.isfinite(a["loss"]).all())
    # against fold_in_exact on the same rows (the last round's posterior)
    last = torch.cat([hx, pool[a["rows"][0]]]), torch.cat([hy, y_pool[a["rows"][0]]])
    start = m._flat.clone()
    o = m.fold_in_exact(*last, field=0, kl_weight=0.9)
    assert _same_bits(_theta_rows(m, a["entities"]), a["theta"][:, -1]) and _same_bits(o["loss"], a["loss"][:, -1])
    m._flat.copy_(start)
    m.params_changed()


def test_independent_of_the_other_respondents_and_of_their_pools_order():
    m = _model(A3, 16, "reg", "softplus", seed=6)
    pool, y_pool, hx, hy = _problem(m, 0, 10, [14, 6, 2, 33], [5, 0, 45], seed=8)
    kw = dict(history=(hx, hy), seed=4, return_theta=True)
    Q = 5
    full = m.elicit_field_exact(pool, y_pool, Q, 0, "variance", **kw)
    row_of = lambda o, p: torch.where((o["rows"] >= 0)[..., None], p[o["rows"].clamp(min=0)], -1)
    ents = full["entities"].tolist()
    for i, e in enumerate(ents):
        sel = pool[:, 0] == e
        hs = hx[:, 0] == e
        one = m.elicit_field_exact(pool[sel], y_pool[sel], Q, 0, "variance", **dict(kw, history=(hx[hs], hy[hs])))
        assert torch.equal(row_of(one, pool[sel]), row_of(full, pool)[i:i + 1])
        for k in ("score", "loss", "theta"):
            assert _same_bits(one[k], full[k][i:i + 1]), (e, k)
    # the OTHER respondents' pools permuted, the first respondent's rows where they were
    mine = torch.nonzero(pool[:, 0] == ents[0]).reshape(-1)
    others = torch.nonzero(pool[:, 0] != ents[0]).reshape(-1)
    perm = torch.arange(pool.shape[0], device=DEV)
    perm[others] = others[torch.randperm(others.numel(), generator=torch.Generator().manual_seed(1)).to(DEV)]
    shuf = m.elicit_field_exact(pool[perm], y_pool[perm], Q, 0, "variance", **kw)
    assert torch.equal(shuf["rows"][0], full["rows"][0]) and bool((perm[mine] == mine).all())
    assert torch.equal(row_of(full, pool), row_of(shuf, pool[perm]))
    for k in ("score", "loss", "theta"):
        assert _same_bits(full[k], shuf[k]), k


def test_write_false_leaves_the_model_alone():
    m = _model(A3, 16, "reg", "abs", seed=5)
    pool, y_pool, hx, hy = _problem(m, 0, 9, [10, 4, 25], [3, 0], seed=1)
    before = m._flat.clone()
    kw = dict(history=(hx, hy), return_theta=True, return_moments=True)
    a = m.elicit_field_exact(pool, y_pool, 5, 0, "variance", **kw)
    assert torch.equal(m._flat, before)
    b = m.elicit_field_exact(pool, y_pool, 5, 0, "variance", **kw)
    assert torch.equal(m._flat, before)
    for k in a:
        assert _same(a[k], b[k]), k
    assert bool(torch.isfinite(a["loss"][a["rows"] >= 0]).all())
    # reset changes round 0's scoring only: from round 0's fold on, a session that asked the same first row agrees
    c = m.elicit_field_exact(pool, y_pool, 1, 0, "variance", history=(hx, hy), reset=True, return_theta=True)
    same_first = c["rows"][:, 0] == a["rows"][:, 0]
    print(f"reset: {int(same_first.sum())} of {same_first.numel()} respondents ask the same first row from the prior")
    assert _same_bits(c["theta"][same_first, 0], a["theta"][same_first, 0])


@pytest.mark.parametrize("link,d", [("abs", 5), ("softplus", 128)])
def test_round_moments_are_field_moments_of_that_rounds_posterior(link, d):
    m = _model(A3, d, "reg", link, seed=9)
    pool, y_pool, _, _ = _problem(m, 0, 8, [11, 3, 20], [0], seed=2)
    Q = 4
    out = m.elicit_field_exact(pool, y_pool, Q, 0, "variance", return_theta=True, return_moments=True)
    ents = out["entities"]
    ent, bia, _ = m._views(m._flat)
    for q in range(Q + 1):
        if q > 0:
            ent[ents] = out["theta"][:, q - 1, :2 * d]
            bia[ents] = out["theta"][:, q - 1, 2 * d:]
            m.params_changed()
        mean, var, _ = m.field_moments(pool, 0)
        assert _same_bits(out["logit_mean"][q], mean) and _same_bits(out["logit_var"][q], var), q


@pytest.mark.parametrize("strategy,reset", [("variance", False), ("top", True)])
def test_equal_contexts_tie_and_the_lower_pool_row_is_asked_first(strategy, reset):
    """One respondent, 300 pool rows: 150 distinct contexts, every context twice, the second copy at least a wave away
    (other threads, other waves, the second trip of the scoring loop).  Two rows of one context have the same operand,
    hence the same score in every round: the lower position of each pair is asked before the higher."""
    m = _model(A3, 16, "reg", "abs", seed=11)
    pool, y_pool, _, _ = _problem(m, 0, 1, [150], [0], seed=5)
    perm = torch.randperm(150, generator=torch.Generator().manual_seed(2)).to(DEV)
    pool2, y2 = torch.cat([pool, pool[perm]]), torch.cat([y_pool, y_pool[perm] + 0.5])
    Q = 40
    out = m.elicit_field_exact(pool2, y2, Q, 0, strategy, reset=reset)
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


def test_guards_an_invalid_context_a_respondent_outside_the_table_and_no_rounds():
    """A context id >= T and a negative one, planted through the torch op past the Python checks: NaN moments in every
    round, never asked, the respondent's other rows asked as if the bad rows were not there.  A respondent id >= T asks
    nothing.  Q = 0 returns empty results and, with return_moments, the one scoring pass."""
    from vae_amd import _lib, elicit
    m = _model(A3, 16, "reg", "softplus", seed=13)
    pool, y_pool, _, _ = _problem(m, 0, 3, [6, 4], [0], seed=6)
    Q = 8
    good = m.elicit_field_exact(pool, y_pool, Q, 0, "variance", return_theta=True)
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
    ws = torch.empty(o.elicit_solve_workspace_bytes(U, P, op_x.shape[0], d, -1), dtype=torch.uint8, device=DEV)
    ent, bia, scal = m._views(m._flat)
    before = m._flat.clone()
    o.elicit_solve(ents, ptr, px, ys, None, None, None, op_x.contiguous(), inv.reshape(-1).contiguous(), None, ent, bia,
                   scal, ws, out_row, score, loss, theta, mean, var, 0, 1, Q, 1, 16, 0, 1, -1, 1.0, 0)
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
    z = m.elicit_field_exact(pool, y_pool, 0, 0, "variance", return_moments=True, return_theta=True, write=True)
    assert z["rows"].shape == (3, 0) and z["loss"].shape == (3, 0) and z["theta"].shape == (3, 0, 2 * d + 2)
    m0, v0, _ = m.field_moments(pool, 0)
    assert _same_bits(z["logit_mean"][0], m0) and _same_bits(z["logit_var"][0], v0)
    assert torch.equal(m._flat, before)                      # (write with no round: the rows written are the rows read)


@pytest.mark.parametrize("name", RX.PLANTED)
def test_against_the_fp64_restatement(name):
    """RF.planted_case's closed-form generators, 8 respondents with 12-row pools, 6 rounds.  The gap between the best
    and second-best score exceeds RX.GAP_FLOOR in every round and an fp32 run asks the same rows
    (test_elicit_exact_cpu.py), so the asked sequences must be identical for all respondents.  Thetas and losses at
    test_gpu_foldin_exact.py's bounds."""
    from vae_amd.model import VFM
    _, _, kind, strategy, reset, n_hist, d, field, _ = RF.PLANTED[name]
    c = RF.planted_case(name)
    torch.manual_seed(0)
    m = VFM(field_sizes=list(RF.PLANTED_SIZES), embedding_size=d, output="reg", link=kind, device=DEV)
    m.entity_params.weight.data.copy_(torch.tensor(c["ent"]))
    m.bias_params.weight.data.copy_(torch.tensor(c["bia"]))
    m._flat[m._off_scal: m._off_scal + 3] = torch.tensor(c["scal"], device=DEV)
    Q = RX.PLANTED_ROUNDS
    hist = (torch.tensor(c["hist_x"], device=DEV), torch.tensor(c["hist_y"], device=DEV)) if n_hist else None
    out = m.elicit_field_exact(torch.tensor(c["pool"], device=DEV), torch.tensor(c["y_pool"], device=DEV), Q, field,
                               strategy, history=hist, reset=reset, return_theta=True)
    ref = RX.planted_sessions(name, c)
    rows, theta, loss = out["rows"].cpu().numpy(), out["theta"].cpu().double(), out["loss"].cpu().numpy()
    assert out["entities"].tolist() == [s["entity"] for s in ref]
    gap = min(min(s["gap"]) for s in ref)
    cond = max(max(s["cond"]) for s in ref)
    assert gap > RX.GAP_FLOOR and cond <= 1e3                # (the conditions on the inputs)
    E, B, S = (torch.tensor(c[k]).double() for k in ("ent", "bia", "scal"))
    worst, worst_loss = 0.0, 0.0
    for u, s in enumerate(ref):
        assert rows[u].tolist() == [int(s["sel"][r]) for r in s["rows"]], u       # the same rows asked, no exception
        for q in range(Q):
            t = s["theta"][q]
            th = theta[u, q].numpy()
            for a, b in ((th[:d], t[0]), (th[d:2 * d], t[1]), (th[2 * d:], np.array(t[2:]))):
                worst = max(worst, rel_err(a, b))
            L = objective_fp64(E, B, S, torch.tensor(s["fold_x"][q]), torch.tensor(s["fold_y"][q]), field,
                               (torch.tensor([s["entity"]]), theta[u, q, :d][None], theta[u, q, d:2 * d][None],
                                theta[u, q, 2 * d][None], theta[u, q, 2 * d + 1][None]), kind, "reg", "closed_form")
            worst_loss = max(worst_loss, abs(float(loss[u, q]) - float(L)) / abs(float(L)))
    print(f"{name}: smallest relative gap {gap:.3e}, cond {cond:.1f}; worst theta rel_err {worst:.3e}; worst loss "
          f"relative error {worst_loss:.3e}")
    assert worst <= 1e-4 and worst_loss <= 1e-5


def test_curve_returns_finite_metrics_and_counts_the_rows_left():
    from vae_amd import elicit
    m = _model(A3, 16, "reg", "abs", seed=12)
    pool, y_pool, _, _ = _problem(m, 0, 12, [9, 15, 2], [0], seed=3, distinct_col=1)
    Q = 4
    start = m._flat.clone()
    c = m.elicitation_curve_field_exact(pool, y_pool, Q, 0, strategies=("random", "variance", "top"), seed=5)
    assert torch.equal(m._flat, start)
    sizes = torch.unique(pool[:, 0], return_counts=True)[1]
    for s in ("random", "variance", "top"):
        assert len(c[s]) == Q + 1 and all(np.isfinite(v) and v >= 0.0 for v in c[s])
        left = c["n_unasked"][s]
        assert left[0] == pool.shape[0]
        for q in range(Q):                                   # one row fewer per respondent that still had one
            assert left[q] - left[q + 1] == int((sizes > q).sum()), (s, q)
    r = m.elicit_field_exact(pool, y_pool, Q, 0, "random", seed=5, return_moments=True)
    keep = elicit.asked_round(r["rows"], pool.shape[0]) >= 2
    assert c["random"][2] == elicit.metric("reg", r["logit_mean"][2][keep], r["logit_var"][2][keep], y_pool[keep])

"""GPU: elicitation sessions in the field form (include/vfm_elicit.h: vfm_elicit_field_f32) -- bitwise against the
composition of select_next_questions_field and fold_in it replaces (both objectives, both links, every strategy, one d
per lane-group shape, F = 3 with field 0, F = 4 with a middle field, F = 2, a non-default key_field, history, reset,
exhausted pools, a respondent past the LDS stage), write=False leaves the model alone, independence of the other
respondents and of the pool's order, the per-round moments against field_moments, the stage size, ties, an invalid
context through the raw op, the fp64 restatement on planted models, and the curve."""
import numpy as np
import pytest
import torch

import elicit_field_restatement as RF
from golden_util import rel_err
from test_gpu_elicit import _same_bits, _set_prior, _theta_rows
from test_gpu_foldin import _model

pytestmark = pytest.mark.gpu
DEV = "cuda"
A3, B4, C2 = (40, 90, 4), (6, 40, 90, 3), (40, 90)


def _problem(m, field, n_resp, pool_sizes, hist_sizes, seed, distinct_col=None):
    """A shuffled pool [P, F] with the given rows per respondent (entities of column `field`; distinct contexts per
    respondent over pool and history together), answers, and a history.  distinct_col: a context column whose ids are
    distinct within a respondent ("random" is keyed on one column: rows that share its id tie, and a tie goes by pool
    position)."""
    g = torch.Generator().manual_seed(seed)
    sizes = list(m.field_sizes)
    lo = [sum(sizes[:f]) for f in range(len(sizes))]
    cols = [f for f in range(len(sizes)) if f != field]
    n_ctx = int(np.prod([sizes[f] for f in cols]))
    resp = lo[field] + torch.randperm(sizes[field], generator=g)[:n_resp]
    pool, hist = [], []
    for i, e in enumerate(resp.tolist()):
        n, h = pool_sizes[i % len(pool_sizes)], hist_sizes[i % len(hist_sizes)]
        pick = torch.randperm(n_ctx, generator=g)[:n + h]
        rows = torch.zeros(n + h, len(sizes), dtype=torch.int64)
        rows[:, field] = e
        for f in reversed(cols):                             # mixed radix: a distinct number is a distinct context
            rows[:, f] = lo[f] + pick % sizes[f]
            pick = pick // sizes[f]
        if distinct_col is not None:
            rows[:, distinct_col] = lo[distinct_col] + torch.randperm(sizes[distinct_col], generator=g)[:n + h]
        pool.append(rows[:n])
        hist.append(rows[n:])
    pool, hist = torch.cat(pool), torch.cat(hist)
    pool = pool[torch.randperm(pool.shape[0], generator=g)]
    hist = hist[torch.randperm(hist.shape[0], generator=g)]
    ans = (lambda n: torch.randn(n, generator=g) + 1.0) if m.output == "reg" else \
        (lambda n: (torch.rand(n, generator=g) < 0.5).float())
    return pool.to(DEV), ans(pool.shape[0]).to(DEV), hist.to(DEV), ans(hist.shape[0]).to(DEV)


def _composed(m, pool, y_pool, Q, field, strategy, hist, n_steps, lr, objective, S, seed, klw, reset, key_field=None):
    """The loop the session replaces, on the public pieces (modifies m): per round select_next_questions_field with
    seed + q on the rows still unasked, then foldin.run of the answering respondents on their history followed by
    everything they were asked so far, with t0 = q (n_steps + 1).  Returns entities, rows, score, loss [U, Q],
    theta [U, Q, 2d + 2]."""
    from vae_amd import foldin
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
            got, ls, _, _ = foldin.run(m, X, y, field, objective, S, seed, klw, foldin.MODE_FIT, n_steps, lr,
                                       t0=q * (n_steps + 1))
            assert torch.equal(got, es)
            loss[epos, q] = ls
        theta[:, q] = _theta_rows(m, ents)
    return ents, rows, score, loss, theta


def _same(a, b):
    return _same_bits(a, b) if a.dtype == torch.float32 else torch.equal(a, b)


# one d per (W, CPL) shape that shape_of picks up to d = 512 (the table of test_gpu_elicit_shapes.py): 5 (8, 1), 16 (16, 1),
# 17 (32, 1), 33 (64, 1), 65 (64, 2), 129 (64, 4), 300 (64, 8); every shape with both objectives
CASES = [  # field sizes, field, output, objective, link, strategy, d, history, reset, n_samples, key_field
    (A3, 0, "reg", "closed_form", "abs", "variance", 5, True, False, 1, None),
    (B4, 1, "reg", "closed_form", "softplus", "top", 16, False, True, 1, None),
    (A3, 0, "reg", "closed_form", "abs", "random", 17, True, False, 1, 2),
    (B4, 1, "reg", "closed_form", "softplus", "variance", 33, True, True, 1, None),
    (A3, 0, "reg", "closed_form", "abs", "top", 65, True, False, 1, None),
    (B4, 1, "reg", "closed_form", "softplus", "variance", 129, True, False, 1, None),
    (A3, 0, "reg", "closed_form", "abs", "variance", 300, True, True, 1, None),
    (A3, 0, "class", "sampled", "softplus", "mean", 5, True, True, 1, None),
    (B4, 1, "class", "sampled", "abs", "variance", 16, False, False, 2, None),
    (B4, 1, "class", "sampled", "abs", "random", 17, True, False, 1, 3),
    (A3, 0, "class", "sampled", "softplus", "top", 33, False, True, 1, None),
    (A3, 0, "reg", "sampled", "softplus", "variance", 65, False, False, 3, None),
    (B4, 1, "class", "sampled", "abs", "mean", 129, True, False, 1, None),
    (A3, 0, "class", "sampled", "softplus", "random", 300, True, True, 2, None),
    (C2, 0, "reg", "closed_form", "abs", "variance", 16, True, False, 1, None),
    (C2, 0, "class", "sampled", "softplus", "mean", 128, False, False, 1, None),
    # d = 9 and 129: the smallest d of shapes (16, 1) and (64, 4), neither a multiple of W (lanes past d), at F = 3
    # (appended, so that the ids of the cases above keep their index)
    (A3, 0, "reg", "closed_form", "abs", "variance", 9, True, False, 1, None),
    (A3, 0, "class", "sampled", "softplus", "mean", 9, True, True, 2, None),
    (A3, 0, "reg", "closed_form", "abs", "top", 129, True, False, 1, None),
    (A3, 0, "class", "sampled", "softplus", "variance", 129, True, False, 2, None),
]


@pytest.mark.parametrize("sizes,field,output,objective,link,strategy,d,with_hist,reset,S,key_field", CASES)
def test_bitwise_against_the_composition(sizes, field, output, objective, link, strategy, d, with_hist, reset, S, key_field):
    Q, n_steps = 6, 9
    m = _model(sizes, d, output, link, seed=d + len(strategy), rng_seed=3)
    # pools of 1 and 3 rows run out before Q; 60 history rows are past the LDS stage at every d (at most 44 rows fit)
    pool, y_pool, hx, hy = _problem(m, field, 11, [3, 9, 17, 30, 1], [60, 0, 4, 11] if with_hist else [0], seed=d)
    hist = (hx, hy) if with_hist else None
    start = m._flat.clone()
    ents, rows, score, loss, theta = _composed(m, pool, y_pool, Q, field, strategy, hist, n_steps, 0.05, objective, S, 21,
                                               0.8, reset, key_field)
    final = m._flat.clone()
    m._flat.copy_(start)
    m.params_changed()
    out = m.elicit_field(pool, y_pool, Q, field, strategy, history=hist, n_steps=n_steps, lr=0.05, objective=objective,
                         n_samples=S, seed=21, kl_weight=0.8, reset=reset, write=True, return_theta=True,
                         key_field=key_field)
    assert ents.numel() == 11 and torch.equal(out["entities"], ents)
    assert torch.equal(out["rows"], rows)
    assert int((rows < 0).sum()) > 0 and int((rows[:, 0] >= 0).sum()) == ents.numel()
    assert _same_bits(out["score"], score)                   # (NaN where nothing was left to ask, in both)
    assert _same_bits(out["loss"], loss)
    assert _same_bits(out["theta"], theta)
    assert torch.equal(m._flat, final)                       # write=True: the composition's table
    assert not torch.equal(final, start)


def test_lds_stage_size_does_not_matter():
    from vae_amd import elicit
    m = _model(A3, 16, "reg", "abs", seed=2)
    pool, y_pool, hx, hy = _problem(m, 0, 7, [12, 5], [7, 0, 50], seed=4)
    kw = dict(history=(hx, hy), n_steps=8, return_theta=True, return_moments=True)
    a = elicit.run_field(m, pool, y_pool, 5, 0, "variance", **kw)
    for cap in (0, 2):
        b = elicit.run_field(m, pool, y_pool, 5, 0, "variance", lds_rows=cap, **kw)
        for k in a:
            assert _same(a[k], b[k]), (cap, k)


@pytest.mark.parametrize("output,objective", [("reg", "closed_form"), ("class", "sampled")])
def test_write_false_leaves_the_model_alone(output, objective):
    m = _model(A3, 16, output, "abs", seed=5)
    pool, y_pool, hx, hy = _problem(m, 0, 9, [10, 4, 25], [3, 0], seed=1)
    before = m._flat.clone()
    kw = dict(history=(hx, hy), n_steps=10, objective=objective, return_theta=True, return_moments=True)
    a = m.elicit_field(pool, y_pool, 5, 0, "variance", **kw)
    assert torch.equal(m._flat, before)
    b = m.elicit_field(pool, y_pool, 5, 0, "variance", **kw)
    assert torch.equal(m._flat, before)
    for k in a:
        assert _same(a[k], b[k]), k
    assert bool(torch.isfinite(a["loss"][a["rows"] >= 0]).all())


@pytest.mark.parametrize("sizes,field,output,objective,strategy", [
    (A3, 0, "reg", "closed_form", "variance"), (B4, 1, "class", "sampled", "mean"), (A3, 0, "class", "sampled", "random")])
def test_independent_of_the_other_respondents_and_of_the_pool_order(sizes, field, output, objective, strategy):
    m = _model(sizes, 16, output, "softplus", seed=6)
    pool, y_pool, hx, hy = _problem(m, field, 10, [14, 6, 2, 33], [5, 0, 45], seed=8,
                                    distinct_col=1 if strategy == "random" else None)      # (1: the default key column)
    kw = dict(history=(hx, hy), n_steps=7, objective=objective, seed=4, return_theta=True)
    Q = 5
    full = m.elicit_field(pool, y_pool, Q, field, strategy, **kw)
    row_of = lambda o, p: torch.where((o["rows"] >= 0)[..., None], p[o["rows"].clamp(min=0)], -1)
    perm = torch.randperm(pool.shape[0], generator=torch.Generator().manual_seed(1)).to(DEV)
    shuf = m.elicit_field(pool[perm], y_pool[perm], Q, field, strategy, **kw)
    assert torch.equal(row_of(full, pool), row_of(shuf, pool[perm]))
    for k in ("score", "loss", "theta"):
        assert _same_bits(full[k], shuf[k]), k
    for i, e in enumerate(full["entities"].tolist()):
        sel = pool[:, field] == e
        hs = hx[:, field] == e
        one = m.elicit_field(pool[sel], y_pool[sel], Q, field, strategy, **dict(kw, history=(hx[hs], hy[hs])))
        assert torch.equal(row_of(one, pool[sel]), row_of(full, pool)[i:i + 1])
        for k in ("score", "loss", "theta"):
            assert _same_bits(one[k], full[k][i:i + 1]), (e, k)


@pytest.mark.parametrize("sizes,field,output,objective,link,d", [(A3, 0, "reg", "closed_form", "abs", 5),
                                                                 (B4, 1, "class", "sampled", "softplus", 128)])
def test_round_moments_are_field_moments_of_that_rounds_posterior(sizes, field, output, objective, link, d):
    m = _model(sizes, d, output, link, seed=9)
    pool, y_pool, _, _ = _problem(m, field, 8, [11, 3, 20], [0], seed=2)
    Q = 4
    out = m.elicit_field(pool, y_pool, Q, field, "variance", n_steps=10, objective=objective, return_theta=True,
                         return_moments=True)
    ents = out["entities"]
    ent, bia, _ = m._views(m._flat)
    for q in range(Q + 1):
        if q > 0:
            ent[ents] = out["theta"][:, q - 1, :2 * d]
            bia[ents] = out["theta"][:, q - 1, 2 * d:]
            m.params_changed()
        mean, var, _ = m.field_moments(pool, field)
        assert _same_bits(out["logit_mean"][q], mean) and _same_bits(out["logit_var"][q], var), q


@pytest.mark.parametrize("strategy,reset", [("variance", False), ("top", True)])
def test_equal_contexts_tie_and_the_lower_pool_row_is_asked_first(strategy, reset):
    """One respondent, 40 pool rows over 20 distinct contexts: every context twice, at positions far apart (other lanes
    of the group, W = 16).  Two rows of one context have the same operand, hence the same score in every round: the
    lower position of each pair is asked before the higher, and with Q = P everything is asked."""
    m = _model(A3, 16, "reg", "abs", seed=11)
    pool, y_pool, _, _ = _problem(m, 0, 1, [20], [0], seed=5)
    perm = torch.randperm(20, generator=torch.Generator().manual_seed(2)).to(DEV)
    pool2, y2 = torch.cat([pool, pool[perm]]), torch.cat([y_pool, y_pool[perm] + 0.5])
    out = m.elicit_field(pool2, y2, 40, 0, strategy, n_steps=5, reset=reset)
    order = out["rows"][0].tolist()
    assert sorted(order) == list(range(40))
    when = {r: q for q, r in enumerate(order)}
    for j in range(20):
        assert when[int(perm.tolist().index(j)) + 20] > when[j], j


def test_an_invalid_context_is_never_asked():
    """A context id >= T and a negative one, planted through the torch op past the Python checks: NaN moments in every
    round, never asked; the respondent's other rows are asked as if the bad rows were not there."""
    from vae_amd import _lib, elicit, foldin
    m = _model(A3, 16, "reg", "softplus", seed=13)
    pool, y_pool, _, _ = _problem(m, 0, 3, [6, 4], [0], seed=6)
    Q = 8
    good = m.elicit_field(pool, y_pool, Q, 0, "variance", n_steps=6, return_theta=True)
    bad = pool[:2].clone()
    bad[0, 1], bad[1, 2] = m.T + 5, -3
    x, y = torch.cat([bad, pool]), torch.cat([y_pool[:2], y_pool])
    order, ents, ptr = elicit.pool_lists(x, 0)
    px, ys = x[order].contiguous(), y[order].contiguous()
    ctx = px.clone()
    ctx[:, 0] = 0
    op_x, inv = torch.unique(ctx, dim=0, return_inverse=True)
    U, P, d = ents.numel(), px.shape[0], m.d
    o = _lib.ops()
    out_row = torch.full((U, Q), -7, dtype=torch.int64, device=DEV)
    score, loss = torch.zeros(U, Q, device=DEV), torch.zeros(U, Q, device=DEV)
    theta = torch.zeros(U, Q, 2 * d + 2, device=DEV)
    mean, var = torch.zeros(Q + 1, P, device=DEV), torch.zeros(Q + 1, P, device=DEV)
    obj = foldin.OBJECTIVES["closed_form"]
    ws = torch.empty(o.elicit_field_workspace_bytes(P, op_x.shape[0], d, obj), dtype=torch.uint8, device=DEV)
    ent, bia, scal = m._views(m._flat)
    o.elicit_field(ents, ptr, px, ys, None, None, None, op_x.contiguous(), inv.reshape(-1).contiguous(), None, ent, bia,
                   scal, ws, out_row, score, loss, theta, mean, var, 0, 1, Q, 1, obj, _lib.LIK_NORMAL, 16, 6, 1, 0, 0, -1,
                   0.05, 1.0, 0, 0)
    rows = elicit.rows_to_caller(out_row, order)
    assert not bool(((rows == 0) | (rows == 1)).any())                  # the planted rows: never asked
    assert torch.equal(torch.where(rows >= 0, rows - 2, rows), good["rows"])
    assert _same_bits(score, good["score"]) and _same_bits(loss, good["loss"]) and _same_bits(theta, good["theta"])
    mean, var = elicit.to_caller_order(mean, order), elicit.to_caller_order(var, order)
    assert bool(torch.isnan(mean[:, :2]).all()) and bool(torch.isnan(var[:, :2]).all())
    assert bool(torch.isfinite(mean[:, 2:]).all())


@pytest.mark.parametrize("name", list(RF.PLANTED))
def test_against_the_fp64_restatement_on_a_planted_model(name):
    """RF.planted_case: a three-field planted model, 8 respondents with 12-row pools, 4 rounds of 20 Adam steps at
    lr = 0.01 (the learning rate and the 1e-4 of test_gpu_elicit.py's restatement test, which bound fp32 rounding).  The
    restatement runs with the kernel's own draws (ops.philox_eps).  Condition on the inputs, asserted on the restatement
    alone: the best and second-best score of every respondent and round differ by more than 1e-3 relative (the closed-form
    cases are checked on the CPU too, test_elicit_field_cpu.py) -- so the asked rows must be the same, no exception.
    theta by rel_err per part and the loss relatively, both within 1e-4."""
    from test_gpu_shape_buckets import _eps_any_d
    from vae_amd.model import VFM
    output, objective, kind, strategy, reset, n_hist, d, field, _ = RF.PLANTED[name]
    c = RF.planted_case(name)
    torch.manual_seed(0)
    m = VFM(field_sizes=list(RF.PLANTED_SIZES), embedding_size=d, output=output, link=kind, device=DEV)
    m.entity_params.weight.data.copy_(torch.tensor(c["ent"]))
    m.bias_params.weight.data.copy_(torch.tensor(c["bia"]))
    m._flat[m._off_scal: m._off_scal + 3] = torch.tensor(c["scal"], device=DEV)
    Q, seed = RF.PLANTED_ROUNDS, 4
    hist = (torch.tensor(c["hist_x"], device=DEV), torch.tensor(c["hist_y"], device=DEV)) if n_hist else None
    out = m.elicit_field(torch.tensor(c["pool"], device=DEV), torch.tensor(c["y_pool"], device=DEV), Q, field, strategy,
                         history=hist, n_steps=RF.PLANTED_STEPS, lr=RF.PLANTED_LR, objective=objective, n_samples=1,
                         seed=seed, reset=reset, return_theta=True)
    draws = {}

    def eps(t):
        if t not in draws:
            ee, eb, eg = _eps_any_d(m, seed, t, 1)[0]
            draws[t] = (ee.numpy(), eb.numpy(), float(eg.reshape(-1)[0]))
        return draws[t]

    ref = RF.planted_sessions(name, c, eps)
    rows, theta, loss = out["rows"].cpu().numpy(), out["theta"].cpu().numpy().astype(np.float64), out["loss"].cpu().numpy()
    assert out["entities"].tolist() == [s["entity"] for s in ref]
    gap = min(min(s["gap"]) for s in ref)
    worst, worst_loss = 0.0, 0.0
    for u, s in enumerate(ref):
        for q in range(Q):
            t = s["theta"][q]
            for a, b in ((theta[u, q, :d], t[0]), (theta[u, q, d:2 * d], t[1]), (theta[u, q, 2 * d:], np.array(t[2:]))):
                worst = max(worst, rel_err(a, b))
            worst_loss = max(worst_loss, abs(float(loss[u, q]) - s["loss"][q]) / abs(s["loss"][q]))
    print(f"{name}: smallest relative gap {gap:.3e}; worst theta rel_err {worst:.3e}; worst loss relative error "
          f"{worst_loss:.3e}")
    assert gap > 1e-3                                        # (the condition on the inputs)
    for u, s in enumerate(ref):
        assert rows[u].tolist() == [int(s["sel"][r]) for r in s["rows"]], u       # the same rows asked, no exception
    assert worst <= 1e-4 and worst_loss <= 1e-4


def test_curve_returns_finite_metrics_and_counts_the_rows_left():
    m = _model(A3, 16, "class", "abs", seed=12)
    pool, y_pool, _, _ = _problem(m, 0, 12, [9, 15, 2], [0], seed=3)
    Q = 4
    start = m._flat.clone()
    c = m.elicitation_curve_field(pool, y_pool, Q, 0, strategies=("random", "variance", "mean"), n_steps=8, seed=5)
    assert torch.equal(m._flat, start)
    sizes = torch.unique(pool[:, 0], return_counts=True)[1]
    for s in ("random", "variance", "mean"):
        assert len(c[s]) == Q + 1 and all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in c[s])
        left = c["n_unasked"][s]
        assert left[0] == pool.shape[0]
        for q in range(Q):                                   # one row fewer per respondent that still had one
            assert left[q] - left[q + 1] == int((sizes > q).sum()), (s, q)
    r = m.elicit_field(pool, y_pool, Q, 0, "random", n_steps=8, seed=5, return_moments=True)
    from vae_amd import elicit
    when = elicit.asked_round(r["rows"], pool.shape[0])
    keep = when >= 2
    assert c["random"][2] == elicit.metric("class", r["logit_mean"][2][keep], r["logit_var"][2][keep], y_pool[keep])


def test_two_field_entry_points_still_refuse_three_fields():
    m = _model(A3, 8, "reg", "abs", seed=1)
    pool, y_pool, _, _ = _problem(m, 0, 2, [3], [0], seed=1)
    with pytest.raises(ValueError, match="two-field"):
        m.select_next_questions(pool)
    with pytest.raises(ValueError, match="two-field"):
        m.elicit(pool, y_pool, 2)

"""GPU: target-aware elicitation (VFM.design_scores_field, select_next_questions_design_field, elicit_field_design;
include/vfm_design.h) on the cases of tests/design_restatement.py (tests/test_design_cpu.py asserts their gaps):
d = 5 (8-lane groups), 20, 128 (two coordinates per lane) and 200 with systems past the LDS cap; both links; pools of 1
row, fewer than 64 and 300 rows; with and without history; targets None, given and empty for one respondent; more
rounds than a pool has rows; 261 respondents at d = 5 with lds_dim = 0 (past the slab grid cap).

Bounds.  Scores against the fp64 restatement: |got - ref| <= 2^-23 |ref| per element -- the kernel does the same fp64
arithmetic in the same order, the bound is the final fp32 rounding (doubled: ref may sit on a rounding boundary).  The
session against the composed loop of the public calls: bitwise.  Realised reduction under |.|: out_score[:, q] against
(sigma_w^2 + sum_k W_k sigma_k^2) recomputed from the returned theta of rounds q - 1 and q, within 4 * 2^-23 of that sum
before the round (the fp32 rounding of two stored scales on each side, a factor 2 of margin).  Softplus: the returned
scales against the restatement's, with solve_reference's metric (elementwise_ok with scale_abs_term)."""
import numpy as np
import pytest
import torch

import design_restatement as DR
import solve_reference as SR
from test_gpu_elicit import _same_bits, _theta_rows
from test_gpu_foldin import _model

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = sorted(DR.CASES)


def _setup(name):
    c, ref = DR.build(name)
    m = _model(c["sizes"], c["d"], "reg", c["link"], seed=1)
    m.entity_params.weight.data.copy_(c["ent"])
    m.bias_params.weight.data.copy_(c["bia"])
    m._flat[m._off_scal: m._off_scal + 3] = c["scal"].to(DEV)
    m.params_changed()
    g = {k: (c[k].to(DEV) if c[k] is not None else None) for k in ("pool", "y_pool", "hist_x", "hist_y", "targets")}
    return c, ref, m, g


def _hist(g):
    return (g["hist_x"], g["hist_y"]) if g["hist_x"].shape[0] else None


def _session(m, c, g, **kw):
    kw.setdefault("lds_dim", c["lds_dim"])
    return m.elicit_field_design(g["pool"], g["y_pool"], c["Q"], c["field"], targets=g["targets"], history=_hist(g),
                                 kl_weight=c["klw"], return_theta=True, **kw)


@pytest.mark.parametrize("name", NAMES)
def test_scores_against_fp64(name):
    c, ref, m, g = _setup(name)
    got = m.design_scores_field(g["pool"], c["field"], targets=g["targets"], history=_hist(g), kl_weight=c["klw"]).cpu()
    assert got.shape == (c["pool"].shape[0],) and got.dtype == torch.float32
    prec, kl = DR.prec_kl(c["scal"], c["link"], c["klw"])
    f, worst = c["field"], 0.0
    for e, r in ref.items():
        pm, hm = c["pool"][:, f] == e, c["hist_x"][:, f] == e
        Mp, Ap = DR.operands(c["ent"], c["bia"], c["scal"], c["pool"][pm].numpy(), f, c["link"])
        Mh, Ah = DR.operands(c["ent"], c["bia"], c["scal"], c["hist_x"][hm].numpy(), f, c["link"])
        want = DR.scores(DR.walk_S(Mh, Ah), r["W"], int(hm.sum()), Mp, Ap, kl, prec)
        err = np.abs(got[pm].double().numpy() - want)
        worst = max(worst, float((err / (SR.EPS32 * np.abs(want))).max()))
        assert (err <= SR.EPS32 * np.abs(want)).all(), (e, worst)
    print(f"{name}: worst |got - ref| / (2^-23 |ref|) = {worst:.3f}")


def _composed(m, c, g):
    """The loop the session replaces, on the public calls (modifies m): per round
    select_next_questions_design_field(n=1) on the rows still unasked with history + asked as the history, then
    fold_in_exact of the answering respondents on those rows.  targets None means the whole pool, asked or not."""
    f, Q, pool, y_pool = c["field"], c["Q"], g["pool"], g["y_pool"]
    ents = torch.unique(pool[:, f])
    U, P = ents.numel(), pool.shape[0]
    tg = pool if g["targets"] is None else g["targets"]
    rows = torch.full((U, Q), -1, dtype=torch.int64, device=DEV)
    score = torch.full((U, Q), float("nan"), device=DEV)
    loss = torch.full((U, Q), float("nan"), device=DEV)
    theta = torch.empty(U, Q, 2 * m.d + 2, device=DEV)
    unasked = torch.ones(P, dtype=torch.bool, device=DEV)
    asked = torch.zeros(0, dtype=torch.int64, device=DEV)
    hx, hy = g["hist_x"], g["hist_y"]
    for q in range(Q):
        idx = torch.nonzero(unasked).reshape(-1)
        if idx.numel():
            sub = pool[idx]
            here = lambda x: torch.isin(x[:, f], sub[:, f])
            hq = torch.cat([hx[here(hx)], pool[asked][here(pool[asked])]])
            kw = dict(targets=tg[here(tg)], history=(hq, torch.zeros(hq.shape[0], device=DEV)), kl_weight=c["klw"])
            es, r = m.select_next_questions_design_field(sub, f, 1, **kw)
            sc = m.design_scores_field(sub, f, **kw)
            assert bool((r[:, 0] >= 0).all())
            epos = torch.searchsorted(ents, es)
            rows[epos, q] = idx[r[:, 0]]
            score[epos, q] = sc[r[:, 0]]
            unasked[idx[r[:, 0]]] = False
            asked = torch.cat([asked, idx[r[:, 0]]])
            ha = torch.isin(hx[:, f], es)
            aa = asked[torch.isin(pool[asked, f], es)]
            o = m.fold_in_exact(torch.cat([hx[ha], pool[aa]]), torch.cat([hy[ha], y_pool[aa]]), field=f,
                                kl_weight=c["klw"])
            assert torch.equal(o["entities"], es)
            loss[epos, q] = o["loss"]
        theta[:, q] = _theta_rows(m, ents)
    return ents, rows, score, loss, theta


@pytest.mark.parametrize("name", NAMES)
def test_session_is_bitwise_the_composition_and_the_restatements_choices(name):
    c, ref, m, g = _setup(name)
    start = m._flat.clone()
    ents, rows, score, loss, theta = _composed(m, c, g)
    final = m._flat.clone()
    m._flat.copy_(start)
    m.params_changed()
    out = _session(m, c, g, write=True)
    assert torch.equal(out["entities"], ents)
    assert torch.equal(out["rows"], rows)
    assert _same_bits(out["score"], score) and _same_bits(out["loss"], loss) and _same_bits(out["theta"], theta)
    assert torch.equal(m._flat, final) and not torch.equal(final, start)
    # the restatement's choices, round by round
    for u, e in enumerate(ents.tolist()):
        r = ref[e]
        want = [int(r["pool_index"][p]) if p >= 0 else -1 for p in r["rows"]]
        assert out["rows"][u].tolist() == want, (e, out["rows"][u].tolist(), want)
        for q, p in enumerate(r["rows"]):
            if p < 0:
                assert torch.isnan(out["score"][u, q]) and torch.isnan(out["loss"][u, q])
            else:
                assert abs(float(out["score"][u, q]) - r["score"][q]) <= SR.EPS32 * abs(r["score"][q])


@pytest.mark.parametrize("name", ["d5_abs", "d20_softplus", "d200_slab"])
def test_independent_of_the_other_respondents_and_of_lds_dim(name):
    c, ref, m, g = _setup(name)
    full = _session(m, c, g)
    keys = ("rows", "score", "loss", "theta")
    for lds_dim in (0, 3):
        o = _session(m, c, g, lds_dim=lds_dim)
        assert all(_same_bits(o[k].float(), full[k].float()) if k != "rows" else torch.equal(o[k], full[k]) for k in keys)
    f = c["field"]
    keep = full["entities"][1::2]
    pm = torch.isin(g["pool"][:, f], keep)
    sub = {"pool": g["pool"][pm], "y_pool": g["y_pool"][pm],
           "hist_x": g["hist_x"][torch.isin(g["hist_x"][:, f], keep)],
           "hist_y": g["hist_y"][torch.isin(g["hist_x"][:, f], keep)],
           "targets": None if g["targets"] is None else g["targets"][torch.isin(g["targets"][:, f], keep)]}
    o = _session(m, c, sub)
    assert torch.equal(o["entities"], keep)
    back = torch.nonzero(pm).reshape(-1)
    assert torch.equal(torch.where(o["rows"] >= 0, back[o["rows"].clamp(min=0)], o["rows"]), full["rows"][1::2])
    for k in ("score", "loss", "theta"):
        assert _same_bits(o[k], full[k][1::2])


@pytest.mark.parametrize("name", ["d5_abs", "d128_abs", "d200_slab"])
def test_realised_reduction_abs(name):
    c, ref, m, g = _setup(name)
    out = _session(m, c, g)
    d, th, sc = c["d"], out["theta"].double().cpu().numpy(), out["score"].double().cpu().numpy()
    worst = 0.0
    for u, e in enumerate(out["entities"].tolist()):
        W = ref[e]["W"]
        obj = lambda t: t[2 * d + 1] ** 2 + float((W * t[d:2 * d] ** 2).sum())
        for q in range(1, c["Q"]):
            if ref[e]["rows"][q] < 0:
                continue
            before, after = obj(th[u, q - 1]), obj(th[u, q])
            err, bound = abs((before - after) - sc[u, q]), 4 * SR.EPS32 * before
            worst = max(worst, err / bound)
            assert err <= bound, (e, q, err, bound)
    print(f"{name}: worst |realised - score| / bound = {worst:.3f}")


@pytest.mark.parametrize("name", ["d20_softplus", "d128_softplus", "d5_past_cap"])
def test_scales_softplus_against_the_restatement(name):
    c, ref, m, g = _setup(name)
    out = _session(m, c, g)
    d, th = c["d"], out["theta"].cpu()
    f = c["field"]
    for u, e in enumerate(out["entities"].tolist()):
        nh = int((c["hist_x"][:, f] == e).sum())
        for q, t in enumerate(ref[e]["theta"]):
            if ref[e]["rows"][q] < 0:
                continue
            want = np.concatenate([t["s"], [t["s_w"]]])
            got = torch.cat([th[u, q, d:2 * d], th[u, q, 2 * d + 1:]])
            ok, worst = SR.elementwise_ok(got, want, SR.scale_abs_term(nh + q + 1, want))
            assert ok, (e, q, worst)


def test_model_bytes_and_params_changed(monkeypatch):
    c, ref, m, g = _setup("d20_softplus")
    start = m._flat.clone()
    calls = []
    real = m.params_changed
    monkeypatch.setattr(m, "params_changed", lambda: calls.append(1) or real())
    out = _session(m, c, g, write=False)
    assert torch.equal(m._flat, start) and not calls
    _session(m, c, g, write=True)
    assert calls == [1]
    ents = out["entities"]
    assert _same_bits(_theta_rows(m, ents), out["theta"][:, -1])
    ent0, bia0, _ = m._views(start)
    ent1, bia1, _ = m._views(m._flat)
    other = torch.ones(m.T, dtype=torch.bool, device=DEV)
    other[ents] = False
    assert torch.equal(ent1[other], ent0[other]) and torch.equal(bia1[other], bia0[other])
    assert torch.equal(m._flat[m._off_scal:], start[m._off_scal:])


def test_existing_exact_sessions_keep_their_bits():
    c, ref, m, g = _setup("d128_abs")
    run = lambda: m.elicit_field_exact(g["pool"], g["y_pool"], 3, c["field"], "variance", history=_hist(g), seed=5,
                                       kl_weight=c["klw"], return_theta=True, return_moments=True)
    a = run()
    d_out = _session(m, c, g, return_moments=True)
    b = run()
    for k in a:
        assert _same_bits(a[k].float(), b[k].float()) if a[k].dtype != torch.int64 else torch.equal(a[k], b[k]), k
    # the moments of the design session are the exact session's: round 0 is scored from the same table rows
    assert _same_bits(d_out["logit_mean"][0], a["logit_mean"][0]) and _same_bits(d_out["logit_var"][0], a["logit_var"][0])


def _raw(m, ents, ptr, px, py, tptr, top, op_x, pool_op, Q, lds_dim=-1):
    """torch.ops.vfm_hip.design_elicit and design_scores on hand-made lists (no history)."""
    from vae_amd import _lib
    o = _lib.ops()
    U, P = ents.numel(), px.shape[0]
    row = torch.full((U, Q), -7, dtype=torch.int64, device=DEV)
    score, loss = torch.zeros(U, Q, device=DEV), torch.zeros(U, Q, device=DEV)
    ps = torch.zeros(P, device=DEV)
    ws = torch.empty(max(o.design_workspace_bytes(U, P, op_x.shape[0], m.d, lds_dim), 1), dtype=torch.uint8, device=DEV)
    m._fresh_params()
    ent, bia, scal = m._views(m._flat)
    o.design_scores(ents, ptr, px, None, None, tptr, top, op_x, pool_op, ent, bia, scal, ws, ps, 0, 0, 1.0)
    o.design_elicit(ents, ptr, px, py, None, None, None, None, tptr, top, op_x, pool_op, ent, bia, scal, ws, row, score,
                    loss, None, None, None, 0, Q, 0, 0, 0, lds_dim, 1.0)
    torch.cuda.synchronize()
    return row, score, loss, ps


def test_guards():
    m = _model((10, 20), 8, "reg", "abs", seed=2)
    start = m._flat.clone()
    T = m.T
    L = lambda v: torch.tensor(v, dtype=torch.int64, device=DEV)
    # respondent 0: fine, but pool row 1 has a partner outside [0, T) and row 2 an operand outside [0, n_ops);
    # respondent 1: an id outside [0, T); respondent 2: a target operand outside the table; respondent 3: pool_ptr
    # out of order (no rows); respondent 4: targets of an invalid context
    ents = L([0, T + 5, 2, 3, 4])
    ptr = L([0, 4, 6, 9, 8, 12])
    px = L([[0, 10], [0, T], [0, 12], [0, 13], [T + 5, 10], [T + 5, 11], [2, 10], [2, 11], [2, 12], [4, 10], [4, 11],
            [4, 12]])
    op_x = L([[0, 10], [0, 11], [0, 12], [0, 13], [0, T], [0, -1]])
    pool_op = L([0, 4, 99, 3, 0, 1, 0, 1, 2, 0, 1, 2])
    tptr = L([0, 2, 3, 5, 7, 9])
    top = L([0, 1, 2, 0, -3, 1, 2, 5, 5])
    py = torch.ones(12, device=DEV)
    row, score, loss, ps = _raw(m, ents, ptr, px, py, tptr, top, op_x, pool_op, 5)
    assert row[0].tolist()[2:] == [-1, -1, -1] and sorted(row[0].tolist()[:2]) == [0, 3]     # NaN is never asked
    assert torch.isnan(ps[[1, 2]]).all() and torch.isfinite(ps[[0, 3]]).all()
    assert torch.isnan(score[0, 2:]).all() and torch.isnan(loss[0, 2:]).all() and torch.isfinite(loss[0, :2]).all()
    for u in (1, 2, 3, 4):                                   # nothing asked at all
        assert row[u].tolist() == [-1] * 5 and torch.isnan(score[u]).all() and torch.isnan(loss[u]).all()
    assert torch.isnan(ps[4:12]).all()
    assert torch.equal(m._flat, start)
    # tgt_ptr out of order: clamped to an empty list, the bias term alone, position decides
    row, score, loss, ps = _raw(m, ents, ptr, px, py, L([2, 0, 3, 5, 7, 9]), top, op_x, pool_op, 5)
    assert row[0].tolist() == [0, 3, -1, -1, -1] and float(ps[0]) == float(ps[3]) > 0
    # U = 0 and P = 0
    e0 = L([])
    row, score, loss, ps = _raw(m, e0, L([0]), px[:0], py[:0], L([0]), top[:0], op_x, pool_op[:0], 2)
    assert row.numel() == 0
    row, score, loss, ps = _raw(m, L([0, 2]), L([0, 0, 0]), px[:0], py[:0], L([0, 1, 2]), L([0, 1]), op_x, pool_op[:0], 2)
    assert row.tolist() == [[-1, -1], [-1, -1]] and torch.isnan(score).all() and torch.isnan(loss).all()
    # the public calls on an empty pool
    out = m.elicit_field_design(px[:0], py[:0], 2, 0)
    assert out["entities"].numel() == 0 and out["rows"].shape == (0, 2)
    assert m.design_scores_field(px[:0], 0).shape == (0,)


@pytest.mark.parametrize("name", ["d5_abs", "d128_softplus", "d20_softplus"])
def test_round_moments_are_field_moments_of_that_rounds_posterior(name):
    """logit_mean[q] / logit_var[q] of the session against field_moments of the whole pool with theta[:, q - 1] put
    into the tables (round 0: the table rows), bitwise: the moments' candidate operands are refreshed every round."""
    c, ref, m, g = _setup(name)
    d, Q = c["d"], c["Q"]
    out = _session(m, c, g, return_moments=True)
    ents = out["entities"]
    ent, bia, _ = m._views(m._flat)
    for q in range(Q + 1):
        if q > 0:
            ent[ents] = out["theta"][:, q - 1, :2 * d]
            bia[ents] = out["theta"][:, q - 1, 2 * d:]
            m.params_changed()
        mean, var, _ = m.field_moments(g["pool"], c["field"])
        assert _same_bits(out["logit_mean"][q], mean) and _same_bits(out["logit_var"][q], var), q


def _nan_eq(a, b):
    return a == b or (a != a and b != b)


def test_curves_with_design():
    """Both curves with "design" against a brute-force loop of the public calls: the composed loop
    (select_next_questions_design_field + fold_in_exact) gives the rows asked and the posterior after every round; per
    round the posteriors go into the tables and field_moments / evaluate_ranking_field_posterior judge them."""
    from vae_amd import elicit
    c, ref, m, g = _setup("d20_softplus")
    f, Q, d = c["field"], c["Q"], c["d"]
    pool, y_pool = g["pool"], g["y_pool"]
    kw = dict(targets=g["targets"], history=_hist(g), kl_weight=c["klw"])
    start = m._flat.clone()
    cv = m.elicitation_curve_field_exact(pool, y_pool, Q, f, strategies=["design", "variance"], seed=3, **kw)
    only = m.elicitation_curve_field_exact(pool, y_pool, Q, f, strategies=["variance"], seed=3, history=_hist(g),
                                           kl_weight=c["klw"])
    assert cv["variance"] == only["variance"]               # (`targets` does not reach the other strategies)
    # held-out rows of the respondents: the context of a ranking query is the respondent alone (F = 2)
    sizes, other = c["sizes"], 1 - f
    lo = [0, sizes[0]]
    gen = torch.Generator().manual_seed(9)
    ents_c = torch.unique(c["pool"][:, f])
    Xt = torch.zeros(40, 2, dtype=torch.int64)
    Xt[:, f] = ents_c[torch.randint(0, ents_c.numel(), (40,), generator=gen)]
    Xt[:, other] = lo[other] + torch.randint(0, sizes[other], (40,), generator=gen)
    yt = torch.full((40,), 5.0)
    rc = m.elicitation_ranking_curve_field(pool, y_pool, Q, f, Xt, yt, other, ks=(5,), strategies=["variance", "design"],
                                           exact=True, seed=3, ineligible="drop", **kw)   # (a test row may have been asked)
    assert len(rc["design"]["ndcg@5"]) == Q + 1 and rc["n_queries"] > 0
    assert torch.equal(m._flat, start)

    # ---- the brute force
    ents, rows, _, _, theta = _composed(m, c, g)
    m._flat.copy_(start)
    m.params_changed()
    when = elicit.asked_round(rows, pool.shape[0])
    qe = torch.unique(Xt[:, f]).to(DEV)                      # the queries: the respondents with held-out rows, ascending
    queries = torch.zeros(qe.numel(), 2, dtype=torch.int64, device=DEV)
    queries[:, f] = qe
    test = (torch.searchsorted(qe, Xt[:, f].to(DEV).contiguous()), Xt[:, other].to(DEV).contiguous())
    ent, bia, _ = m._views(m._flat)
    theta0 = torch.cat([ent[ents], bia[ents]], 1).clone()
    for q in range(Q + 1):
        post = theta0 if q == 0 else theta[:, q - 1]
        ent[ents], bia[ents] = post[:, :2 * d], post[:, 2 * d:]
        m.params_changed()
        mean, var, _ = m.field_moments(pool, f)
        keep = when >= q
        want = elicit.metric("reg", mean[keep], var[keep], y_pool[keep])
        assert cv["design"][q] == want and cv["n_unasked"]["design"][q] == int(keep.sum()), q
        asked = rows[:, :q].reshape(-1)
        seen = torch.cat([g["hist_x"], pool[asked[asked >= 0]]])
        seen = seen[torch.isin(seen[:, f], qe)]
        qx = (torch.searchsorted(qe, seen[:, f].contiguous()), seen[:, other].contiguous())
        means = m.evaluate_ranking_field_posterior(queries, test, yt.to(DEV), post[torch.searchsorted(ents, qe)], f, other,
                                                   ks=(5,), ineligible="drop", query_exclude=qx)
        for key, val in means.items():
            assert _nan_eq(rc["design"][key][q], val), (key, q, rc["design"][key][q], val)
    m._flat.copy_(start)
    m.params_changed()

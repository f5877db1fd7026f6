"""GPU: the implicit field-form elicitation session (VFM.elicit_field_implicit, include/vfm_elicit_implicit.h:
vfm_elicit_implicit_f32) -- bitwise against the composition of select_next_questions_field and fold_in_implicit it
replaces (both links, both fields, the three strategies, history, reset, exhausted pools, d = 1, 8, 9, 33, 128, the LDS
edge 134 / 135 and 257 in the slab), the triangle in LDS against the workspace past the slab grid cap, learnt priors, a
base of several chunks, independence of the other respondents, write=False, ragged pools over more than one wave, ties,
the guards of the ABI, the fp64 restatement on the planted cases of tests/elicit_implicit_restatement.py, and the ranking
curve.

Bounds of the restatement test: those of test_gpu_fit_implicit.py for fold_in_implicit against implicit_solve_fp64 (per
element |got - ref| <= 2^-23 |ref| + 4 (d + 1) 2^-52 cond(H) max|ref| after cond(H) <= 1e3 on the reference's own matrix,
the scales with scale_abs_term over the dense row count; losses 1e-5 relative at the returned parameters): the
arithmetic is the same kernel text (vfm_implicit_body.hpp).

Measured on an MI355X: worst elementwise ratio 0.490 (1 = at the bound), losses within 5.83e-8 relative, the asked
sequences identical in all four planted cases."""
import numpy as np
import pytest
import torch

import elicit_implicit_restatement as EI
import implicit_prior_reference as IPR
import implicit_reference as IR
import solve_reference as R
from test_gpu_elicit import _same_bits, _set_prior, _theta_rows
from test_gpu_elicit_field import _problem
from test_gpu_foldin import _model

pytestmark = pytest.mark.gpu
DEV = "cuda"
C2 = (40, 90)
W0, W1, KLW = 0.125, 1.25, 0.75          # (the C ABI takes the weights and kl_weight as floats)
CHUNK = 2048
NO_SPLIT = 1 << 40                       # split_rows: no respondent takes the chunk form


def _composed(m, pool, y_pool, Q, field, strategy, hist, seed, reset, priors=None, chunk_rows=CHUNK, w0=W0, w1=W1,
              klw=KLW):
    """The loop the session replaces, on the public pieces (modifies m): per round select_next_questions_field with
    seed + q on the rows still unasked, then fold_in_implicit (row-list form) of the answering respondents on their
    history followed by everything they were asked so far.  Returns entities, rows, score, loss [U, Q], theta."""
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
    kw = {} if priors is None else dict(priors=priors)
    for q in range(Q):
        idx = torch.nonzero(unasked).reshape(-1)
        if idx.numel():
            sub = pool[idx]
            es, r = m.select_next_questions_field(sub, field, 1, strategy, seed + q)
            _, _, sc = m.field_moments(sub, field, strategy, seed + q)
            epos = torch.searchsorted(ents, es)
            rows[epos, q] = idx[r[:, 0]]
            score[epos, q] = sc[r[:, 0]]
            unasked[idx[r[:, 0]]] = False
            asked = torch.cat([asked, idx[r[:, 0]]])
            ha = torch.isin(hx[:, field], es)
            aa = asked[torch.isin(pool[asked, field], es)]
            X, y = torch.cat([hx[ha], pool[aa]]), torch.cat([hy[ha], y_pool[aa]])
            o = m.fold_in_implicit(X, y, field, w0=w0, w1=w1, kl_weight=klw, entities=es, split_rows=NO_SPLIT,
                                   chunk_rows=chunk_rows, **kw)
            assert torch.equal(o["entities"], es)
            loss[epos, q] = o["loss"]
        theta[:, q] = _theta_rows(m, ents)
    return ents, rows, score, loss, theta


def _session(m, pool, y_pool, Q, field, strategy, priors=None, **kw):
    kw.setdefault("w0", W0)
    kw.setdefault("w1", W1)
    kw.setdefault("kl_weight", KLW)
    if priors is not None:
        kw["priors"] = priors
    return m.elicit_field_implicit(pool, y_pool, Q, field, strategy=strategy, **kw)


def _against_the_composition(m, pool, y_pool, Q, field, strategy, hist, reset, priors=None, lds_dim=-1, seed=21,
                             chunk_rows=CHUNK):
    start = m._flat.clone()
    ents, rows, score, loss, theta = _composed(m, pool, y_pool, Q, field, strategy, hist, seed, reset, priors, chunk_rows)
    final = m._flat.clone()
    m._flat.copy_(start)
    m.params_changed()
    out = _session(m, pool, y_pool, Q, field, strategy, priors, history=hist, seed=seed, reset=reset, write=True,
                   return_theta=True, lds_dim=lds_dim, chunk_rows=chunk_rows)
    assert torch.equal(out["entities"], ents)
    assert torch.equal(out["rows"], rows)
    assert _same_bits(out["score"], score)                   # (NaN where nothing was left to ask, in both)
    assert _same_bits(out["loss"], loss)
    assert _same_bits(out["theta"], theta)
    assert torch.equal(m._flat, final)                       # write=True: the composition's table
    assert not torch.equal(final, start)
    return out


# 37 respondents; pools of 1 and 3 rows run out before Q; 134: the last (d + 1) x (d + 1) triangle in LDS, 135 and 257:
# the slab
CASES = [  # field, link, strategy, d, history, reset, Q
    (0, "abs", "variance", 1, True, False, 6),
    (0, "softplus", "top", 8, False, True, 6),
    (1, "abs", "random", 9, True, False, 6),
    (1, "softplus", "variance", 33, True, True, 5),
    (0, "abs", "top", 128, True, False, 4),
    (0, "softplus", "random", 128, False, False, 4),
    (1, "abs", "variance", 134, False, True, 3),
    (0, "softplus", "variance", 135, True, False, 3),
    (0, "abs", "top", 257, True, True, 3),
]


@pytest.mark.parametrize("field,link,strategy,d,with_hist,reset,Q", CASES)
def test_bitwise_against_the_composition(field, link, strategy, d, with_hist, reset, Q):
    m = _model(C2, d, "reg", link, seed=d + len(strategy), scale=0.3)
    pool, y_pool, hx, hy = _problem(m, field, 37, [3, 9, 17, 30, 1], [5, 0, 2] if with_hist else [0], seed=d)
    out = _against_the_composition(m, pool, y_pool, Q, field, strategy, (hx, hy) if with_hist else None, reset)
    assert out["entities"].numel() == 37
    assert int((out["rows"] < 0).sum()) > 0 and bool(torch.isfinite(out["loss"][out["rows"] >= 0]).all())
    assert bool(torch.isnan(out["score"][out["rows"] < 0]).all()) and bool(torch.isnan(out["loss"][out["rows"] < 0]).all())


@pytest.mark.parametrize("d", [8, 134])
def test_where_the_triangle_lives_does_not_matter(d):
    """lds_dim -1 (LDS) against 0 (every system in its workgroup's slab), with more respondents than slabs."""
    from vae_amd import _lib
    U = _lib.FOLDIN_SOLVE_SLABS + 44 if d == 8 else 37
    m = _model((320, 50), d, "reg", "abs", seed=5, scale=0.3)
    pool, y_pool, hx, hy = _problem(m, 0, U, [4, 2, 7], [2, 0], seed=9)
    a = _session(m, pool, y_pool, 3, 0, "variance", history=(hx, hy), return_theta=True, lds_dim=-1)
    b = _session(m, pool, y_pool, 3, 0, "variance", history=(hx, hy), return_theta=True, lds_dim=0)
    assert a["entities"].numel() == U
    for k in ("rows", "score", "loss", "theta"):
        assert torch.equal(a[k], b[k]) if a[k].dtype == torch.int64 else _same_bits(a[k], b[k]), k
    assert bool(torch.isfinite(a["theta"]).all())


def _drawn_priors(d, seed):
    from vae_amd import sweep
    g = torch.Generator().manual_seed(seed)
    gp = sweep.GroupPriors(2, d, device=DEV)
    gp.mean.copy_((0.2 * torch.randn(2, d + 1, generator=g)).to(DEV))
    gp.prec.copy_((0.5 + 1.5 * torch.rand(2, d + 1, generator=g)).to(DEV))
    return gp


@pytest.mark.parametrize("field,link,d", [(0, "abs", 9), (1, "softplus", 33), (0, "abs", 135)])
def test_priors_bitwise_against_the_composition(field, link, d):
    m = _model(C2, d, "reg", link, seed=d, scale=0.3)
    pool, y_pool, hx, hy = _problem(m, field, 37, [3, 9, 17], [4, 0], seed=d + 1)
    gp = _drawn_priors(d, d)
    out = _against_the_composition(m, pool, y_pool, 4, field, "variance", (hx, hy), False, priors=gp)
    plain = _session(m, pool, y_pool, 4, field, "variance", history=(hx, hy), seed=21, return_theta=True)
    assert not _same_bits(out["theta"], plain["theta"])      # the prior is felt


@pytest.mark.parametrize("reset", [False, True])
def test_standard_priors_reproduce_the_bits(reset):
    from vae_amd import sweep
    m = _model(C2, 17, "reg", "softplus", seed=3, scale=0.3)
    pool, y_pool, hx, hy = _problem(m, 0, 37, [3, 9, 17], [4, 0], seed=4)
    kw = dict(history=(hx, hy), seed=5, reset=reset, return_theta=True, return_moments=True)
    a = _session(m, pool, y_pool, 4, 0, "top", **kw)
    b = _session(m, pool, y_pool, 4, 0, "top", sweep.GroupPriors(2, 17, device=DEV), **kw)
    for k in ("rows", "score", "loss", "theta", "logit_mean", "logit_var"):
        assert torch.equal(a[k], b[k]) if a[k].dtype == torch.int64 else _same_bits(a[k], b[k]), k


def test_base_of_several_chunks_is_fold_in_implicits():
    """A catalog longer than one chunk_rows (200 items in chunks of 64): the session's base has the bits of
    fold_in_implicit's at that chunk_rows."""
    m = _model((40, 200), 8, "reg", "abs", seed=7, scale=0.3)
    pool, y_pool, hx, hy = _problem(m, 0, 37, [3, 9, 17], [4, 0], seed=8)
    out = _against_the_composition(m, pool, y_pool, 3, 0, "variance", (hx, hy), False, chunk_rows=64)
    assert bool((out["rows"] >= 0).all())


def test_independence_and_write_false():
    m = _model(C2, 33, "reg", "abs", seed=11, scale=0.3)
    pool, y_pool, hx, hy = _problem(m, 0, 37, [3, 9, 17, 30], [4, 0, 2], seed=12)
    start = m._flat.clone()
    kw = dict(history=(hx, hy), seed=3, return_theta=True, return_moments=True)
    full = _session(m, pool, y_pool, 4, 0, "variance", **kw)
    assert torch.equal(m._flat, start)                       # write=False: not a byte of the model moves
    keep = full["entities"][::3]
    sel = torch.nonzero(torch.isin(pool[:, 0], keep)).reshape(-1)
    g = torch.Generator().manual_seed(1)
    # the pool's row order across respondents changes, the order within a respondent stays
    blocks = [sel[pool[sel, 0] == e] for e in keep[torch.randperm(keep.numel(), generator=g)].tolist()]
    sel2 = torch.cat(blocks)
    hs = torch.isin(hx[:, 0], keep)
    part = _session(m, pool[sel2], y_pool[sel2], 4, 0, "variance", history=(hx[hs], hy[hs]), seed=3, return_theta=True)
    assert torch.equal(part["entities"], keep)
    rows_full = full["rows"][::3]
    back = torch.where(part["rows"] >= 0, sel2[part["rows"].clamp(min=0)], part["rows"])
    assert torch.equal(back, rows_full)
    for k in ("score", "loss", "theta"):
        assert _same_bits(part[k], full[k][::3]), k


def test_ragged_pools_over_more_than_one_wave():
    m = _model((8, 300), 8, "reg", "softplus", seed=13, scale=0.3)
    sizes = [1, 63, 64, 65, 259]
    pool, y_pool, _, _ = _problem(m, 0, 5, sizes, [0], seed=14)
    out = _against_the_composition(m, pool, y_pool, 3, 0, "top", None, False)
    n_rows = torch.bincount(pool[:, 0], minlength=8)[out["entities"]]
    assert sorted(n_rows.tolist()) == sizes
    one = int(torch.nonzero(n_rows == 1))
    assert out["rows"][one].tolist()[1:] == [-1, -1] and out["rows"][one, 0] >= 0
    assert bool(torch.isnan(out["score"][one, 1:]).all()) and bool(torch.isnan(out["loss"][one, 1:]).all())
    assert bool((out["rows"][n_rows > 1] >= 0).all())


def test_ties_go_to_the_lower_row():
    m = _model(C2, 9, "reg", "abs", seed=15, scale=0.3)
    ent, bia, _ = m._views(m._flat)
    ent[40:] = ent[40].clone()                               # every item alike: every score of a respondent ties
    bia[40:] = bia[40].clone()
    m.params_changed()
    pool, y_pool, _, _ = _problem(m, 0, 6, [5, 2, 9], [0], seed=16)
    y_pool = torch.ones_like(y_pool)                         # ... and stays tied after every answer
    for strategy in ("variance", "top"):
        out = _session(m, pool, y_pool, 4, 0, strategy)
        for i, e in enumerate(out["entities"].tolist()):
            mine = torch.nonzero(pool[:, 0] == e).reshape(-1).tolist()
            want = (mine + [-1] * 4)[:4]
            assert out["rows"][i].tolist() == want, (strategy, e)


def _raw_call(m, pool, y_pool, hist, Q, lo, n, base_range=None, tamper=None, field=0, strategy=1, seed=0):
    """torch.ops.vfm_hip.elicit_implicit on the lists Python would build, with inputs Python would have refused."""
    from vae_amd import _lib, elicit, sweep
    o = _lib.ops()
    hx, hy = hist if hist is not None else (None, None)
    L = elicit.field_lists(pool, y_pool, hx, hy, field)
    if tamper:
        tamper(L)
    U, P, d = L["ents"].numel(), L["px"].shape[0], m.d
    out_row, score, loss, theta, _, _ = elicit._outputs(DEV, U, Q, P, d, True, False)
    blo, bhi = base_range if base_range is not None else (lo, lo + n)
    base = sweep.implicit_base(m, blo, bhi, CHUNK)
    ws = torch.empty(max(o.elicit_implicit_workspace_bytes(U, P, L["op_x"].shape[0], d, -1), 1), dtype=torch.uint8,
                     device=DEV)
    ent, bia, scal = m._views(m._flat)
    o.elicit_implicit(L["ents"], L["ptr"], L["px"], L["ys"], L["hptr"], L["hxs"], L["hys"], L["op_x"], L["pool_op"],
                      L["hist_op"], ent, bia, scal, ws, out_row, score, loss, theta, None, None, base, field, 1 - field, Q,
                      strategy, 0, 0, 0, -1, KLW, seed, lo, n, W0, W1)
    torch.cuda.synchronize()
    return L, out_row, score, loss, theta


def test_guards_of_the_abi():
    m = _model(C2, 8, "reg", "abs", seed=17, scale=0.3)
    pool, y_pool, hx, hy = _problem(m, 0, 6, [12], [2], seed=18)
    start = m._flat.clone()
    # a base over the items [45, 130) only: pool rows naming the items 40 .. 44 are never candidates
    L, rows, score, loss, theta = _raw_call(m, pool, y_pool, None, 12, 45, 85)
    outside = L["px"][:, 1] < 45
    assert int(outside.sum()) > 0
    asked = rows[rows >= 0]
    assert not bool(outside[asked].any())
    n_in = torch.stack([(~outside[L["ptr"][g]:L["ptr"][g + 1]]).sum() for g in range(6)])
    assert torch.equal((rows >= 0).sum(1), n_in)             # every row inside the range is asked, then -1
    assert bool(torch.isfinite(theta).all())
    # a history row with such a partner: NaN means, factor scales and losses; s_w, a function of the counts, is finite
    bad_h = hx.clone()
    bad_h[0, 1] = 41
    L, rows, score, loss, theta = _raw_call(m, pool, y_pool, (bad_h, hy), 2, 45, 85)
    g = int(torch.searchsorted(L["ents"], bad_h[0, 0]))
    assert rows[g, 0] >= 0 and rows[g, 1] == -1              # asked once from the table row, then nothing scores
    assert bool(torch.isnan(theta[g, 0, :16]).all()) and bool(torch.isnan(theta[g, 0, 16])) and bool(torch.isnan(loss[g, 0]))
    assert bool(torch.isfinite(theta[g, 0, 17]))
    others = torch.arange(6, device=DEV) != g
    assert bool(torch.isfinite(theta[others]).all()) and bool((rows[others] >= 0).all())
    # ... under "random" (code 3), whose score does not read the posterior, it keeps being asked; every fold stays NaN
    L, rows, score, loss, theta = _raw_call(m, pool, y_pool, (bad_h, hy), 3, 45, 85, strategy=3, seed=5)
    inside = int((L["px"][L["ptr"][g]:L["ptr"][g + 1], 1] >= 45).sum())
    assert inside >= 3 and bool((rows[g] >= 0).all()) and bool(torch.isfinite(score[g]).all())
    assert bool(torch.isnan(theta[g, :, :17]).all()) and bool(torch.isnan(loss[g]).all())
    assert bool(torch.isfinite(theta[g, :, 17]).all())
    assert bool(torch.isfinite(theta[others]).all()) and bool((rows[others] >= 0).all())
    # a respondent id outside the table asks nothing

    def outside_table(L):
        L["ents"] = L["ents"].clone()
        L["ents"][5] = m.T + 7
    L, rows, score, loss, theta = _raw_call(m, pool, y_pool, None, 2, 40, 90, tamper=outside_table)
    assert rows[5].tolist() == [-1, -1] and bool(torch.isnan(score[5]).all()) and bool(torch.isnan(loss[5]).all())
    assert bool((rows[:5] >= 0).all())
    # Q = 0: nothing to write
    L, rows, score, loss, theta = _raw_call(m, pool, y_pool, None, 0, 40, 90)
    assert rows.numel() == 0
    assert torch.equal(m._flat, start)


@pytest.fixture(scope="module")
def planted():
    out = {}
    for name in EI.PLANTED:
        case = EI.planted_case(name)
        out[name] = (case, EI.planted_sessions(name, case))
    return out


@pytest.mark.parametrize("name", sorted(EI.PLANTED))
def test_fp64_restatement_on_the_planted_cases(planted, name):
    """The asked sequences are the restatement's; theta and the losses are within test_gpu_fit_implicit.py's bounds of
    the fp64 optimum on the same rows."""
    from vae_amd import sweep
    from vae_amd.model import VFM
    case, ref = planted[name]
    N, M, d, link, field = case["N"], case["M"], case["d"], case["kind"], case["field"]
    m = VFM(field_sizes=[N, M], embedding_size=d, output="reg", link=link, device=DEV)
    m.entity_params.weight.data.copy_(torch.as_tensor(case["ent"]))
    m.bias_params.weight.data.copy_(torch.as_tensor(case["bia"]))
    m._flat[m._off_scal: m._off_scal + 3] = torch.as_tensor(case["scal"]).to(DEV)
    kw = {}
    if case["prior"] is not None:
        gp = sweep.GroupPriors(2, d, device=DEV)
        gp.mean[field].copy_(torch.as_tensor(case["prior"][0]))
        gp.prec[field].copy_(torch.as_tensor(case["prior"][1]))
        kw["priors"] = gp
    hist = (torch.as_tensor(case["hist_x"]).to(DEV), torch.as_tensor(case["hist_y"]).to(DEV)) if case["hist_x"].shape[0] else None
    out = m.elicit_field_implicit(torch.as_tensor(case["pool"]).to(DEV), torch.as_tensor(case["y_pool"]).to(DEV), EI.ROUNDS,
                                  field, w0=EI.W0, w1=EI.W1, strategy=case["strategy"], history=hist, return_theta=True,
                                  **kw)
    ent, bia, scal = (torch.as_tensor(case[k]) for k in ("ent", "bia", "scal"))
    n_dense = M if field == 0 else N
    worst, worst_l = 0.0, 0.0
    for i, s in enumerate(ref):
        assert int(out["entities"][i]) == s["entity"]
        assert out["rows"][i].tolist() == [int(s["sel"][r]) for r in s["rows"]], s["entity"]
        for q in range(EI.ROUNDS):
            assert s["cond"][q] <= 1e3
            mu, sp, mw, sw = s["theta"][q]
            rt, rs = np.concatenate([[mw], mu]), np.concatenate([[sw], sp])
            got = out["theta"][i, q].cpu()
            gt, gs = torch.cat([got[2 * d:2 * d + 1], got[:d]]), torch.cat([got[2 * d + 1:], got[d:2 * d]])
            ok_t, w_t = R.elementwise_ok(gt, rt, R.solve_abs_term(d, s["cond"][q], rt))
            ok_s, w_s = R.elementwise_ok(gs, rs, R.scale_abs_term(2 * n_dense, rs))
            assert ok_t and ok_s, (name, s["entity"], q, w_t, w_s)
            worst = max(worst, w_t, w_s)
            x, y = torch.as_tensor(s["fold_x"][q]), torch.as_tensor(s["fold_y"][q])
            a = (ent, bia, scal, x, y, field, N, M, link, EI.W0, EI.W1, 1.0, s["entity"], gt, IR.link_t(gs, link))
            if case["prior"] is None:
                L = float(IR.entity_loss_fp64(*a))
            else:
                L = float(IPR.entity_loss_fp64_prior(*a, torch.as_tensor(case["prior"][0]), torch.as_tensor(case["prior"][1])))
            err = abs(float(out["loss"][i, q]) - L) / abs(L)
            assert err <= 1e-5, (name, s["entity"], q, float(out["loss"][i, q]), L)
            worst_l = max(worst_l, err)
    print(f"IMPLICIT SESSION {name}: worst ratio {worst:.3f}, loss rel_err {worst_l:.2e}")


def test_ranking_curve(monkeypatch):
    from vae_amd import rank
    m = _model(C2, 8, "reg", "abs", seed=19, scale=0.3)
    pool, y_pool, hx, hy = _problem(m, 0, 12, [9], [3], seed=20)
    g = torch.Generator().manual_seed(2)
    ents = torch.unique(pool[:, 0])
    rows = []
    for e in ents.tolist():                                  # two held-out positives per respondent, never asked about
        used = torch.cat([pool[pool[:, 0] == e, 1], hx[hx[:, 0] == e, 1]]).cpu()
        free = torch.tensor([i for i in range(40, 130) if i not in set(used.tolist())])
        rows += [[e, int(i)] for i in free[torch.randperm(free.numel(), generator=g)[:2]]]
    X_test = torch.tensor(rows, device=DEV)
    y_test = torch.full((24,), 5.0, device=DEV)
    seen = []
    real = rank.rank_heldout_field_posterior

    def spy(model, queries, pos, post, *a, **k):
        seen.append((queries.clone(), post.clone()))
        return real(model, queries, pos, post, *a, **k)

    monkeypatch.setattr(rank, "rank_heldout_field_posterior", spy)
    start = m._flat.clone()
    Q = 4
    c = m.elicitation_ranking_curve_field(pool, y_pool, Q, 0, X_test, y_test, 1, ks=(5, 10), strategies=("variance",),
                                          implicit=True, w0=W0, w1=W1, kl_weight=KLW, history=(hx, hy), seed=3)
    assert torch.equal(m._flat, start)
    assert c["n_queries"] == (Q + 1) * 12 and set(c) == {"variance", "n_queries"}
    for key in ("recall@5", "recall@10", "ndcg@10", "mrr", "auc"):
        assert len(c["variance"][key]) == Q + 1 and all(np.isfinite(v) for v in c["variance"][key]), key
    s = _session(m, pool, y_pool, Q, 0, "variance", history=(hx, hy), seed=3, return_theta=True)
    (queries, post), = seen
    Nc = queries.shape[0] // (Q + 1)
    resp = torch.searchsorted(s["entities"], queries[:, 0].contiguous())
    rnd = torch.arange(Q + 1, device=DEV).repeat_interleave(Nc)
    want = torch.where((rnd == 0)[:, None], _theta_rows(m, s["entities"])[resp], s["theta"][resp, (rnd - 1).clamp(min=0)])
    assert _same_bits(post, want)

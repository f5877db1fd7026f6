"""GPU: the field form of the ranking (VFM.rank_field / VFM.field_moments, include/vfm_rank.h) -- against an fp64 oracle
that uses the general-F closed form per (context, candidate) with a derived fp32 rounding bound, bitwise against
field_moments and across splits / streams / calls, against rank_items on a two-field model, its edge cases, and at the
ML-20M shape against a torch fp32 composition."""
import math

import numpy as np
import pytest
import torch

from test_rank_cpu import closed_form
from test_rank_field_cpu import field_form
from test_gpu_rank import philox_uniform_np

pytestmark = pytest.mark.gpu
DEV = "cuda"
U24 = 2.0 ** -24


def tables(sizes, d, seed, scale):
    """The parameter tables of a test model (CPU draws: the oracle alone can be studied without a GPU)."""
    T = int(sum(sizes))
    g = torch.Generator().manual_seed(seed)
    ent = torch.randn(T, 2 * d, generator=g) * scale
    bia = torch.randn(T, 2, generator=g) * scale
    return ent, bia, torch.tensor([0.7, 0.2, 0.3])


def _model(sizes, d, output="reg", link="abs", seed=0, scale=0.5):
    from vae_amd.model import VFM
    m = VFM(field_sizes=sizes, embedding_size=d, output=output, link=link, device=DEV)
    ent, bia, scal = tables(sizes, d, seed, scale)
    m.entity_params.weight.data.copy_(ent)
    m.bias_params.weight.data.copy_(bia)
    m._flat[m._off_scal: m._off_scal + 3] = scal.to(DEV)
    return m


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def oracle(ent, bia, scal, link, ctx, field, cand, strategy, seed=0, key_field=None):
    """fp64 (score, mean, var, bound_score, bound_mean, bound_var) [Q, C].  The moments: the general-F closed form of
    vfm_rank.h evaluated per (context, candidate) row straight from the tables (no operand decomposition).  The bounds:
    (K + 16) 2^-24 (sum_k |a_k b_k| + |constants|), K = d resp. 3d the unpadded chain lengths -- one rounding per fma
    step, one per stored operand, a few ulps for the fp32 link and squares -- propagated through the score function."""
    ent, bia, scal = (np.asarray(t, np.float64) for t in (ent, bia, scal))
    d = ent.shape[1] // 2
    Q, C = len(ctx), len(cand)
    mean, var = np.empty((Q, C)), np.empty((Q, C))
    for q in range(Q):
        x = np.repeat(ctx[q][None, :], C, 0)
        x[:, field] = cand
        mean[q], var[q] = closed_form(ent, bia, scal, x, link)
    _, _, am, av = field_form(ent, bia, scal, np.delete(ctx, field, 1), cand, link)
    bm, bv = (d + 16) * U24 * am, (3 * d + 16) * U24 * av
    if strategy == "top":
        sc, bs = mean, bm
    elif strategy == "variance":
        sc, bs = var, bv
    elif strategy == "mean":
        g = np.sqrt(1 + math.pi * var / 8)
        sc = -np.abs(mean) / g
        bs = bm / g + np.abs(mean) * (math.pi / 16) / g ** 3 * bv + 4 * U24 * np.abs(sc)
    else:
        kf = key_field if key_field is not None else (1 if field == 0 else 0)
        sc = philox_uniform_np(seed, ctx[:, kf][:, None], np.asarray(cand)[None, :])
        bs = np.zeros_like(sc)
    return sc, mean, var, bs, bm, bv


def undecidable_share(S, B, excluded, k):
    """The share of queries whose oracle gap between places k and k + 1 (eligible candidates) is below twice the bound."""
    n = 0
    for q in range(S.shape[0]):
        el = np.flatnonzero(~excluded[q])
        if len(el) <= k:
            continue
        o = el[np.argsort(-S[q, el], kind="stable")]
        a, b = o[k - 1], o[k]
        n += (S[q, a] - S[q, b]) < 2 * max(B[q, a], B[q, b])
    return n / S.shape[0]


def check_ranking(out, cand, S, Mo, Vo, B, Bm, Bv, excluded, k):
    """As check_ranking of test_gpu_rank.py with per-pair bounds: ids distinct, eligible and in order; scores and moments
    within the bound; every eligible candidate that beats the returned k-th by more than the bounds is returned; padding."""
    items, sc = out["items"].cpu().numpy(), out["score"].cpu().numpy().astype(np.float64)
    lm, lv = out["logit_mean"].cpu().numpy(), out["logit_var"].cpu().numpy()
    cand = np.asarray(cand)
    for q in range(items.shape[0]):
        avail = ~excluded[q]
        n = min(k, int(avail.sum()))
        valid = items[q] >= 0
        assert valid.sum() == n and valid[:n].all(), (q, items[q])
        it = items[q][:n]
        assert len(set(it.tolist())) == n
        j = np.searchsorted(cand, it)
        assert (j < len(cand)).all() and (cand[np.minimum(j, len(cand) - 1)] == it).all()
        assert not excluded[q, j].any()
        assert np.all(np.abs(sc[q][:n] - S[q, j]) <= B[q, j]), (q, sc[q][:n] - S[q, j], B[q, j])
        assert np.all(np.abs(lm[q][:n] - Mo[q, j]) <= Bm[q, j]), (q, lm[q][:n] - Mo[q, j], Bm[q, j])
        assert np.all(np.abs(lv[q][:n] - Vo[q, j]) <= Bv[q, j]), (q, lv[q][:n] - Vo[q, j], Bv[q, j])
        assert np.all(np.diff(sc[q][:n]) <= 0)
        assert np.all((np.diff(sc[q][:n]) < 0) | (np.diff(it) > 0))            # equal scores: id ascending
        if n == k:
            must = cand[avail & (S[q] > sc[q][n - 1] + B[q])]          # (c is not returned => its score <= the k-th's)
            assert set(must.tolist()) <= set(it.tolist()), q
        assert (items[q][n:] == -1).all()
        assert np.all(np.isneginf(sc[q][n:])) and np.isnan(lm[q][n:]).all() and np.isnan(lv[q][n:]).all()


# one configuration for the oracle cases: sizes and parameter scale chosen so that the oracle alone keeps the share of
# undecidable queries (gap at place k below twice the bound) within 5 % -- see undecidable_share, asserted per case
Q_CASE, RANKED, OTHER, KS_CASE = 100, 160, 60, (1, 10)


def _case(F, d, field, seed):
    sizes = [OTHER] * F
    sizes[field] = RANKED
    off = _offsets(sizes)
    rng = np.random.default_rng(seed)
    ctx = (rng.integers(0, np.array(sizes)[None, :], size=(Q_CASE, F)) + off[None, :-1]).astype(np.int64)
    ctx[:, field] = 0
    ctx = np.unique(ctx, axis=0)
    ctx = ctx[rng.permutation(len(ctx))]
    all_c = np.arange(off[field], off[field + 1], dtype=np.int64)
    sub = rng.choice(all_c, RANKED // 2, replace=False)
    rows = []
    for c in ctx:                                            # 15 % of the catalog excluded per context ...
        for i in all_c[rng.random(len(all_c)) < 0.15]:
            r = c.copy()
            r[field] = i
            rows.append(r)
    for c in ctx[:5]:                                        # ... and rows of contexts that differ in one column: no match
        r = c.copy()
        f = (field + 1) % F
        r[f] = off[f] + (r[f] - off[f] + 1) % sizes[f]
        r[field] = all_c[3]
        rows.append(r)
    return sizes, ctx, all_c, sub, np.array(rows, np.int64)


def _excluded(ctx, cand, ex, field, match):
    s = {(tuple(r[list(match)]), int(r[field])) for r in ex} if ex is not None else set()
    return np.array([[(tuple(c[list(match)]), int(i)) in s for i in cand] for c in ctx], bool)


@pytest.mark.parametrize("output", ["reg", "class"])
@pytest.mark.parametrize("link", ["abs", "softplus"])
@pytest.mark.parametrize("d", [5, 20, 128])
@pytest.mark.parametrize("F", [2, 3, 8])
def test_rank_field_matches_fp64_oracle(F, d, link, output):
    strategies = ["top", "variance", "random"] + (["mean"] if output == "class" else [])
    for field in sorted({0, F // 2, F - 1}):
        sizes, ctx, all_c, sub, ex = _case(F, d, field, seed=F * 1000 + d + field)
        m = _model(sizes, d, output=output, link=link, seed=d + F, scale=0.5)
        T = _offsets(sizes)
        match = [f for f in range(F) if f != field]
        ent, bia, scal = tables(sizes, d, d + F, 0.5)
        for strategy in strategies:
            S, Mo, Vo, B, Bm, Bv = oracle(ent, bia, scal, link, ctx, field, all_c, strategy, seed=9)
            for cands in (None, sub):
                cand = all_c if cands is None else np.sort(sub)
                cols = cand - T[field]
                for exclude in (None, ex):
                    excl = _excluded(ctx, cand, exclude, field, match)
                    for k in KS_CASE:
                        share = undecidable_share(S[:, cols], B[:, cols], excl, k)
                        print(f"F={F} d={d} {link} {output} field={field} {strategy} cand={cands is not None} "
                              f"excl={exclude is not None} k={k}: undecidable share {share:.3f}")
                        assert share <= 0.05
                        out = m.rank_field(torch.tensor(ctx), field, k=k, strategy=strategy,
                                           candidates=None if cands is None else torch.tensor(cands),
                                           exclude=None if exclude is None else torch.tensor(exclude), seed=9)
                        check_ranking(out, cand, S[:, cols], Mo[:, cols], Vo[:, cols], B[:, cols], Bm[:, cols],
                                      Bv[:, cols], excl, k)


def test_field_moments_match_the_oracle_and_predictive_moments():
    sizes, d = [70, 90, 5, 11], 20
    m = _model(sizes, d, output="class", link="softplus", seed=4)
    off = _offsets(sizes)
    rng = np.random.default_rng(2)
    x = (rng.integers(0, np.array(sizes)[None, :], size=(500, 4)) + off[None, :-1]).astype(np.int64)
    ent, bia, scal = tables(sizes, d, 4, 0.5)
    rm, rv = closed_form(ent.numpy(), bia.numpy(), scal.numpy(), x, "softplus")
    pm, pv = m.predictive_moments(torch.tensor(x, device=DEV))
    for field in range(4):
        for dt in (torch.int64, torch.int32):
            mean, var, sc = m.field_moments(torch.tensor(x).to(dt), field, strategy="mean")
            _, _, am, av = field_form(ent.numpy(), bia.numpy(), scal.numpy(), np.delete(x, field, 1), x[:, field], "softplus")
            am, av = np.diagonal(am), np.diagonal(av)
            assert np.all(np.abs(mean.cpu().numpy() - rm) <= (d + 16) * U24 * am)
            assert np.all(np.abs(var.cpu().numpy() - rv) <= (3 * d + 16) * U24 * av)
            want = -mean.abs() / torch.sqrt(1.0 + 0.39269908169872414 * var)
            assert torch.allclose(sc, want, rtol=1e-6, atol=0)
        assert torch.allclose(mean, pm, rtol=0, atol=2e-5 * float(pm.abs().max()))
        assert torch.allclose(var, pv, rtol=0, atol=2e-5 * float(pv.abs().max()))


# ---------------------------------------------------------------------------------------------------- bitwise
def _rows_of(ctx, items, field):
    Q, k = items.shape
    x = ctx.to(DEV)[:, None, :].expand(-1, k, -1).clone()
    x[:, :, field] = items
    return x.reshape(Q * k, -1)


# d -> padded depths (KA, KB): 1:(16,16) 17:(32,64) 20:(32,64) 1024:(1024,3072)
@pytest.mark.parametrize("d", [1, 17, 20, 1024])
def test_rank_field_scores_are_the_field_moments_bitwise(d):
    sizes = [60, 300, 4]
    m = _model(sizes, d, output="class", seed=8, scale=0.5 if d < 1024 else 0.2)
    rng = np.random.default_rng(d)
    ctx = torch.tensor(np.stack([rng.integers(0, 60, 50), np.zeros(50, np.int64), 360 + rng.integers(0, 4, 50)], 1))
    for field, c in ((1, ctx), (2, torch.tensor(np.stack([rng.integers(0, 60, 30), 60 + rng.integers(0, 300, 30),
                                                           np.zeros(30, np.int64)], 1)))):
        for strategy in ("top", "variance", "mean", "random"):
            k = 16 if field == 1 else 3
            out = m.rank_field(c, field, k=k, strategy=strategy, seed=5)
            assert (out["items"] >= 0).all()
            mean, var, sc = m.field_moments(_rows_of(c, out["items"], field), field, strategy=strategy, seed=5)
            assert torch.equal(out["logit_mean"].reshape(-1), mean), (field, strategy)
            assert torch.equal(out["logit_var"].reshape(-1), var), (field, strategy)
            assert torch.equal(out["score"].reshape(-1), sc), (field, strategy)
            if strategy == "top":
                assert torch.equal(sc, mean)
            if strategy == "variance":
                assert torch.equal(sc, var)


def test_rank_field_is_bitwise_deterministic_across_calls_splits_and_streams():
    sizes = [400, 5000, 6]
    rng = np.random.default_rng(0)
    for strategy, output in (("top", "reg"), ("variance", "reg"), ("mean", "class"), ("random", "reg")):
        m = _model(sizes, 20, output=output, seed=3)
        ctx = torch.tensor(np.stack([rng.integers(0, 400, 300), np.zeros(300, np.int64), 5400 + rng.integers(0, 6, 300)], 1))
        ex = ctx[rng.integers(0, 300, 6000)].clone()
        ex[:, 1] = torch.tensor(400 + rng.integers(0, 5000, 6000))
        ref = m.rank_field(ctx, 1, k=10, strategy=strategy, exclude=ex, seed=4)
        for n_splits in (0, 1, 3, 64):
            for _ in range(2):
                out = m.rank_field(ctx, 1, k=10, strategy=strategy, exclude=ex, seed=4, n_splits=n_splits)
                for key in ref:
                    assert torch.equal(ref[key], out[key]), (strategy, n_splits, key)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            out = m.rank_field(ctx, 1, k=10, strategy=strategy, exclude=ex, seed=4)
        s.synchronize()
        for key in ref:
            assert torch.equal(ref[key], out[key])
        # k past the register list (k > 16): the same lists' heads
        big = m.rank_field(ctx, 1, k=40, strategy=strategy, exclude=ex, seed=4, n_splits=5)
        assert torch.equal(big["items"][:, :10], ref["items"]) and torch.equal(big["score"][:, :10], ref["score"])


def test_duplicate_contexts_give_identical_rows_and_the_ranked_column_is_ignored():
    m = _model([50, 400, 3], 12, seed=6)
    base = torch.tensor([[3, 0, 451], [7, 0, 450], [3, 0, 452]])
    ref = m.rank_field(base, 1, k=5, strategy="variance")
    ctx = base[[0, 1, 0, 2, 1, 0]].clone()
    ctx[:, 1] = torch.tensor([50, 51, 52, 449, 0, 7])               # any value: ignored
    out = m.rank_field(ctx, 1, k=5, strategy="variance")
    for key in ref:
        assert torch.equal(out[key], ref[key][[0, 1, 0, 2, 1, 0]]), key


# ---------------------------------------------------------------------------------------------------- other cases
@pytest.mark.parametrize("strategy,output", [("top", "reg"), ("variance", "reg"), ("mean", "class")])
def test_two_field_model_agrees_with_rank_items_where_the_gap_is_clear(strategy, output):
    """F = 2, field 1: the same closed form through a different chain, so the item sets agree wherever the oracle's gap at
    place k exceeds the sum of the two kernels' bounds (rank_items' chains are K = d and 2d over the same terms)."""
    N, M, d, k = 300, 2000, 20, 10
    m = _model([N, M], d, output=output, seed=12)
    users = np.arange(0, N, 3, dtype=np.int64)
    ctx = np.stack([users, np.zeros_like(users)], 1)
    ent, bia, scal = tables([N, M], d, 12, 0.5)
    all_c = np.arange(N, N + M, dtype=np.int64)
    S, _, _, B, Bm, Bv = oracle(ent, bia, scal, "abs", ctx, 1, all_c, strategy)
    a = m.rank_field(torch.tensor(ctx), 1, k=k, strategy=strategy)
    b = m.rank_items(torch.tensor(users), k=k, strategy=strategy)
    tol = 2 * B                                                     # (the two-field chains are no longer than these)
    assert (a["score"] - b["score"]).abs().max().item() <= tol.max()
    n_clear = 0
    for q in range(len(users)):
        o = np.argsort(-S[q], kind="stable")
        if S[q, o[k - 1]] - S[q, o[k]] > tol[q, o[k - 1]] + tol[q, o[k]]:
            n_clear += 1
            assert set(a["items"][q].tolist()) == set(b["items"][q].tolist()), q
    assert n_clear >= 0.9 * len(users)
    with pytest.raises(ValueError, match="two-field"):
        _model([20, 30, 4], 4).rank_items([0])


def test_invalid_ids_give_nan_and_are_never_returned():
    from vae_amd import _lib
    sizes, d, k = [30, 100, 3], 8, 4
    m = _model(sizes, d, seed=1)
    ent, bia, scal = m._views(m._flat)
    T = m.T
    ctx = torch.tensor([[2, 0, 131], [T + 5, 0, 130], [4, 0, -1], [5, 0, 132]], device=DEV)
    cand = torch.tensor([-3, 31, 40, 77, T + 9], device=DEV)
    o = _lib.ops()
    for code in (0, 1):
        ws = torch.empty(o.rank_field_workspace_bytes(4, 5, 3, d, k, code, 0), dtype=torch.uint8, device=DEV)
        items = torch.empty(4, k, dtype=torch.int64, device=DEV)
        sc, lm, lv = (torch.empty(4, k, device=DEV) for _ in range(3))
        o.rank_field(ctx, 1, None, cand, 5, 0, None, None, ent, bia, scal, ws, items, sc, lm, lv, k, code, 0, 0, 0)
        assert sorted(items[0, :3].tolist()) == [31, 40, 77] and items[0, 3].item() == -1
        assert sorted(items[3, :3].tolist()) == [31, 40, 77]
        assert (items[1] == -1).all() and (items[2] == -1).all()
        assert torch.isneginf(sc[1]).all() and torch.isnan(lm[2]).all() and torch.isnan(lv[1]).all()
    x = torch.tensor([[2, 31, 131], [T, 31, 131], [2, -1, 131], [2, 31, T + 1]], device=DEV)
    mean, var, s = (torch.empty(4, device=DEV) for _ in range(3))
    o.field_moments(x, 1, None, ent, bia, scal, mean, var, s, 0, 1, 0)
    assert torch.isfinite(mean[0]) and torch.isnan(mean[1:]).all() and torch.isnan(var[1:]).all() and torch.isnan(s[1:]).all()


def test_short_candidate_lists_are_padded():
    m = _model([20, 50, 3], 8, seed=1)
    ctx = torch.tensor([[0, 0, 70], [3, 0, 71]])
    out = m.rank_field(ctx, 1, k=5, candidates=[27, 29], exclude=torch.tensor([[3, 29, 71], [3, 27, 70]]))
    assert out["items"][0, 2:].tolist() == [-1, -1, -1] and out["items"][1].tolist() == [27, -1, -1, -1, -1]
    assert torch.isneginf(out["score"][1, 1:]).all() and torch.isnan(out["logit_mean"][1, 1:]).all()
    assert torch.isnan(out["logit_var"][0, 2:]).all() and not torch.isnan(out["logit_var"][0, :2]).any()
    out = m.rank_field(ctx, 1, k=3, candidates=[])
    assert out["items"].tolist() == [[-1, -1, -1]] * 2
    out = m.rank_field(ctx[:0], 1, k=3)
    assert out["items"].shape == (0, 3)


def test_match_fields_widens_the_exclusion():
    """(0,): anything this user has seen, in any format."""
    m = _model([20, 50, 3], 8, seed=2)
    ctx = torch.tensor([[4, 0, 70], [4, 0, 71], [5, 0, 70]])
    full = m.rank_field(ctx, 1, k=50)
    seen = torch.tensor([[4, int(full["items"][0, 0]), 70], [4, int(full["items"][1, 1]), 72]])
    strict = m.rank_field(ctx, 1, k=50, exclude=seen)
    wide = m.rank_field(ctx, 1, k=50, exclude=seen, match_fields=(0,))
    gone = {int(seen[0, 1]), int(seen[1, 1])}
    assert set(full["items"][0].tolist()) - set(strict["items"][0].tolist()) == {int(seen[0, 1])}
    assert strict["items"][1].tolist() == full["items"][1].tolist()
    for q in (0, 1):
        assert set(full["items"][q].tolist()) - set(wide["items"][q].tolist()) == gone
    assert wide["items"][2].tolist() == full["items"][2].tolist()


def test_random_is_reproducible_in_seed_key_and_id_and_independent_of_the_other_queries():
    m = _model([40, 300, 5], 8, seed=3)
    ctx = torch.tensor([[7, 0, 341], [9, 0, 342], [7, 0, 343], [11, 0, 341]])
    a = m.rank_field(ctx, 1, k=6, strategy="random", seed=21)
    b = m.rank_field(ctx[[3, 0]], 1, k=6, strategy="random", seed=21)
    assert torch.equal(b["items"], a["items"][[3, 0]]) and torch.equal(b["score"], a["score"][[3, 0]])
    assert torch.equal(a["items"][0], a["items"][2])                   # keyed on column 0 (the lowest context column)
    c = m.rank_field(ctx, 1, k=6, strategy="random", seed=21, key_field=2)
    assert torch.equal(c["items"][0], c["items"][3]) and not torch.equal(c["items"][0], c["items"][2])
    assert not torch.equal(m.rank_field(ctx, 1, k=6, strategy="random", seed=22)["items"], a["items"])
    want = philox_uniform_np(21, ctx[:, 0].numpy()[:, None], a["items"].cpu().numpy())
    assert np.array_equal(a["score"].cpu().numpy().astype(np.float64), want)
    full = philox_uniform_np(21, np.array([[7]]), np.arange(40, 340)[None, :])[0]
    assert a["items"][0].tolist() == (40 + np.argsort(-full, kind="stable")[:6]).tolist()


def test_rank_field_after_lazy_fit_equals_rank_field_after_sync():
    from vae_amd.model import VFM
    from vae_amd.data import synthetic_triples

    def trained():
        torch.manual_seed(3)
        m = VFM(field_sizes=[300, 500, 4], embedding_size=16, device=DEV, rng_seed=11)
        m.lazy_adam, m.pipeline = True, False
        X, y = synthetic_triples([300, 500, 4], 12 * 48, seed=4, device=DEV)
        m.set_training_data(X, nb_train=X.shape[0])
        plans = [m.plan(X[i * 48:(i + 1) * 48], y[i * 48:(i + 1) * 48]) for i in range(12)]
        for s in range(40):
            m.train_step(plans[s % 12], lr=0.05)
        return m, X
    a, X = trained()
    b, _ = trained()
    assert a._lazy_dirty and b._lazy_dirty                             # rows are lagging
    b.sync_lazy()
    ctx = X[::5].clone()
    for strategy in ("top", "variance"):
        ra = a.rank_field(ctx, 1, k=10, strategy=strategy, exclude=X)
        rb = b.rank_field(ctx, 1, k=10, strategy=strategy, exclude=X)
        for key in ra:
            assert torch.equal(ra[key], rb[key])
    assert not a._lazy_dirty and torch.equal(a._flat, b._flat)


# ---------------------------------------------------------------------------------------------------- large shape
@pytest.mark.parametrize("strategy", ["top", "variance"])
def test_ml20m_shape_three_fields_matches_torch_composition(strategy):
    """Q = 4,096 contexts x 26,744 items, F = 3, d = 128 against a torch fp32 composition (query operands in torch, mm,
    masking, topk).  The tolerance is relative to the largest score: the composition's own mm does not share the
    kernel's summation order, so the per-pair bound does not apply to it."""
    N, M, Fm, d, Q, k = 138_493, 26_744, 4, 128, 4096, 10
    m = _model([N, M, Fm], d, seed=20, scale=0.3)
    g = torch.Generator(device=DEV).manual_seed(1)
    users = torch.randperm(N, device=DEV, generator=g)[:Q].sort().values
    fmt = N + M + torch.randint(0, Fm, (Q,), device=DEV, generator=g)
    ctx = torch.stack([users, torch.zeros_like(users), fmt], 1)
    ex_items = N + torch.randint(0, M, (Q, 100), device=DEV, generator=g)
    ex = torch.stack([users[:, None].expand(-1, 100).reshape(-1), ex_items.reshape(-1),
                      fmt[:, None].expand(-1, 100).reshape(-1)], 1)
    out = m.rank_field(ctx, 1, k=k, strategy=strategy, exclude=ex)
    ent, bia, scal = m._views(m._flat)
    mu, s2 = ent[:, :d], ent[:, d:].abs() ** 2
    mu_u, mu_f, s_u, s_f = mu[users], mu[fmt], s2[users], s2[fmt]
    Mq, Aq = mu_u + mu_f, s_u + s_f
    if strategy == "top":
        c = scal[1] + bia[users, 0] + bia[fmt, 0] + (mu_u * mu_f).sum(1)
        S = Mq @ mu[N:N + M].T + c[:, None] + bia[N:N + M, 0][None, :]
    else:
        Cq = 2 * (s_u * mu_f + s_f * mu_u)
        c = scal[2] ** 2 + bia[users, 1] ** 2 + bia[fmt, 1] ** 2 + (s_u * s_f + s_u * mu_f ** 2 + s_f * mu_u ** 2).sum(1)
        S = (Aq @ (mu[N:N + M] ** 2).T + (Aq + Mq ** 2) @ s2[N:N + M].T + Cq @ mu[N:N + M].T + c[:, None]
             + (bia[N:N + M, 1] ** 2)[None, :])
    S[torch.arange(Q, device=DEV)[:, None].expand(-1, 100), ex_items - N] = -float("inf")
    tv, ti = torch.topk(S, k, dim=1)
    tol = 2e-5 * float(S[torch.isfinite(S)].abs().max())
    got = out["score"]
    gathered = S.gather(1, out["items"] - N)
    assert torch.isfinite(gathered).all()
    assert (gathered - got).abs().max().item() <= tol
    assert ((tv - got).abs().max().item()) <= tol
    kth = got[:, -1:]
    clear = (tv > kth + tol)
    hit = (ti[:, :, None] + N == out["items"][:, None, :]).any(2)
    assert bool((hit | ~clear).all())

"""GPU: held-out ranking evaluation in the field form (VFM.rank_heldout_field / VFM.evaluate_ranking_field,
include/vfm_rank.h: vfm_rank_heldout_field_f32) -- exact ranks against an oracle that scores every (context, candidate)
row with field_moments and orders them with a stable sort, rank intervals from the fp64 oracle, agreement with rank_field,
shape edges, heavy and degenerate queries, independence of the other queries, match_fields, lazy training state, and the
metrics against brute force and sklearn."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_rank_field import _case, _excluded, _model, _offsets, oracle, tables

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEYS = ("contexts", "ptr", "items", "query_index", "rank", "rank_neg", "n_eligible", "n_neg")


# ---------------------------------------------------------------------------------------------------- helpers
def scores_of(m, ctx, field, cand, strategy, seed=0, key_field=None):
    """[Q, C] fp32 scores of every (context, candidate) row: field_moments (bitwise the ranking's scores)."""
    c = torch.as_tensor(np.asarray(cand), device=DEV)
    x = torch.as_tensor(np.asarray(ctx), device=DEV)[:, None, :].expand(-1, c.numel(), -1).clone()
    x[:, :, field] = c[None, :]
    _, _, sc = m.field_moments(x.reshape(-1, x.shape[2]), field, strategy=strategy, seed=seed, key_field=key_field)
    return sc.reshape(len(ctx), c.numel()).cpu().numpy()


def exact_ranks(S, excl, pos):
    """S [Q, C] scores over ascending candidate ids, excl, pos [Q, C] bool.  Per query and its positives (ascending):
    rank, rank_neg; per query n_eligible, n_neg.  The order: a stable descending sort of the eligible candidates."""
    rank, rank_neg, n_el, n_neg = [], [], [], []
    for q in range(S.shape[0]):
        el = np.flatnonzero(~excl[q])
        order = torch.sort(torch.from_numpy(S[q, el]), descending=True, stable=True).indices.numpy()
        where = np.empty(len(el), np.int64)
        where[order] = np.arange(len(el))
        is_pos = pos[q, el]
        assert not (pos[q] & excl[q]).any()
        w = where[is_pos]                                            # (ascending ids)
        wp = np.sort(w)
        rank += w.tolist()
        rank_neg += (w - np.searchsorted(wp, w)).tolist()            # minus the positives ahead of it
        n_el.append(len(el))
        n_neg.append(len(el) - int(is_pos.sum()))
    return [np.array(a, np.int64) for a in (rank, rank_neg, n_el, n_neg)]


def rows_of(ctx, pos, cand, field, rng, n_dup=3):
    """The full rows [P, F] of the positives pos [Q, C] bool, shuffled, with a few duplicates."""
    q, j = np.nonzero(pos)
    rows = ctx[q].copy()
    rows[:, field] = np.asarray(cand)[j]
    rows = np.concatenate([rows, rows[:n_dup]])
    return rows[rng.permutation(len(rows))]


def draw_positives(excl, rng, mean=6.0):
    """pos [Q, C] bool: a geometric number of positives (at least one) per query among its eligible candidates."""
    pos = np.zeros_like(excl)
    for q in range(excl.shape[0]):
        el = np.flatnonzero(~excl[q])
        n = min(len(el), int(rng.geometric(1.0 / mean)))
        pos[q, rng.choice(el, n, replace=False)] = True
    return pos


def check_exact(r, S, excl, pos, ctx_sorted):
    assert torch.equal(r["contexts"].cpu(), torch.as_tensor(ctx_sorted))
    rank, rank_neg, n_el, n_neg = exact_ranks(S, excl, pos)
    np.testing.assert_array_equal(r["rank"].cpu().numpy(), rank)
    np.testing.assert_array_equal(r["rank_neg"].cpu().numpy(), rank_neg)
    np.testing.assert_array_equal(r["n_eligible"].cpu().numpy(), n_el)
    np.testing.assert_array_equal(r["n_neg"].cpu().numpy(), n_neg)
    np.testing.assert_array_equal(r["ptr"].cpu().numpy(), np.concatenate([[0], np.cumsum(pos.sum(1))]))
    assert r["rank"].dtype == r["rank_neg"].dtype == r["n_eligible"].dtype == r["n_neg"].dtype == torch.int64


@functools.lru_cache(maxsize=None)
def case(F, d, field):
    """_case of test_gpu_rank_field.py with the contexts in sorted row order (the order of the returned queries), and per
    (candidate list, exclusions) variant: the candidate ids, the excluded mask, the positives and their rows."""
    sizes, ctx, all_c, sub, ex = _case(F, d, field, seed=F * 1000 + d + field)
    ctx = np.unique(ctx, axis=0)
    match = [f for f in range(F) if f != field]
    rng = np.random.default_rng(F * 100 + d + field)
    variants = []
    for cands in (None, sub):
        cand = all_c if cands is None else np.sort(sub)
        for exclude in (None, ex):
            excl = _excluded(ctx, cand, exclude, field, match)
            pos = draw_positives(excl, rng)
            variants.append((cands, cand, exclude, excl, pos, rows_of(ctx, pos, cand, field, rng)))
    return sizes, ctx, all_c, variants


def strategies_of(output, with_random=True):
    return ["top", "variance"] + (["random"] if with_random else []) + (["mean"] if output == "class" else [])


def call(m, rows, field, cands, exclude, **kw):
    return m.rank_heldout_field(torch.tensor(rows), field, candidates=None if cands is None else torch.tensor(cands),
                                exclude=None if exclude is None else torch.tensor(exclude), **kw)


# ---------------------------------------------------------------------------------------------------- 1. exact ranks
@pytest.mark.parametrize("output", ["reg", "class"])
@pytest.mark.parametrize("link", ["abs", "softplus"])
@pytest.mark.parametrize("d", [5, 20, 128])
@pytest.mark.parametrize("F", [2, 3, 8])
def test_ranks_match_the_bitwise_oracle(F, d, link, output):
    for field in sorted({0, F // 2, F - 1}):
        sizes, ctx, all_c, variants = case(F, d, field)
        m = _model(sizes, d, output=output, link=link, seed=d + F, scale=0.5)
        off = _offsets(sizes)
        for strategy in strategies_of(output):
            S = scores_of(m, ctx, field, all_c, strategy, seed=9)
            for cands, cand, exclude, excl, pos, rows in variants:
                r = call(m, rows, field, cands, exclude, strategy=strategy, seed=9)
                check_exact(r, S[:, cand - off[field]], excl, pos, ctx)
                assert r["n_dropped"] == 0 and r["items"].numel() == int(pos.sum())


# ---------------------------------------------------------------------------------------------------- 2. fp64 oracle
@pytest.mark.parametrize("output", ["reg", "class"])
@pytest.mark.parametrize("link", ["abs", "softplus"])
@pytest.mark.parametrize("d", [5, 20, 128])
@pytest.mark.parametrize("F", [2, 3, 8])
def test_ranks_lie_in_the_intervals_of_the_fp64_oracle(F, d, link, output):
    """lo = #{c in E_q : S_c - B_c > S_p + B_p} <= rank <= hi = #{c in E_q, c != p : S_c + B_c >= S_p - B_p} with the
    per-pair bounds B of test_gpu_rank_field.oracle; per case the oracle alone pins the rank (hi == lo) for at least
    75 % of the positives, so the check is not vacuous."""
    for field in sorted({0, F // 2, F - 1}):
        sizes, ctx, all_c, variants = case(F, d, field)
        m = _model(sizes, d, output=output, link=link, seed=d + F, scale=0.5)
        ent, bia, scal = tables(sizes, d, d + F, 0.5)
        off = _offsets(sizes)
        # one oracle pass per field: its moments and their bounds are the scores of "top" and "variance"
        Sm, Mo, Vo, Bs, Bm, Bv = oracle(ent, bia, scal, link, ctx, field, all_c, "mean" if output == "class" else "top")
        for strategy in strategies_of(output, with_random=False):
            So, Bo = {"top": (Mo, Bm), "variance": (Vo, Bv), "mean": (Sm, Bs)}[strategy]
            for cands, cand, exclude, excl, pos, rows in variants:
                r = call(m, rows, field, cands, exclude, strategy=strategy)
                rank = r["rank"].cpu().numpy()
                S, B = So[:, cand - off[field]], Bo[:, cand - off[field]]
                lo, hi = [], []
                for q in range(len(ctx)):
                    el, p = ~excl[q], np.flatnonzero(pos[q])
                    lo += ((S[q, el] - B[q, el])[None, :] > (S[q, p] + B[q, p])[:, None]).sum(1).tolist()
                    hi += (((S[q, el] + B[q, el])[None, :] >= (S[q, p] - B[q, p])[:, None]).sum(1) - 1).tolist()
                lo, hi = np.array(lo), np.array(hi)
                pinned = float((hi == lo).mean())
                print(f"F={F} d={d} {link} {output} field={field} {strategy} cand={cands is not None} "
                      f"excl={exclude is not None}: pinned share {pinned:.3f}, widest interval {int((hi - lo).max())}")
                assert np.all(lo <= rank) and np.all(rank <= hi), (field, strategy, np.flatnonzero((rank < lo) | (rank > hi)))
                assert pinned >= 0.75


# ---------------------------------------------------------------------------------------------------- 3. rank_field
@pytest.mark.parametrize("strategy,output", [("top", "reg"), ("variance", "reg"), ("mean", "class"), ("random", "reg")])
def test_positives_sit_at_their_rank_in_rank_field(strategy, output):
    sizes, ctx, all_c, variants = case(3, 20, 1)
    m = _model(sizes, 20, output=output, seed=23)
    for cands, cand, exclude, excl, pos, rows in variants:
        kw = dict(candidates=None if cands is None else torch.tensor(cands),
                  exclude=None if exclude is None else torch.tensor(exclude), strategy=strategy, seed=9)
        r = m.rank_heldout_field(torch.tensor(rows), 1, **kw)
        top = m.rank_field(r["contexts"], 1, k=128, **kw)["items"]
        qi, inside = r["query_index"], r["rank"] < 128
        assert torch.equal(top[qi[inside], r["rank"][inside]], r["items"][inside]), (strategy, cands is None)
        absent = ~(top[qi[~inside]] == r["items"][~inside][:, None]).any(1)
        assert bool(absent.all())
        if cands is None:
            assert bool((~inside).any()) and bool(inside.any())


# ---------------------------------------------------------------------------------------------------- 4. shape edges
def _small_case(sizes, Q, rng, frac=0.15):
    """Q distinct sorted contexts of a three-field model ranked on field 1, 15 % exclusion rows."""
    off = _offsets(sizes)
    ctx = np.stack([rng.integers(0, sizes[0], Q), np.zeros(Q, np.int64), off[2] + rng.integers(0, sizes[2], Q)], 1)
    ctx = np.unique(ctx.astype(np.int64), axis=0)
    all_c = np.arange(off[1], off[2], dtype=np.int64)
    ex = []
    for c in ctx:
        for i in all_c[rng.random(len(all_c)) < frac]:
            ex.append([c[0], i, c[2]])
    return ctx, all_c, np.array(ex, np.int64).reshape(-1, 3)


# d -> padded depths (KA, KB): 1:(16,16) 17:(32,64) 1024:(1024,3072)
@pytest.mark.parametrize("d", [1, 17, 1024])
def test_k_padding(d):
    sizes = [60, 300, 4]
    m = _model(sizes, d, output="class", seed=8, scale=0.5 if d < 1024 else 0.2)
    rng = np.random.default_rng(d)
    ctx, all_c, ex = _small_case(sizes, 12 if d == 1024 else 50, rng)
    excl = _excluded(ctx, all_c, ex, 1, (0, 2))
    pos = draw_positives(excl, rng)
    rows = rows_of(ctx, pos, all_c, 1, rng)
    for strategy in ("top", "variance", "mean", "random"):
        r = call(m, rows, 1, None, ex, strategy=strategy, seed=5)
        check_exact(r, scores_of(m, ctx, 1, all_c, strategy, seed=5), excl, pos, ctx)


def test_partial_query_and_item_tiles():
    """Q = 300: two 256-query tiles, the second partial; 70 candidates: a partial second item tile; 1 candidate."""
    sizes = [400, 100, 6]
    m = _model(sizes, 12, seed=31)
    rng = np.random.default_rng(3)
    ctx, all_c, ex = _small_case(sizes, 380, rng)
    ctx = ctx[:300]
    assert len(ctx) == 300
    sub = np.sort(rng.choice(all_c, 70, replace=False))
    excl = _excluded(ctx, sub, ex, 1, (0, 2))
    pos = draw_positives(excl, rng)
    for strategy in ("top", "variance", "random"):
        r = call(m, rows_of(ctx, pos, sub, 1, rng), 1, sub, ex, strategy=strategy, seed=2)
        check_exact(r, scores_of(m, ctx, 1, sub, strategy, seed=2), excl, pos, ctx)
        one = all_c[41:42]
        none = np.zeros((300, 1), bool)
        r = call(m, rows_of(ctx, ~none, one, 1, rng), 1, one, None, strategy=strategy, seed=2)
        check_exact(r, scores_of(m, ctx, 1, one, strategy, seed=2), none, ~none, ctx)
        assert r["rank"].tolist() == [0] * 300 and r["n_eligible"].tolist() == [1] * 300 and int(r["n_neg"].sum()) == 0


def test_bitwise_deterministic_across_splits_and_streams():
    sizes = [400, 1000, 6]
    rng = np.random.default_rng(0)
    ctx, all_c, ex = _small_case(sizes, 330, rng, frac=0.05)
    excl = _excluded(ctx, all_c, ex, 1, (0, 2))
    pos = draw_positives(excl, rng, mean=20)
    rows = rows_of(ctx, pos, all_c, 1, rng)
    for strategy, output in (("top", "reg"), ("variance", "reg"), ("mean", "class"), ("random", "reg")):
        m = _model(sizes, 20, output=output, seed=3)
        ref = call(m, rows, 1, None, ex, strategy=strategy, seed=4)
        check_exact(ref, scores_of(m, ctx, 1, all_c, strategy, seed=4), excl, pos, ctx)
        for n_splits in (0, 1, 3, 64):
            out = call(m, rows, 1, None, ex, strategy=strategy, seed=4, n_splits=n_splits)
            for key in KEYS:
                assert torch.equal(ref[key], out[key]), (strategy, n_splits, key)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            out = call(m, rows, 1, None, ex, strategy=strategy, seed=4)
        s.synchronize()
        for key in KEYS:
            assert torch.equal(ref[key], out[key]), (strategy, "stream", key)


def test_op_without_query_keys_uses_the_query_positions():
    """The op called directly with qkey = None: the context prep writes the position keys into the workspace (for
    `random` it is launched for them alone), and the positives' scores and the scan read them.  `top` does not depend on
    the keys: its outputs equal the keyed call's.  `random` is keyed on (seed, the query's position, candidate id)."""
    from vae_amd import _lib, rank
    sizes = [400, 100, 6]
    m = _model(sizes, 12, seed=31)
    rng = np.random.default_rng(8)
    ctx, all_c, ex = _small_case(sizes, 380, rng)
    ctx = ctx[:300]                                                # two query tiles, the second partial
    excl = _excluded(ctx, all_c, ex, 1, (0, 2))
    pos = draw_positives(excl, rng)
    ent, bia, scal = m._views(m._flat)
    T, Q, C = m.T, len(ctx), len(all_c)
    tctx = torch.tensor(ctx, device=DEV)
    eptr, eitems = rank.field_exclusion_csr(tctx, torch.tensor(ex, device=DEV), 1, [0, 2], T)
    q, j = np.nonzero(pos)
    pptr = torch.tensor(np.concatenate([[0], np.cumsum(pos.sum(1))]), device=DEV)
    pitems = torch.tensor(all_c[j], device=DEV)
    o = _lib.ops()
    x = tctx[:, None, :].expand(-1, C, -1).clone()
    x[:, :, 1] = torch.tensor(all_c, device=DEV)[None, :]
    x = x.reshape(Q * C, 3)
    pos_key = torch.arange(Q, device=DEV)[:, None].expand(-1, C).reshape(-1).contiguous()
    for strategy in ("top", "random"):
        code = rank.STRATEGIES[strategy]
        outs = []
        for qkey in (None, tctx[:, 0].contiguous()):
            out = [torch.full((int(pos.sum()),), -7, dtype=torch.int64, device=DEV) for _ in range(2)] + \
                  [torch.full((Q,), -7, dtype=torch.int64, device=DEV) for _ in range(2)]
            ws = torch.empty(o.rank_eval_field_workspace_bytes(Q, C, int(pos.sum()), 3, 12, code, 3), dtype=torch.uint8,
                             device=DEV)
            o.rank_heldout_field(tctx, 1, qkey, None, C, int(all_c[0]), eptr, eitems, pptr, pitems, ent, bia, scal, ws,
                                 *out, code, 0, 5, 3)
            outs.append(out)
        mean, var, sc = (torch.empty(Q * C, device=DEV) for _ in range(3))
        o.field_moments(x, 1, pos_key, ent, bia, scal, mean, var, sc, 0, code, 5)
        want = exact_ranks(sc.reshape(Q, C).cpu().numpy(), excl, pos)
        for got, w in zip(outs[0], want):
            np.testing.assert_array_equal(got.cpu().numpy(), w)
        if strategy == "top":
            assert all(torch.equal(a, b) for a, b in zip(*outs))
        else:
            assert not torch.equal(outs[0][0], outs[1][0])            # (other keys, another order)


# ---------------------------------------------------------------------------------------------------- 5. heavy, degenerate
def test_heavy_and_degenerate_queries():
    sizes = [50, 3000, 4]
    m = _model(sizes, 16, seed=11)
    items = np.arange(50, 3050, dtype=np.int64)
    rng = np.random.default_rng(5)
    ctx = np.array([[0, 0, 3050], [1, 0, 3050], [2, 0, 3051], [3, 0, 3052], [4, 0, 3053]], np.int64)
    pos = np.zeros((5, 3000), bool)
    excl = np.zeros((5, 3000), bool)
    pos[0, rng.choice(3000, 2500, replace=False)] = True          # 2,500 positives: the merge's multi-chunk prefix sum
    excl[1, 40:] = True
    pos[1, :40] = True                                            # every eligible candidate a positive
    excl[2] = True
    excl[2, 77] = False
    pos[2, 77] = True                                             # a single eligible candidate
    excl[3, [5, 900]] = True                                      # query 3: both of its positives are excluded
    pos[4, [5, 900, 2999]] = True
    q, j = np.nonzero(excl)
    ex = ctx[q].copy()
    ex[:, 1] = items[j]
    rows = rows_of(ctx, pos, items, 1, rng)
    bad = np.array([[3, items[900], 3052], [3, items[5], 3052]], np.int64)
    with pytest.raises(ValueError, match=r"\[3, 55, 3052\]"):      # the first offending row, in (query, id) order
        call(m, np.concatenate([rows, bad]), 1, None, ex)
    for strategy in ("top", "variance"):
        r = call(m, np.concatenate([bad[:1], rows, bad[1:]]), 1, None, ex, strategy=strategy, ineligible="drop")
        check_exact(r, scores_of(m, ctx, 1, items, strategy), excl, pos, ctx)
        assert r["n_dropped"] == 2
        ptr = r["ptr"].tolist()
        assert ptr[3] == ptr[4] and ptr[5] - ptr[4] == 3                                   # an empty segment
        assert r["n_eligible"].tolist() == [3000, 40, 1, 2998, 3000] and r["n_neg"].tolist() == [500, 0, 0, 2998, 2997]
        assert sorted(r["rank"][ptr[1]:ptr[2]].tolist()) == list(range(40))               # a permutation of 0..39
        assert int(r["rank_neg"][ptr[1]:ptr[2]].abs().sum()) == 0
        assert r["rank"][ptr[2]].item() == 0 and r["rank_neg"][ptr[2]].item() == 0
        assert sorted((r["rank"] - r["rank_neg"])[:ptr[1]].tolist()) == list(range(2500))  # positives ahead: 0..2499
    res = m.evaluate_ranking_field(torch.tensor(np.concatenate([rows, bad])), torch.full((len(rows) + 2,), 5.0), 1,
                                   exclude=torch.tensor(ex), per_query=True, ineligible="drop")
    per = res["per_query"]
    assert torch.equal(per["contexts"].cpu(), torch.tensor(ctx)) and res["n_users"] == 4
    assert np.isnan(per["auc"][1].item()) and np.isnan(per["auc"][2].item()) and not np.isnan(per["auc"][0].item())
    assert all(np.isnan(per[key][3].item()) for key in per if key != "contexts")
    assert per["mrr"][2].item() == 1.0 and per["recall@10"][1].item() == 0.25
    assert per["ndcg@10"][1].item() == pytest.approx(1.0, rel=1e-12)       # (a ratio of two fp64 sums of ten terms)


# ---------------------------------------------------------------------------------------------------- 6. independence
def test_a_query_does_not_depend_on_the_other_queries():
    sizes = [300, 500, 5]
    rng = np.random.default_rng(7)
    ctx, all_c, ex = _small_case(sizes, 260, rng)
    ctx = ctx[:200]
    assert len(ctx) == 200
    excl = _excluded(ctx, all_c, ex, 1, (0, 2))
    pos = draw_positives(excl, rng)
    rows = rows_of(ctx, pos, all_c, 1, rng)
    for strategy, output in (("top", "reg"), ("variance", "reg"), ("mean", "class"), ("random", "reg")):
        m = _model(sizes, 16, output=output, seed=13)
        full = call(m, rows, 1, None, ex, strategy=strategy, seed=6)
        ptr = full["ptr"].tolist()
        for q in (0, 57, 199):
            mine = rows[(rows[:, [0, 2]] == ctx[q, [0, 2]]).all(1)]                      # (the full rows of this context)
            alone = call(m, mine, 1, None, ex, strategy=strategy, seed=6)
            assert alone["contexts"].cpu().tolist() == [ctx[q].tolist()]
            for key in ("items", "rank", "rank_neg"):
                assert torch.equal(alone[key], full[key][ptr[q]:ptr[q + 1]]), (strategy, q, key)
            for key in ("n_eligible", "n_neg"):
                assert torch.equal(alone[key], full[key][q:q + 1]), (strategy, q, key)


def test_duplicate_contexts_form_one_query():
    m = _model([50, 400, 3], 12, seed=6)
    rows = torch.tensor([[3, 60, 451], [7, 61, 450], [3, 99, 451], [3, 60, 451], [7, 300, 450], [3, 449, 452]])
    r = m.rank_heldout_field(rows, 1, strategy="variance")
    assert r["contexts"].tolist() == [[3, 0, 451], [3, 0, 452], [7, 0, 450]]
    assert r["ptr"].tolist() == [0, 2, 3, 5] and r["items"].tolist() == [60, 99, 449, 61, 300]
    assert r["query_index"].tolist() == [0, 0, 1, 2, 2] and r["n_eligible"].tolist() == [400] * 3
    assert r["n_neg"].tolist() == [398, 399, 398]
    ctx = r["contexts"].cpu().numpy()
    pos = np.zeros((3, 400), bool)
    pos[[0, 0, 1, 2, 2], np.array([60, 99, 449, 61, 300]) - 50] = True
    check_exact(r, scores_of(m, ctx, 1, np.arange(50, 450), "variance"), np.zeros((3, 400), bool), pos, ctx)
    empty = m.rank_heldout_field(rows[:0], 1)                          # no positive: no query, nothing launched
    assert empty["contexts"].shape == (0, 3) and empty["ptr"].tolist() == [0] and empty["n_dropped"] == 0
    assert all(empty[key].numel() == 0 for key in ("items", "query_index", "rank", "rank_neg", "n_eligible", "n_neg"))


# ---------------------------------------------------------------------------------------------------- 7. match_fields
def test_match_fields_widens_the_exclusion():
    """(0,): anything this user has seen, in any format -- n_eligible drops accordingly."""
    sizes = [30, 120, 4]
    m = _model(sizes, 8, seed=2)
    rng = np.random.default_rng(4)
    ctx, all_c, _ = _small_case(sizes, 60, rng)
    ex = np.stack([rng.integers(0, 30, 900), 30 + rng.integers(0, 120, 900), 150 + rng.integers(0, 4, 900)], 1)
    strict = _excluded(ctx, all_c, ex, 1, (0, 2))
    wide = _excluded(ctx, all_c, ex, 1, (0,))
    assert (wide | ~strict).all() and wide.sum() > 2 * strict.sum()
    pos = draw_positives(wide, rng)                              # eligible under both
    rows = rows_of(ctx, pos, all_c, 1, rng)
    S = scores_of(m, ctx, 1, all_c, "top")
    a = call(m, rows, 1, None, ex)
    check_exact(a, S, strict, pos, ctx)
    b = call(m, rows, 1, None, ex, match_fields=(0,))
    check_exact(b, S, wide, pos, ctx)
    np.testing.assert_array_equal((a["n_eligible"] - b["n_eligible"]).cpu().numpy(), (wide & ~strict).sum(1))
    # a positive excluded only under the wide match: raised, or dropped and counted
    q, j = np.nonzero(wide & ~strict)
    extra = ctx[q[:1]].copy()
    extra[:, 1] = all_c[j[:1]]
    more = np.concatenate([rows, extra])
    assert call(m, more, 1, None, ex)["n_dropped"] == 0
    with pytest.raises(ValueError, match="not an eligible candidate"):
        call(m, more, 1, None, ex, match_fields=(0,))
    c = call(m, more, 1, None, ex, match_fields=(0,), ineligible="drop")
    assert c["n_dropped"] == 1
    for key in KEYS:
        assert torch.equal(b[key], c[key]), key


# ---------------------------------------------------------------------------------------------------- 8. lazy state
def test_rank_heldout_field_after_lazy_fit_equals_the_call_after_sync():
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
    for strategy in ("top", "variance"):
        ra = a.rank_heldout_field(X[::2], 1, exclude=X[1::2], strategy=strategy, ineligible="drop")
        rb = b.rank_heldout_field(X[::2], 1, exclude=X[1::2], strategy=strategy, ineligible="drop")
        for key in KEYS:
            assert torch.equal(ra[key], rb[key]), key
        assert ra["n_dropped"] == rb["n_dropped"] and ra["rank"].numel() > 200
    assert not a._lazy_dirty and torch.equal(a._flat, b._flat)


# ---------------------------------------------------------------------------------------------------- 9. metrics
@pytest.mark.parametrize("output", ["class", "reg"])
def test_evaluate_ranking_field_matches_brute_force_and_sklearn(output):
    from sklearn.metrics import ndcg_score, roc_auc_score
    sizes, field, ks = [40, 120, 3], 1, (1, 5, 10)
    m = _model(sizes, 8, output=output, seed=17)
    rng = np.random.default_rng(9)
    all_c = np.arange(40, 160, dtype=np.int64)

    def rows(n):
        x = np.stack([rng.integers(0, 40, n), 40 + rng.integers(0, 120, n), 160 + rng.integers(0, 3, n)], 1)
        return np.unique(x.astype(np.int64), axis=0)
    Xtr = rows(1500)
    train = set(map(tuple, Xtr.tolist()))
    Xte = np.array([r for r in rows(900).tolist() if tuple(r) not in train], np.int64)
    Xte = Xte[rng.permutation(len(Xte))]
    yte = rng.integers(0, 2, len(Xte)) if output == "class" else rng.integers(1, 6, len(Xte))
    relevant = (yte == 1) if output == "class" else (yte >= 4)
    res = m.evaluate_ranking_field(torch.tensor(Xte), torch.tensor(yte, dtype=torch.float32), field, ks=ks,
                                   exclude=torch.tensor(Xtr), per_query=True)
    per = res["per_query"]
    ctx = per["contexts"].cpu().numpy()
    want_ctx = Xte[relevant].copy()
    want_ctx[:, field] = 0
    np.testing.assert_array_equal(ctx, np.unique(want_ctx, axis=0))
    assert res["n_users"] == len(ctx) and set(per) == {"contexts", "mrr", "auc"} | {f"{n}@{k}" for k in ks for n in
                                                                                     ("hit", "precision", "recall", "ndcg")}
    S = scores_of(m, ctx, field, all_c, "top")
    rel = set(map(tuple, Xte[relevant].tolist()))
    want = {key: [] for key in per if key != "contexts"}
    for q, c in enumerate(ctx.tolist()):
        elig = np.array([(c[0], i, c[2]) not in train for i in all_c.tolist()])
        y = np.array([(c[0], i, c[2]) in rel for i in all_c[elig].tolist()], int)
        s = S[q, elig].astype(np.float64)
        assert len(np.unique(s)) == len(s) and y.sum() > 0                 # (no ties: sklearn's 1/2 never applies)
        order = np.argsort(-s)
        for k in ks:
            hits = int(y[order[:k]].sum())
            want[f"hit@{k}"].append(float(hits > 0))
            want[f"precision@{k}"].append(hits / k)
            want[f"recall@{k}"].append(hits / y.sum())
            want[f"ndcg@{k}"].append(ndcg_score(y[None], s[None], k=k))
        want["mrr"].append(1.0 / (1 + int(np.flatnonzero(y[order])[0])))
        want["auc"].append(roc_auc_score(y, s))
    for key, w in want.items():
        np.testing.assert_allclose(per[key].cpu().numpy(), np.array(w), rtol=1e-12, atol=0, err_msg=key)
        assert res[key] == pytest.approx(float(np.mean(w)), rel=1e-12), key
    plain = m.evaluate_ranking_field(torch.tensor(Xte), torch.tensor(yte, dtype=torch.float32), field, ks=ks,
                                     exclude=torch.tensor(Xtr))
    assert "per_query" not in plain and plain == {key: v for key, v in res.items() if key != "per_query"}
    if output == "reg":                                                    # the threshold moves the relevant set
        low = m.evaluate_ranking_field(torch.tensor(Xte), torch.tensor(yte, dtype=torch.float32), field, ks=ks,
                                       exclude=torch.tensor(Xtr), threshold=2.0)
        want_low = Xte[yte >= 2].copy()
        want_low[:, field] = 0
        assert low["n_users"] == len(np.unique(want_low, axis=0)) >= res["n_users"]


def test_two_field_model_counts_equal_rank_heldout():
    """F = 2, field 1: the same queries, exclusions and positives as rank_heldout, so n_eligible and n_neg agree exactly;
    the ranks come from a different fp32 chain and agree wherever the two scores do not tie within rounding."""
    N, M = 120, 500
    m = _model([N, M], 20, seed=12)
    rng = np.random.default_rng(2)
    users = np.sort(rng.choice(N, 60, replace=False)).astype(np.int64)
    items = np.arange(N, N + M, dtype=np.int64)
    ex = np.array([(u, i) for u in users.tolist() for i in items[rng.random(M) < 0.2].tolist()], np.int64)
    ctx = np.stack([users, np.zeros_like(users)], 1)
    excl = _excluded(ctx, items, ex, 1, (0,))
    pos = draw_positives(excl, rng)
    rows = rows_of(ctx, pos, items, 1, rng)
    a = m.rank_heldout_field(torch.tensor(rows), 1, exclude=torch.tensor(ex))
    b = m.rank_heldout(torch.tensor(rows), exclude=torch.tensor(ex))
    assert torch.equal(a["contexts"][:, 0], b["users"]) and torch.equal(a["ptr"], b["ptr"])
    assert torch.equal(a["items"], b["items"]) and torch.equal(a["query_index"], b["user_index"])
    assert torch.equal(a["n_eligible"], b["n_eligible"]) and torch.equal(a["n_neg"], b["n_neg"])
    ea = m.evaluate_ranking_field(torch.tensor(rows), torch.full((len(rows),), 5.0), 1, exclude=torch.tensor(ex))
    eb = m.evaluate_ranking(torch.tensor(rows), torch.full((len(rows),), 5.0), exclude=torch.tensor(ex))
    assert ea["n_users"] == eb["n_users"] == len(users)

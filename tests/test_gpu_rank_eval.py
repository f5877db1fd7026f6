"""GPU: held-out ranking evaluation (include/vfm_rank.h: vfm_rank_heldout_f32) -- exact ranks against an oracle that
scores every (user, candidate) pair with the moments kernel and orders them with a stable sort, agreement with
rank_items, determinism, heavy and degenerate users, the ML-20M shape, and the metrics of a fitted model against
sklearn."""
import os

import numpy as np
import pytest
import torch

from test_gpu_rank import _model

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def scores_of(m, users, cand, strategy, seed=0):
    """[U, C] fp32 scores of every (user, candidate) pair: the moments kernel (bitwise the ranking's scores)."""
    from vae_amd.rank import predictive_moments
    u = torch.as_tensor(np.asarray(users), device=DEV)
    c = torch.as_tensor(np.asarray(cand), device=DEV)
    x = torch.stack([u[:, None].expand(-1, c.numel()).reshape(-1), c[None, :].expand(u.numel(), -1).reshape(-1)], 1)
    _, _, sc = predictive_moments(x, *m._views(m._flat), m.link, strategy, seed)
    return sc.reshape(u.numel(), c.numel()).cpu().numpy()


def oracle_ranks(S, cand, users, pos_rows, excl_rows):
    """Per query user (ascending) and its positives (ascending): rank, rank_neg, and per user n_eligible, n_neg; the
    order is a stable sort of the eligible candidates (ascending ids) by score descending."""
    excl = set(map(tuple, np.asarray(excl_rows).tolist())) if excl_rows is not None else set()
    pos = {}
    for u, i in np.asarray(pos_rows).tolist():
        pos.setdefault(u, set()).add(i)
    rank, rank_neg, n_el, n_neg = [], [], [], []
    for q, u in enumerate(users):
        elig = np.array([(u, i) not in excl for i in cand.tolist()], bool)
        ids, s = cand[elig], S[q, elig]
        order = torch.sort(torch.from_numpy(-s), stable=True).indices.numpy()
        where = np.empty(len(ids), np.int64)
        where[order] = np.arange(len(ids))
        is_pos = np.isin(ids, sorted(pos.get(u, ())))
        for i in sorted(pos.get(u, ())):
            j = int(np.searchsorted(ids, i))
            assert ids[j] == i
            r = int(where[j])
            rank.append(r)
            rank_neg.append(r - int((is_pos & (where < r)).sum()))
        n_el.append(len(ids))
        n_neg.append(len(ids) - int(is_pos.sum()))
    return [np.array(a, np.int64) for a in (rank, rank_neg, n_el, n_neg)]


def check_against_oracle(m, r, cand, pos_rows, excl_rows, strategy, seed=0):
    users = r["users"].cpu().numpy()
    S = scores_of(m, users, cand, strategy, seed)
    rank, rank_neg, n_el, n_neg = oracle_ranks(S, cand, users, pos_rows, excl_rows)
    np.testing.assert_array_equal(r["rank"].cpu().numpy(), rank)
    np.testing.assert_array_equal(r["rank_neg"].cpu().numpy(), rank_neg)
    np.testing.assert_array_equal(r["n_eligible"].cpu().numpy(), n_el)
    np.testing.assert_array_equal(r["n_neg"].cpu().numpy(), n_neg)


def draw_positives(users, cand, excl_rows, rng, mean=6.0):
    excl = set(map(tuple, np.asarray(excl_rows).tolist())) if excl_rows is not None else set()
    rows = []
    for u in users.tolist():
        elig = [i for i in cand.tolist() if (u, i) not in excl]
        n = min(len(elig), int(rng.geometric(1.0 / mean)))
        rows += [(u, i) for i in rng.choice(elig, n, replace=False).tolist()]
    rows += rows[:3]                                                   # duplicates are dropped
    return np.array(rows, np.int64)


def _exclusions(users, items, rng, frac=0.2):
    return np.array([(u, i) for u in users.tolist() for i in items[rng.random(len(items)) < frac].tolist()], np.int64)


@pytest.mark.parametrize("output", ["reg", "class"])
@pytest.mark.parametrize("link", ["abs", "softplus"])
@pytest.mark.parametrize("d", [5, 20, 128])
def test_ranks_match_oracle_and_rank_items(output, link, d):
    N, M = 700, 1500
    m = _model(N, M, d, output=output, link=link, seed=d)
    rng = np.random.default_rng(d + (link == "abs"))
    users = np.sort(rng.choice(N, 24, replace=False)).astype(np.int64)
    all_items = np.arange(N, N + M, dtype=np.int64)
    ex = _exclusions(users, all_items, rng)
    sub = rng.choice(all_items, 400, replace=False)                    # (unsorted: the library sorts)
    strategies = ["top", "variance", "random"] + (["mean"] if output == "class" else [])
    for strategy in strategies:
        for items in (None, sub):
            cand = all_items if items is None else np.sort(sub)
            for exclude in (None, ex):
                pos = draw_positives(users, cand, exclude, rng)
                kw = dict(items=None if items is None else torch.tensor(items),
                          exclude=None if exclude is None else torch.tensor(exclude), strategy=strategy, seed=9)
                r = m.rank_heldout(torch.tensor(pos), **kw)
                check_against_oracle(m, r, cand, pos, exclude, strategy, seed=9)
                # rank_items agreement at k = 128: rank < k <=> item [rank] of the list, else absent
                top = m.rank_items(r["users"], k=128, **kw)["items"]
                uq = r["user_index"]
                inside = r["rank"] < 128
                got = top[uq[inside], r["rank"][inside]]
                assert torch.equal(got, r["items"][inside]), (strategy, items is None, exclude is None)
                absent = ~(top[uq[~inside]] == r["items"][~inside][:, None]).any(1)
                assert bool(absent.all())


def test_bitwise_deterministic_across_splits_calls_and_streams():
    N, M = 3000, 5000
    for strategy, output in (("top", "reg"), ("variance", "reg"), ("mean", "class"), ("random", "reg")):
        m = _model(N, M, 20, output=output, seed=3)
        rng = np.random.default_rng(0)
        users = np.arange(0, 600, 2)
        ex = _exclusions(users, np.arange(N, N + M), rng, 0.05)
        pos = draw_positives(users, np.arange(N, N + M), ex, rng, mean=20)
        ref = m.rank_heldout(torch.tensor(pos), exclude=torch.tensor(ex), strategy=strategy, seed=4)
        for n_splits in (0, 1, 3, 64, 0):
            out = m.rank_heldout(torch.tensor(pos), exclude=torch.tensor(ex), strategy=strategy, seed=4,
                                 n_splits=n_splits)
            for key in ref:
                assert torch.equal(ref[key], out[key]), (strategy, n_splits, key)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            out = m.rank_heldout(torch.tensor(pos), exclude=torch.tensor(ex), strategy=strategy, seed=4)
        s.synchronize()
        for key in ref:
            assert torch.equal(ref[key], out[key])


def test_heavy_and_degenerate_users():
    N, M = 50, 3000
    m = _model(N, M, 16, seed=11)
    items = np.arange(N, N + M, dtype=np.int64)
    rng = np.random.default_rng(5)
    heavy = [(0, i) for i in rng.choice(items, 2500, replace=False).tolist()]            # 2,500 positives
    sub = items[:40]
    all_pos = [(1, int(i)) for i in sub]                                                 # every candidate a positive
    lone_ex = [(2, int(i)) for i in items if i != items[77]]                             # one eligible candidate
    few = [(3, int(i)) for i in items[[5, 900, 2999]]]
    ex = np.array(lone_ex + [(1, int(i)) for i in items[40:]], np.int64)
    pos = np.array(heavy + all_pos + [(2, int(items[77]))] + few, np.int64)
    for strategy in ("top", "variance"):
        r = m.rank_heldout(torch.tensor(pos), exclude=torch.tensor(ex), strategy=strategy)
        check_against_oracle(m, r, items, pos, ex, strategy)
        assert r["users"].tolist() == [0, 1, 2, 3]
        assert r["n_neg"].tolist()[1:3] == [0, 0] and r["n_eligible"].tolist()[1:3] == [40, 1]
        lone = int(r["ptr"][2])
        assert r["rank"][lone] == 0 and r["rank_neg"][lone] == 0
        ranks_all = r["rank"][int(r["ptr"][1]): int(r["ptr"][2])]
        assert sorted(ranks_all.tolist()) == list(range(40))                            # a permutation of 0..39
        assert int(r["rank_neg"][int(r["ptr"][1]): int(r["ptr"][2])].abs().sum()) == 0
    res = m.evaluate_ranking(torch.tensor(pos), torch.full((len(pos),), 5.0), ks=(10,), exclude=torch.tensor(ex),
                             per_user=True)
    per = res["per_user"]
    assert per["users"].tolist() == [0, 1, 2, 3] and res["n_users"] == 4
    assert np.isnan(per["auc"][1].item()) and np.isnan(per["auc"][2].item()) and not np.isnan(per["auc"][0].item())
    assert per["mrr"][2].item() == 1.0 and per["recall@10"][1].item() == 0.25 and per["ndcg@10"][1].item() == 1.0


def test_ml20m_shape_exact_on_a_sample():
    N, M, d, U = 138_493, 26_744, 128, 4096
    m = _model(N, M, d, seed=20, scale=0.3)
    g = torch.Generator(device=DEV).manual_seed(1)
    users = torch.randperm(N, device=DEV, generator=g)[:U].sort().values
    ex_items = N + torch.randint(0, M, (U, 100), device=DEV, generator=g)
    ex = torch.stack([users[:, None].expand(-1, 100).reshape(-1), ex_items.reshape(-1)], 1)
    n = torch.distributions.Geometric(probs=torch.tensor(1 / 14.0)).sample((U,)).long().to(DEV) + 1
    pu = torch.repeat_interleave(users, n)
    pi = N + torch.randint(0, M, (pu.numel(),), device=DEV, generator=g)
    pos = torch.stack([pu, pi], 1)
    exk = set((ex[:, 0] * (N + M) + ex[:, 1]).cpu().tolist())
    pos = pos[torch.tensor([k not in exk for k in (pos[:, 0] * (N + M) + pos[:, 1]).cpu().tolist()], device=DEV)]
    r = m.rank_heldout(pos, exclude=ex)
    sample = r["users"][::64][:64].contiguous()
    q = torch.searchsorted(r["users"], sample)
    sel = torch.isin(r["user_index"], q)
    cand = np.arange(N, N + M, dtype=np.int64)
    excl_s = ex[torch.isin(ex[:, 0], sample)].cpu().numpy()
    pos_s = torch.stack([r["users"][r["user_index"][sel]], r["items"][sel]], 1).cpu().numpy()
    S = scores_of(m, sample.cpu().numpy(), cand, "top")
    rank, rank_neg, n_el, n_neg = oracle_ranks(S, cand, sample.cpu().numpy(), pos_s, excl_s)
    np.testing.assert_array_equal(r["rank"][sel].cpu().numpy(), rank)
    np.testing.assert_array_equal(r["rank_neg"][sel].cpu().numpy(), rank_neg)
    np.testing.assert_array_equal(r["n_eligible"][q].cpu().numpy(), n_el)
    np.testing.assert_array_equal(r["n_neg"][q].cpu().numpy(), n_neg)


def test_evaluate_ranking_on_fraction_matches_sklearn():
    from sklearn.metrics import ndcg_score, roc_auc_score
    from vae_amd.data import load_fraction
    from vae_amd.model import VFM
    N, M, Xtr, Xte, ytr, yte = load_fraction(os.path.join(GOLDEN, "fraction"))
    torch.manual_seed(42)
    m = VFM(N, M, 5, output="class", device=DEV)
    m.fit(Xtr, ytr, n_epochs=30, batch_size=100000, verbose=False)
    res = m.evaluate_ranking(Xte, yte, ks=(1, 5, 10), exclude=Xtr, per_user=True)
    per = res["per_user"]
    users = per["users"].cpu().numpy()
    cand = np.arange(N, N + M, dtype=np.int64)
    S = scores_of(m, users, cand, "top")
    Xtr_n, Xte_n, yte_n = (np.asarray(torch.as_tensor(a).cpu()) for a in (Xtr, Xte, yte))
    train = set(map(tuple, Xtr_n.tolist()))
    rel = set(map(tuple, Xte_n[yte_n == 1].tolist()))
    n_auc = 0
    for q, u in enumerate(users.tolist()):
        elig = np.array([(u, i) not in train for i in cand.tolist()])
        y = np.array([(u, i) in rel for i in cand[elig].tolist()], int)
        s = S[q, elig]
        assert len(np.unique(s)) == len(s)                                 # (no ties: sklearn's 1/2 never applies)
        for k in (1, 5, 10):
            want = ndcg_score(y[None], s[None], k=k) if len(y) > 1 else 1.0      # (sklearn needs two documents)
            assert per[f"ndcg@{k}"][q].item() == pytest.approx(want, abs=1e-12)
        if 0 < y.sum() < len(y):
            assert per["auc"][q].item() == pytest.approx(roc_auc_score(y, s), abs=1e-12)
            n_auc += 1
        else:
            assert np.isnan(per["auc"][q].item())
    assert n_auc > 10 and res["n_users"] == len(users)
    assert 0.5 < res["auc"] <= 1.0 and 0.0 < res["ndcg@10"] <= 1.0


def test_bad_arguments_raise():
    N, M = 50, 60
    m = _model(N, M, 8)
    pos = torch.tensor([[0, N + 1], [1, N + 2]])
    with pytest.raises(ValueError):
        m.rank_heldout(pos, exclude=torch.tensor([[0, N + 1]]))             # a positive that is excluded
    with pytest.raises(ValueError):
        m.rank_heldout(pos, items=[N + 2, N + 3])                            # a positive outside the candidates
    for bad in ([[N, N + 1]], [[0, N - 1]], [[0, N + M]], [[-1, N]]):
        with pytest.raises(ValueError):
            m.rank_heldout(torch.tensor(bad))
    with pytest.raises(ValueError):
        m.rank_heldout(pos, exclude=torch.tensor([[0, 5]]))
    with pytest.raises(ValueError):
        m.rank_heldout(pos, strategy="mean")                                 # 'mean' needs a 'class' model
    with pytest.raises(ValueError):
        m.rank_heldout(pos, strategy="best")
    with pytest.raises(ValueError):
        m.rank_heldout(pos, n_splits=65)
    for ks in ((0,), (10, -1), ()):
        with pytest.raises(ValueError):
            m.evaluate_ranking(pos, torch.tensor([5.0, 5.0]), ks=ks)
    from vae_amd.model import VFM
    with pytest.raises(ValueError):
        VFM(field_sizes=[10, 10, 10], embedding_size=4, device=DEV).rank_heldout(torch.tensor([[0, 10]]))

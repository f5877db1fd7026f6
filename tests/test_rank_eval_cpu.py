"""CPU: the ranking metrics of the held-out evaluation (vae_amd.rank.ranking_metrics) from exact ranks against brute
force and sklearn, their edge cases, the eligibility and candidates helpers every ranking form shares against Python
sets, and the argument checks of the two C entry points (include/vfm_rank.h)."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def ranks_from_scores(S, pos, elig):
    """Brute force over a dense score matrix S [U, M] (no ties): per positive (user-major, ascending item) its rank and
    rank among negatives; per user n_neg.  pos, elig: [U, M] bool."""
    rank, rank_neg, ptr, n_neg = [], [], [0], []
    for u in range(S.shape[0]):
        neg = elig[u] & ~pos[u]
        for i in np.flatnonzero(pos[u]):
            rank.append(int((elig[u] & (S[u] > S[u, i])).sum()))
            rank_neg.append(int((neg & (S[u] > S[u, i])).sum()))
        ptr.append(len(rank))
        n_neg.append(int(neg.sum()))
    return np.array(rank), np.array(rank_neg), np.array(ptr), np.array(n_neg)


def test_metrics_match_brute_force_and_sklearn():
    from sklearn.metrics import ndcg_score, roc_auc_score
    from vae_amd.rank import ranking_metrics
    rng = np.random.default_rng(0)
    U, M = 40, 300
    S = rng.normal(size=(U, M))
    elig = rng.random((U, M)) > 0.2
    pos = elig & (rng.random((U, M)) < rng.uniform(0.005, 0.2, size=(U, 1)))
    pos[0] = False
    pos[1] = elig[1]                                   # no negatives: auc undefined
    pos[2] = False
    pos[2, np.flatnonzero(elig[2])[0]] = True          # one positive
    rank, rank_neg, ptr, n_neg = ranks_from_scores(S, pos, elig)
    ks = [1, 5, 10, 500]
    means, per = ranking_metrics(torch.tensor(rank), torch.tensor(rank_neg), torch.tensor(ptr), torch.tensor(n_neg), ks)
    want = {key: [] for key in per}
    for u in range(U):
        e = np.flatnonzero(elig[u])
        y, s = pos[u, e].astype(int), S[u, e]
        npos = int(y.sum())
        order = np.argsort(-s)
        if npos == 0:
            for key in want:
                want[key].append(np.nan)
            continue
        for k in ks:
            hits = int(y[order[:k]].sum())
            want[f"hit@{k}"].append(float(hits > 0))
            want[f"precision@{k}"].append(hits / k)
            want[f"recall@{k}"].append(hits / npos)
            want[f"ndcg@{k}"].append(ndcg_score(y[None, :], s[None, :], k=k))
        want["mrr"].append(1.0 / (1 + int(np.flatnonzero(y[order])[0])))
        want["auc"].append(roc_auc_score(y, s) if npos < len(e) else np.nan)
    for key, v in per.items():
        np.testing.assert_allclose(v.numpy(), np.array(want[key]), rtol=1e-12, atol=1e-12, err_msg=key)
        w = np.array(want[key])
        assert means[key] == pytest.approx(np.nanmean(w), rel=1e-12), key
    assert means["n_users"] == int((pos.sum(1) > 0).sum())
    assert math.isnan(per["auc"][1]) and not math.isnan(per["ndcg@5"][1])
    assert all(math.isnan(per[key][0]) for key in per)


def test_metric_edge_cases():
    from vae_amd.rank import ranking_metrics
    # user 0: one positive at rank 0 of 1 eligible (k > n_eligible); user 1: none; user 2: two positives, no negative
    means, per = ranking_metrics(torch.tensor([0, 1, 0]), torch.tensor([0, 0, 0]), torch.tensor([0, 1, 1, 3]),
                                 torch.tensor([0, 4, 0]), ks=[10])
    assert per["recall@10"].tolist()[0] == 1.0 and per["precision@10"].tolist()[0] == 0.1
    assert per["ndcg@10"][0] == 1.0 and per["ndcg@10"][2] == 1.0 and per["mrr"][2] == 1.0
    assert math.isnan(per["auc"][0]) and math.isnan(per["auc"][2]) and math.isnan(means["auc"])
    assert all(math.isnan(v[1]) for v in per.values())
    assert means["n_users"] == 2 and means["recall@10"] == 1.0
    # a single positive at rank r: ndcg = 1 / log2(r + 2) within k, mrr = 1 / (r + 1), auc from rank_neg / n_neg
    means, per = ranking_metrics(torch.tensor([3]), torch.tensor([2]), torch.tensor([0, 1]), torch.tensor([8]), ks=[3, 4])
    assert per["ndcg@3"][0] == 0.0 and per["ndcg@4"][0] == pytest.approx(1 / math.log2(5))
    assert per["mrr"][0] == 0.25 and per["auc"][0] == pytest.approx(0.75)
    for ks in ([], [0], [3, -1]):
        with pytest.raises(ValueError):
            ranking_metrics(torch.tensor([0]), torch.tensor([0]), torch.tensor([0, 1]), torch.tensor([1]), ks)


def test_eligibility_helpers_match_python_sets():
    """rank._ineligible and rank._apply_ineligible against sets, through the CSRs of the pair form (the queries are the
    users) and of the field form (the queries are contexts), and rank._candidates with both wordings of its errors."""
    from vae_amd import rank
    Q, lo, n_items = 7, 20, 9                               # ids lo .. lo + 8; T past them
    T = lo + n_items + 3
    g = torch.Generator().manual_seed(5)
    all_ids = list(range(lo, lo + n_items))

    def pairs(n, skip=()):
        q = torch.randint(0, Q, (n,), generator=g)
        ids = lo + torch.randint(0, n_items, (n,), generator=g)
        keep = torch.tensor([int(v) not in skip for v in q])
        return q[keep], ids[keep]

    pos_q, pos_id = pairs(30, skip=(3,))                    # query 3 has no positive
    ex_q, ex_id = pairs(25, skip=(5,))                      # query 5 has an empty exclusion list
    # the pair form: users 100 .. 106 in a scrambled order are the queries; the field form: contexts [u, 0, c]
    users = torch.tensor([104, 100, 106, 101, 105, 103, 102])
    ctx = torch.stack([users, torch.zeros_like(users), 200 + torch.arange(Q)], 1)
    forms = {
        "pair": (rank.exclusion_csr(users, torch.stack([users[pos_q], pos_id], 1), T),
                 rank.exclusion_csr(users, torch.stack([users[ex_q], ex_id], 1), T)),
        "field": (rank.query_csr(pos_q, pos_id, Q, T),
                  rank.field_exclusion_csr(ctx, torch.stack([users[ex_q], ex_id, 200 + ex_q], 1), 1, [0, 2], T)),
    }
    excluded = {(int(q), int(i)) for q, i in zip(ex_q, ex_id)}
    assert not any(q == 5 for q, _ in excluded) and 3 not in set(pos_q.tolist())
    cands = {"explicit": [lo + 1, lo + 2, lo + 4, lo + 7, lo + 8], "range": None, "empty": []}
    for form, ((pptr, pitems), (eptr, ex_items)) in forms.items():
        pq = torch.repeat_interleave(torch.arange(Q), pptr[1:] - pptr[:-1])
        assert {(int(q), int(i)) for q, i in zip(pq, pitems)} == {(int(q), int(i)) for q, i in zip(pos_q, pos_id)}
        assert int(eptr[6] - eptr[5]) == 0 and int(pptr[4] - pptr[3]) == 0
        for name, values in cands.items():
            for with_excl in (True, False):
                cand, n_cand = rank._candidates(values, lo, lo + n_items, "cpu")
                assert n_cand == (n_items if values is None else len(values))
                allowed = set(all_ids if values is None else values)
                want = [int(i) not in allowed or (with_excl and (int(q), int(i)) in excluded) for q, i in zip(pq, pitems)]
                e = (eptr, ex_items) if with_excl else (None, None)
                bad = rank._ineligible(pitems, pq, cand, *e, Q, T)
                assert bad.tolist() == want, (form, name, with_excl)
                # the drop step: the survivors, their CSR, the count
                ptr2, items2, pq2, n_dropped = rank._apply_ineligible(bad, pptr, pitems, pq, Q, "drop", None)
                kept = [(int(q), int(i)) for (q, i), b in zip(zip(pq, pitems), want) if not b]
                assert list(zip(pq2.tolist(), items2.tolist())) == kept and n_dropped == sum(want)
                assert ptr2.tolist() == [sum(q < u for q, _ in kept) for u in range(Q + 1)]
                if any(want):
                    first = want.index(True)
                    with pytest.raises(ValueError, match=f"positive {first} of its form"):
                        rank._apply_ineligible(bad, pptr, pitems, pq, Q, "raise", lambda j: f"positive {j} of its form")
                else:
                    assert ptr2 is pptr and items2 is pitems
        no_lists = (torch.zeros(Q + 1, dtype=torch.int64), torch.zeros(0, dtype=torch.int64))      # every list empty
        assert not rank._ineligible(pitems, pq, None, *no_lists, Q, T).any()
    # the candidates parser: sorted, and its two errors in the wording of either form
    cand, n_cand = rank._candidates([lo + 5, lo, lo + 3], lo, lo + n_items, "cpu")
    assert cand.tolist() == [lo, lo + 3, lo + 5] and n_cand == 3 and cand.dtype == torch.int64
    with pytest.raises(ValueError, match=r"candidate ids must lie in the field's range \[20, 29\)"):
        rank._candidates([lo + n_items], lo, lo + n_items, "cpu")
    with pytest.raises(ValueError, match="duplicate candidates"):
        rank._candidates([lo, lo + 1, lo], lo, lo + n_items, "cpu")
    with pytest.raises(ValueError, match=r"item ids must lie in \[20, 29\)"):
        rank._candidates([lo - 1], lo, lo + n_items, "cpu", rank._ITEM_WORDS)
    with pytest.raises(ValueError, match="duplicate candidate items"):
        rank._candidates([lo + 2, lo + 2], lo, lo + n_items, "cpu", rank._ITEM_WORDS)


def _lib():
    from vae_amd import _lib as L
    lib = L.load()
    i64, i32, vp = C.c_int64, C.c_int32, C.c_void_p
    lib.vfm_rank_heldout_f32.argtypes = ([i64, vp, i64, vp, i64, i64, i32, i32, i32, i32, C.c_uint64, i32, vp, vp, i64,
                                          vp, vp, i64] + [vp] * 4 + [i64] + [vp] * 5)
    lib.vfm_rank_heldout_f32.restype = C.c_int
    lib.vfm_rank_eval_workspace_bytes.argtypes = [i64, i64, i64, i32, i32, i32]
    lib.vfm_rank_eval_workspace_bytes.restype = i64
    return lib


FAKE = C.c_void_p(4096)          # a non-NULL pointer the library must never dereference: every call below fails its checks


def _heldout(lib, F=2, users=FAKE, pos_ptr=FAKE, pos_items=FAKE, n_pos=20, ent=FAKE, out=FAKE, ws=FAKE, ws_bytes=1 << 30,
             strategy=0, n_splits=0, d=16, flags=0, n_cand=100, cand=None, item_lo=10, T=200, U=8):
    return lib.vfm_rank_heldout_f32(U, users, n_cand, cand, item_lo, T, F, d, strategy, flags, 0, n_splits, None, None, 0,
                                    pos_ptr, pos_items, n_pos, ent, FAKE, FAKE, ws, ws_bytes, out, FAKE, FAKE, FAKE, None)


def test_rank_heldout_rejects_bad_arguments_without_a_gpu():
    from vae_amd._lib import load
    lib = _lib()
    E = -1
    assert _heldout(lib, F=3) == E and b"F == 2" in load().vfm_last_error()
    assert _heldout(lib, users=None) == E and b"null" in load().vfm_last_error()
    assert _heldout(lib, pos_ptr=None) == E
    assert _heldout(lib, pos_items=None) == E and b"pos_items" in load().vfm_last_error()
    assert _heldout(lib, ent=None) == E
    assert _heldout(lib, out=None) == E
    assert _heldout(lib, ws=None) == E
    assert _heldout(lib, strategy=4) == E
    assert _heldout(lib, n_splits=65) == E and _heldout(lib, n_splits=-1) == E
    assert _heldout(lib, n_pos=-1) == E
    assert _heldout(lib, d=0) == E and _heldout(lib, flags=8) == E
    assert _heldout(lib, n_cand=1 << 31) == E
    assert _heldout(lib, item_lo=150) == E and b"item range" in load().vfm_last_error()
    assert _heldout(lib, U=-1) == E
    assert _heldout(lib, ws_bytes=16) == E and b"workspace" in load().vfm_last_error()
    assert _heldout(lib, ws=C.c_void_p(4096 + 8)) == E and b"aligned" in load().vfm_last_error()
    assert _heldout(lib, U=0, users=None, ent=None, out=None, ws=None) == 0          # nothing to do: no launch
    assert lib.vfm_rank_eval_workspace_bytes(8, 100, 20, 16, 0, 0) > 0
    assert lib.vfm_rank_eval_workspace_bytes(8, 100, -1, 16, 0, 0) == E
    assert lib.vfm_rank_eval_workspace_bytes(8, 100, 20, 16, 9, 0) == E
    assert lib.vfm_rank_eval_workspace_bytes(8, 100, 20, 16, 0, 65) == E
    # O(S (U + n_pos)) past the packed operands: the split count and the positives grow it, never U x n_cand
    w1 = lib.vfm_rank_eval_workspace_bytes(4096, 26744, 50_000, 128, 0, 1)
    w8 = lib.vfm_rank_eval_workspace_bytes(4096, 26744, 50_000, 128, 0, 8)
    assert 0 < w1 < w8 < 4096 * 26744 * 4


def test_cpu_model_rank_eval_fails_loudly():
    from vae_amd.model import VFM
    from vae_amd._lib import VfmLibraryError
    m = VFM(5, 5, 4, device="cpu")
    with pytest.raises(VfmLibraryError):
        m.rank_heldout(torch.tensor([[0, 5]]))
    with pytest.raises(VfmLibraryError):
        m.evaluate_ranking(torch.tensor([[0, 5], [1, 6]]), torch.tensor([5.0, 3.0]))

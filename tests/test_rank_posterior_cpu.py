"""CPU: the field-form ranking under supplied posteriors (include/vfm_rank.h: vfm_field_moments_post_f32,
vfm_rank_field_post_f32, vfm_rank_heldout_field_post_f32) -- the exports, the argument checks of the three C entry
points with pointers that are never dereferenced, the Python argument errors of the four VFM methods and of the ranking
curve, and the curve's host-side bookkeeping (vae_amd.elicit.ranking_curve_plan, round_posteriors) against a brute-force
Python loop."""
import ctypes as C
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FAKE = C.c_void_p(4096)          # a non-NULL pointer the library must never dereference: every call below fails its checks
E = -1                           # VFM_E_INVALID


def _lib():
    from vae_amd import _lib as L
    return L.load()


def _err():
    return _lib().vfm_last_error()


def _moments(B=8, F=3, d=16, T=200, id_bits=64, flags=0, x=FAKE, field=1, post_field=0, post=FAKE, ent=FAKE, bias=FAKE,
             scal=FAKE, strategy=0, m=FAKE, v=FAKE):
    return _lib().vfm_field_moments_post_f32(B, F, d, T, id_bits, flags, x, field, post_field, post, ent, bias, scal,
                                             strategy, 0, None, m, v, None, None)


def _rank(Q=8, ctx=FAKE, field=1, post_field=0, post=FAKE, n_cand=100, cand_lo=10, T=200, F=3, d=16, k=10, strategy=0,
          flags=0, n_splits=0, ent=FAKE, ws=FAKE, ws_bytes=1 << 30, items=FAKE):
    return _lib().vfm_rank_field_post_f32(Q, ctx, field, post_field, post, None, n_cand, None, cand_lo, T, F, d, k,
                                          strategy, flags, 0, n_splits, None, None, 0, ent, FAKE, FAKE, ws, ws_bytes,
                                          items, FAKE, FAKE, FAKE, None)


def _heldout(Q=8, ctx=FAKE, field=1, post_field=0, post=FAKE, n_cand=100, cand_lo=10, T=200, F=3, d=16, strategy=0,
             flags=0, n_splits=0, pos_ptr=FAKE, pos_items=FAKE, n_pos=20, ent=FAKE, ws=FAKE, ws_bytes=1 << 30, rank=FAKE):
    return _lib().vfm_rank_heldout_field_post_f32(Q, ctx, field, post_field, post, None, n_cand, None, cand_lo, T, F, d,
                                                  strategy, flags, 0, n_splits, None, None, 0, pos_ptr, pos_items, n_pos,
                                                  ent, FAKE, FAKE, ws, ws_bytes, rank, FAKE, FAKE, FAKE, None)


# ---------------------------------------------------------------------------------------------------- exports
def test_the_library_exports_the_posterior_entry_points():
    from vae_amd import _lib as L
    assert L.ABI_VERSION == 5 and _lib().vfm_abi_version() == 5
    assert L.RANK_POST_EXPORTS == ("vfm_field_moments_post_f32", "vfm_rank_field_post_f32",
                                   "vfm_rank_heldout_field_post_f32")
    for name in L.RANK_POST_EXPORTS:
        assert hasattr(_lib(), name), name
        assert name not in L.EXPORTS                       # (the pinned set of include/vfm_hip.h is not touched)
    hdr = open(os.path.join(ROOT, "include", "vfm_rank.h")).read()
    for name in L.RANK_POST_EXPORTS:
        assert f"int {name}(" in hdr
    ops = L.ops()
    for name in ("field_moments_post", "rank_field_post", "rank_heldout_field_post"):
        assert hasattr(ops, name)


# ---------------------------------------------------------------------------------------------------- the C entries
@pytest.mark.parametrize("call", [_moments, _rank, _heldout])
def test_the_posterior_entries_reject_bad_arguments_without_a_gpu(call):
    assert call(post_field=1) == E and b"post_field must differ from field" in _err()
    assert call(post_field=-1) == E and b"post_field out of range" in _err()
    assert call(post_field=3) == E and b"post_field out of range" in _err()
    assert call(F=2, field=0, post_field=2) == E and b"post_field out of range" in _err()
    assert call(post=None) == E and b"post" in _err() and b"null" in _err()
    # everything the table forms reject
    assert call(F=1) == E and b"F out of range" in _err()
    assert call(field=3) == E and b"field out of range" in _err()
    assert call(field=-1) == E and b"field out of range" in _err()
    assert call(strategy=4) == E and b"strategy" in _err()
    assert call(d=0) == E and call(flags=8) == E
    assert call(ent=None) == E and b"null" in _err()
    # F == 2: the one context column is the supplied one
    assert call(F=2, field=1, post_field=0, post=None) == E and b"post" in _err()


def test_the_ranking_entries_keep_their_table_form_checks():
    for call in (_rank, _heldout):
        assert call(n_splits=65) == E and b"n_splits" in _err()
        assert call(n_cand=1 << 31) == E and b"n_cand" in _err()
        assert call(cand_lo=150) == E and b"candidate range" in _err()
        assert call(ctx=None) == E and b"null" in _err()
        assert call(ws_bytes=16) == E and b"workspace too small" in _err()
        assert call(ws=C.c_void_p(4096 + 8)) == E and b"aligned" in _err()
        assert call(Q=-1) == E
    assert _rank(k=0) == E and _rank(k=129) == E and b"k out of range" in _err()
    assert _heldout(n_pos=-1) == E and b"n_pos" in _err()
    assert _heldout(pos_items=None) == E and b"pos_items" in _err()
    assert _moments(B=-1) == E and _moments(id_bits=16) == E and b"id_bits" in _err()
    # the workspace functions of the table forms serve the posterior forms: exactly their size is accepted
    lib = _lib()
    lib.vfm_rank_field_workspace_bytes.argtypes = [C.c_int64, C.c_int64] + [C.c_int32] * 5
    lib.vfm_rank_field_workspace_bytes.restype = C.c_int64
    lib.vfm_rank_eval_field_workspace_bytes.argtypes = [C.c_int64] * 3 + [C.c_int32] * 4
    lib.vfm_rank_eval_field_workspace_bytes.restype = C.c_int64
    need = lib.vfm_rank_field_workspace_bytes(8, 100, 3, 16, 10, 0, 0)
    assert need > 0 and _rank(ws_bytes=need - 1) == E and b"workspace too small" in _err()
    need = lib.vfm_rank_eval_field_workspace_bytes(8, 100, 20, 3, 16, 0, 0)
    assert need > 0 and _heldout(ws_bytes=need - 1) == E and b"workspace too small" in _err()


def test_no_query_launches_nothing():
    # every pointer NULL: Q == 0 returns before anything is read or launched (no GPU on this path)
    assert _moments(B=0, x=None, post=None, ent=None, bias=None, scal=None, m=None, v=None) == 0
    assert _rank(Q=0, ctx=None, post=None, ent=None, ws=None, ws_bytes=0, items=None) == 0
    assert _heldout(Q=0, ctx=None, post=None, pos_ptr=None, pos_items=None, n_pos=0, ent=None, ws=None, ws_bytes=0,
                    rank=None) == 0


# ---------------------------------------------------------------------------------------------------- Python arguments
def _cpu_model(output="reg"):
    from vae_amd.model import VFM
    return VFM(field_sizes=[5, 6, 3], embedding_size=4, output=output, device="cpu")      # ranges [0,5) [5,11) [11,14)


def test_python_argument_errors_need_no_gpu():
    m = _cpu_model()
    ctx = torch.tensor([[0, 5, 11], [1, 6, 12]])
    th = torch.zeros(2, 10)
    pos = (torch.tensor([0, 1]), torch.tensor([5, 6]))
    y = torch.tensor([5.0, 5.0])

    def every(match, contexts=ctx, theta=th, post_field=0, field=1, heldout=True, moments=True, **kw):
        with pytest.raises(ValueError, match=match):
            m.rank_field_posterior(contexts, theta, post_field, field, **kw)
        if heldout:
            kw.pop("k", None)
            with pytest.raises(ValueError, match=match):
                m.rank_heldout_field_posterior(contexts, pos, theta, post_field, field, **kw)
            kw.pop("strategy", None), kw.pop("key_field", None), kw.pop("n_splits", None)
            with pytest.raises(ValueError, match=match):
                m.evaluate_ranking_field_posterior(contexts, pos, y, theta, post_field, field, **kw)
        if moments and not kw:                                         # (field_moments leaves the ids to the kernel)
            with pytest.raises(ValueError, match=match):
                m.field_moments_posterior(contexts, theta, post_field, field)

    every("theta must be", theta=torch.zeros(2, 9))                      # 2d + 2 = 10
    every("theta must be", theta=torch.zeros(3, 10))                     # one row per context
    every("theta must be", theta=torch.zeros(2, 1, 10))
    every("float32", theta=torch.zeros(2, 10, dtype=torch.float64))
    every("float32", theta=torch.zeros(2, 10, dtype=torch.int64))
    every("theta must be", theta=[[0.0] * 10] * 2)
    every("post_field must differ", post_field=1)
    for bad in (-1, 3, True, 1.0):
        every("post_field must be", post_field=bad)
    for bad in (-1, 3, True):
        every("field must be", field=bad)
    # everything the table forms reject
    every("ranked field's range", contexts=torch.tensor([[5, 5, 11], [1, 6, 12]]), moments=False)
    every("context ids must lie", contexts=torch.tensor([[0, 5, 14], [1, 6, 12]]), moments=False)
    every(r"must be \[R, 3\]|must be \[B, 3\]", contexts=torch.tensor([[0, 5], [1, 6]]))
    every("match_fields", match_fields=(1,))
    every("exclude", exclude=torch.tensor([[0, 4, 11]]))
    every("candidate ids", candidates=[4, 5])
    every("duplicate candidates", candidates=[5, 5])
    every("query_exclude", query_exclude=(torch.tensor([2]), torch.tensor([5])))          # query index out of range
    every("query_exclude", query_exclude=(torch.tensor([0]), torch.tensor([4])))          # id outside the field
    every("k must lie", heldout=False, k=0)
    every("k must lie", heldout=False, k=129)
    for n_splits in (-1, 65):
        with pytest.raises(ValueError, match="n_splits"):
            m.rank_field_posterior(ctx, th, 0, 1, n_splits=n_splits)
        with pytest.raises(ValueError, match="n_splits"):
            m.rank_heldout_field_posterior(ctx, pos, th, 0, 1, n_splits=n_splits)
    for fn in (lambda **kw: m.rank_field_posterior(ctx, th, 0, 1, **kw),
               lambda **kw: m.rank_heldout_field_posterior(ctx, pos, th, 0, 1, **kw),
               lambda **kw: m.field_moments_posterior(ctx, th, 0, 1, **kw)):
        with pytest.raises(ValueError, match="'mean'"):
            fn(strategy="mean")                                            # 'mean' needs a 'class' model
        for s in ("thompson", "best"):
            with pytest.raises(ValueError, match="strategy must be"):
                fn(strategy=s)
        with pytest.raises(ValueError, match="key_field"):
            fn(key_field=1)
    with pytest.raises(ValueError, match="pos"):
        m.rank_heldout_field_posterior(ctx, (torch.tensor([0, 2]), torch.tensor([5, 6])), th, 0, 1)
    with pytest.raises(ValueError, match="pos"):
        m.rank_heldout_field_posterior(ctx, (torch.tensor([0, 1]), torch.tensor([5, 11])), th, 0, 1)
    with pytest.raises(ValueError, match="pos"):
        m.rank_heldout_field_posterior(ctx, torch.tensor([[0, 5, 11]]), th, 0, 1)
    with pytest.raises(ValueError, match="ineligible"):
        m.rank_heldout_field_posterior(ctx, pos, th, 0, 1, ineligible="skip")
    with pytest.raises(ValueError, match="ks"):
        m.evaluate_ranking_field_posterior(ctx, pos, y, th, 0, 1, ks=(0,))
    with pytest.raises(ValueError, match="one .* pair per y_test"):
        m.evaluate_ranking_field_posterior(ctx, pos, y[:1], th, 0, 1)
    from vae_amd.rank import STRATEGIES
    assert STRATEGIES == {"top": 0, "variance": 1, "mean": 2, "random": 3}


def test_cpu_models_fail_loudly():
    from vae_amd._lib import VfmLibraryError
    ctx = torch.tensor([[0, 5, 11], [1, 6, 12]])
    th = torch.zeros(2, 10)
    pos = (torch.tensor([0, 1]), torch.tensor([5, 6]))
    for output in ("reg", "class"):
        m = _cpu_model(output)
        before = m._flat.clone()
        with pytest.raises(VfmLibraryError):
            m.field_moments_posterior(ctx, th, 0, 1)
        with pytest.raises(VfmLibraryError):
            m.rank_field_posterior(ctx, th, 0, 1)
        with pytest.raises(VfmLibraryError):
            m.rank_field_posterior(ctx, th, 2, 1, exclude=torch.tensor([[0, 5, 11]]),
                                   query_exclude=(torch.tensor([1]), torch.tensor([6])))
        with pytest.raises(VfmLibraryError):
            m.rank_heldout_field_posterior(ctx, pos, th, 0, 1)
        with pytest.raises(VfmLibraryError):
            m.evaluate_ranking_field_posterior(ctx, pos, torch.tensor([5.0, 1.0]), th, 0, 1)
        assert torch.equal(m._flat, before)
    # the curve: its own arguments first, then the session's, then the device
    m = _cpu_model()
    pool = torch.tensor([[0, 5, 11], [0, 6, 11], [1, 7, 12]])
    yp = torch.tensor([4.0, 2.0, 5.0])
    Xt, yt = torch.tensor([[0, 8, 11], [1, 9, 12]]), torch.tensor([5.0, 5.0])
    with pytest.raises(ValueError, match="rank_field must differ"):
        m.elicitation_ranking_curve_field(pool, yp, 2, 0, Xt, yt, 0)
    with pytest.raises(ValueError, match="field must be"):
        m.elicitation_ranking_curve_field(pool, yp, 2, 0, Xt, yt, 3)
    with pytest.raises(ValueError, match="ks"):
        m.elicitation_ranking_curve_field(pool, yp, 2, 0, Xt, yt, 1, ks=())
    with pytest.raises(ValueError, match="sets write itself"):
        m.elicitation_ranking_curve_field(pool, yp, 2, 0, Xt, yt, 1, write=True)
    with pytest.raises(ValueError, match="strategy must be"):
        m.elicitation_ranking_curve_field(pool, yp, 2, 0, Xt, yt, 1, strategies=("best",))
    with pytest.raises(ValueError, match="one y_test value per row"):
        m.elicitation_ranking_curve_field(pool, yp, 2, 0, Xt, yt[:1], 1)
    with pytest.raises(ValueError, match="column 1 must lie"):
        m.elicitation_ranking_curve_field(pool, yp, 2, 0, torch.tensor([[0, 4, 11], [1, 9, 12]]), yt, 1)
    with pytest.raises(ValueError, match="n_questions"):
        m.elicitation_ranking_curve_field(pool, yp, -1, 0, Xt, yt, 1)
    with pytest.raises(ValueError, match="'reg' model"):
        _cpu_model("class").elicitation_ranking_curve_field(pool, yp, 2, 0, Xt, torch.tensor([1.0, 1.0]), 1, exact=True)
    for exact in (False, True):
        with pytest.raises(VfmLibraryError):
            m.elicitation_ranking_curve_field(pool, yp, 2, 0, Xt, yt, 1, exact=exact)


# ---------------------------------------------------------------------------------------------------- the curve's plan
def _brute_plan(ents, rows, pool, hist, exclude, X_rel, field, rank_field, match):
    """Per round: the queries, each one's respondent, positives and exclusion set, by plain Python loops."""
    Q = len(rows[0])
    ctxs = {}
    for r in X_rel:
        if r[field] not in ents:
            continue
        c = list(r)
        item, c[rank_field] = c[rank_field], 0
        ctxs.setdefault(tuple(c), set()).add(item)
    order = sorted(ctxs)
    out = []
    for q in range(Q + 1):
        E = [list(r) for r in exclude] + [list(r) for r in hist]
        for u in range(len(ents)):
            E += [list(pool[p]) for p in rows[u][:q] if p >= 0]
        for c in order:
            excl = {r[rank_field] for r in E if all(r[f] == c[f] for f in match)}
            out.append({"query": list(c), "resp": ents.index(c[field]), "round": q, "pos": sorted(ctxs[c]),
                        "excl": sorted(excl)})
    return out


def _plan_as_lists(plan):
    n = plan["queries"].shape[0]
    pos, excl = [[] for _ in range(n)], [[] for _ in range(n)]
    for qi, i in zip(plan["pos"][0].tolist(), plan["pos"][1].tolist()):
        pos[qi].append(i)
    for qi, i in zip(plan["excl"][0].tolist(), plan["excl"][1].tolist()):
        excl[qi].append(i)
    return [{"query": plan["queries"][j].tolist(), "resp": int(plan["resp"][j]), "round": int(plan["round"][j]),
             "pos": sorted(pos[j]), "excl": sorted(set(excl[j]))} for j in range(n)]


@pytest.mark.parametrize("match", [[0, 2], [0]])
def test_the_curve_plan_matches_a_brute_force_loop(match):
    """2 respondents, 3 rounds, a 6-row pool of a three-field model (respondents 1 and 3 in column 0, the ranked column
    1 in [5, 11), a format column 2 in [11, 14)); respondent 3 has two pool rows and runs out in round 2 (rows == -1)."""
    from vae_amd.elicit import ranking_curve_plan, round_posteriors
    field, rank_field, T = 0, 1, 14
    ents = [1, 3]
    pool = [[1, 5, 11], [3, 6, 11], [1, 7, 12], [1, 8, 11], [3, 9, 12], [1, 10, 11]]
    rows = [[2, 0, 5], [4, 1, -1]]
    hist = [[1, 9, 11], [3, 5, 12]]
    exclude = [[1, 6, 11], [3, 10, 12], [2, 7, 11], [3, 10, 11]]
    # relevant test rows: two contexts for respondent 1, one for respondent 3, one row of a non-respondent (left out),
    # and a duplicate row
    X_rel = [[1, 6, 12], [1, 10, 12], [1, 9, 12], [3, 7, 11], [3, 8, 11], [2, 5, 11], [1, 6, 12], [1, 7, 11]]
    t = lambda v: torch.tensor(v, dtype=torch.int64)
    plan = ranking_curve_plan(t(ents), t(rows), t(pool), t(hist), t(exclude), t(X_rel), field, rank_field, match, T)
    want = _brute_plan(ents, rows, pool, hist, exclude, X_rel, field, rank_field, match)
    got = _plan_as_lists(plan)
    assert plan["n_contexts"] == 3 and len(got) == len(want) == 4 * 3
    assert got == want
    # round-major: query q Nc + c
    assert plan["round"].tolist() == [0] * 3 + [1] * 3 + [2] * 3 + [3] * 3
    assert plan["resp"].tolist() == [0, 0, 1] * 4
    # the exclusions grow with the rounds and, with the format column matched, differ between a respondent's contexts
    by = {(w["round"], tuple(w["query"])): w["excl"] for w in want}
    if match == [0, 2]:
        assert by[(0, (1, 0, 11))] == [6, 9] and by[(3, (1, 0, 11))] == [5, 6, 9, 10]
        assert by[(0, (1, 0, 12))] == [] and by[(1, (1, 0, 12))] == [7]
        assert by[(3, (3, 0, 11))] == [6, 10] == by[(2, (3, 0, 11))]         # nothing asked in round 2: nothing added
    else:
        assert by[(0, (1, 0, 12))] == [6, 9] and by[(3, (1, 0, 12))] == [5, 6, 7, 9, 10]
    # without history, exclusions or asked rows round 0 has no exclusion at all
    bare = ranking_curve_plan(t(ents), t(rows), t(pool), None, None, t(X_rel), field, rank_field, match, T)
    assert got_rounds(bare, 0) == [[]] * 3 and _plan_as_lists(bare) == _brute_plan(ents, rows, pool, [], [], X_rel, field,
                                                                                 rank_field, match)
    # which theta row: the round-0 posterior for round 0, theta[:, q - 1] after
    U, Q, W = 2, 3, 4
    theta = torch.arange(U * Q * W, dtype=torch.float32).reshape(U, Q, W) + 100.0
    theta0 = torch.arange(U * W, dtype=torch.float32).reshape(U, W)
    post = round_posteriors(theta0, theta, plan["resp"], plan["round"])
    for j, w in enumerate(want):
        src = theta0[w["resp"]] if w["round"] == 0 else theta[w["resp"], w["round"] - 1]
        assert torch.equal(post[j], src), j
    # no rounds at all: only the round-0 posterior
    p0 = ranking_curve_plan(t(ents), torch.zeros(2, 0, dtype=torch.int64), t(pool), None, None, t(X_rel), field,
                            rank_field, match, T)
    assert p0["queries"].shape[0] == 3
    assert torch.equal(round_posteriors(theta0, theta[:, :0], p0["resp"], p0["round"]), theta0[p0["resp"]])


def got_rounds(plan, q):
    return [w["excl"] for w in _plan_as_lists(plan) if w["round"] == q]

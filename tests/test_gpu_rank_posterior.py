"""GPU: the field-form ranking under supplied posteriors (VFM.field_moments_posterior / rank_field_posterior /
rank_heldout_field_posterior / elicitation_ranking_curve_field; include/vfm_rank.h: the *_post_f32 entry points).

The oracle is the table path, tested on its own (test_gpu_rank_field*.py), on a second model with the same tables whose
rows of the ids in column post_field were overwritten with theta; where several queries share an id with different
theta rows the oracle loops over groups of queries with distinct ids.  Equality is bitwise on every output.

Shapes: d in {5, 16, 70} (70 crosses the 64-lane chunk of the prep's ordered sum and the KS = 16 padding), F in {2, 3}
with post_field below and above field, Q in {3, 257} (257 crosses UT = 256), n_cand in {63, 65} (IT = 64) and an
explicit candidate subset, both links, every strategy, k in {1, 10}, n_splits in {0, 3}."""
import numpy as np
import pytest
import torch

from test_gpu_rank_field import _model, _offsets

pytestmark = pytest.mark.gpu
DEV = "cuda"
OUT = ("items", "score", "logit_mean", "logit_var")
HELD = ("rank", "rank_neg", "n_eligible", "n_neg")
# (F, field, post_field): the one-column context of a two-field model both ways; post_field below and above field
LAYOUTS = [(2, 1, 0), (2, 0, 1), (3, 1, 0), (3, 1, 2), (3, 0, 2)]
N_POST = 300                     # entities of the post_field column: 257 queries with mostly distinct ids


# ---------------------------------------------------------------------------------------------------- helpers
def same(a, b):
    """Bit for bit, NaN in the same places (the padding of a list: item -1, score -inf, NaN moments)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if not a.dtype.is_floating_point:
        return torch.equal(a, b)
    na, nb = torch.isnan(a), torch.isnan(b)
    z = torch.zeros_like(a)
    return torch.equal(na, nb) and torch.equal(torch.where(na, z, a).view(torch.int32), torch.where(nb, z, b).view(torch.int32))


def sizes_of(F, field, post_field, n_cand):
    sizes = [7] * F
    sizes[field], sizes[post_field] = n_cand, N_POST
    return sizes


def queries_of(sizes, field, post_field, Q, rng):
    """Q contexts, their ids in column post_field distinct but for a few repeats (the same id, another theta row)."""
    off = _offsets(sizes)
    ctx = (rng.integers(0, np.array(sizes)[None, :], size=(Q, len(sizes))) + off[None, :-1]).astype(np.int64)
    ctx[:, post_field] = off[post_field] + rng.permutation(N_POST)[:Q]
    ctx[1] = ctx[0]                                                  # the same context twice ...
    if Q > 8:
        ctx[5, post_field] = ctx[4, post_field]                      # ... the same id in another context ...
        ctx[Q - 1] = ctx[0]                                          # ... and a third time past the first tile of queries
    ctx[:, field] = 0
    return ctx


def theta_of(Q, d, rng, scale=0.5):
    return torch.tensor(rng.standard_normal((Q, 2 * d + 2)) * scale, dtype=torch.float32)


def groups_of(ids):
    """The queries split into groups with distinct ids: group g holds the g-th occurrence of every id."""
    seen, occ = {}, []
    for i in ids.tolist():
        occ.append(seen.get(i, 0))
        seen[i] = occ[-1] + 1
    occ = np.array(occ)
    return [np.flatnonzero(occ == g) for g in range(occ.max() + 1)]


class Overwritten:
    """The oracle's model: the fixture's tables with the rows of `ids` holding `theta`; restored on exit."""

    def __init__(self, mo, ids, theta):
        self.mo, self.ids, self.theta = mo, torch.as_tensor(ids, device=DEV), theta.to(DEV)

    def __enter__(self):
        d = self.mo.d
        self.e = self.mo.entity_params.weight.data[self.ids].clone()
        self.b = self.mo.bias_params.weight.data[self.ids].clone()
        self.mo.entity_params.weight.data[self.ids] = self.theta[:, :2 * d]
        self.mo.bias_params.weight.data[self.ids] = self.theta[:, 2 * d:]
        self.mo.params_changed()
        return self.mo

    def __exit__(self, *a):
        self.mo.entity_params.weight.data[self.ids] = self.e
        self.mo.bias_params.weight.data[self.ids] = self.b
        self.mo.params_changed()


def oracle_rank(mo, ctx, theta, post_field, field, **kw):
    """rank_field on the overwritten tables, group by group, in the caller's row order."""
    out = None
    for g in groups_of(ctx[:, post_field]):
        with Overwritten(mo, ctx[g, post_field], theta[g]) as m2:
            r = m2.rank_field(torch.tensor(ctx[g]), field, **kw)
        if out is None:
            out = {key: torch.empty((len(ctx),) + r[key].shape[1:], dtype=r[key].dtype, device=DEV) for key in OUT}
        for key in OUT:
            out[key][torch.as_tensor(g, device=DEV)] = r[key]
    return out


def oracle_moments(mo, X, theta, post_field, field, **kw):
    out = [torch.empty(len(X), device=DEV) for _ in range(3)]
    for g in groups_of(X[:, post_field]):
        with Overwritten(mo, X[g, post_field], theta[g]) as m2:
            r = m2.field_moments(torch.tensor(X[g]), field, **kw)
        for o, v in zip(out, r):
            o[torch.as_tensor(g, device=DEV)] = v
    return out


def oracle_heldout(mo, ctx, pos_q, pos_i, theta, post_field, field, **kw):
    """rank_heldout_field on the overwritten tables, group by group: per query (items, rank, rank_neg, n_eligible,
    n_neg).  Every query has a positive, so every query of a group is one of the table form's distinct contexts."""
    res = [None] * len(ctx)
    for g in groups_of(ctx[:, post_field]):
        rows = []
        for q in g:
            for i in pos_i[pos_q == q]:
                r = ctx[q].copy()
                r[field] = i
                rows.append(r)
        with Overwritten(mo, ctx[g, post_field], theta[g]) as m2:
            r = m2.rank_heldout_field(torch.tensor(np.array(rows)), field, **kw)
        where = {tuple(c): j for j, c in enumerate(r["contexts"].cpu().tolist())}
        ptr = r["ptr"].cpu().tolist()
        for q in g:
            j = where[tuple(ctx[q].tolist())]
            a, b = ptr[j], ptr[j + 1]
            res[q] = (r["items"][a:b], r["rank"][a:b], r["rank_neg"][a:b], r["n_eligible"][j], r["n_neg"][j])
    return res


def check_heldout(h, want):
    ptr = h["ptr"].cpu().tolist()
    for q, w in enumerate(want):
        a, b = ptr[q], ptr[q + 1]
        assert torch.equal(h["items"][a:b], w[0]), q
        assert torch.equal(h["rank"][a:b], w[1]) and torch.equal(h["rank_neg"][a:b], w[2]), q
        assert int(h["n_eligible"][q]) == int(w[3]) and int(h["n_neg"][q]) == int(w[4]), q


def draw_positives(ctx, cand, excluded, rng):
    """(query_index, ids): one to four positives per query among its candidates that are not excluded."""
    pq, pi = [], []
    for q in range(len(ctx)):
        el = np.array([c for c in cand if (q, int(c)) not in excluded])
        n = min(len(el), int(rng.integers(1, 5)))
        pq += [q] * n
        pi += rng.choice(el, n, replace=False).tolist()
    return np.array(pq, np.int64), np.array(pi, np.int64)


# ---------------------------------------------------------------------------------------------------- 1. the oracle
@pytest.mark.parametrize("link,output", [("abs", "reg"), ("softplus", "class")])
@pytest.mark.parametrize("d", [5, 16, 70])
@pytest.mark.parametrize("F,field,post_field", LAYOUTS)
def test_posterior_forms_equal_the_overwritten_table_oracle(F, field, post_field, d, link, output):
    rng = np.random.default_rng(F * 1000 + d * 10 + field * 3 + post_field)
    strategies = ["top", "variance", "random"] + (["mean"] if output == "class" else [])
    for Q, n_cand, subset in ((3, 63, False), (257, 65, False), (257, 65, True)):
        sizes = sizes_of(F, field, post_field, n_cand)
        off = _offsets(sizes)
        m = _model(sizes, d, output=output, link=link, seed=d + F)
        mo = _model(sizes, d, output=output, link=link, seed=d + F)
        before = m._flat.clone()
        ctx = queries_of(sizes, field, post_field, Q, rng)
        theta = theta_of(Q, d, rng)
        all_c = np.arange(off[field], off[field + 1], dtype=np.int64)
        cand = np.sort(rng.choice(all_c, 40, replace=False)) if subset else all_c
        ckw = dict(candidates=torch.tensor(cand)) if subset else {}
        tctx = torch.tensor(ctx)
        # exclusions that remove a would-be winner: the best candidate of every other query, as full rows
        win = m.rank_field_posterior(tctx, theta, post_field, field, k=1, **ckw)["items"][:, 0].cpu().numpy()
        ex = ctx[::2].copy()
        ex[:, field] = win[::2]
        tex = torch.tensor(ex)
        by_ctx = {}
        for q in range(Q):
            by_ctx.setdefault(tuple(np.delete(ctx[q], field)), []).append(q)
        excluded = {(q, int(r[field])) for r in ex for q in by_ctx[tuple(np.delete(r, field))]}
        for strategy in strategies:
            for k, n_splits in ((1, 0), (10, 3)):
                kw = dict(k=k, strategy=strategy, seed=9, n_splits=n_splits, exclude=tex, **ckw)
                r = m.rank_field_posterior(tctx, theta, post_field, field, **kw)
                w = oracle_rank(mo, ctx, theta, post_field, field, **kw)
                for key in OUT:
                    assert same(r[key], w[key]), (Q, n_cand, subset, strategy, k, key)
                got = r["items"].cpu().numpy()
                assert not any(i in got[q] for q, i in excluded)                     # the would-be winners are gone
            # the returned moments are field_moments_posterior of the same rows
            items = r["items"]
            ok = (items >= 0).reshape(-1)
            X = tctx.to(DEV)[:, None, :].expand(-1, items.shape[1], -1).clone()
            X[:, :, field] = items
            X = X.reshape(-1, F)[ok]
            th = theta.to(DEV)[:, None, :].expand(-1, items.shape[1], -1).reshape(-1, 2 * d + 2)[ok]
            mm, vv, ss = m.field_moments_posterior(X, th, post_field, field, strategy=strategy, seed=9)
            assert same(mm, r["logit_mean"].reshape(-1)[ok]) and same(vv, r["logit_var"].reshape(-1)[ok])
            assert same(ss, r["score"].reshape(-1)[ok])
            X0, th0 = X[:Q].clone(), theta.to(DEV)
            X0[:, field] = torch.where(items[:, 0] >= 0, items[:, 0], X0.new_tensor(int(cand[0])))
            got0 = m.field_moments_posterior(X0, th0, post_field, field, strategy=strategy, seed=9)
            want0 = oracle_moments(mo, X0.cpu().numpy(), theta, post_field, field, strategy=strategy, seed=9)
            assert all(same(u, v) for u, v in zip(got0, want0))
            # held-out ranks
            pq, pi = draw_positives(ctx, cand, excluded, rng)
            for n_splits in (0, 3):
                hkw = dict(exclude=tex, strategy=strategy, seed=9, n_splits=n_splits, **ckw)
                h = m.rank_heldout_field_posterior(tctx, (torch.tensor(pq), torch.tensor(pi)), theta, post_field, field,
                                                   **hkw)
                assert torch.equal(h["contexts"].cpu(), tctx) and h["n_dropped"] == 0
                check_heldout(h, oracle_heldout(mo, ctx, pq, pi, theta, post_field, field, **hkw))
        # int32 ids in the moments form
        m32 = m.field_moments_posterior(X.to(torch.int32), th, post_field, field, strategy="top")
        m64 = m.field_moments_posterior(X, th, post_field, field, strategy="top")
        assert all(same(a, b) for a, b in zip(m32, m64))
        assert torch.equal(m._flat, before)                                            # the model is not modified


# ---------------------------------------------------------------------------------------------------- 2. never read
@pytest.mark.parametrize("F,field,post_field", [(2, 1, 0), (3, 1, 2)])
def test_the_table_rows_of_the_supplied_ids_are_never_read(F, field, post_field):
    d, Q = 16, 40
    rng = np.random.default_rng(7)
    sizes = sizes_of(F, field, post_field, 65)
    m = _model(sizes, d, seed=3)
    before = m._flat.clone()
    poisoned = _model(sizes, d, seed=3)                                # a clone, its rows of the ids set to NaN
    ctx = queries_of(sizes, field, post_field, Q, rng)
    ids = torch.tensor(np.unique(ctx[:, post_field]), device=DEV)
    poisoned.entity_params.weight.data[ids] = float("nan")
    poisoned.bias_params.weight.data[ids] = float("nan")
    poisoned.params_changed()
    theta, tctx = theta_of(Q, d, rng), torch.tensor(ctx)
    pq, pi = draw_positives(ctx, np.arange(_offsets(sizes)[field], _offsets(sizes)[field + 1]), set(), rng)
    pos = (torch.tensor(pq), torch.tensor(pi))
    X = ctx.copy()
    X[:, field] = _offsets(sizes)[field] + rng.integers(0, 65, Q)
    for strategy in ("top", "variance", "random"):
        a = m.rank_field_posterior(tctx, theta, post_field, field, k=10, strategy=strategy, seed=2)
        assert torch.equal(m._flat, before)
        b = poisoned.rank_field_posterior(tctx, theta, post_field, field, k=10, strategy=strategy, seed=2)
        assert all(same(a[key], b[key]) for key in OUT) and not torch.isnan(b["score"]).any()
        ha = m.rank_heldout_field_posterior(tctx, pos, theta, post_field, field, strategy=strategy, seed=2)
        assert torch.equal(m._flat, before)
        hb = poisoned.rank_heldout_field_posterior(tctx, pos, theta, post_field, field, strategy=strategy, seed=2)
        assert all(torch.equal(ha[key], hb[key]) for key in HELD)
        ma = m.field_moments_posterior(torch.tensor(X), theta, post_field, field, strategy=strategy, seed=2)
        assert torch.equal(m._flat, before)
        mb = poisoned.field_moments_posterior(torch.tensor(X), theta, post_field, field, strategy=strategy, seed=2)
        assert all(same(u, v) for u, v in zip(ma, mb)) and not torch.isnan(mb[0]).any()
    # the table form on the poisoned clone does read them: the poison is where the test says it is
    assert torch.isnan(poisoned.field_moments(torch.tensor(X), field)[0]).all()


# ---------------------------------------------------------------------------------------------------- 3. duplicate ids
def test_duplicate_ids_carry_their_own_posteriors():
    F, field, post_field, d = 3, 1, 0, 16
    rng = np.random.default_rng(11)
    sizes = sizes_of(F, field, post_field, 63)
    m = _model(sizes, d, seed=5)
    off = _offsets(sizes)
    ctx = np.repeat(np.array([[off[0] + 4, 0, off[2] + 1]], np.int64), 4, 0)          # one context, four posteriors
    theta = theta_of(4, d, rng, scale=1.0)
    kw = dict(k=10, strategy="top")
    r = m.rank_field_posterior(torch.tensor(ctx), theta, post_field, field, **kw)
    assert len({tuple(r["items"][q].tolist()) for q in range(4)}) == 4                # each query its own result
    perm = [2, 0, 3, 1]
    rp = m.rank_field_posterior(torch.tensor(ctx), theta[perm], post_field, field, **kw)
    for key in OUT:
        assert same(rp[key], r[key][perm])                                            # swapping theta swaps the results
    pos = (torch.arange(4).repeat_interleave(2), torch.tensor([off[1] + 3, off[1] + 40] * 4))
    h = m.rank_heldout_field_posterior(torch.tensor(ctx), pos, theta, post_field, field)
    hp = m.rank_heldout_field_posterior(torch.tensor(ctx), pos, theta[perm], post_field, field)
    assert torch.equal(hp["rank"].reshape(4, 2), h["rank"].reshape(4, 2)[perm])
    assert len({tuple(h["rank"].reshape(4, 2)[q].tolist()) for q in range(4)}) > 1
    # a query stands alone: the same row alone gives the same list
    one = m.rank_field_posterior(torch.tensor(ctx[2:3]), theta[2:3], post_field, field, **kw)
    assert all(same(one[key], r[key][2:3]) for key in OUT)
    # per-query exclusions hit their query only
    top = r["items"][:, 0]
    rq = m.rank_field_posterior(torch.tensor(ctx), theta, post_field, field, query_exclude=(torch.tensor([1]), top[1:2]),
                                **kw)
    assert int(rq["items"][1, 0]) == int(r["items"][1, 1]) and all(same(rq[key][[0, 2, 3]], r[key][[0, 2, 3]]) for key in OUT)


# ---------------------------------------------------------------------------------------------------- 4. a real session
def _session_case(output="reg", d=16):
    """A three-field model (respondents: column 0, ranked: column 1, formats: column 2), 4 respondents, a 6-row pool."""
    sizes = [6, 65, 3]
    off = _offsets(sizes)
    m = _model(sizes, d, output=output, seed=21, scale=0.4)
    pool = torch.tensor([[0, off[1] + 3, off[2]], [1, off[1] + 7, off[2] + 1], [0, off[1] + 9, off[2] + 1],
                         [2, off[1] + 11, off[2]], [0, off[1] + 20, off[2]], [4, off[1] + 30, off[2] + 2]])
    y = torch.tensor([4.5, 2.0, 3.0, 5.0, 1.0, 4.0])
    return sizes, off, m, pool, y


def test_theta_of_a_session_ranks_like_the_written_model():
    sizes, off, m, pool, y = _session_case()
    mo = _model(sizes, 16, seed=21, scale=0.4)
    before = m._flat.clone()
    kw = dict(field=0, strategy="variance", n_steps=20, lr=0.05, seed=3)
    r = m.elicit_field(pool, y, 3, write=False, return_theta=True, **kw)
    assert torch.equal(m._flat, before) and r["entities"].tolist() == [0, 1, 2, 4]
    mo.elicit_field(pool, y, 3, write=True, **kw)
    ctx = torch.tensor([[e, 0, off[2] + f] for e in (0, 1, 2, 4) for f in (0, 2)])
    theta = r["theta"][:, -1].repeat_interleave(2, 0)
    for strategy in ("top", "variance"):
        a = m.rank_field_posterior(ctx, theta, 0, 1, k=10, strategy=strategy)
        b = mo.rank_field(ctx, 1, k=10, strategy=strategy)
        assert all(same(a[key], b[key]) for key in OUT)
    assert torch.equal(m._flat, before)


# ---------------------------------------------------------------------------------------------------- 5. the curve
@pytest.mark.parametrize("exact,reset", [(False, False), (True, False), (True, True)])
def test_ranking_curve_equals_the_composed_loop(exact, reset):
    from vae_amd import elicit, foldin, rank
    sizes, off, m, pool, y = _session_case()
    d, Q, field, rank_field, ks = 16, 3, 0, 1, (1, 10)
    mo = _model(sizes, d, seed=21, scale=0.4)
    before = m._flat.clone()
    rng = np.random.default_rng(5)
    hist = (torch.tensor([[0, off[1] + 50, off[2]], [2, off[1] + 51, off[2] + 1]]), torch.tensor([3.0, 4.0]))
    exclude = torch.tensor([[0, off[1] + 40, off[2]], [1, off[1] + 41, off[2] + 1], [4, off[1] + 42, off[2]]])
    # test rows of the respondents (items 55 .. 64: in no pool row, history or exclusion) and of a stranger (5)
    X_test = torch.tensor([[e, off[1] + 55 + int(i), off[2] + int(f)] for e in (0, 1, 2, 4, 5)
                           for i, f in zip(rng.permutation(10)[:4], rng.integers(0, 3, 4))])
    y_test = torch.tensor(rng.choice([2.0, 4.0, 5.0], len(X_test)), dtype=torch.float32)
    y_test[::4] = 5.0                                                                  # every respondent has a relevant row
    skw = dict(history=hist, seed=4, reset=reset)
    if not exact:
        skw.update(n_steps=15, lr=0.05)
    strategies = ("random", "variance")
    got = m.elicitation_ranking_curve_field(pool, y, Q, field, X_test, y_test, rank_field, ks=ks, strategies=strategies,
                                            exact=exact, exclude=exclude, **skw)
    assert torch.equal(m._flat, before)
    session = m.elicit_field_exact if exact else m.elicit_field
    mine = X_test[:, field] != 5
    for s in strategies:
        r = session(pool, y, Q, field=field, strategy=s, write=False, return_theta=True, **skw)
        ents = r["entities"]
        if reset:
            theta0 = torch.zeros(len(ents), 2 * d + 2, device=DEV)
            theta0[:, d:2 * d] = foldin.prior_s(m.link)
            theta0[:, 2 * d + 1] = foldin.prior_s(m.link)
        else:
            theta0 = torch.cat([m.entity_params.weight.data[ents], m.bias_params.weight.data[ents]], 1)
        # the pieces the curve is made of, for the ranks
        plan = elicit.ranking_curve_plan(ents, r["rows"], pool.to(DEV), hist[0].to(DEV), exclude.to(DEV),
                                         X_test[y_test >= 4.0].to(DEV), field, rank_field, [0, 2], m.T)
        post = elicit.round_posteriors(theta0, r["theta"], plan["resp"], plan["round"])
        h = m.rank_heldout_field_posterior(plan["queries"], plan["pos"], post, field, rank_field,
                                           query_exclude=plan["excl"])
        Nc = plan["n_contexts"]
        assert got["n_queries"] == (Q + 1) * Nc and Nc >= 4
        for q in range(Q + 1):
            th = theta0 if q == 0 else r["theta"][:, q - 1]
            asked = r["rows"][:, :q].reshape(-1)
            E_q = torch.cat([exclude, hist[0], pool[asked[asked >= 0].cpu()]])
            with Overwritten(mo, ents, th) as m2:
                w = m2.rank_heldout_field(X_test[mine & (y_test >= 4.0)], rank_field, exclude=E_q)
                wm = m2.evaluate_ranking_field(X_test[mine], y_test[mine], rank_field, ks=ks, exclude=E_q)
            a, b = int(h["ptr"][q * Nc]), int(h["ptr"][(q + 1) * Nc])
            assert torch.equal(h["contexts"][q * Nc:(q + 1) * Nc], w["contexts"])
            assert torch.equal(h["items"][a:b], w["items"]) and torch.equal(h["rank"][a:b], w["rank"])
            assert torch.equal(h["rank_neg"][a:b], w["rank_neg"])
            assert torch.equal(h["n_eligible"][q * Nc:(q + 1) * Nc], w["n_eligible"])
            for key, v in wm.items():
                assert got[s][key][q] == v or (v != v and got[s][key][q] != got[s][key][q]), (s, q, key)
        assert set(got[s]) == set(wm) and all(len(v) == Q + 1 for v in got[s].values())
    assert torch.equal(m._flat, before)


# ---------------------------------------------------------------------------------------------------- 6. NaN queries
def _ops_rank(m, ctx, field, k, post=None, post_field=-1):
    """The two torch ops themselves (the Python layer refuses ids outside [0, T) before any launch)."""
    from vae_amd import _lib
    from vae_amd.foldin import field_range
    o = _lib.ops()
    lo, hi = field_range(m, field)
    Q = ctx.shape[0]
    ent, bia, scal = m._views(m._flat)
    out = [torch.empty(Q, k, dtype=torch.int64, device=DEV)] + [torch.empty(Q, k, device=DEV) for _ in range(3)]
    ws = torch.empty(max(o.rank_field_workspace_bytes(Q, hi - lo, m.F, m.d, k, 0, 0), 1), dtype=torch.uint8, device=DEV)
    if post is None:
        o.rank_field(ctx, field, None, None, hi - lo, lo, None, None, ent, bia, scal, ws, *out, k, 0, 0, 0, 0)
    else:
        o.rank_field_post(ctx, field, post, post_field, None, None, hi - lo, lo, None, None, ent, bia, scal, ws, *out, k,
                          0, 0, 0, 0)
    return out


def test_bad_ids_and_nan_posteriors_give_what_the_table_oracle_gives():
    F, field, post_field, d, Q = 3, 1, 0, 16, 6
    rng = np.random.default_rng(13)
    sizes = sizes_of(F, field, post_field, 65)
    m = _model(sizes, d, seed=8)
    mo = _model(sizes, d, seed=8)
    ctx = queries_of(sizes, field, post_field, Q, rng)
    theta = theta_of(Q, d, rng)
    # an id outside [0, T) in column post_field: a NaN query, as in the table form (nothing of it is ever returned)
    bad = ctx.copy()
    bad[2, post_field], bad[3, post_field] = m.T + 5, -1
    ok = [0, 1, 4, 5]
    a = _ops_rank(m, torch.tensor(bad, device=DEV), field, 10, theta.to(DEV), post_field)
    b = _ops_rank(m, torch.tensor(bad, device=DEV), field, 10)
    good = m.rank_field_posterior(torch.tensor(ctx), theta, post_field, field, k=10)
    for x, y, key in zip(a, b, OUT):
        assert same(x[[2, 3]], y[[2, 3]])                               # item -1, score -inf, NaN moments
        assert same(x[ok], good[key][ok])                               # the other queries are untouched by it
    assert (a[0][[2, 3]] == -1).all() and torch.isinf(a[1][[2, 3]]).all() and torch.isnan(a[2][[2, 3]]).all()
    X = torch.tensor(bad)
    X[:, field] = _offsets(sizes)[field] + 3
    mm = m.field_moments_posterior(X, theta, post_field, field, strategy="top")
    assert all(torch.isnan(v[[2, 3]]).all() and not torch.isnan(v[ok]).any() for v in mm)
    # a NaN in theta: the overwritten-table oracle
    th = theta.clone()
    th[1, 3], th[4, 2 * d + 1] = float("nan"), float("nan")
    for strategy in ("top", "variance"):
        r = m.rank_field_posterior(torch.tensor(ctx), th, post_field, field, k=10, strategy=strategy)
        w = oracle_rank(mo, ctx, th, post_field, field, k=10, strategy=strategy)
        assert all(same(r[key], w[key]) for key in OUT)
        assert (r["items"][1] == -1).all() and (r["items"][0] >= 0).all()
    pos = (torch.arange(Q), torch.full((Q,), int(_offsets(sizes)[field]) + 3))
    h = m.rank_heldout_field_posterior(torch.tensor(ctx), pos, th, post_field, field)
    check_heldout(h, oracle_heldout(mo, ctx, pos[0].numpy(), pos[1].numpy(), th, post_field, field))

"""Preference elicitation: closed-form predictive moments and the fused top-k ranking (include/vfm_rank.h).

The reference's caller of the posterior is select_next_question / predict_proba (vfm.py:1024-1057): every unasked
(user, item) pair of a pool is scored by the mean probability or the logit variance over S posterior samples and each
user's best pair is asked next.  Here the moments are the exact S -> infinity limit, in closed form
(`predictive_moments`), and a whole catalog is ranked per user in one fused kernel (`rank_items`: the scores are two
GEMMs on the fp32 MFMA, the top k stays on chip).  The calls go through torch.ops.vfm_hip; the exclusion lists are
built here with torch (plumbing).
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib, ops

STRATEGIES = {"top": 0, "variance": 1, "mean": 2, "random": 3}
MAX_K = 128
MAX_SPLITS = 64


def _seed64(seed: int) -> int:
    s = int(seed) & (2 ** 64 - 1)
    return s - 2 ** 64 if s >= 2 ** 63 else s          # (the op takes the 64 bits as a signed int)


def strategy_code(strategy: str) -> int:
    if strategy not in STRATEGIES:
        raise ValueError(f"strategy must be one of {sorted(STRATEGIES)}, not {strategy!r}")
    return STRATEGIES[strategy]


def _link_flags(link: str) -> int:
    return ops.FLAG_LINK_SOFTPLUS if link == "softplus" else 0


def flags_of(model) -> int:
    """The `flags` argument of every ranking op for this model."""
    return _link_flags(model.link)


def _score_args(model, strategy, k=None, n_splits=None, optional=False) -> int:
    """The one check of (strategy, k, n_splits) against the model; returns the strategy's code.  k, n_splits None: the
    form has no such argument; optional: strategy None asks for no score (code 0)."""
    code = 0 if optional and strategy is None else strategy_code(strategy)
    if strategy == "mean" and model.output != "class":
        raise ValueError("strategy 'mean' (closest to p = 0.5) needs a 'class' model")
    if k is not None and not 1 <= int(k) <= MAX_K:
        raise ValueError(f"k must lie in [1, {MAX_K}]")
    if n_splits is not None and not 0 <= int(n_splits) <= MAX_SPLITS:
        raise ValueError(f"n_splits must lie in [0, {MAX_SPLITS}]")
    return code


def _moment_outputs(x, scored: bool):
    m = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    return m, torch.empty_like(m), torch.empty_like(m) if scored else None


def predictive_moments(x, ent, bia, scal, link: str = "abs", strategy: Optional[str] = None, seed: int = 0):
    """(logit_mean [B], logit_var [B], score [B] or None) of the rows x [B, F] under the mean-field posterior."""
    ops._need_cuda(x, "x")
    x = x if x.dtype in (torch.int32, torch.int64) else x.to(torch.int64)
    m, v, sc = _moment_outputs(x, strategy is not None)
    _lib.ops().predictive_moments(x.contiguous(), ent, bia, scal, m, v, sc, _link_flags(link),
                                  strategy_code(strategy) if strategy is not None else 0, _seed64(seed))
    return m, v, sc


def exclusion_csr(users: torch.Tensor, exclude: torch.Tensor, T: int):
    """CSR of the (user, item) rows of `exclude` [R, 2] over the query users (distinct, any order): (ptr [U+1] int64,
    items [n] int64 ascending per user, duplicates dropped)."""
    su, order = torch.sort(users)
    ex = exclude.to(users.device, torch.int64)
    pos = torch.searchsorted(su, ex[:, 0].contiguous()).clamp_(max=max(su.numel() - 1, 0))
    hit = su[pos] == ex[:, 0] if su.numel() > 0 else torch.zeros_like(pos, dtype=torch.bool)
    q = order[pos[hit]]                                   # query position of each kept row
    key = torch.unique(q * T + ex[hit, 1])                # sorted: by query position, then item id
    qk = key // T
    counts = torch.bincount(qk, minlength=users.numel())
    ptr = torch.zeros(users.numel() + 1, dtype=torch.int64, device=users.device)
    torch.cumsum(counts, 0, out=ptr[1:])
    return ptr, (key - qk * T).contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# the preparation and launch path every ranking form shares: the candidates, the positives' eligibility, the two
# launchers.  A form is named by the leading arguments of its ops (`_pair_head`, `_field_head`).
# ---------------------------------------------------------------------------------------------------------------------
_ITEM_WORDS = ("item ids must lie in", "duplicate candidate items")
_FIELD_WORDS = ("candidate ids must lie in the field's range", "duplicate candidates")


def _candidates(values, lo: int, hi: int, dev, words=_FIELD_WORDS):
    """(cand sorted int64 or None, n_cand) of a candidates argument over the id range [lo, hi); None: the whole range.
    words: the wording of the range error and of the duplicate error."""
    if values is None:
        return None, hi - lo
    cand = torch.as_tensor(values).to(dev, torch.int64).reshape(-1)
    if cand.numel() and (int(cand.min()) < lo or int(cand.max()) >= hi):
        raise ValueError(f"{words[0]} [{lo}, {hi})")
    cand = torch.sort(cand).values
    if cand.numel() > 1 and bool((cand[1:] == cand[:-1]).any()):
        raise ValueError(words[1])
    return cand, cand.numel()


def _ineligible(pitems, pq, cand, eptr, ex_items, Q: int, T: int):
    """bad [n_pos] bool: positive j (id pitems[j] of query pq[j]) is no eligible candidate of its query -- outside `cand`
    (sorted; None: every id is a candidate) or in the query's list of the exclusion CSR (eptr [Q+1], ex_items; None:
    nothing excluded).  The queries are the users of the pair form, the contexts of the field form."""
    dev = pitems.device
    bad = torch.zeros(pitems.numel(), dtype=torch.bool, device=dev)
    if cand is not None:
        j = torch.searchsorted(cand, pitems).clamp_(max=max(cand.numel() - 1, 0))
        bad |= (cand[j] != pitems) if cand.numel() > 0 else torch.ones_like(bad)
    if eptr is not None:
        ekey = torch.repeat_interleave(torch.arange(Q, device=dev), eptr[1:] - eptr[:-1]) * T + ex_items   # sorted
        if ekey.numel():
            pkey = pq * T + pitems
            j = torch.searchsorted(ekey, pkey).clamp_(max=ekey.numel() - 1)
            bad |= ekey[j] == pkey
    return bad


def _apply_ineligible(bad, pptr, pitems, pq, Q: int, ineligible: str, describe):
    """(pptr, pitems, pq, n_dropped) without the positives marked in `bad`; ineligible 'raise': a ValueError with
    describe(j) for the first of them instead."""
    n_dropped = int(bad.sum())
    if n_dropped:
        if ineligible == "raise":
            raise ValueError(describe(int(torch.nonzero(bad)[0, 0])))
        keep = ~bad
        pitems, pq = pitems[keep].contiguous(), pq[keep]
        pptr = torch.zeros(Q + 1, dtype=torch.int64, device=pitems.device)
        torch.cumsum(torch.bincount(pq, minlength=Q), 0, out=pptr[1:])
    return pptr, pitems, pq, n_dropped


def _pair_head(users):
    return "", (users,)


def _field_head(ctx, field, kf, post=None, post_field=None):
    """The field form's leading op arguments: the table form or, with `post`, the form under supplied posteriors."""
    if post is None:
        return "_field", (ctx.contiguous(), field, ctx[:, kf].contiguous())
    return "_field_post", (ctx.contiguous(), field, post, post_field, ctx[:, kf].contiguous())


def _workspace(o, name, dev, *sizes):
    return torch.empty(max(getattr(o, name)(*sizes), 1), dtype=torch.uint8, device=dev)


def _launch_topk(model, head, Q, cand, n_cand, lo, ptr, ex_items, k, code, seed, n_splits):
    """Allocates the top-k outputs [Q, k] and the workspace, runs the form's ranking op, returns the outputs."""
    form, lead = head
    dev, k, n_splits = model.device, int(k), int(n_splits)
    model._fresh_params()
    ent, bia, scal = model._views(model._flat)
    f32 = dict(dtype=torch.float32, device=dev)
    out = {"items": torch.empty(Q, k, dtype=torch.int64, device=dev), "score": torch.empty(Q, k, **f32),
           "logit_mean": torch.empty(Q, k, **f32), "logit_var": torch.empty(Q, k, **f32)}
    o = _lib.ops()
    if form:
        ws = _workspace(o, "rank_field_workspace_bytes", dev, Q, n_cand, model.F, model.d, k, code, n_splits)
    else:
        ws = _workspace(o, "rank_workspace_bytes", dev, Q, n_cand, model.d, k, code, n_splits)
    getattr(o, "rank" + (form or "_items"))(*lead, cand, n_cand, lo, ptr, ex_items, ent, bia, scal, ws, *out.values(),
                                            *(() if form else (2,)), k, code, flags_of(model), _seed64(seed), n_splits)
    return out


def _launch_heldout(model, head, Q, cand, n_cand, lo, eptr, ex_items, pptr, pitems, code, seed, n_splits):
    """Allocates the held-out outputs (rank, rank_neg [n_pos]; n_eligible, n_neg [Q]) and the workspace, runs the form's
    evaluation op, returns the outputs."""
    form, lead = head
    dev, n_pos, n_splits = model.device, pitems.numel(), int(n_splits)
    model._fresh_params()
    ent, bia, scal = model._views(model._flat)
    i64 = dict(dtype=torch.int64, device=dev)
    out = {"rank": torch.empty(n_pos, **i64), "rank_neg": torch.empty(n_pos, **i64), "n_eligible": torch.empty(Q, **i64),
           "n_neg": torch.empty(Q, **i64)}
    o = _lib.ops()
    if form:
        ws = _workspace(o, "rank_eval_field_workspace_bytes", dev, Q, n_cand, n_pos, model.F, model.d, code, n_splits)
    else:
        ws = _workspace(o, "rank_eval_workspace_bytes", dev, Q, n_cand, n_pos, model.d, code, n_splits)
    getattr(o, "rank_heldout" + form)(*lead, cand, n_cand, lo, eptr, ex_items, pptr, pitems, ent, bia, scal, ws,
                                      *out.values(), *(() if form else (2,)), code, flags_of(model), _seed64(seed),
                                      n_splits)
    return out


def _pair_rows(x, name, N, T, dev):
    x = torch.as_tensor(x).to(dev, torch.int64)
    if x.dim() != 2 or x.shape[1] != 2:
        raise ValueError(f"{name} must be an [R, 2] tensor of (user, item) rows")
    if x.numel() and (int(x[:, 0].min()) < 0 or int(x[:, 0].max()) >= N or int(x[:, 1].min()) < N
                      or int(x[:, 1].max()) >= T):
        raise ValueError(f"{name} holds ids outside the user / item ranges")
    return x


def rank_items(model, users, k: int = 10, strategy: str = "top", items=None, exclude=None, seed: int = 0,
               n_splits: int = 0):
    """The k best candidate items of each query user (model.rank_items documents the arguments)."""
    ops._need_cuda(model._flat, "the model's parameters")
    if model.F != 2:
        raise ValueError("rank_items ranks (user, item) pairs: two-field models only")
    code = _score_args(model, strategy, k, n_splits)
    dev, N, T = model.device, model.N, model.T
    users = torch.as_tensor(users).to(dev, torch.int64).reshape(-1)
    if users.numel() and (int(users.min()) < 0 or int(users.max()) >= N):
        raise ValueError(f"user ids must lie in [0, {N})")
    uq, inv = torch.unique(users, return_inverse=True)       # (each distinct user ranked once)
    cand, n_cand = _candidates(items, N, T, dev, _ITEM_WORDS)
    ptr = ex_items = None
    if exclude is not None:
        ptr, ex_items = exclusion_csr(uq, _pair_rows(exclude, "exclude", N, T, dev), T)
    out = _launch_topk(model, _pair_head(uq), uq.numel(), cand, n_cand, N, ptr, ex_items, k, code, seed, n_splits)
    if uq.numel() != users.numel() or not bool((uq == users).all()):
        out = {key: val[inv] for key, val in out.items()}
    return out


def rank_heldout(model, pos, exclude=None, items=None, strategy: str = "top", seed: int = 0, n_splits: int = 0):
    """Exact full-catalog positions of held-out positives (model.rank_heldout documents the arguments and outputs)."""
    ops._need_cuda(model._flat, "the model's parameters")
    if model.F != 2:
        raise ValueError("rank_heldout ranks (user, item) pairs: two-field models only")
    code = _score_args(model, strategy, None, n_splits)
    dev, N, T = model.device, model.N, model.T
    pos = _pair_rows(pos, "pos", N, T, dev)
    users = torch.unique(pos[:, 0])                          # sorted: every user with a positive
    pptr, pitems = exclusion_csr(users, pos, T)              # (ascending per user, duplicates dropped)
    cand, n_cand = _candidates(items, N, T, dev, _ITEM_WORDS)
    U = users.numel()
    puser = torch.repeat_interleave(torch.arange(U, device=dev), pptr[1:] - pptr[:-1])
    eptr = ex_items = None
    if exclude is not None:
        eptr, ex_items = exclusion_csr(users, _pair_rows(exclude, "exclude", N, T, dev), T)
    _apply_ineligible(_ineligible(pitems, puser, cand, eptr, ex_items, U, T), pptr, pitems, puser, U, "raise",
                      lambda j: f"positive (user {int(users[puser[j]])}, item {int(pitems[j])}) is not an eligible "
                                "candidate (excluded, or outside `items`)")
    out = {"users": users, "ptr": pptr, "items": pitems, "user_index": puser}
    out.update(_launch_heldout(model, _pair_head(users), U, cand, n_cand, N, eptr, ex_items, pptr, pitems, code, seed,
                               n_splits))
    return out


def select_next_questions(model, pool, n: int = 1, strategy: str = "variance", seed: int = 0):
    """Per user of the pool [P, 2] of (user, item) rows, the indices of its n best rows under `strategy` (the score of
    rank_items, from the closed-form moments).  Ties go to the lower row index.  Returns (users [U'] ascending,
    rows [U', n] int64, -1 where a user has fewer than n rows)."""
    ops._need_cuda(model._flat, "the model's parameters")
    if model.F != 2:
        raise ValueError("select_next_questions: two-field models only")
    _score_args(model, strategy)
    if int(n) < 1:
        raise ValueError("n must be >= 1")
    pool = torch.as_tensor(pool).to(model.device, torch.int64).contiguous()
    if pool.dim() != 2 or pool.shape[1] != 2:
        raise ValueError("pool must be an [P, 2] tensor of (user, item) rows")
    if pool.numel() and (int(pool.min()) < 0 or int(pool.max()) >= model.T):
        raise ValueError(f"pool ids must lie in [0, {model.T})")
    model._fresh_params()
    ent, bia, scal = model._views(model._flat)
    _, _, score = predictive_moments(pool, ent, bia, scal, model.link, strategy, seed)
    return best_rows_per_entity(pool, score, 0, int(n))


def field_exclusion_csr(ctx: torch.Tensor, exclude: torch.Tensor, field: int, match_fields, T: int):
    """CSR of rank_field's exclusions over the query contexts ctx [Q, F] (any order): candidate c is excluded for query q
    when a row of `exclude` [R, F] holds c in column `field` and agrees with q on the columns `match_fields`.  Returns
    (ptr [Q+1] int64, items [n] int64 ascending per query, duplicates dropped).  The distinct keys are numbered by one
    `unique` over the key columns of queries and rows together; the per-key lists are exclusion_csr's, and every query
    takes a copy of its key's list."""
    dev, Q = ctx.device, ctx.shape[0]
    ex = exclude.to(dev, torch.int64)
    cols = list(match_fields)
    if cols:
        keys = torch.cat([ctx[:, cols], ex[:, cols]], 0)
        g = torch.unique(keys, dim=0, return_inverse=True)[1].reshape(-1)
    else:                                                                    # (no key column: every row matches every query)
        g = torch.zeros(Q + ex.shape[0], dtype=torch.int64, device=dev)
    gq, ge = g[:Q], g[Q:]
    ug, ginv = torch.unique(gq, return_inverse=True)                         # the keys the queries hold
    gptr, gitems = exclusion_csr(ug, torch.stack([ge, ex[:, field]], 1), T)
    counts = (gptr[1:] - gptr[:-1])[ginv]
    ptr = torch.zeros(Q + 1, dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, out=ptr[1:])
    qi = torch.repeat_interleave(torch.arange(Q, device=dev), counts)
    src = gptr[ginv[qi]] + (torch.arange(qi.numel(), device=dev) - ptr[qi])
    return ptr, gitems[src].contiguous()


def _field_arg(model, field):
    if isinstance(field, bool) or not isinstance(field, int) or not 0 <= field < model.F:
        raise ValueError(f"field must be an int in [0, {model.F})")
    if model.F < 2:
        raise ValueError("the field form needs a model with at least two fields")
    return field


def _key_field(model, field, key_field):
    ctx_cols = [f for f in range(model.F) if f != field]
    if key_field is None:
        return ctx_cols[0]
    if isinstance(key_field, bool) or not isinstance(key_field, int) or key_field not in ctx_cols:
        raise ValueError(f"key_field must be a context column, one of {ctx_cols}")
    return key_field


def _context_rows(model, x, name, field, check_field_column=False):
    """x [R, F] int64 on the model's device: context ids inside [0, T) and outside the ranked field's range (they would
    be candidates, not context), and -- for full rows -- column `field` inside that range."""
    from .foldin import field_range
    x = torch.as_tensor(x)
    if x.dtype.is_floating_point or x.dtype == torch.bool:
        raise ValueError(f"{name} must hold integer ids")
    x = x.to(model.device, torch.int64)
    if x.dim() != 2 or x.shape[1] != model.F:
        raise ValueError(f"{name} must be [R, {model.F}]")
    if x.shape[0]:
        lo, hi = field_range(model, field)
        p = torch.cat([x[:, :field], x[:, field + 1:]], 1)
        if int(p.min()) < 0 or int(p.max()) >= model.T:
            raise ValueError(f"{name}: context ids must lie in [0, {model.T})")
        if bool(((p >= lo) & (p < hi)).any()):
            raise ValueError(f"{name}: context columns hold ids of the ranked field's range [{lo}, {hi})")
        if check_field_column and (int(x[:, field].min()) < lo or int(x[:, field].max()) >= hi):
            raise ValueError(f"{name}: column {field} must lie in the field's range [{lo}, {hi})")
    return x


def _field_moments(model, X, field, strategy, seed, key_field, post=None):
    """field_moments (post None) and field_moments_posterior (post = (theta, post_field))."""
    field = _field_arg(model, field)
    kf = _key_field(model, field, key_field)
    code = _score_args(model, strategy, optional=True)
    x = torch.as_tensor(X)
    if x.dim() != 2 or x.shape[1] != model.F:
        raise ValueError(f"X must be [B, {model.F}]")
    if post is not None:
        post = (_posterior_args(model, post[0], post[1], field, x.shape[0], "X"), post[1])
    ops._need_cuda(model._flat, "the model's parameters")
    x = x.to(model.device)
    x = (x if x.dtype in (torch.int32, torch.int64) else x.to(torch.int64)).contiguous()
    model._fresh_params()
    ent, bia, scal = model._views(model._flat)
    m, v, sc = _moment_outputs(x, strategy is not None)
    qkey = x[:, kf].to(torch.int64).contiguous()
    tail = (qkey, ent, bia, scal, m, v, sc, flags_of(model), code, _seed64(seed))
    if post is None:
        _lib.ops().field_moments(x, field, *tail)
    else:
        _lib.ops().field_moments_post(x, field, *post, *tail)
    return m, v, sc


def field_moments(model, X, field, strategy: Optional[str] = None, seed: int = 0, key_field=None):
    """(logit_mean [B], logit_var [B], score [B] or None) of the rows X [B, F] in the field form: the bitwise definition
    of what rank_field returns (model.field_moments documents the arguments)."""
    return _field_moments(model, X, field, strategy, seed, key_field)


def select_next_questions_field(model, pool, field, n: int = 1, strategy: str = "variance", seed: int = 0, key_field=None):
    """select_next_questions in the field form: per entity of column `field` of the pool [P, F] of full rows, the indices
    of its n best rows under `strategy` (the score of field_moments for this field, seed and key_field).  Ties go to the
    lower row index.  Returns (entities [U'] ascending, rows [U', n] int64, -1 where an entity has fewer than n rows)."""
    field = _field_arg(model, field)
    _key_field(model, field, key_field)
    _score_args(model, strategy)
    if isinstance(n, bool) or int(n) < 1:
        raise ValueError("n must be >= 1")
    n = int(n)
    pool = _context_rows(model, pool, "pool", field, check_field_column=True).contiguous()
    _, _, score = field_moments(model, pool, field, strategy, seed, key_field)
    return best_rows_per_entity(pool, score, field, n)


def best_rows_per_entity(pool, score, field, n, drop_nan=False):
    """(entities [U'] ascending, rows [U', n] int64, -1 padded): per entity of column `field` of pool [P, F] the indices
    of its n best rows by score [P]; ties go to the lower row index.  A NaN score ranks last; with drop_nan it is never
    chosen."""
    dev = pool.device
    nan = torch.isnan(score)
    score = torch.nan_to_num(score, nan=-float("inf"))
    o1 = torch.sort(score, descending=True, stable=True).indices            # best first; ties: lower row first
    o2 = torch.sort(pool[o1, field], stable=True).indices                    # grouped by entity, order kept
    order = o1[o2]
    pe = pool[order, field]
    ents, counts = torch.unique_consecutive(pe, return_counts=True)
    start = torch.cumsum(counts, 0) - counts
    grp = torch.repeat_interleave(torch.arange(ents.numel(), device=dev), counts)
    rank = torch.arange(pe.numel(), device=dev) - start[grp]
    keep = rank < n
    if drop_nan:
        keep = keep & ~nan[order]
    rows = torch.full((ents.numel(), n), -1, dtype=torch.int64, device=dev)
    rows[grp[keep], rank[keep]] = order[keep]
    return ents, rows


def _query_contexts(model, contexts, name, field):
    ctx = _context_rows(model, contexts, name, field).clone()
    ctx[:, field] = 0                                          # (ignored by the kernels; zeroed so that duplicates meet)
    return ctx


def _rank_field(model, contexts, field, k, strategy, candidates, exclude, match_fields, key_field, seed, n_splits,
                post=None, query_exclude=None, merge=True):
    """rank_field (post None; merge: each distinct context is ranked once) and rank_field_posterior
    (post = (theta, post_field); every row its own query, which `query_exclude` names by index)."""
    from .foldin import field_range
    field = _field_arg(model, field)
    code = _score_args(model, strategy, k, n_splits)
    kf = _key_field(model, field, key_field)
    match = _match_arg(model, field, match_fields)
    lo, hi = field_range(model, field)
    ctx = _query_contexts(model, contexts, "contexts", field)
    if post is not None:
        post = (_posterior_args(model, post[0], post[1], field, ctx.shape[0]), post[1])
    cand, n_cand = _candidates(candidates, lo, hi, model.device)
    ex = _context_rows(model, exclude, "exclude", field, check_field_column=True) if exclude is not None else None
    qex = _query_pairs(model, query_exclude, "query_exclude", ctx.shape[0], lo, hi) if query_exclude is not None else None
    ops._need_cuda(model._flat, "the model's parameters")
    uq, inv = ctx, None
    if merge:
        uq, inv = torch.unique(ctx, dim=0, return_inverse=True)
        inv = inv.reshape(-1)
    ptr, ex_items = posterior_exclusions(model, uq, field, match, ex, qex, lo, hi)
    out = _launch_topk(model, _field_head(uq, field, kf, *(post or ())), uq.shape[0], cand, n_cand, lo, ptr, ex_items, k,
                       code, seed, n_splits)
    if merge and (uq.shape[0] != ctx.shape[0] or not bool((uq == ctx).all())):
        out = {key: val[inv] for key, val in out.items()}
    return out


def rank_field(model, contexts, field, k: int = 10, strategy: str = "top", candidates=None, exclude=None,
               match_fields=None, key_field=None, seed: int = 0, n_splits: int = 0):
    """The k best entities of `field` for each context row (model.rank_field documents the arguments)."""
    return _rank_field(model, contexts, field, k, strategy, candidates, exclude, match_fields, key_field, seed, n_splits)


def field_positive_csr(rows: torch.Tensor, field: int, T: int):
    """The positives of rank_heldout_field grouped by query: rows [P, F] int64 full rows (column `field` the positive
    candidate, the other columns its context; any device).  Returns (contexts [Q, F] -- the distinct contexts with column
    `field` zeroed, in the row order of torch.unique(dim=0) --, ptr [Q+1] int64, items [n] int64 ascending per query,
    duplicate rows dropped)."""
    x = rows.to(torch.int64)
    if x.shape[0] == 0:
        return x.clone(), torch.zeros(1, dtype=torch.int64, device=x.device), x.new_zeros(0)
    ids = x[:, field].clone()
    ctx = x.clone()
    ctx[:, field] = 0
    uq, inv = torch.unique(ctx, dim=0, return_inverse=True)
    q = torch.arange(uq.shape[0], device=x.device)
    ptr, items = exclusion_csr(q, torch.stack([inv.reshape(-1), ids], 1), T)
    return uq, ptr, items


def _rank_heldout_field(model, pos, field, exclude, candidates, match_fields, key_field, strategy, seed, n_splits,
                        ineligible, post=None, queries=None, query_exclude=None):
    """rank_heldout_field (post None: `pos` holds full rows, the queries are their distinct contexts) and
    rank_heldout_field_posterior (post = (theta, post_field): `queries` are given, `pos` and `query_exclude` name them by
    index)."""
    from .foldin import field_range
    field = _field_arg(model, field)
    code = _score_args(model, strategy, None, n_splits)
    if ineligible not in ("raise", "drop"):
        raise ValueError(f"ineligible must be 'raise' or 'drop', not {ineligible!r}")
    kf = _key_field(model, field, key_field)
    match = _match_arg(model, field, match_fields)
    dev, T = model.device, model.T
    lo, hi = field_range(model, field)
    if post is None:
        pos = _context_rows(model, pos, "pos", field, check_field_column=True)
        n_queries = 0                                          # (no argument names a query by index)
    else:
        ctx = _query_contexts(model, queries, "queries", field)
        n_queries = ctx.shape[0]
        post = (_posterior_args(model, post[0], post[1], field, n_queries, "queries"), post[1])
        pqi, pids = _query_pairs(model, pos, "pos", n_queries, lo, hi)
    cand, n_cand = _candidates(candidates, lo, hi, dev)
    ex = _context_rows(model, exclude, "exclude", field, check_field_column=True) if exclude is not None else None
    qex = _query_pairs(model, query_exclude, "query_exclude", n_queries, lo, hi) if query_exclude is not None else None
    ops._need_cuda(model._flat, "the model's parameters")
    if post is None:
        ctx, pptr, pitems = field_positive_csr(pos, field, T)
    else:
        pptr, pitems = query_csr(pqi, pids, n_queries, T)      # (ascending per query, duplicates dropped)
    Q = ctx.shape[0]
    pq = torch.repeat_interleave(torch.arange(Q, device=dev), pptr[1:] - pptr[:-1])
    eptr, ex_items = posterior_exclusions(model, ctx, field, match, ex, qex, lo, hi)

    def describe(j):
        if post is not None:
            return (f"positive {int(pitems[j])} of query {int(pq[j])} is not an eligible candidate of its query "
                    "(excluded, or outside `candidates`); ineligible='drop' removes such positives")
        row = ctx[pq[j]].clone()
        row[field] = pitems[j]
        return (f"positive row {row.tolist()} is not an eligible candidate of its context (excluded, or outside "
                "`candidates`); ineligible='drop' removes such rows")

    pptr, pitems, pq, n_dropped = _apply_ineligible(_ineligible(pitems, pq, cand, eptr, ex_items, Q, T), pptr, pitems, pq,
                                                    Q, ineligible, describe)
    out = {"contexts": ctx, "ptr": pptr, "items": pitems, "query_index": pq}
    out.update(_launch_heldout(model, _field_head(ctx, field, kf, *(post or ())), Q, cand, n_cand, lo, eptr, ex_items,
                               pptr, pitems, code, seed, n_splits))
    out["n_dropped"] = n_dropped
    return out


def rank_heldout_field(model, pos, field, exclude=None, candidates=None, match_fields=None, key_field=None,
                       strategy: str = "top", seed: int = 0, n_splits: int = 0, ineligible: str = "raise"):
    """Exact positions of held-out positives in their contexts' full rankings of one field (model.rank_heldout_field
    documents the arguments and outputs)."""
    return _rank_heldout_field(model, pos, field, exclude, candidates, match_fields, key_field, strategy, seed, n_splits,
                               ineligible)


def ranking_metrics(rank, rank_neg, ptr, n_neg, ks=(10,)):
    """Per-user top-k metrics from exact ranks (pure torch, any device).

    rank, rank_neg [P]: per positive, the number of eligible candidates resp. eligible negatives ranked above it (ties
    broken by item id, as rank_items orders them -- never counted 1/2); ptr [U+1]: the positives of user u are
    [ptr[u], ptr[u+1]); n_neg [U]: the user's eligible negatives.  Per user with at least one positive, for each k:
    hit@k (any positive in the top k), precision@k = hits / k, recall@k = hits / |Pos|,
    ndcg@k = sum_{rank < k} 1 / log2(rank + 2) / sum_{j < min(k, |Pos|)} 1 / log2(j + 2); and mrr = 1 / (1 + best rank),
    auc = 1 - mean_p rank_neg_p / n_neg (the fraction of (positive, negative) pairs ordered right; NaN if n_neg == 0).
    Returns (means, per_user): means = {metric: float}, the mean over users with a positive (auc: and a negative), plus
    "n_users"; per_user = {metric: [U] float64, NaN where the metric is undefined}."""
    ks = [int(k) for k in ks]
    if not ks or any(k <= 0 for k in ks):
        raise ValueError("ks must be a non-empty list of positive ints")
    rank = torch.as_tensor(rank).to(torch.int64).reshape(-1)
    dev = rank.device
    rank_neg = torch.as_tensor(rank_neg, device=dev).to(torch.int64).reshape(-1)
    ptr = torch.as_tensor(ptr, device=dev).to(torch.int64).reshape(-1)
    n_neg = torch.as_tensor(n_neg, device=dev).to(torch.int64).reshape(-1)
    U = ptr.numel() - 1
    counts = ptr[1:] - ptr[:-1]
    seg = torch.repeat_interleave(torch.arange(U, device=dev), counts)
    f64 = dict(dtype=torch.float64, device=dev)
    has = counts > 0
    nan = torch.full((U,), float("nan"), **f64)
    npos = counts.to(torch.float64)

    def seg_sum(v):
        return torch.zeros(U, **f64).index_add_(0, seg, v.to(torch.float64))

    per = {}
    disc = 1.0 / torch.log2(rank.to(torch.float64) + 2.0)
    kmax = max(ks)
    ideal = torch.cumsum(1.0 / torch.log2(torch.arange(kmax, **f64) + 2.0), 0)        # ideal[j] = sum_{i <= j}
    for k in ks:
        inside = rank < k
        hits = torch.zeros(U, dtype=torch.int64, device=dev).index_add_(0, seg, inside.to(torch.int64)).to(torch.float64)
        dcg = seg_sum(torch.where(inside, disc, torch.zeros_like(disc)))
        idcg = ideal[(torch.clamp(counts, max=k) - 1).clamp(min=0)]
        per[f"hit@{k}"] = torch.where(has, (hits > 0).to(torch.float64), nan)
        per[f"precision@{k}"] = torch.where(has, hits / k, nan)
        per[f"recall@{k}"] = torch.where(has, hits / npos.clamp(min=1), nan)
        per[f"ndcg@{k}"] = torch.where(has, dcg / idcg, nan)
    best = torch.full((U,), torch.iinfo(torch.int64).max, dtype=torch.int64, device=dev)
    best = best.scatter_reduce(0, seg, rank, reduce="amin")
    per["mrr"] = torch.where(has, 1.0 / (1.0 + best.to(torch.float64)), nan)
    frac = seg_sum(rank_neg) / npos.clamp(min=1)
    per["auc"] = torch.where(has & (n_neg > 0), 1.0 - frac / n_neg.to(torch.float64).clamp(min=1), nan)
    means = {}
    for key, v in per.items():
        ok = ~torch.isnan(v)
        means[key] = float(v[ok].mean()) if bool(ok.any()) else float("nan")
    means["n_users"] = int(has.sum())
    return means, per


# ---------------------------------------------------------------------------------------------------------------------
# the field form under supplied posteriors (include/vfm_rank.h: the *_post_f32 entry points): one context column's
# parameters come from the caller's theta rows, not from the model's tables, which are never written
# ---------------------------------------------------------------------------------------------------------------------
def _posterior_args(model, theta, post_field, field, n_rows, what="contexts"):
    """The checks of (theta, post_field) shared by the posterior forms (no GPU needed).  Returns theta [n_rows, 2d + 2]
    fp32, contiguous, on the model's device."""
    if isinstance(post_field, bool) or not isinstance(post_field, int) or not 0 <= post_field < model.F:
        raise ValueError(f"post_field must be an int in [0, {model.F})")
    if post_field == field:
        raise ValueError("post_field must differ from field: the posterior is a context column's, the ranked field's "
                         "parameters are the candidates'")
    if not isinstance(theta, torch.Tensor):
        raise ValueError("theta must be a torch tensor [Q, 2d + 2] of dtype float32")
    if theta.dtype != torch.float32:
        raise ValueError(f"theta must be float32, not {theta.dtype}")
    W = 2 * model.d + 2
    if theta.dim() != 2 or theta.shape[0] != n_rows or theta.shape[1] != W:
        raise ValueError(f"theta must be [{n_rows}, {W}] = [mu | s | mu_w | s_w], one row per row of {what}, not "
                         f"{list(theta.shape)}")
    return theta.to(model.device).contiguous()


def _match_arg(model, field, match_fields):
    ctx_cols = [f for f in range(model.F) if f != field]
    if match_fields is None:
        return ctx_cols
    match = sorted({int(f) for f in match_fields})
    if any(f not in ctx_cols for f in match):
        raise ValueError(f"match_fields must be context columns, a subset of {ctx_cols}")
    return match


def _query_pairs(model, pairs, name, Q, lo, hi):
    """(query_index [R], ids [R]) int64 on the model's device: query indices in [0, Q), ids in the ranked field's range."""
    if not isinstance(pairs, (tuple, list)) or len(pairs) != 2:
        raise ValueError(f"{name} must be a pair (query_index [R], ids [R])")
    qi, ids = torch.as_tensor(pairs[0]), torch.as_tensor(pairs[1])
    for t in (qi, ids):
        if t.dtype.is_floating_point or t.dtype == torch.bool:
            raise ValueError(f"{name} must hold integers")
    qi, ids = qi.to(model.device, torch.int64).reshape(-1), ids.to(model.device, torch.int64).reshape(-1)
    if qi.numel() != ids.numel():
        raise ValueError(f"{name}: one id per query index")
    if qi.numel():
        if int(qi.min()) < 0 or int(qi.max()) >= Q:
            raise ValueError(f"{name}: query indices must lie in [0, {Q})")
        if int(ids.min()) < lo or int(ids.max()) >= hi:
            raise ValueError(f"{name}: ids must lie in the field's range [{lo}, {hi})")
    return qi, ids


def query_csr(qi: torch.Tensor, ids: torch.Tensor, Q: int, T: int):
    """CSR over the queries 0 .. Q - 1 of the (query index, id) pairs: (ptr [Q+1] int64, items [n] int64 ascending per
    query, duplicates dropped)."""
    return exclusion_csr(torch.arange(Q, device=qi.device), torch.stack([qi, ids], 1), T)


def posterior_exclusions(model, ctx, field, match, exclude, query_exclude, lo, hi):
    """The exclusion CSR of the posterior forms over the queries ctx [Q, F] (every row a query): the rows of `exclude`
    matched on ids as rank_field matches them, united with the per-query pairs `query_exclude`.  (None, None) without
    either."""
    Q, T = ctx.shape[0], model.T
    qi = ids = None
    if exclude is not None:
        ptr, items = field_exclusion_csr(ctx, exclude, field, match, T)
        if query_exclude is None:
            return ptr, items
        qi = torch.repeat_interleave(torch.arange(Q, device=ctx.device), ptr[1:] - ptr[:-1])
        ids = items
    if query_exclude is not None:
        qi = query_exclude[0] if qi is None else torch.cat([qi, query_exclude[0]])
        ids = query_exclude[1] if ids is None else torch.cat([ids, query_exclude[1]])
    if qi is None:
        return None, None
    return query_csr(qi, ids, Q, T)


def field_moments_posterior(model, X, theta, post_field, field, strategy: Optional[str] = None, seed: int = 0,
                            key_field=None):
    """field_moments with column post_field's parameters taken from theta (model.field_moments_posterior documents the
    arguments)."""
    return _field_moments(model, X, field, strategy, seed, key_field, post=(theta, post_field))


def rank_field_posterior(model, contexts, theta, post_field, field, k: int = 10, strategy: str = "top", candidates=None,
                         exclude=None, match_fields=None, key_field=None, seed: int = 0, n_splits: int = 0,
                         query_exclude=None):
    """rank_field with column post_field's parameters taken from theta, every row its own query
    (model.rank_field_posterior documents the arguments)."""
    return _rank_field(model, contexts, field, k, strategy, candidates, exclude, match_fields, key_field, seed, n_splits,
                       post=(theta, post_field), query_exclude=query_exclude, merge=False)


def rank_heldout_field_posterior(model, queries, pos, theta, post_field, field, exclude=None, candidates=None,
                                 match_fields=None, key_field=None, strategy: str = "top", seed: int = 0,
                                 n_splits: int = 0, ineligible: str = "raise", query_exclude=None):
    """rank_heldout_field with column post_field's parameters taken from theta: the queries are given, the positives
    name their query by index (model.rank_heldout_field_posterior documents the arguments and outputs)."""
    return _rank_heldout_field(model, pos, field, exclude, candidates, match_fields, key_field, strategy, seed, n_splits,
                               ineligible, post=(theta, post_field), queries=queries, query_exclude=query_exclude)

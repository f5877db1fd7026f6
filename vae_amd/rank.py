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


def predictive_moments(x, ent, bia, scal, link: str = "abs", strategy: Optional[str] = None, seed: int = 0):
    """(logit_mean [B], logit_var [B], score [B] or None) of the rows x [B, F] under the mean-field posterior."""
    ops._need_cuda(x, "x")
    x = x if x.dtype in (torch.int32, torch.int64) else x.to(torch.int64)
    B = x.shape[0]
    m = torch.empty(B, dtype=torch.float32, device=x.device)
    v = torch.empty_like(m)
    sc = torch.empty_like(m) if strategy is not None else None
    _lib.ops().predictive_moments(x.contiguous(), ent, bia, scal, m, v, sc, ops.FLAG_LINK_SOFTPLUS if link == "softplus"
                                  else 0, strategy_code(strategy) if strategy is not None else 0, _seed64(seed))
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


def rank_items(model, users, k: int = 10, strategy: str = "top", items=None, exclude=None, seed: int = 0,
               n_splits: int = 0):
    """The k best candidate items of each query user (model.rank_items documents the arguments)."""
    ops._need_cuda(model._flat, "the model's parameters")
    code = strategy_code(strategy)
    if model.F != 2:
        raise ValueError("rank_items ranks (user, item) pairs: two-field models only")
    if strategy == "mean" and model.output != "class":
        raise ValueError("strategy 'mean' (closest to p = 0.5) needs a 'class' model")
    if not 1 <= int(k) <= MAX_K:
        raise ValueError(f"k must lie in [1, {MAX_K}]")
    if not 0 <= int(n_splits) <= MAX_SPLITS:
        raise ValueError(f"n_splits must lie in [0, {MAX_SPLITS}]")
    k = int(k)
    dev = model.device
    N, M, T = model.N, model.M, model.T
    users = torch.as_tensor(users).to(dev, torch.int64).reshape(-1)
    if users.numel() and (int(users.min()) < 0 or int(users.max()) >= N):
        raise ValueError(f"user ids must lie in [0, {N})")
    uq, inv = torch.unique(users, return_inverse=True)       # (each distinct user ranked once)
    cand, n_cand = None, M
    if items is not None:
        cand = torch.as_tensor(items).to(dev, torch.int64).reshape(-1)
        if cand.numel() and (int(cand.min()) < N or int(cand.max()) >= T):
            raise ValueError(f"item ids must lie in [{N}, {T})")
        cand = torch.sort(cand).values
        if cand.numel() > 1 and bool((cand[1:] == cand[:-1]).any()):
            raise ValueError("duplicate candidate items")
        n_cand = cand.numel()
    ptr = ex_items = None
    if exclude is not None:
        ex = torch.as_tensor(exclude).to(dev, torch.int64)
        if ex.dim() != 2 or ex.shape[1] != 2:
            raise ValueError("exclude must be an [R, 2] tensor of (user, item) rows")
        if ex.numel() and (int(ex[:, 0].min()) < 0 or int(ex[:, 0].max()) >= N or int(ex[:, 1].min()) < N
                           or int(ex[:, 1].max()) >= T):
            raise ValueError("exclude holds ids outside the user / item ranges")
        ptr, ex_items = exclusion_csr(uq, ex, T)
    model._fresh_params()
    ent, bia, scal = model._views(model._flat)
    U = uq.numel()
    f32 = dict(dtype=torch.float32, device=dev)
    out = {"items": torch.empty(U, k, dtype=torch.int64, device=dev), "score": torch.empty(U, k, **f32),
           "logit_mean": torch.empty(U, k, **f32), "logit_var": torch.empty(U, k, **f32)}
    o = _lib.ops()
    ws = torch.empty(max(o.rank_workspace_bytes(U, n_cand, model.d, k, code, int(n_splits)), 1), dtype=torch.uint8,
                     device=dev)
    o.rank_items(uq, cand, n_cand, N, ptr, ex_items, ent, bia, scal, ws, out["items"], out["score"], out["logit_mean"],
                 out["logit_var"], 2, k, code, ops.FLAG_LINK_SOFTPLUS if model.link == "softplus" else 0, _seed64(seed),
                 int(n_splits))
    if U != users.numel() or not bool((uq == users).all()):
        out = {key: val[inv] for key, val in out.items()}
    return out


def select_next_questions(model, pool, n: int = 1, strategy: str = "variance", seed: int = 0):
    """Per user of the pool [P, 2] of (user, item) rows, the indices of its n best rows under `strategy` (the score of
    rank_items, from the closed-form moments).  Ties go to the lower row index.  Returns (users [U'] ascending,
    rows [U', n] int64, -1 where a user has fewer than n rows)."""
    ops._need_cuda(model._flat, "the model's parameters")
    strategy_code(strategy)
    if model.F != 2:
        raise ValueError("select_next_questions: two-field models only")
    if strategy == "mean" and model.output != "class":
        raise ValueError("strategy 'mean' (closest to p = 0.5) needs a 'class' model")
    if int(n) < 1:
        raise ValueError("n must be >= 1")
    n = int(n)
    dev = model.device
    pool = torch.as_tensor(pool).to(dev, torch.int64).contiguous()
    if pool.dim() != 2 or pool.shape[1] != 2:
        raise ValueError("pool must be an [P, 2] tensor of (user, item) rows")
    if pool.numel() and (int(pool.min()) < 0 or int(pool.max()) >= model.T):
        raise ValueError(f"pool ids must lie in [0, {model.T})")
    model._fresh_params()
    ent, bia, scal = model._views(model._flat)
    _, _, score = predictive_moments(pool, ent, bia, scal, model.link, strategy, seed)
    score = torch.nan_to_num(score, nan=-float("inf"))
    o1 = torch.sort(score, descending=True, stable=True).indices            # best first; ties: lower row first
    o2 = torch.sort(pool[o1, 0], stable=True).indices                        # grouped by user, order kept
    order = o1[o2]
    pu = pool[order, 0]
    users, counts = torch.unique_consecutive(pu, return_counts=True)
    start = torch.cumsum(counts, 0) - counts
    grp = torch.repeat_interleave(torch.arange(users.numel(), device=dev), counts)
    rank = torch.arange(pu.numel(), device=dev) - start[grp]
    keep = rank < n
    rows = torch.full((users.numel(), n), -1, dtype=torch.int64, device=dev)
    rows[grp[keep], rank[keep]] = order[keep]
    return users, rows

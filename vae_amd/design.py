"""Target-aware elicitation: ask the question that most reduces the predictive variance over a target set
(include/vfm_design.h; DESIGN.md §4 "Target-aware elicitation").

For a 'reg' model the scales of the exact fold-in's optimum do not depend on the answers, so the posterior variance a
question would leave behind is known before it is asked.  The score of a candidate is the expected drop of the mean
predictive variance over the respondent's target contexts (Cohn's ALC, A-optimal design under the mean-field
posterior), a closed form of O(d) per candidate.  This module checks the arguments, builds the per-respondent lists of
the pool, the history and the targets (stable sorts: the caller's order is kept within a respondent) and one operand
per distinct context of all three; the scores are one HIP launch (torch.ops.vfm_hip.design_scores) and the sessions
one more (design_elicit), beside the operand passes.
"""
from __future__ import annotations

import torch

from . import _lib, elicit, ops

STRATEGY = "design"                      # the name the exact curves route here (rank.STRATEGIES does not hold it)


def _history_rows(history, F):
    """history, the pair (X [H, F], y [H]) of the sessions; the score does not read y."""
    return None if history is None else elicit._history_pair(history, F)


def check_args(model, pool, y_pool, n_questions, field, targets, history, kl_weight):
    """Validate a call (no GPU needed): the exact session's checks ('reg', kl_weight > 0 and finite, F >= 2, the pool and
    the history), then the targets.  y_pool None: a scores call.  Returns (pool [P, F], y_pool [P], hist_x, hist_y,
    targets [R, F] or None, field) on the model's device."""
    from .rank import _context_rows
    if y_pool is None:
        p = torch.as_tensor(pool)
        y_pool = torch.zeros(p.shape[0] if p.dim() else 0, dtype=torch.float32)
    x, y, hx, hy, _, field, _ = elicit.check_args_field_exact(model, pool, y_pool, n_questions, field, "variance",
                                                              _history_rows(history, model.F), kl_weight,
                                                              None)
    tx = None
    if targets is not None:
        tx = _context_rows(model, targets, "targets", field, check_field_column=True)
        if tx.shape[0] and not bool(torch.isin(tx[:, field], x[:, field]).all()):
            raise ValueError("targets hold respondents without a pool row")
    return x, y, hx, hy, tx, field


def _lists(x, y, hx, hy, tx, field):
    """The per-respondent lists and the operand table of pool, history and targets together: dict(order, ents, ptr, px,
    ys, hptr, hxs, hys, tptr, op_x, pool_op, hist_op, tgt_op).  targets None: each respondent's own pool rows."""
    order, ents, ptr = elicit.pool_lists(x, field)
    px, ys = x[order].contiguous(), y[order].contiguous()
    P = px.shape[0]
    hptr = hxs = hys = hist_op = None
    if hx is not None and hx.shape[0]:
        horder, hptr = elicit.history_lists(ents, hx, field)
        hxs, hys = hx[horder].contiguous(), hy[horder].contiguous()
    H = 0 if hxs is None else hxs.shape[0]
    if tx is None:
        txs, tptr = None, ptr
    else:
        torder, tptr = elicit.history_lists(ents, tx, field)
        txs = tx[torder]
    parts = [px] + ([hxs] if hxs is not None else []) + ([txs] if txs is not None else [])
    ctx = torch.cat(parts).clone()                                    # one operand per DISTINCT context: it is frozen
    ctx[:, field] = 0
    op_x, inv = torch.unique(ctx, dim=0, return_inverse=True)
    inv = inv.reshape(-1)
    pool_op = inv[:P].contiguous()
    if hxs is not None:
        hist_op = inv[P:P + H].contiguous()
    tgt_op = pool_op if txs is None else inv[P + H:].contiguous()
    return dict(order=order, ents=ents, ptr=ptr, px=px, ys=ys, hptr=hptr, hxs=hxs, hys=hys, tptr=tptr,
                op_x=op_x.contiguous(), pool_op=pool_op, hist_op=hist_op, tgt_op=tgt_op)


def _flags(model):
    return ops.FLAG_LINK_SOFTPLUS if model.link == "softplus" else 0


def scores(model, pool, field, targets=None, history=None, kl_weight=1.0):
    """VFM.design_scores_field: [P] fp32, the score of every pool row in the caller's order."""
    x, y, hx, hy, tx, field = check_args(model, pool, None, 0, field, targets, history, kl_weight)
    ops._need_cuda(model._flat, "the model's parameters")
    dev, d = model.device, model.d
    L = _lists(x, y, hx, hy, tx, field)
    U, P = L["ents"].numel(), L["px"].shape[0]
    out = torch.full((P,), float("nan"), dtype=torch.float32, device=dev)
    if U:
        o = _lib.ops()
        ws = torch.empty(max(o.design_workspace_bytes(U, P, L["op_x"].shape[0], d, -1), 1), dtype=torch.uint8, device=dev)
        model._fresh_params()
        ent, bia, scal = model._views(model._flat)
        o.design_scores(L["ents"], L["ptr"], L["px"], L["hptr"], L["hist_op"], L["tptr"], L["tgt_op"], L["op_x"],
                        L["pool_op"], ent, bia, scal, ws, out, field, _flags(model), float(kl_weight))
    return elicit.to_caller_order(out, L["order"])


def select_next_questions(model, pool, field, n=1, targets=None, history=None, kl_weight=1.0):
    """VFM.select_next_questions_design_field: (entities [U'] ascending, rows [U', n] int64, -1 padded), the n best rows
    of each respondent by the design score; ties go to the lower row, NaN is never chosen."""
    from .rank import best_rows_per_entity
    if isinstance(n, bool) or int(n) < 1:
        raise ValueError("n must be >= 1")
    sc = scores(model, pool, field, targets, history, kl_weight)
    x = torch.as_tensor(pool).to(model.device, torch.int64)
    return best_rows_per_entity(x, sc, field, int(n), drop_nan=True)


def run_field_design(model, pool, y_pool, n_questions, field=0, targets=None, history=None, kl_weight=1.0, reset=False,
                     write=False, return_moments=False, return_theta=False, lds_dim=-1):
    """The design sessions of every entity of column `field` of the pool (VFM.elicit_field_design documents the
    arguments and the result): the lists above and one call of torch.ops.vfm_hip.design_elicit."""
    x, y, hx, hy, tx, field = check_args(model, pool, y_pool, n_questions, field, targets, history, kl_weight)
    if int(lds_dim) < -1:
        raise ValueError("lds_dim must be -1 or >= 0")
    ops._need_cuda(model._flat, "the model's parameters")
    dev, d, Q = model.device, model.d, int(n_questions)
    L = _lists(x, y, hx, hy, tx, field)
    ents = L["ents"]
    U, P = ents.numel(), L["px"].shape[0]
    out_row, score, loss, theta, mean, var = elicit._outputs(dev, U, Q, P, d, return_theta, return_moments)
    res = {"entities": ents}
    if U:
        o = _lib.ops()
        ws = torch.empty(max(o.design_workspace_bytes(U, P, L["op_x"].shape[0], d, int(lds_dim)), 1), dtype=torch.uint8,
                         device=dev)
        model._fresh_params()
        ent, bia, scal = model._views(model._flat)
        o.design_elicit(ents, L["ptr"], L["px"], L["ys"], L["hptr"], L["hxs"], L["hys"], L["hist_op"], L["tptr"],
                        L["tgt_op"], L["op_x"], L["pool_op"], ent, bia, scal, ws, out_row, score, loss, theta, mean, var,
                        field, Q, _flags(model), int(bool(reset)), int(bool(write)), int(lds_dim), float(kl_weight))
        if write:
            model.params_changed()      # (rows written outside the step kernels: derived caches are stale)
    return elicit._result(res, L["order"], out_row, score, loss, theta, mean, var)


def session_for(strategy, session, kw):
    """The runner and options of one strategy of an exact curve: "design" goes to run_field_design with the options it
    takes (targets among them; seed and key_field are the other strategies'), every other name to `session` without
    `targets`.  `session` must be elicit.run_field_exact for "design" to be a name at all (the curves check that)."""
    if strategy == STRATEGY:
        kw = {k: v for k, v in kw.items() if k not in ("seed", "key_field")}
        return (lambda model, pool, y_pool, n_questions, field=0, strategy=None, **k:
                run_field_design(model, pool, y_pool, n_questions, field, **k)), kw
    return session, {k: v for k, v in kw.items() if k != "targets"}

"""Target-aware elicitation: ask the question that most reduces the predictive variance over a target set
(include/vfm_design.h; DESIGN.md §4 "Target-aware elicitation").

For a 'reg' model the scales of the exact fold-in's optimum do not depend on the answers, so the posterior variance a
question would leave behind is known before it is asked.  The score of a candidate is the expected drop of the mean
predictive variance over the respondent's target contexts (Cohn's ALC, A-optimal design under the mean-field
posterior), a closed form of O(d) per candidate.  This module checks the arguments; elicit.field_lists builds the
per-respondent lists of the pool, the history and the targets (stable sorts: the caller's order is kept within a
respondent) and one operand per distinct context of all three; the scores are one HIP launch
(torch.ops.vfm_hip.design_scores) and the sessions one more (design_elicit, through elicit.run_field_session), beside
the operand passes.

With `priors` (a sweep.GroupPriors) the scales are those of the optimum under the respondents' field prior,
v_k(S) = kl / (kl lam_k + prec S), and the sessions fold under it (include/vfm_elicit_prior.h: design_scores_prior,
design_elicit_prior); priors=None is the parent op itself.
"""
from __future__ import annotations

import torch

from . import _lib, elicit, foldin, ops, sweep

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


def scores(model, pool, field, targets=None, history=None, kl_weight=1.0, priors=None):
    """VFM.design_scores_field: [P] fp32, the score of every pool row in the caller's order."""
    x, y, hx, hy, tx, field = check_args(model, pool, None, 0, field, targets, history, kl_weight)
    sweep.check_priors(model, priors)
    ops._need_cuda(model._flat, "the model's parameters")
    dev, d = model.device, model.d
    L = elicit.field_lists(x, y, hx, hy, field, tx)
    U, P = L["ents"].numel(), L["px"].shape[0]
    out = torch.full((P,), float("nan"), dtype=torch.float32, device=dev)
    if U:
        o = _lib.ops()
        ws = torch.empty(max(o.design_workspace_bytes(U, P, L["op_x"].shape[0], d, -1), 1), dtype=torch.uint8, device=dev)
        model._fresh_params()
        ent, bia, scal = model._views(model._flat)
        call, mid = ((o.design_scores, ()) if priors is None else
                     (o.design_scores_prior, (priors.row(int(field)).to(dev),)))
        call(L["ents"], L["ptr"], L["px"], L["hptr"], L["hist_op"], L["tptr"], L["tgt_op"], L["op_x"], L["pool_op"], ent,
             bia, scal, ws, out, *mid, field, elicit.link_flags(model), float(kl_weight))
    return elicit.to_caller_order(out, L["order"])


def select_next_questions(model, pool, field, n=1, targets=None, history=None, kl_weight=1.0, priors=None):
    """VFM.select_next_questions_design_field: (entities [U'] ascending, rows [U', n] int64, -1 padded), the n best rows
    of each respondent by the design score; ties go to the lower row, NaN is never chosen."""
    from .rank import best_rows_per_entity
    if isinstance(n, bool) or int(n) < 1:
        raise ValueError("n must be >= 1")
    sc = scores(model, pool, field, targets, history, kl_weight, priors)
    x = torch.as_tensor(pool).to(model.device, torch.int64)
    return best_rows_per_entity(x, sc, field, int(n), drop_nan=True)


def run_field_design(model, pool, y_pool, n_questions, field=0, targets=None, history=None, kl_weight=1.0, reset=False,
                     write=False, return_moments=False, return_theta=False, lds_dim=-1, priors=None):
    """The design sessions of every entity of column `field` of the pool (VFM.elicit_field_design documents the
    arguments and the result): elicit.run_field_session with the targets' lists and torch.ops.vfm_hip.design_elicit
    (with priors: design_elicit_prior)."""
    x, y, hx, hy, tx, field = check_args(model, pool, y_pool, n_questions, field, targets, history, kl_weight)
    sweep.check_priors(model, priors)
    foldin._check_lds_dim(lds_dim)
    return elicit.run_field_session(
        model, x, y, hx, hy, field, n_questions,
        lambda o, U, P, H, n_ops, d: o.design_workspace_bytes(U, P, n_ops, d, int(lds_dim)), "design_elicit",
        (field, int(n_questions), elicit.link_flags(model), int(bool(reset)), int(bool(write)), int(lds_dim),
         float(kl_weight)), write, return_moments, return_theta, targets=tx, priors=priors)


def session_for(strategy, session, kw):
    """The runner and options of one strategy of an exact curve: "design" goes to run_field_design with the options it
    takes (targets among them; seed and key_field are the other strategies'), every other name to `session` without
    `targets`.  `session` must be elicit.run_field_exact for "design" to be a name at all (the curves check that)."""
    if strategy == STRATEGY:
        kw = {k: v for k, v in kw.items() if k not in ("seed", "key_field")}
        return (lambda model, pool, y_pool, n_questions, field=0, strategy=None, **k:
                run_field_design(model, pool, y_pool, n_questions, field, **k)), kw
    return session, {k: v for k, v in kw.items() if k != "targets"}

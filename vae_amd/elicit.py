"""Elicitation sessions: ask, fold in and ask again, every round of every user in one launch (include/vfm_elicit.h).

The reference's interactive experiment (vfm.py:1236-1251) asks every test user a number of questions: the next question
is picked by a strategy from the user's current posterior, the answer is taken, and the user's parameters alone are
refitted.  `VFM.select_next_questions` and `VFM.fold_in` are the two halves; this module runs the whole loop for all
users inside one kernel ("Elicitation sessions").  It checks the arguments, builds the per-user lists of
the pool and of the history once (stable sorts: the caller's order is kept within a user) and maps the results back to
the caller's pool order; the sessions themselves are one HIP launch (plus one operand pass for the closed form)
through torch.ops.vfm_hip.elicit.  `run_field` is the same for the entities of any one column of a model with any
number of fields (vfm_elicit_field_f32): full rows, one operand per distinct context.  `run_field_exact` is the field
form with each round's Adam fit replaced by the exact fold-in's closed-form optimum (vfm_elicit_solve_f32), and
`run_field_bound` the same for 'class' models with the bound fold-in's rounds (include/vfm_bound.h: vfm_elicit_bound_f32).
`run_field_implicit` is the exact form for a two-field click model: each round's fold is the optimum over EVERY
(respondent, partner) pair, the objective fit_implicit trains under (include/vfm_elicit_implicit.h).
The field forms, design.run_field_design among them, are their argument checks and one call of `run_field_session`
over the lists of `field_lists`; SESSION_KINDS says which of them the curves run under which strategy names.

The exact, bound and design sessions take `priors` (a sweep.GroupPriors, what fit_exact / fit_bound learn with
learn_priors=True): every round's fold then runs under the respondents' field prior, `reset` starts a respondent at it
(foldin.prior_theta) and the design score is taken under it (include/vfm_elicit_prior.h; DESIGN.md §4 "Sessions under
learnt priors").  priors=None is the parent op itself.  The Adam sessions (`run`, `run_field`) keep N(0, 1) and take
no priors.
"""
from __future__ import annotations

import math

import torch

from . import _lib, foldin, ops, sweep
from .rank import _seed64, strategy_code

MAX_ROUNDS = _lib.ELICIT_MAX_ROUNDS


def _check_questions(model, strategy, n_questions):
    """The strategy / n_questions checks of both forms (after strategy_code)."""
    if strategy == "mean" and model.output != "class":
        raise ValueError("strategy 'mean' (closest to p = 0.5) needs a 'class' model")
    if isinstance(n_questions, bool) or not isinstance(n_questions, int) or not 0 <= n_questions <= MAX_ROUNDS:
        raise ValueError(f"n_questions must be an int in [0, {MAX_ROUNDS}]")


def _history_pair(history, width):
    if not isinstance(history, (tuple, list)) or len(history) != 2:
        raise ValueError(f"history must be a pair (X [H, {width}], y [H])")
    return history


def check_args(model, pool, y_pool, n_questions, strategy, history, n_steps, lr, objective, n_samples, kl_weight):
    """Validate a session call (no GPU needed).  Returns (pool [P, 2] int64, y_pool [P] fp32, hist_x [H, 2] or None,
    hist_y [H] or None, objective name, strategy code) on the model's device."""
    code = strategy_code(strategy)
    if model.F != 2:
        raise ValueError("elicit: two-field models only")
    _check_questions(model, strategy, n_questions)
    pool = torch.as_tensor(pool)
    if pool.dim() != 2 or pool.shape[1] != 2:
        raise ValueError("pool must be an [P, 2] tensor of (user, item) rows")
    x, y, objective = foldin.check_args(model, pool, y_pool, 0, objective, n_samples, n_steps, lr, kl_weight)
    hx = hy = None
    if history is not None:
        hx = torch.as_tensor(_history_pair(history, 2)[0])
        if hx.dim() != 2 or hx.shape[1] != 2:
            raise ValueError("history X must be an [H, 2] tensor of (user, item) rows")
        hx, hy, _ = foldin.check_args(model, hx, history[1], 0, objective, n_samples, n_steps, lr, kl_weight)
        if hx.shape[0] and not bool(torch.isin(hx[:, 0], x[:, 0]).all()):
            raise ValueError("history holds users without a pool row")
    return x, y, hx, hy, objective, code


def pool_lists(pool, col=0):
    """Stable sort of the pool rows by user (column `col`): (order [P] -- position in the sorted pool -> caller's row
    index --, users [U] ascending, ptr [U + 1])."""
    order = torch.sort(pool[:, col], stable=True).indices
    users, counts = torch.unique_consecutive(pool[order, col], return_counts=True)
    ptr = torch.zeros(users.numel() + 1, dtype=torch.int64, device=pool.device)
    torch.cumsum(counts, 0, out=ptr[1:])
    return order, users.contiguous(), ptr


def history_lists(users, hx, col=0):
    """The history rows grouped by the session users (stable: given order kept per user): (order [H], ptr [U + 1])."""
    order = torch.sort(hx[:, col], stable=True).indices
    pos = torch.searchsorted(users, hx[order, col].contiguous())
    counts = torch.bincount(pos, minlength=users.numel())
    ptr = torch.zeros(users.numel() + 1, dtype=torch.int64, device=hx.device)
    torch.cumsum(counts, 0, out=ptr[1:])
    return order, ptr


def rows_to_caller(out_row, order):
    """out_row [U, Q] (positions in the sorted pool, -1 padded) as indices into the caller's pool."""
    if order.numel() == 0:
        return out_row.clone()
    return torch.where(out_row >= 0, order[out_row.clamp(min=0)], out_row)


def to_caller_order(v, order):
    """v [.., P] over the sorted pool -> the same over the caller's pool."""
    out = torch.empty_like(v)
    out[..., order] = v
    return out


def _outputs(dev, U, Q, P, d, return_theta, return_moments):
    """The outputs of a session launch: out_row, score, loss [U, Q] (padded: -1, NaN), theta [U, Q, 2d + 2] or None,
    mean and var [Q + 1, P] or None."""
    f32 = dict(dtype=torch.float32, device=dev)
    out_row = torch.full((U, Q), -1, dtype=torch.int64, device=dev)
    score, loss = torch.full((U, Q), float("nan"), **f32), torch.full((U, Q), float("nan"), **f32)
    theta = torch.empty(U, Q, 2 * d + 2, **f32) if return_theta else None
    mean = torch.empty(Q + 1, P, **f32) if return_moments else None
    var = torch.empty(Q + 1, P, **f32) if return_moments else None
    return out_row, score, loss, theta, mean, var


def _result(res, order, out_row, score, loss, theta, mean, var):
    """The session's outputs added to res, rows and moments mapped back to the caller's pool order."""
    res.update(rows=rows_to_caller(out_row, order), score=score, loss=loss)
    if theta is not None:
        res["theta"] = theta
    if mean is not None:
        res["logit_mean"], res["logit_var"] = to_caller_order(mean, order), to_caller_order(var, order)
    return res


def run(model, pool, y_pool, n_questions, strategy="variance", history=None, n_steps=200, lr=0.05, objective=None,
        n_samples=1, seed=0, kl_weight=1.0, reset=False, write=False, return_moments=False, return_theta=False, t0=0,
        lds_rows=-1):
    """The sessions of every user of the pool (VFM.elicit documents the arguments and the result)."""
    x, y, hx, hy, objective, code = check_args(model, pool, y_pool, n_questions, strategy, history, n_steps, lr,
                                               objective, n_samples, kl_weight)
    ops._need_cuda(model._flat, "the model's parameters")
    dev, d, Q = model.device, model.d, int(n_questions)
    order, users, ptr = pool_lists(x)
    items, ys = x[order, 1].contiguous(), y[order].contiguous()
    U, P = users.numel(), items.numel()
    hptr = hitems = hys = None
    if hx is not None and hx.shape[0]:
        horder, hptr = history_lists(users, hx)
        hitems, hys = hx[horder, 1].contiguous(), hy[horder].contiguous()
    out_row, score, loss, theta, mean, var = _outputs(dev, U, Q, P, d, return_theta, return_moments)
    res = {"users": users}
    if U:
        o = _lib.ops()
        obj = foldin.OBJECTIVES[objective]
        op_x = pool_op = hist_op = None
        n_ops = 0
        if objective == "closed_form":     # one operand per DISTINCT item of pool and history: the items are frozen
            allit = items if hitems is None else torch.cat([items, hitems])
            uq, inv = torch.unique(allit, return_inverse=True)
            op_x = torch.zeros(uq.numel(), 2, dtype=torch.int64, device=dev)
            op_x[:, 1] = uq
            pool_op = inv[:P].contiguous()
            hist_op = inv[P:].contiguous() if hitems is not None else None
            n_ops = uq.numel()
        ws = torch.empty(max(o.elicit_workspace_bytes(P, n_ops, d, obj), 1), dtype=torch.uint8, device=dev)
        model._fresh_params()
        ent, bia, scal = model._views(model._flat)
        lik = _lib.LIK_NORMAL if model.output == "reg" else _lib.LIK_BERNOULLI
        o.elicit(users, ptr, items, ys, hptr, hitems, hys, op_x, pool_op, hist_op, ent, bia, scal, ws, out_row, score,
                 loss, theta, mean, var, Q, code, obj, lik, link_flags(model), int(n_steps), int(n_samples),
                 int(bool(reset)), int(bool(write)), int(lds_rows), float(lr), float(kl_weight), _seed64(seed), int(t0))
        if write:
            model.params_changed()      # (rows written outside the step kernels: derived caches are stale)
    return _result(res, order, out_row, score, loss, theta, mean, var)


# ---------------------------------------------------------------------------------------------------------------------
# the field form: respondents are the entities of one column of a model with any number of fields
# ---------------------------------------------------------------------------------------------------------------------
NO_TARGETS = object()                    # field_lists' `targets` when the caller has no use for target lists


def field_lists(x, y, hx, hy, field, targets=NO_TARGETS):
    """The per-respondent lists of a field-form session (torch, any device; stable sorts: the caller's order is kept
    within a respondent) and one operand per distinct context of all the rows listed: dict(order, ents, ptr, px, ys,
    hptr, hxs, hys, tptr, op_x, pool_op, hist_op, tgt_op).  hx None or without rows: no history (None for its four).
    targets: [R, F] rows grouped as the history's; None: each respondent's own pool rows (tptr is ptr, tgt_op is
    pool_op); NO_TARGETS: none are built (tptr, tgt_op None) and op_x is the distinct contexts of pool and history."""
    order, ents, ptr = pool_lists(x, field)
    px, ys = x[order].contiguous(), y[order].contiguous()
    hptr = hxs = hys = hist_op = txs = tptr = tgt_op = None
    if hx is not None and hx.shape[0]:
        horder, hptr = history_lists(ents, hx, field)
        hxs, hys = hx[horder].contiguous(), hy[horder].contiguous()
    if targets is None:
        tptr = ptr
    elif targets is not NO_TARGETS:
        torder, tptr = history_lists(ents, targets, field)
        txs = targets[torder]
    parts = [t for t in (px, hxs, txs) if t is not None]
    ctx = (px if len(parts) == 1 else torch.cat(parts)).clone()       # one operand per DISTINCT context: it is frozen
    ctx[:, field] = 0
    op_x, inv = torch.unique(ctx, dim=0, return_inverse=True)
    inv = inv.reshape(-1)
    P, H = px.shape[0], 0 if hxs is None else hxs.shape[0]
    pool_op = inv[:P].contiguous()
    if hxs is not None:
        hist_op = inv[P:P + H].contiguous()
    if targets is None:
        tgt_op = pool_op
    elif txs is not None:
        tgt_op = inv[P + H:P + H + txs.shape[0]].contiguous()
    return dict(order=order, ents=ents, ptr=ptr, px=px, ys=ys, hptr=hptr, hxs=hxs, hys=hys, tptr=tptr,
                op_x=op_x.contiguous(), pool_op=pool_op, hist_op=hist_op, tgt_op=tgt_op)


def link_flags(model):
    return ops.FLAG_LINK_SOFTPLUS if model.link == "softplus" else 0


def run_field_session(model, x, y, hx, hy, field, n_questions, workspace, op, options, write, return_moments,
                      return_theta, targets=NO_TARGETS, priors=None):
    """One launch of a field-form session over checked arguments, whichever form: the lists, the outputs, the workspace,
    the call and the result in the caller's pool order.  workspace(o, U, P, H, n_ops, d): the form's size call on
    o = torch.ops.vfm_hip; op: the session op's name there; options: what follows out_var in its schema.  targets (as
    field_lists'): given or None for the one form that has tgt_ptr and tgt_op, which sit where its schema has them.
    priors (checked by the caller: sweep.check_priors): None runs `op`; a GroupPriors runs `op`_prior, whose schema has
    the field's prior row [2, d + 1] between out_var and the options."""
    ops._need_cuda(model._flat, "the model's parameters")
    if priors is not None:
        op, options = op + "_prior", (priors.row(int(field)).to(model.device), *options)
    dev, d, Q = model.device, model.d, int(n_questions)
    L = field_lists(x, y, hx, hy, field, targets)
    ents, px = L["ents"], L["px"]
    U, P = ents.numel(), px.shape[0]
    out_row, score, loss, theta, mean, var = _outputs(dev, U, Q, P, d, return_theta, return_moments)
    res = {"entities": ents}
    if U:
        o = _lib.ops()
        H = 0 if L["hxs"] is None else L["hxs"].shape[0]
        ws = torch.empty(max(workspace(o, U, P, H, L["op_x"].shape[0], d), 1), dtype=torch.uint8, device=dev)
        model._fresh_params()
        ent, bia, scal = model._views(model._flat)
        operands = ((L["op_x"], L["pool_op"], L["hist_op"]) if targets is NO_TARGETS else
                    (L["hist_op"], L["tptr"], L["tgt_op"], L["op_x"], L["pool_op"]))
        getattr(o, op)(ents, L["ptr"], px, L["ys"], L["hptr"], L["hxs"], L["hys"], *operands, ent, bia, scal, ws, out_row,
                       score, loss, theta, mean, var, *options)
        if write:
            model.params_changed()      # (rows written outside the step kernels: derived caches are stale)
    return _result(res, L["order"], out_row, score, loss, theta, mean, var)


def check_args_field(model, pool, y_pool, n_questions, field, strategy, history, n_steps, lr, objective, n_samples,
                     kl_weight, key_field):
    """Validate a field-form session call (no GPU needed).  Returns (pool [P, F] int64, y_pool [P] fp32, hist_x [H, F] or
    None, hist_y [H] or None, objective name, strategy code, field, key column) on the model's device."""
    from .rank import _context_rows, _field_arg, _key_field
    field = _field_arg(model, field)
    kf = _key_field(model, field, key_field)
    code = strategy_code(strategy)
    _check_questions(model, strategy, n_questions)
    x = _context_rows(model, pool, "pool", field, check_field_column=True)
    x, y, objective = foldin.check_args(model, x, y_pool, field, objective, n_samples, n_steps, lr, kl_weight)
    hx = hy = None
    if history is not None:
        hx = _context_rows(model, _history_pair(history, model.F)[0], "history X", field, check_field_column=True)
        hx, hy, _ = foldin.check_args(model, hx, history[1], field, objective, n_samples, n_steps, lr, kl_weight)
        if hx.shape[0] and not bool(torch.isin(hx[:, field], x[:, field]).all()):
            raise ValueError("history holds respondents without a pool row")
    return x, y, hx, hy, objective, code, field, kf


def run_field(model, pool, y_pool, n_questions, field=0, strategy="variance", history=None, n_steps=200, lr=0.05,
              objective=None, n_samples=1, seed=0, kl_weight=1.0, reset=False, write=False, return_moments=False,
              return_theta=False, key_field=None, t0=0, lds_rows=-1):
    """The sessions of every entity of column `field` of the pool (VFM.elicit_field documents the arguments and the
    result): the lists of `run` over column `field`, one operand per distinct context of pool and history together, and
    one call of torch.ops.vfm_hip.elicit_field."""
    x, y, hx, hy, objective, code, field, kf = check_args_field(model, pool, y_pool, n_questions, field, strategy,
                                                                history, n_steps, lr, objective, n_samples, kl_weight,
                                                                key_field)
    obj = foldin.OBJECTIVES[objective]
    lik = _lib.LIK_NORMAL if model.output == "reg" else _lib.LIK_BERNOULLI
    return run_field_session(
        model, x, y, hx, hy, field, n_questions,
        lambda o, U, P, H, n_ops, d: o.elicit_field_workspace_bytes(P, n_ops, d, obj), "elicit_field",
        (field, kf, int(n_questions), code, obj, lik, link_flags(model), int(n_steps), int(n_samples), int(bool(reset)),
         int(bool(write)), int(lds_rows), float(lr), float(kl_weight), _seed64(seed), int(t0)),
        write, return_moments, return_theta)


# ---------------------------------------------------------------------------------------------------------------------
# the exact field form: each round's Adam fit replaced by the closed-form optimum (vfm_elicit_solve_f32)
# ---------------------------------------------------------------------------------------------------------------------
def check_args_field_exact(model, pool, y_pool, n_questions, field, strategy, history, kl_weight, key_field):
    """Validate an exact field-form session call (no GPU needed): the exact fold-in's conditions ('reg', kl_weight > 0
    and finite), then check_args_field's pool and history checks with the closed-form objective."""
    if model.output != "reg":
        raise ValueError("the exact session needs a 'reg' model (Gaussian likelihood): the closed form it solves has "
                         "none for 'class'; use elicit_field")
    foldin._check_kl_positive(kl_weight)
    if model.F < 2:
        raise ValueError("elicit_field_exact needs a model with at least two fields")
    x, y, hx, hy, _, code, field, kf = check_args_field(model, pool, y_pool, n_questions, field, strategy, history, 0,
                                                        0.0, "closed_form", 1, kl_weight, key_field)
    return x, y, hx, hy, code, field, kf


def run_field_exact(model, pool, y_pool, n_questions, field=0, strategy="variance", history=None, seed=0,
                    kl_weight=1.0, reset=False, write=False, return_moments=False, return_theta=False, key_field=None,
                    lds_dim=-1, priors=None):
    """The exact sessions of every entity of column `field` of the pool (VFM.elicit_field_exact documents the arguments
    and the result): run_field's lists and operands, and one call of torch.ops.vfm_hip.elicit_solve (with priors:
    elicit_solve_prior)."""
    x, y, hx, hy, code, field, kf = check_args_field_exact(model, pool, y_pool, n_questions, field, strategy, history,
                                                           kl_weight, key_field)
    sweep.check_priors(model, priors)
    foldin._check_lds_dim(lds_dim)
    return run_field_session(
        model, x, y, hx, hy, field, n_questions,
        lambda o, U, P, H, n_ops, d: o.elicit_solve_workspace_bytes(U, P, n_ops, d, int(lds_dim)), "elicit_solve",
        (field, kf, int(n_questions), code, link_flags(model), int(bool(reset)), int(bool(write)), int(lds_dim),
         float(kl_weight), _seed64(seed)), write, return_moments, return_theta, priors=priors)


# ---------------------------------------------------------------------------------------------------------------------
# the bound field form ('class' models): each round's Adam fit replaced by the bound fold-in (vfm_elicit_bound_f32)
# ---------------------------------------------------------------------------------------------------------------------
DESIGN_NEEDS_REG = ("strategy 'design' is not available for the bound sessions: its score is the drop of the optimum's "
                    "scales, which for a 'reg' model depend on the rows alone; under the bound the scales of the optimum "
                    "depend on the answers through xi, so there is no answer-free score to rank the questions by")


def check_args_field_bound(model, pool, y_pool, n_questions, field, strategy, history, kl_weight, n_iters, key_field):
    """Validate a bound field-form session call (no GPU needed): the bound fold-in's conditions ('class', kl_weight > 0
    and finite, n_iters >= 1, labels in {0, 1}), F >= 2, then check_args_field's pool and history checks."""
    if model.output != "class":
        raise ValueError("the bound session needs a 'class' model (Bernoulli likelihood): a 'reg' model has the exact "
                         "optimum itself; use elicit_field_exact")
    if strategy == "design":
        raise ValueError(DESIGN_NEEDS_REG)
    foldin._check_kl_positive(kl_weight)
    foldin._check_n_iters(n_iters)
    if model.F < 2:
        raise ValueError("elicit_field_bound needs a model with at least two fields")
    x, y, hx, hy, _, code, field, kf = check_args_field(model, pool, y_pool, n_questions, field, strategy, history, 0,
                                                        0.0, "sampled", 1, kl_weight, key_field)
    for v, what in ((y, "y_pool"), (hy, "the history's y")):
        if v is not None and v.numel() and not bool(((v == 0) | (v == 1)).all()):
            raise ValueError(f"{what} must hold the labels 0 and 1 of a 'class' model")
    return x, y, hx, hy, code, field, kf


def run_field_bound(model, pool, y_pool, n_questions, field=0, strategy="variance", history=None, seed=0, kl_weight=1.0,
                    n_iters=8, reset=False, write=False, return_moments=False, return_theta=False, key_field=None,
                    lds_dim=-1, priors=None):
    """The bound sessions of every entity of column `field` of the pool (VFM.elicit_field_bound documents the arguments
    and the result): run_field's lists and operands, and one call of torch.ops.vfm_hip.elicit_bound (with priors:
    elicit_bound_prior)."""
    x, y, hx, hy, code, field, kf = check_args_field_bound(model, pool, y_pool, n_questions, field, strategy, history,
                                                           kl_weight, n_iters, key_field)
    sweep.check_priors(model, priors)
    foldin._check_lds_dim(lds_dim)
    Q = int(n_questions)
    return run_field_session(
        model, x, y, hx, hy, field, Q,
        lambda o, U, P, H, n_ops, d: o.elicit_bound_workspace_bytes(U, P, H, n_ops, d, Q, int(lds_dim)), "elicit_bound",
        (field, kf, Q, code, link_flags(model), int(bool(reset)), int(bool(write)), int(lds_dim), float(kl_weight),
         _seed64(seed), int(n_iters)), write, return_moments, return_theta, priors=priors)


# ---------------------------------------------------------------------------------------------------------------------
# the implicit field form (two-field 'reg' models): each round's fold is the optimum over every (respondent, partner)
# pair, fold_in_implicit's (vfm_elicit_implicit_f32)
# ---------------------------------------------------------------------------------------------------------------------
DESIGN_NEEDS_ROWS = ("strategy 'design' is not available for the implicit sessions: its score is the drop of the optimum's "
                     "scales over the rows asked alone; under J_imp the scales carry the w0 mass of every partner, and "
                     "that target-aware score is not built")


def check_args_field_implicit(model, pool, y_pool, n_questions, field, strategy, history, kl_weight, w0, w1):
    """Validate an implicit field-form session call (no GPU needed): the implicit solves' conditions (a two-field 'reg'
    model, kl_weight > 0 and finite, finite weights with w1 >= w0 > 0 once rounded to fp32), no "mean" / "design"
    strategy, check_args_field's pool and history checks, and no partner named twice for a respondent by pool and history
    together.  Returns (x, y, hx, hy, strategy code, field, key column, w0, w1)."""
    if model.output != "reg":
        raise ValueError("the implicit session needs a 'reg' model (Gaussian likelihood): the closed form it solves has "
                         "none for 'class'; use elicit_field_bound")
    if model.F != 2:
        raise ValueError(f"the implicit session needs a two-field model (F = 2), not F = {model.F}")
    foldin._check_kl_positive(kl_weight)
    w0, w1 = (float(torch.tensor(float(w), dtype=torch.float32)) for w in (w0, w1))     # (the kernels take them in fp32)
    if not (math.isfinite(w0) and math.isfinite(w1)):
        raise ValueError("w0 and w1 must be finite")
    if not w0 > 0.0:
        raise ValueError("w0 must be > 0: it is the weight of every unobserved pair")
    if w1 < w0:
        raise ValueError("w1 must be >= w0: an observed pair weighs at least what an unobserved one does")
    if strategy == "design":
        raise ValueError(DESIGN_NEEDS_ROWS)
    x, y, hx, hy, _, code, field, kf = check_args_field(model, pool, y_pool, n_questions, field, strategy, history, 0,
                                                        0.0, "closed_form", 1, kl_weight, None)
    rows = x if hx is None else torch.cat([x, hx])
    if rows.shape[0]:
        key = rows[:, 0] * model.T + rows[:, 1]
        if int(torch.unique(key).numel()) != rows.shape[0]:
            raise ValueError("duplicate (user, item) pairs in pool and history: every pair is one row of the implicit "
                             "objective")
    return x, y, hx, hy, code, field, kf, w0, w1


def run_field_implicit(model, pool, y_pool, n_questions, field=0, w0=None, w1=1.0, strategy="variance", history=None,
                       seed=0, kl_weight=1.0, reset=False, write=False, return_moments=False, return_theta=False,
                       chunk_rows=2048, lds_dim=-1, priors=None):
    """The implicit sessions of every entity of column `field` of the pool (VFM.elicit_field_implicit documents the
    arguments and the result): run_field's lists and operands, one base block of the partner field
    (sweep.implicit_base at chunk_rows: fold_in_implicit's bits) and one call of torch.ops.vfm_hip.elicit_implicit (with
    priors: elicit_implicit_prior)."""
    if w0 is None:
        raise TypeError("run_field_implicit needs w0, the weight of an unobserved pair")
    x, y, hx, hy, code, field, kf, w0, w1 = check_args_field_implicit(model, pool, y_pool, n_questions, field, strategy,
                                                                      history, kl_weight, w0, w1)
    sweep.check_priors(model, priors)
    foldin._check_lds_dim(lds_dim)
    sweep.check_chunk_rows(chunk_rows)
    ops._need_cuda(model._flat, "the model's parameters")
    model._fresh_params()
    lo, hi = foldin.field_range(model, 1 - field)
    base = sweep.implicit_base(model, lo, hi, chunk_rows)      # (the partner field is frozen over the session)
    return run_field_session(
        model, x, y, hx, hy, field, n_questions,
        lambda o, U, P, H, n_ops, d: o.elicit_implicit_workspace_bytes(U, P, n_ops, d, int(lds_dim)), "elicit_implicit",
        (base, field, kf, int(n_questions), code, link_flags(model), int(bool(reset)), int(bool(write)), int(lds_dim),
         float(kl_weight), _seed64(seed), lo, hi - lo, w0, w1), write, return_moments, return_theta, priors=priors)


# ---------------------------------------------------------------------------------------------------------------------
# the curve of quality against questions asked (torch; any device)
# ---------------------------------------------------------------------------------------------------------------------
def asked_round(rows, P):
    """[P] the round in which each pool row was asked (rows [U, Q], -1 padded); Q for a row never asked."""
    U, Q = rows.shape
    out = torch.full((P,), Q, dtype=torch.int64, device=rows.device)
    q = torch.arange(Q, device=rows.device).expand(U, Q)
    hit = rows >= 0
    out[rows[hit]] = q[hit]
    return out


def auc(score, y):
    """Area under the ROC curve of `score` for the labels y in {0, 1} (ties count 1/2); NaN with one class only."""
    pos = y > 0.5
    n1 = int(pos.sum())
    n0 = int(y.numel()) - n1
    if n1 == 0 or n0 == 0:
        return float("nan")
    _, inv, cnt = torch.unique(score.to(torch.float64), return_inverse=True, return_counts=True)
    cum = torch.cumsum(cnt, 0).to(torch.float64)
    rank = (cum - (cnt.to(torch.float64) - 1.0) / 2.0)[inv]              # 1-based, ties averaged
    return float((rank[pos].sum() - n1 * (n1 + 1) / 2.0) / (float(n1) * float(n0)))


def metric(output, mean, var, y):
    """The reference's test metric from closed-form moments: 'class' the AUC of the probit mean probability
    sigmoid(mean / sqrt(1 + pi var / 8)), 'reg' the RMSE of the mean.  Rows with NaN moments are left out."""
    ok = ~(torch.isnan(mean) | torch.isnan(var))
    mean, var, y = mean[ok].to(torch.float64), var[ok].to(torch.float64), y[ok].to(torch.float64)
    if mean.numel() == 0:
        return float("nan")
    if output == "reg":
        return float(torch.sqrt(torch.mean((mean - y) ** 2)))
    return auc(torch.sigmoid(mean / torch.sqrt(1.0 + math.pi / 8.0 * var)), y)


# The session kinds of the curves: the runner (by its name in this module, looked up when used), the strategy names
# beyond rank.STRATEGIES that the kind accepts -- they run under design.session_for -- and the ones it refuses, with why.
# The two-field `run` and any other runner count as "adam": rank.STRATEGIES' names and nothing else.
SESSION_KINDS = {
    "adam": dict(runner="run_field", accepts=(), refuses={}),
    "exact": dict(runner="run_field_exact", accepts=("design",), refuses={}),
    "bound": dict(runner="run_field_bound", accepts=(), refuses={"design": DESIGN_NEEDS_REG}),
    "implicit": dict(runner="run_field_implicit", accepts=(), refuses={"design": DESIGN_NEEDS_ROWS}),
}


def _kind_of(session):
    return next((k for k, e in SESSION_KINDS.items() if session is globals()[e["runner"]]), "adam")


def _curve_strategy(s, kind):
    """Check a curve's strategy name: rank.STRATEGIES', or one the session kind accepts."""
    if s in SESSION_KINDS[kind]["refuses"]:
        raise ValueError(SESSION_KINDS[kind]["refuses"][s])
    if s not in SESSION_KINDS[kind]["accepts"]:
        strategy_code(s)


def _session_of(s, kind, session, kw):
    """(runner, options) of strategy s of a curve: a kind with names of its own routes through design.session_for (the
    exact curves: "design" to design.run_field_design, where alone `targets` is an option); everything else is
    `session` with the caller's options."""
    if SESSION_KINDS[kind]["accepts"]:
        from . import design
        return design.session_for(s, session, kw)
    return session, kw


def curve(model, pool, y_pool, n_questions, strategies=("mean", "random", "variance"), session=None, **kw):
    """VFM.elicitation_curve: {strategy: [metric before round 0, .., metric after round Q - 1]} on the rows still
    unasked, plus "n_unasked": {strategy: [Q + 1] ints}.  The model is left untouched.  session: the runner (`run`, or
    `run_field` for the field form, `run_field_exact` for the exact one, `run_field_bound` for the bound one)."""
    session = run if session is None else session
    for key in ("write", "return_moments", "return_theta"):
        if key in kw:
            raise ValueError(f"elicitation_curve sets {key} itself")
    kind, strategies = _kind_of(session), list(strategies)
    for s in strategies:
        _curve_strategy(s, kind)
    out, left = {}, {}
    for s in strategies:
        run_s, kw_s = _session_of(s, kind, session, kw)
        r = run_s(model, pool, y_pool, n_questions, strategy=s, write=False, return_moments=True, **kw_s)
        y = torch.as_tensor(y_pool).to(model.device, torch.float32).reshape(-1)
        when = asked_round(r["rows"], y.numel())
        out[s], left[s] = [], []
        for q in range(int(n_questions) + 1):
            keep = when >= q
            out[s].append(metric(model.output, r["logit_mean"][q][keep], r["logit_var"][q][keep], y[keep]))
            left[s].append(int(keep.sum()))
    out["n_unasked"] = left
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the ranking curve of a session: held-out ranking metrics under the posteriors of every round, one launch per strategy
# ---------------------------------------------------------------------------------------------------------------------
def ranking_curve_plan(ents, rows, pool, hist_x, exclude, X_rel, field, rank_field, match, T):
    """The host-side bookkeeping of the ranking curve (torch, any device; every tensor int64): which queries, which
    posterior of which round, which positives and which exclusions.

    ents [U] ascending: the session's respondents (column `field`); rows [U, Q]: the pool rows asked per round (-1 once
    a respondent has nothing left); pool [P, F]; hist_x [H, F] or None; exclude [R, F] or None; X_rel [B, F]: the
    relevant test rows (rows of other respondents are left out).  Nc distinct contexts of X_rel (column `rank_field`
    zeroed, in torch.unique's row order) times the rounds 0 .. Q, round-major: query q Nc + c is context c under its
    respondent's posterior BEFORE round q.  The exclusions of round q are the rows of `exclude`, of the history and of
    the pool rows asked (by anyone) before round q, matched to the contexts on the columns `match` as rank_field
    matches them.
    Returns dict(contexts [Nc, F], queries [(Q + 1) Nc, F], resp [(Q + 1) Nc] (index into ents), round [(Q + 1) Nc],
    pos = (query_index, ids), excl = (query_index, ids), n_contexts = Nc)."""
    from .rank import field_exclusion_csr, field_positive_csr
    dev = ents.device
    Q = rows.shape[1]
    mine = torch.isin(X_rel[:, field], ents)
    C, pptr, pitems = field_positive_csr(X_rel[mine], rank_field, T)
    Nc = C.shape[0]
    resp = torch.searchsorted(ents, C[:, field].contiguous()) if Nc else torch.zeros(0, dtype=torch.int64, device=dev)
    pc = torch.repeat_interleave(torch.arange(Nc, device=dev), pptr[1:] - pptr[:-1])
    fixed = [t for t in (exclude, hist_x) if t is not None and t.shape[0]]
    pos_q, pos_i, ex_q, ex_i = [], [], [], []
    for q in range(Q + 1):
        asked = rows[:, :q].reshape(-1)
        asked = asked[asked >= 0]
        parts = fixed + ([pool[asked]] if asked.numel() else [])
        pos_q.append(q * Nc + pc)
        pos_i.append(pitems)
        if parts and Nc:
            eptr, eitems = field_exclusion_csr(C, torch.cat(parts), rank_field, match, T)
            ex_q.append(q * Nc + torch.repeat_interleave(torch.arange(Nc, device=dev), eptr[1:] - eptr[:-1]))
            ex_i.append(eitems)
    empty = torch.zeros(0, dtype=torch.int64, device=dev)
    cat = lambda v: torch.cat(v) if v else empty
    return {"contexts": C, "queries": C.repeat(Q + 1, 1), "resp": resp.repeat(Q + 1),
            "round": torch.repeat_interleave(torch.arange(Q + 1, device=dev), Nc), "pos": (cat(pos_q), cat(pos_i)),
            "excl": (cat(ex_q), cat(ex_i)), "n_contexts": Nc}


def round_posteriors(theta0, theta, resp, rnd):
    """[n, 2d + 2]: per query the posterior of respondent resp[i] before round rnd[i] -- theta0 [U, 2d + 2] for round 0,
    theta[:, q - 1] (theta [U, Q, 2d + 2], the session's return_theta) for round q > 0."""
    if theta.shape[1] == 0:
        return theta0[resp].contiguous()
    later = theta[resp, (rnd - 1).clamp(min=0)]
    return torch.where((rnd == 0)[:, None], theta0[resp], later).contiguous()


def ranking_curve(model, pool, y_pool, n_questions, field, X_test, y_test, rank_field, ks=(10,),
                  strategies=("random", "variance"), exact=False, exclude=None, match_fields=None, threshold=None,
                  ineligible="raise", bound=False, implicit=False, **session_kw):
    """VFM.elicitation_ranking_curve_field (which documents the arguments and the result)."""
    from . import rank
    for key in ("write", "return_moments", "return_theta", "strategy"):
        if key in session_kw:
            raise ValueError(f"elicitation_ranking_curve_field sets {key} itself")
    if bound and exact:
        raise ValueError("bound=True and exact=True: the exact sessions are for 'reg' models, the bound ones for 'class'")
    if implicit and (exact or bound):
        raise ValueError("implicit=True excludes exact=True and bound=True: a session has one fold")
    if implicit and session_kw.get("w0") is None:
        raise ValueError("implicit=True needs w0, the weight of an unobserved pair")
    if not implicit and any(k in session_kw for k in ("w0", "w1")):
        raise ValueError("w0 and w1 are options of the implicit sessions: implicit=True")
    kind, strategies = "implicit" if implicit else "bound" if bound else "exact" if exact else "adam", list(strategies)
    for s in strategies:
        _curve_strategy(s, kind)
    field = rank._field_arg(model, field)
    rank_field = rank._field_arg(model, rank_field)
    if rank_field == field:
        raise ValueError("rank_field must differ from field: the respondents' column is a context column of the ranking")
    ks = [int(k) for k in ks]
    if not ks or any(k <= 0 for k in ks):
        raise ValueError("ks must be a non-empty list of positive ints")
    if ineligible not in ("raise", "drop"):
        raise ValueError(f"ineligible must be 'raise' or 'drop', not {ineligible!r}")
    match = rank._match_arg(model, rank_field, match_fields)
    X = torch.as_tensor(X_test)
    y = torch.as_tensor(y_test).reshape(-1)
    if X.dim() != 2 or X.shape[1] != model.F or X.shape[0] != y.numel():
        raise ValueError(f"X_test must be [B, {model.F}] with one y_test value per row")
    relevant = (y >= (4.0 if threshold is None else float(threshold))) if model.output == "reg" else (y == 1)
    X_rel = rank._context_rows(model, X[relevant.to(X.device)], "X_test", rank_field, check_field_column=True)
    ex = rank._context_rows(model, exclude, "exclude", rank_field, check_field_column=True) if exclude is not None else None
    session = globals()[SESSION_KINDS[kind]["runner"]]
    dev, d = model.device, model.d
    out = {}
    n_queries = 0
    for s in strategies:
        run_s, kw_s = _session_of(s, kind, session, session_kw)
        r = run_s(model, pool, y_pool, n_questions, field, strategy=s, write=False, return_theta=True, **kw_s)
        ents, Q = r["entities"], int(n_questions)
        U = ents.numel()
        if session_kw.get("reset", False):     # (the row the session scored round 0 from: the prior's)
            theta0 = foldin.prior_theta(model, session_kw.get("priors"), field).to(dev).expand(U, 2 * d + 2)
        else:
            model._fresh_params()
            ent, bia, _ = model._views(model._flat)
            theta0 = torch.cat([ent[ents], bia[ents]], 1)
        hist = session_kw.get("history")
        hx = torch.as_tensor(hist[0]).to(dev, torch.int64) if hist is not None else None
        px = torch.as_tensor(pool).to(dev, torch.int64)
        plan = ranking_curve_plan(ents, r["rows"], px, hx, ex, X_rel, field, rank_field, match, model.T)
        Nc = plan["n_contexts"]
        n_queries = (Q + 1) * Nc
        post = round_posteriors(theta0, r["theta"], plan["resp"], plan["round"])
        h = rank.rank_heldout_field_posterior(model, plan["queries"], plan["pos"], post, field, rank_field,
                                              ineligible=ineligible, query_exclude=plan["excl"])
        curve_s = {}
        for q in range(Q + 1):
            a, b = int(h["ptr"][q * Nc]), int(h["ptr"][(q + 1) * Nc])
            means, _ = rank.ranking_metrics(h["rank"][a:b], h["rank_neg"][a:b], h["ptr"][q * Nc:(q + 1) * Nc + 1] - a,
                                            h["n_neg"][q * Nc:(q + 1) * Nc], ks)
            for key, v in means.items():
                curve_s.setdefault(key, []).append(v)
        out[s] = curve_s
    out["n_queries"] = n_queries
    return out

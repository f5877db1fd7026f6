"""Fold-in: fit chosen entities' posteriors with the rest of the model frozen (include/vfm_foldin.h).

With every parameter but one entity's variational factors frozen, the mean-field ELBO splits into independent
per-entity problems ("Fold-in").  This module checks the arguments, sorts the rows by the folded id
(stable), builds the per-entity row lists and, for the closed form, the distinct frozen-partner tuples; the fit itself
is one HIP launch (plus the operand prep) through torch.ops.vfm_hip.foldin.
"""
from __future__ import annotations

import math

import torch

from . import _lib, ops
from .rank import _seed64

OBJECTIVES = {"sampled": _lib._gen.VFM_OBJ_SAMPLED, "closed_form": _lib._gen.VFM_OBJ_CLOSED_FORM}
MAX_D = 512
MAX_SAMPLES = 4
MODE_FIT, MODE_OBJECTIVE = 0, 1


def prior_s(link: str) -> float:
    """The scale parameter whose sigma = link(s) is 1: 1 for |.|, log(e - 1) for softplus."""
    return 1.0 if link == "abs" else math.log(math.e - 1.0)


def prior_theta(model, priors=None, field=0):
    """[2d + 2] fp32 = [mu | s | mu_w | s_w]: the row a session's reset=True starts a respondent of column `field` at,
    with the kernels' bits (prior_row_s of csrc_rank/vfm_foldin_solve_body.hpp).  priors None: (0, prior_s).  A
    sweep.GroupPriors: mu_c = mean_c, sigma_c = sqrt(1 / prec_c) in fp64 from the fp32 precision, stored as (float)
    sigma_c for the |.| link and (float) log(expm1(sigma_c)) for softplus.  A function of the prior and the link alone."""
    d = model.d
    if priors is None:
        out = torch.zeros(2 * d + 2, dtype=torch.float32)
        out[d:2 * d] = prior_s(model.link)
        out[2 * d + 1] = prior_s(model.link)
        return out
    row = priors.row(int(field)).detach().cpu()
    sg = torch.sqrt(1.0 / row[1].double())
    s = (sg if model.link == "abs" else torch.log(torch.expm1(sg))).float()
    return torch.cat([row[0, 1:], s[1:], row[0, :1], s[:1]]).contiguous()


def field_range(model, field: int):
    lo = sum(model.field_sizes[:field])
    return lo, lo + model.field_sizes[field]


def _check_kl_positive(kl_weight):
    """The exact and the bound solves' condition on kl_weight (the sessions over them and the design score share it)."""
    if not float(kl_weight) > 0.0 or not math.isfinite(float(kl_weight)):
        raise ValueError("kl_weight must be > 0 and finite: the prior term is what makes each system positive definite")


def _check_n_iters(n_iters):
    if isinstance(n_iters, bool) or int(n_iters) != n_iters or int(n_iters) < 1:
        raise ValueError("n_iters must be an integer >= 1")


def _check_lds_dim(lds_dim):
    if int(lds_dim) < -1:
        raise ValueError("lds_dim must be -1 or >= 0")


def check_args(model, X, y, field, objective, n_samples, n_steps=0, lr=0.0, kl_weight=1.0):
    """Validate a fold-in call (no GPU needed).  Returns (x [R, F] int64, y [R] fp32, objective name) on the model's
    device."""
    if isinstance(field, bool) or not isinstance(field, int) or not 0 <= field < model.F:
        raise ValueError(f"field must be an int in [0, {model.F})")
    if objective is None:
        objective = "closed_form" if model.output == "reg" else "sampled"
    if objective not in OBJECTIVES:
        raise ValueError(f"objective must be one of {sorted(OBJECTIVES)}, not {objective!r}")
    if objective == "closed_form" and model.output != "reg":
        raise ValueError("the closed-form objective needs a 'reg' model (Gaussian likelihood); use 'sampled'")
    if not 1 <= int(n_samples) <= MAX_SAMPLES:
        raise ValueError(f"n_samples must lie in [1, {MAX_SAMPLES}]")
    if int(n_steps) < 0:
        raise ValueError("n_steps must be >= 0")
    if not float(lr) >= 0.0 or not float(kl_weight) >= 0.0:
        raise ValueError("lr and kl_weight must be >= 0")
    if model.d > MAX_D:
        raise ValueError(f"fold-in supports embedding sizes up to {MAX_D}")
    dev = model.device
    x = torch.as_tensor(X)
    if x.dtype.is_floating_point or x.dtype == torch.bool:
        raise ValueError("X must hold integer ids")
    x = x.to(dev, torch.int64)
    if x.dim() != 2 or x.shape[1] != model.F:
        raise ValueError(f"X must be [R, {model.F}]")
    y = torch.as_tensor(y).to(dev, torch.float32).reshape(-1)
    if y.numel() != x.shape[0]:
        raise ValueError(f"y must hold one value per row of X ({x.shape[0]}), not {y.numel()}")
    if x.shape[0]:
        lo, hi = field_range(model, field)
        f = x[:, field]
        if int(f.min()) < lo or int(f.max()) >= hi:
            raise ValueError(f"folded ids (column {field}) must lie in the field's range [{lo}, {hi})")
        if model.F > 1:
            p = torch.cat([x[:, :field], x[:, field + 1:]], 1)
            if int(p.min()) < 0 or int(p.max()) >= model.T:
                raise ValueError(f"partner ids must lie in [0, {model.T})")
            if bool(((p >= lo) & (p < hi)).any()):
                raise ValueError(f"partner columns hold ids of the folded field's range [{lo}, {hi}): they would not be frozen")
    return x.contiguous(), y.contiguous(), objective


def row_lists(x, y, field):
    """Stable sort of the rows by the folded id: (xs, ys, entities [E] ascending, row_ptr [E + 1], rows [E])."""
    order = torch.sort(x[:, field], stable=True).indices
    xs, ys = x[order].contiguous(), y[order].contiguous()
    ents, counts = torch.unique_consecutive(xs[:, field], return_counts=True)
    ptr = torch.zeros(ents.numel() + 1, dtype=torch.int64, device=x.device)
    torch.cumsum(counts, 0, out=ptr[1:])
    return xs, ys, ents.contiguous(), ptr, counts


def partner_tuples(xs, field):
    """The distinct frozen-partner tuples (the folded column zeroed) and each row's tuple: (op_x [n_ops, F], row_op [R])."""
    xp = xs.clone()
    xp[:, field] = 0
    if xp.shape[1] == 1:
        return xp[:1].contiguous(), torch.zeros(xp.shape[0], dtype=torch.int64, device=xs.device)
    if xp.shape[1] == 2:                   # (one partner column: a 1-D unique)
        pc = xp[:, 1 - field]
        u, inv = torch.unique(pc, return_inverse=True)
        op_x = torch.zeros(u.numel(), 2, dtype=torch.int64, device=xs.device)
        op_x[:, 1 - field] = u
        return op_x, inv.contiguous()
    u, inv = torch.unique(xp, dim=0, return_inverse=True)
    return u.contiguous(), inv.contiguous()


def _link_flags(model):
    return ops.FLAG_LINK_SOFTPLUS if model.link == "softplus" else 0


def _launch(model, x, y, field, ws_bytes, call, tuples=True, grad=False, writes=True):
    """The host path of the three fold-in forms over checked rows: the row lists, the outputs, the partner tuples and
    the workspace of ws_bytes(o, E, R, n_ops) bytes where the form has them (`tuples`), the table views and one op call,
    call(o, a, xs, grad, flags) with a = (entities, row_ptr, ys, op_x, row_op, entity, bias, scalars, workspace, loss):
    the leading arguments of every solve op.  Returns (entities [E], loss [E], rows [E], grad [E, 2d + 2] or None)."""
    ops._need_cuda(model._flat, "the model's parameters")
    dev, d = model.device, model.d
    xs, ys, ents, ptr, counts = row_lists(x, y, field)
    E = ents.numel()
    loss = torch.empty(E, dtype=torch.float32, device=dev)
    g = torch.empty(E, 2 * d + 2, dtype=torch.float32, device=dev) if grad else None
    if E == 0:
        return ents, loss, counts, g
    o = _lib.ops()
    op_x = row_op = ws = None
    if tuples:
        op_x, row_op = partner_tuples(xs, field)
        ws = torch.empty(max(ws_bytes(o, E, ys.numel(), op_x.shape[0]), 1), dtype=torch.uint8, device=dev)
    model._fresh_params()
    ent, bia, scal = model._views(model._flat)
    call(o, (ents, ptr, ys, op_x, row_op, ent, bia, scal, ws, loss), xs, g, _link_flags(model))
    if writes:
        model.params_changed()          # (rows written outside the step kernels: derived caches are stale)
    return ents, loss, counts, g


def run(model, X, y, field=0, objective=None, n_samples=1, seed=0, kl_weight=1.0, mode=MODE_FIT, n_steps=0, lr=0.0,
        reset=False, t0=0, lds_rows=-1):
    """One fold-in launch.  Returns (entities [E], loss [E], rows [E], grad [E, 2d + 2] or None)."""
    x, y, objective = check_args(model, X, y, field, objective, n_samples, n_steps, lr, kl_weight)
    code, d = OBJECTIVES[objective], model.d
    lik = _lib.LIK_NORMAL if model.output == "reg" else _lib.LIK_BERNOULLI
    return _launch(model, x, y, field, lambda o, E, R, n_ops: o.foldin_workspace_bytes(n_ops, d, code),
                   lambda o, a, xs, grad, flags: o.foldin(
                       *a[:2], xs, *a[2:], grad, int(field), code, lik, flags, int(mode), int(n_steps), int(n_samples),
                       int(bool(reset)), int(lds_rows), float(lr), float(kl_weight), _seed64(seed), int(t0)),
                   tuples=objective == "closed_form", grad=mode == MODE_OBJECTIVE, writes=mode == MODE_FIT)


def check_args_exact(model, X, y, field, kl_weight=1.0):
    """Validate an exact fold-in call (no GPU needed): check_args, a 'reg' model and kl_weight > 0."""
    if model.output != "reg":
        raise ValueError("the exact fold-in needs a 'reg' model (Gaussian likelihood): the closed form it solves has "
                         "none for 'class'; use fold_in or fold_in_bound")
    _check_kl_positive(kl_weight)
    x, y, _ = check_args(model, X, y, field, "closed_form", 1, 0, 0.0, kl_weight)
    return x, y


def run_exact(model, X, y, field=0, kl_weight=1.0, lds_dim=-1, priors=None):
    """One exact fold-in launch (vfm_foldin_solve_f32): the closed-form optimum of every folded entity.  priors (a
    sweep.GroupPriors): under the folded field's prior, by vfm_foldin_solve_prior_f32 (include/vfm_prior.h).  Returns
    (entities [E], loss [E], rows [E])."""
    x, y = check_args_exact(model, X, y, field, kl_weight)
    if priors is not None:
        from . import sweep
        sweep.check_priors(model, priors)
    _check_lds_dim(lds_dim)
    d, tail = model.d, (int(field), OBJECTIVES["closed_form"], _lib.LIK_NORMAL)
    prior = None if priors is None else priors.row(int(field)).to(model.device)

    def call(o, a, xs, grad, flags):
        if prior is None:
            o.foldin_solve(*a, *tail, flags, int(lds_dim), float(kl_weight))
        else:
            o.foldin_solve_prior(*a, prior, *tail, flags, int(lds_dim), float(kl_weight))

    return _launch(model, x, y, field, lambda o, E, R, n_ops: o.foldin_solve_workspace_bytes(E, n_ops, d, int(lds_dim)),
                   call)[:3]


def objective_under_prior(model, ents, loss, grad, prior, kl_weight):
    """fold_in_objective's closed-form L_e and gradient moved from the N(0, 1) prior to `prior` [2, d + 1]: the rows'
    term is the kernel's; the KL terms differ by kl_weight (KL(q || N(m, 1 / lam)) - KL(q || N(0, 1))) per coordinate,
    O(E d) elementwise work taken in torch fp64 on the device from the table rows.  Returns (loss [E] fp32,
    grad [E, 2d + 2] fp32 = dL/d[mu | s | mu_w | s_w])."""
    d, kl = model.d, float(kl_weight)
    ent, bia, _ = model._views(model._flat)
    m, lam = prior[0].double(), prior[1].double()
    m = torch.cat([m[1:], m[:1]])                              # (the gradient's order: factors, then the weight)
    lam = torch.cat([lam[1:], lam[:1]])
    mu = torch.cat([ent[ents, :d], bia[ents, :1]], 1).double()
    s = torch.cat([ent[ents, d:], bia[ents, 1:]], 1).double()
    sg = s.abs() if model.link == "abs" else torch.nn.functional.softplus(s)
    dsg = torch.sign(s) if model.link == "abs" else torch.sigmoid(s)
    dkl = 0.5 * ((lam - 1.0) * sg * sg + lam * (mu - m) ** 2 - mu * mu - torch.log(lam))
    g_mu = kl * (lam * (mu - m) - mu)
    g_s = kl * (lam - 1.0) * sg * dsg
    loss = (loss.double() + kl * dkl.sum(1)).float()
    g = grad.double()
    g = g + torch.cat([g_mu[:, :d], g_s[:, :d], g_mu[:, d:], g_s[:, d:]], 1)
    return loss, g.float()


def check_args_bound(model, X, y, field, kl_weight=1.0, n_iters=8):
    """Validate a bound fold-in call (no GPU needed): check_args, a 'class' model, kl_weight > 0 and finite,
    n_iters >= 1 and y in {0, 1}."""
    if model.output != "class":
        raise ValueError("the bound fold-in needs a 'class' model (Bernoulli likelihood): a 'reg' model has the exact "
                         "optimum itself; use fold_in_exact")
    _check_kl_positive(kl_weight)
    _check_n_iters(n_iters)
    x, y, _ = check_args(model, X, y, field, "sampled", 1, 0, 0.0, kl_weight)
    if y.numel() and not bool(((y == 0) | (y == 1)).all()):
        raise ValueError("y must hold the labels 0 and 1 of a 'class' model")
    return x, y


def run_bound(model, X, y, field=0, kl_weight=1.0, n_iters=8, reset=False, lds_dim=-1, mode=MODE_FIT, priors=None):
    """One bound fold-in launch (include/vfm_bound.h: vfm_foldin_bound_f32): n_iters rounds of the Jaakkola-Jordan
    bound's two exact block minimisers for every folded entity (mode=MODE_OBJECTIVE: B_e at the current rows, nothing
    written; n_iters is not used).  priors (a sweep.GroupPriors): under the folded field's prior, by
    vfm_foldin_bound_prior_f32 (include/vfm_bound_prior.h).  Returns (entities [E], loss [E] = B_e, rows [E])."""
    x, y = check_args_bound(model, X, y, field, kl_weight, n_iters)
    if priors is not None:
        from . import sweep
        sweep.check_priors(model, priors)
    _check_lds_dim(lds_dim)
    d = model.d
    mid = () if priors is None else (priors.row(int(field)).to(model.device),)
    tail = (int(field), OBJECTIVES["closed_form"], _lib.LIK_BERNOULLI)
    return _launch(model, x, y, field,
                   lambda o, E, R, n_ops: o.foldin_bound_workspace_bytes(E, R, n_ops, d, int(lds_dim)),
                   lambda o, a, xs, grad, flags: (o.foldin_bound_prior if mid else o.foldin_bound)(
                       *a, *mid, *tail, flags, int(lds_dim),
                       float(kl_weight), int(n_iters) if mode == MODE_FIT else 0, int(bool(reset)), int(mode)),
                   writes=mode == MODE_FIT)[:3]

"""ELBO variants of the reference's sibling scripts on the general HIP kernels of
`csrc/vfm_variants.hip`:

  * closed-form expected log-likelihood   vfm-tomasrch.py:369-451 (+ its loss, :569-588)
  * learnable group priors                vfm-tomasrch.py:206-290
  * sparse features with values != 1      vfm.py:483-509

`variant_forward / variant_backward` are the launch wrappers, `VariantElbo` the autograd.Function,
`VFMClosedForm` the module with the parameter names of vfm-tomasrch.py's `CF`.  All arithmetic runs in the
HIP kernels (no CPU / PyTorch fallback); torch provides memory, autograd plumbing and the optimizer.

`variant_adam_step` is the fused training step (include/vfm_variant_step.h, csrc_var/vfm_variant_step.hip): the backward
and torch.optim.Adam's dense update in one pass over the tables, the gradient rows never written.  `VFMClosedForm.train_step`
/ `fit(fused=True)` train on it; `VariantStepState` holds the flat scalars and priors, the moments and the step count.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch
from torch import nn

from . import _lib, ops
from ._lib import check, ptr, current_stream_ptr

OBJECTIVES = {"sampled": _lib.OBJ_SAMPLED, "closed_form": _lib.OBJ_CLOSED_FORM}


def priors_len(G: int, d: int) -> int:
    """Floats of the flat prior vector [mean0, scale0 | mean_w[G] | scale_w[G] | mean_v[G,d] | scale_v[G,d]]."""
    return 2 + 2 * G + 2 * G * d


_index_struct = ops._index_struct


def variant_forward(plan: ops.BatchPlan, objective: str, entity_params, bias_params, scalars, inv_occ, *,
                    priors=None, values=None, eps=None, seed=0, step=0, train=True):
    """Launch vfm_variant_fwd_f32.  Returns dict(pred [B], loss3 [3] or None, state, grow, partials, problem)."""
    spec, dev = plan.spec, plan.x.device
    for t, n in ((entity_params, "entity_params"), (bias_params, "bias_params"), (scalars, "scalars")):
        ops._need_cuda(t, n)
    B, d = plan.B, spec.d
    train = train and plan.y is not None
    ns = 3 if objective == "closed_form" else 1
    pred = torch.empty(B, dtype=torch.float32, device=dev)
    partials = torch.empty(_lib.PARTIALS_LEN, dtype=torch.float64, device=dev)
    state = torch.empty(B, ns * d, dtype=torch.float32, device=dev) if train else None
    grow = torch.empty(B, dtype=torch.float32, device=dev) if train else None
    loss3 = torch.empty(3, dtype=torch.float32, device=dev) if train else None
    if priors is not None and priors.numel() != priors_len(spec.F, d):
        raise ValueError("priors must hold 2 + 2G + 2Gd floats")
    if values is not None:
        values = values.to(torch.float32).contiguous()
        if values.shape != (B, spec.F):
            raise ValueError("values must be [B,F]")
    p = ops._problem(spec, B, plan.B_global, plan.id_bits, seed, step, 0)
    e = eps if eps is not None else (None, None, None)
    check(_lib.load().vfm_variant_fwd_f32(
        C.byref(p), OBJECTIVES[objective], ptr(plan.x), ptr(values), ptr(plan.y if train else None), ptr(entity_params),
        ptr(bias_params), ptr(inv_occ), ptr(scalars), ptr(plan.W if train else None), ptr(priors), ptr(e[0]), ptr(e[1]),
        ptr(e[2]), ptr(pred), ptr(partials), ptr(state), ptr(grow), ptr(loss3), current_stream_ptr(dev)),
        "vfm_variant_fwd_f32")
    return {"pred": pred, "loss3": loss3, "state": state, "grow": grow, "partials": partials, "problem": p,
            "objective": objective, "priors": priors, "values": values, "eps": eps}


def variant_backward(plan: ops.BatchPlan, st, entity_params, bias_params, scalars, inv_occ, grad_out):
    """Launch vfm_variant_bwd_f32: dense gradients of both tables, the scalars and (if given) the priors."""
    spec, dev = plan.spec, plan.x.device
    g_ent, g_bias = torch.empty_like(entity_params), torch.empty_like(bias_params)
    g_sc = torch.empty(3, dtype=torch.float32, device=dev)
    g_pr = torch.empty_like(st["priors"]) if st["priors"] is not None else None
    ws = torch.empty(int(_lib.load().vfm_variant_workspace_elems(plan.B, spec.F, spec.d)), dtype=torch.int32, device=dev)
    ix = _index_struct(plan)
    e = st["eps"] if st["eps"] is not None else (None, None, None)
    check(_lib.load().vfm_variant_bwd_f32(
        C.byref(st["problem"]), OBJECTIVES[st["objective"]], C.byref(ix), ptr(ws), ptr(plan.x), ptr(st["values"]),
        ptr(entity_params), ptr(bias_params), ptr(inv_occ), ptr(scalars), ptr(plan.W), ptr(st["priors"]), ptr(e[0]),
        ptr(e[1]), ptr(e[2]), ptr(st["state"]), ptr(st["grow"]), ptr(st["partials"]), ptr(grad_out), ptr(g_ent),
        ptr(g_bias), ptr(g_sc), ptr(g_pr), current_stream_ptr(dev)), "vfm_variant_bwd_f32")
    return g_ent, g_bias, g_sc, g_pr


class VariantMoments:
    """Adam's first and second moments (plain, fp32) of the four tensors `variant_adam_step` updates: m_entity / v_entity
    [T,2d], m_bias / v_bias [T,2], m_scalars / v_scalars [3], m_priors / v_priors [priors_len] (None without priors)."""
    NAMES = ("m_entity", "v_entity", "m_bias", "v_bias", "m_scalars", "v_scalars", "m_priors", "v_priors")

    def __init__(self, entity_params, bias_params, scalars, priors=None):
        self.m_entity, self.v_entity = torch.zeros_like(entity_params), torch.zeros_like(entity_params)
        self.m_bias, self.v_bias = torch.zeros_like(bias_params), torch.zeros_like(bias_params)
        self.m_scalars, self.v_scalars = torch.zeros_like(scalars), torch.zeros_like(scalars)
        self.m_priors = torch.zeros_like(priors) if priors is not None else None
        self.v_priors = torch.zeros_like(priors) if priors is not None else None

    def state_dict(self):
        return {n: (None if getattr(self, n) is None else getattr(self, n).detach().cpu().clone()) for n in self.NAMES}

    def load_state_dict(self, sd):
        for n in self.NAMES:
            if (getattr(self, n) is None) != (sd[n] is None):
                raise ValueError(f"moments: {n} present on one side only")
            if sd[n] is not None:
                getattr(self, n).copy_(sd[n].to(getattr(self, n).device))


def variant_step_workspace(plan: ops.BatchPlan) -> torch.Tensor:
    """Scratch of `variant_adam_step` for plans of this batch size (contents need not be kept between steps)."""
    n = int(_lib.load().vfm_variant_step_workspace_bytes(plan.B, plan.spec.F, plan.spec.d))
    if n < 0:
        raise ValueError("variant step: B, F or d out of range")
    return torch.empty(n // 4, dtype=torch.int32, device=plan.x.device)


def variant_adam_step(plan: ops.BatchPlan, st, entity_params, bias_params, scalars, priors, inv_occ, moments: VariantMoments,
                      lr, step, *, betas=(0.9, 0.999), eps=1e-8, grad_out=None, workspace=None):
    """Launch vfm_variant_step_f32: from the state `st` of `variant_forward` (same tensors), one torch.optim.Adam step
    number `step` (>= 1) on entity_params, bias_params, scalars[3] and priors (or None) IN PLACE, moments included.
    Rows the batch does not touch take their zero-gradient step, as under dense Adam.  No host synchronisation."""
    dev = plan.x.device
    for t, n in ((entity_params, "entity_params"), (bias_params, "bias_params"), (scalars, "scalars")):
        ops._need_cuda(t, n)
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"{n} must be a contiguous float32 tensor (it is updated in place)")
    if (priors is None) != (st["priors"] is None) or (priors is not None and priors.data_ptr() != st["priors"].data_ptr()):
        raise ValueError("priors must be the tensor the forward was given")
    if priors is not None and (priors.dtype != torch.float32 or not priors.is_contiguous()):
        raise ValueError("priors must be a contiguous float32 tensor (it is updated in place)")
    if (priors is None) != (moments.m_priors is None):
        raise ValueError("moments of the priors go with the priors")
    if workspace is None:
        workspace = variant_step_workspace(plan)
    if grad_out is None:
        grad_out = torch.ones(1, dtype=torch.float32, device=dev)
    ix = _index_struct(plan)
    e = st["eps"] if st["eps"] is not None else (None, None, None)
    mo = moments
    check(_lib.load().vfm_variant_step_f32(
        C.byref(st["problem"]), OBJECTIVES[st["objective"]], C.byref(ix), ptr(workspace), ptr(plan.x), ptr(st["values"]),
        ptr(entity_params), ptr(bias_params), ptr(inv_occ), ptr(scalars), ptr(plan.W), ptr(priors), ptr(e[0]), ptr(e[1]),
        ptr(e[2]), ptr(st["state"]), ptr(st["grow"]), ptr(st["partials"]), ptr(grad_out), ptr(mo.m_entity), ptr(mo.v_entity),
        ptr(mo.m_bias), ptr(mo.v_bias), ptr(mo.m_scalars), ptr(mo.v_scalars), ptr(mo.m_priors), ptr(mo.v_priors),
        float(lr), float(betas[0]), float(betas[1]), float(eps), int(step), current_stream_ptr(dev)), "vfm_variant_step_f32")


class VariantElbo(torch.autograd.Function):
    """loss, pred, loss3 = VariantElbo.apply(entity_params, bias_params, scalars[3], priors_flat | None, plan,
    inv_occ, objective, values, eps, seed, step) -- differentiable in the first four."""

    @staticmethod
    def forward(ctx, entity_params, bias_params, scalars, priors, plan, inv_occ, objective, values, eps, seed, step):
        ent, bia, sc = entity_params.detach().contiguous(), bias_params.detach().contiguous(), scalars.detach().contiguous()
        pr = priors.detach().contiguous() if priors is not None else None
        st = variant_forward(plan, objective, ent, bia, sc, inv_occ, priors=pr, values=values, eps=eps, seed=seed, step=step)
        ctx.plan, ctx.st, ctx.inv_occ, ctx.args = plan, st, inv_occ, (ent, bia, sc)
        ctx.has_priors = priors is not None
        ctx.mark_non_differentiable(st["pred"], st["loss3"])
        return st["loss3"][0:1].clone(), st["pred"], st["loss3"]

    @staticmethod
    def backward(ctx, g_loss, _gp, _g3):
        ent, bia, sc = ctx.args
        gout = g_loss.to(torch.float32).reshape(1).contiguous()
        g_ent, g_bias, g_sc, g_pr = variant_backward(ctx.plan, ctx.st, ent, bia, sc, ctx.inv_occ, gout)
        return (g_ent, g_bias, g_sc, g_pr if ctx.has_priors else None, None, None, None, None, None, None, None)


class VariantStepState:
    """What `VFMClosedForm.train_step` trains on beside the two tables: the flat scalars[3] = (alpha, mean_global_bias,
    scale_global_bias), the flat prior vector (`priors_len(G, d)`), Adam's moments of all four tensors and the step
    count.  Built once from the model's named parameters; `VFMClosedForm.sync_parameters()` scatters the flat values back."""

    def __init__(self, model: "VFMClosedForm"):
        with torch.no_grad():
            self.scalars = torch.cat([model.alpha, model.mean_global_bias, model.scale_global_bias]).detach().float().contiguous()
            self.priors = model.priors_flat().detach().float().contiguous()
        self.moments = VariantMoments(model.entity_params.data, model.bias_params.data, self.scalars, self.priors)
        self.t = 0                       # Adam steps taken
        self.dirty = False               # the flat buffers are ahead of the named parameters
        self.grad_out = torch.ones(1, dtype=torch.float32, device=self.scalars.device)
        self._ws, self._ws_B = None, -1

    def workspace(self, plan):
        if self._ws is None or plan.B > self._ws_B:
            self._ws, self._ws_B = variant_step_workspace(plan), plan.B
        return self._ws


class VFMClosedForm(nn.Module):
    """The model of vfm-tomasrch.py (`class CF`, :186-453): G id groups, learnable group priors, closed-form
    expected log-likelihood -- same parameter names and shapes, so state_dicts of the two line up.
    `elbo(x, y)` is the loss of :569-588 (differentiable); `fit` its Adam loop (:464-590, lr as given there)."""

    def __init__(self, group_sizes: Sequence[int], embedding_size: int = 2, alpha_0: float = 300.0, device="cuda"):
        super().__init__()
        self.group_sizes = [int(s) for s in group_sizes]
        self.G, self.T, self.d = len(self.group_sizes), int(sum(self.group_sizes)), int(embedding_size)
        G, d, start_scale = self.G, self.d, 0.2
        # same construction order as the reference (RNG: mean_global_bias, bias means per group, entity means per group)
        self.alpha = nn.Parameter(torch.tensor([float(alpha_0)]))
        self.mean_global_bias_prior = nn.Parameter(torch.zeros(1))
        self.scale_global_bias_prior = nn.Parameter(torch.ones(1))
        self.mean_global_bias = nn.Parameter(torch.normal(torch.zeros(1), torch.ones(1)))
        self.scale_global_bias = nn.Parameter(torch.tensor([start_scale]))
        self.mean_group_bias_prior = nn.ParameterList([nn.Parameter(torch.zeros(1)) for _ in range(G)])
        self.scale_group_bias_prior = nn.ParameterList([nn.Parameter(torch.ones(1)) for _ in range(G)])
        self.bias_params = nn.Parameter(torch.cat([
            torch.cat((torch.normal(torch.zeros(n, 1), 1e-1 * torch.ones(n, 1)), start_scale * torch.ones(n, 1)), 1)
            for n in self.group_sizes]))
        self.mean_group_entity_prior = nn.ParameterList([nn.Parameter(torch.zeros(d)) for _ in range(G)])
        self.scale_group_entity_prior = nn.ParameterList([nn.Parameter(torch.ones(d)) for _ in range(G)])
        self.entity_params = nn.Parameter(torch.cat([
            torch.cat((torch.normal(torch.zeros(n, d), 1e-7 * torch.ones(n, d)), start_scale * torch.ones(n, d)), 1)
            for n in self.group_sizes]))
        self.to(device)
        self.nb_train, self.inv_occ = 1, None
        self._step = None                # VariantStepState of train_step / fit(fused=True)

    def spec(self) -> ops.Spec:
        return ops.Spec(T=self.T, F=self.G, d=self.d, group_hi=tuple(int(v) for v in np.cumsum(self.group_sizes)),
                        group_n=tuple(float(s) for s in self.group_sizes), likelihood=_lib.LIK_NORMAL,
                        nb_train=int(self.nb_train))

    def set_training_data(self, X_train, nb_train: Optional[int] = None, nb_occ=None):
        """entity_count = bincount(X_train.flatten()) (vfm-tomasrch.py:182)."""
        X_train = torch.as_tensor(X_train)
        self.nb_train = int(nb_train if nb_train is not None else X_train.shape[0])
        dev = self.alpha.device
        if nb_occ is None:
            nb_occ = torch.bincount(X_train.reshape(-1).to(dev).to(torch.int64), minlength=self.T)
        self.inv_occ = ops.inv_occ_from_counts(torch.as_tensor(nb_occ).to(dev).to(torch.int64).contiguous())

    def priors_flat(self) -> torch.Tensor:
        return torch.cat([self.mean_global_bias_prior, self.scale_global_bias_prior,
                          torch.cat(list(self.mean_group_bias_prior)), torch.cat(list(self.scale_group_bias_prior)),
                          torch.cat(list(self.mean_group_entity_prior)), torch.cat(list(self.scale_group_entity_prior))])

    def plan(self, x, y=None) -> ops.BatchPlan:
        dev = self.alpha.device
        x = torch.as_tensor(x).to(dev).contiguous()
        y = torch.as_tensor(y).to(dev) if y is not None else None
        return ops.BatchPlan(self.spec(), x, y, self.inv_occ if y is not None else None)

    def elbo(self, x=None, y=None, plan=None, values=None):
        """(loss[1], y_bar[B], (loss, likelihood term, KL term)) of one batch -- vfm-tomasrch.py:548-588."""
        self.sync_parameters()
        if plan is None:
            plan = self.plan(x, y)
        scalars = torch.cat([self.alpha, self.mean_global_bias, self.scale_global_bias])
        return VariantElbo.apply(self.entity_params, self.bias_params, scalars, self.priors_flat(), plan, self.inv_occ,
                                 "closed_form", values, None, 0, 0)

    @torch.no_grad()
    def forward(self, x, values=None):
        """y_bar of the rows x (the mean prediction the reference reports, vfm-tomasrch.py:342-347 for two groups)."""
        self.sync_parameters()
        plan = self.plan(x, None)
        scalars = torch.cat([self.alpha, self.mean_global_bias, self.scale_global_bias]).contiguous()
        return variant_forward(plan, "closed_form", self.entity_params.detach(), self.bias_params.detach(), scalars, None,
                               values=values, train=False)["pred"]

    # ------------------------------------------------------------------ fused step (include/vfm_variant_step.h)
    def step_state(self) -> VariantStepState:
        """The state `train_step` trains on (built from the named parameters on first use)."""
        if self._step is None:
            self._step = VariantStepState(self)
        return self._step

    @torch.no_grad()
    def sync_parameters(self):
        """Scatter the flat scalars and priors `train_step` updates back into alpha, mean_global_bias, ... and the
        ParameterLists, so that state_dict(), forward() and the ranking / fold-in callers see the trained values.  (The two
        tables are updated in place and need no copy.)"""
        s = self._step
        if s is None or not s.dirty:
            return
        G, d = self.G, self.d
        for i, p in enumerate((self.alpha, self.mean_global_bias, self.scale_global_bias)):
            p.copy_(s.scalars[i:i + 1])
        pr = s.priors
        self.mean_global_bias_prior.copy_(pr[0:1])
        self.scale_global_bias_prior.copy_(pr[1:2])
        pv = 2 + 2 * G
        for g in range(G):
            self.mean_group_bias_prior[g].copy_(pr[2 + g:3 + g])
            self.scale_group_bias_prior[g].copy_(pr[2 + G + g:3 + G + g])
            self.mean_group_entity_prior[g].copy_(pr[pv + g * d:pv + (g + 1) * d])
            self.scale_group_entity_prior[g].copy_(pr[pv + G * d + g * d:pv + G * d + (g + 1) * d])
        s.dirty = False

    @torch.no_grad()
    def train_step(self, plan: ops.BatchPlan, lr: float):
        """One fused training step on `plan` (built with y): vfm_variant_fwd_f32, then backward + torch.optim.Adam's update
        in vfm_variant_step_f32.  Returns the device tensor loss3 = (loss, likelihood term, KL term) of the batch BEFORE the
        update; no host synchronisation.  The named scalar / prior parameters lag until `sync_parameters()`."""
        s = self.step_state()
        ent, bia = self.entity_params.data, self.bias_params.data
        st = variant_forward(plan, "closed_form", ent, bia, s.scalars, self.inv_occ, priors=s.priors)
        variant_adam_step(plan, st, ent, bia, s.scalars, s.priors, self.inv_occ, s.moments, lr, s.t + 1,
                          grad_out=s.grad_out, workspace=s.workspace(plan))
        s.t += 1
        s.dirty = True
        return st["loss3"]

    def state_dict(self, *args, **kwargs):
        self.sync_parameters()
        return super().state_dict(*args, **kwargs)

    def load_state_dict(self, *args, **kwargs):
        self._step = None                # (the flat buffers and moments belonged to the parameters being replaced)
        return super().load_state_dict(*args, **kwargs)

    def training_state_dict(self):
        """Parameters (state_dict) plus the fused step's Adam moments and step count: what `train_step` needs to go on
        bit for bit (named after VFM.training_state_dict)."""
        self.sync_parameters()
        adam = None
        if self._step is not None:
            adam = dict(self._step.moments.state_dict(), t=int(self._step.t))
        return {"model": {k: v.detach().cpu().clone() for k, v in self.state_dict().items()}, "adam": adam,
                "nb_train": int(self.nb_train)}

    def load_training_state_dict(self, state):
        self.load_state_dict(state["model"])
        self.nb_train = int(state.get("nb_train", self.nb_train))
        self._step = None
        if state.get("adam") is not None:
            s = self.step_state()        # (flat buffers from the parameters just loaded)
            s.moments.load_state_dict(state["adam"])
            s.t = int(state["adam"]["t"])

    def fit(self, X_train, y_train, n_epochs=10, batch_size=8000, lr=0.02, verbose=False, fused=False, on_epoch=None):
        """The Adam loop of vfm-tomasrch.py:464-590 (sequential batches, no shuffle, :177-178).  fused=True: the same loop
        on `train_step` (a fresh optimiser state, as the loop below builds a fresh torch.optim.Adam); the named parameters
        are synced at the end and before `on_epoch(epoch, mean loss)` is called."""
        X_train, y_train = torch.as_tensor(X_train), torch.as_tensor(y_train, dtype=torch.float32)
        self.set_training_data(X_train)
        if fused:
            return self._fit_fused(X_train, y_train, n_epochs, batch_size, lr, verbose, on_epoch)
        opt = torch.optim.Adam(self.parameters(), lr=lr)
        plans = [self.plan(X_train[lo:lo + batch_size], y_train[lo:lo + batch_size])
                 for lo in range(0, len(y_train), batch_size)]
        hist = []
        for epoch in range(n_epochs):
            tot = 0.0
            for plan in plans:
                loss, _, _ = self.elbo(plan=plan)
                opt.zero_grad()
                loss.backward()
                opt.step()
                tot += float(loss.detach())
            hist.append(tot / len(plans))
            if verbose:
                print(f"epoch {epoch}: elbo {hist[-1]:.4f}")
            if on_epoch is not None:
                on_epoch(epoch, hist[-1])
        return hist

    def _fit_fused(self, X_train, y_train, n_epochs, batch_size, lr, verbose, on_epoch):
        self._step = VariantStepState(self)
        plans = [self.plan(X_train[lo:lo + batch_size], y_train[lo:lo + batch_size])
                 for lo in range(0, len(y_train), batch_size)]
        hist, self.batch_losses = [], []          # batch_losses: [epoch] -> fp32 tensor of the epoch's batch losses (host)
        for epoch in range(n_epochs):
            losses = torch.cat([self.train_step(plan, lr)[0:1] for plan in plans]).cpu()      # one readback per epoch
            self.batch_losses.append(losses)
            hist.append(float(losses.double().mean()))
            for plan in plans:
                plan.check_status()
            if verbose:
                print(f"epoch {epoch}: elbo {hist[-1]:.4f}")
            if on_epoch is not None:
                self.sync_parameters()
                on_epoch(epoch, hist[-1])
        self.sync_parameters()
        return hist

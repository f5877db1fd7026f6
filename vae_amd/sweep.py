"""Coordinate-ascent training by per-entity solves: VFM.fit_exact ('reg', include/vfm_sweep.h) and VFM.fit_bound ('class',
include/vfm_bound_sweep.h), and the split solves behind them.

`fold_in_exact` over every row of a training set, field after field, is exact coordinate-ascent variational inference
on one objective J ("Exact sweeps"): each call is the exact minimiser of J over one field's factors.  This
module holds what such a sweep needs beyond foldin.run_exact:

  SweepPlan        the sorted rows, row lists, partner tuples and chunk table of one (X, y, field), built once
  exact_objective  J itself, from the predictive_moments kernel's per-row moments and the tables, summed in fp64
  update_scalars   the exact block minimisers of the global bias and of the precision
  fit              the sweeps

Entities with more rows than the plan's threshold go through vfm_foldin_solve_split_f32 (their system assembled by a
workgroup per chunk of rows), the others through vfm_foldin_solve_f32, unchanged.

With a GroupPriors (include/vfm_prior.h; DESIGN.md §4, "Hierarchical sweeps") every field has a Gaussian prior
N(m, 1 / lam) per coordinate in place of N(0, 1): the same plan solves under it (vfm_foldin_solve_prior_f32,
vfm_foldin_solve_split_prior_f32), update_prior is the prior's own exact block minimiser, and J carries the KL to it.
The prior's minimiser depends on q alone, so fit_bound takes the same GroupPriors (include/vfm_bound_prior.h; DESIGN.md
§4, "Hierarchical bound sweeps"): vfm_foldin_bound_prior_f32 and vfm_foldin_bound_split_prior_f32 run the rounds under it.

For a 'class' model the same plan runs the Jaakkola-Jordan bound's rounds ("Bound sweeps"): light
entities through vfm_foldin_bound_f32, unchanged, heavy ones through vfm_foldin_bound_split_f32;

  bound_objective  J of fit_bound, from the same moments
  update_bias_bound  the global bias' exact block minimiser under the bound at the current xi
  fit_bound        the sweeps

For clicks or plays a two-field 'reg' model takes every (user, item) pair as a row ("Implicit sweeps";
include/vfm_implicit.h): an observed pair with its target and weight w1, every other pair with target 0 and weight w0;

  ImplicitPlan        a SweepPlan of the observed rows, each row's partner id and the entities without rows
  implicit_sums       the weighted all-pairs sums, closed forms of the two fields' Grams corrected at the observed rows
  fit_implicit        the sweeps: per field one base block of the partner field, then every entity's solve from it

and under a GroupPriors (include/vfm_implicit_prior.h; DESIGN.md §4, "Hierarchical implicit sweeps") the same plan solves
under the folded field's prior (vfm_foldin_solve_implicit_prior_f32), J_imp carries every entity's KL to its field's prior
and the prior block (update_prior) runs over the field's whole id range: an entity without observed rows is in J_imp.
With weights= (include/vfm_implicit_weights.h; DESIGN.md §4, "Weighted implicit sweeps") every observed row carries a
weight of its own in place of the one w1 (hkv_weights: Hu, Koren & Volinsky's confidence from counts): the plan carries
the weights into its row order as it carries the targets, the solves are vfm_foldin_solve_implicit_weights_f32 and
implicit_sums corrects the all-pairs sums with each row's own weight.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib, foldin, ops, rank

LOG_2PI_HALF = 0.5 * math.log(2.0 * math.pi)
MAX_WORKSPACE_BYTES = 1 << 30


class GroupPriors:
    """The Gaussian prior of every field of a model: mean [F, d + 1] and prec [F, d + 1] fp32 (column 0: the
    first-order weight, 1 .. d: the factors), N(mean, 1 / prec) per coordinate.  It starts at (0, 1), the N(0, 1) every
    other path of the package assumes.  Held outside the model, like a session's theta: a model file stays a model file;
    state_dict / load_state_dict keep it beside one."""

    def __init__(self, F, d, device="cpu"):
        if isinstance(F, bool) or isinstance(d, bool) or int(F) != F or int(d) != d or F < 1 or d < 1:
            raise ValueError("GroupPriors(F, d): F and d must be integers >= 1")
        self.F, self.d = int(F), int(d)
        self.mean = torch.zeros(self.F, self.d + 1, dtype=torch.float32, device=device)
        self.prec = torch.ones(self.F, self.d + 1, dtype=torch.float32, device=device)

    def state_dict(self):
        return {"mean": self.mean.detach().clone(), "prec": self.prec.detach().clone()}

    def load_state_dict(self, state):
        if set(state) != {"mean", "prec"}:
            raise ValueError('a GroupPriors state holds "mean" and "prec"')
        for k in ("mean", "prec"):
            t = torch.as_tensor(state[k])
            if tuple(t.shape) != (self.F, self.d + 1):
                raise ValueError(f"{k} must be [{self.F}, {self.d + 1}], not {list(t.shape)}")
        mean = torch.as_tensor(state["mean"]).to(self.mean.device, torch.float32)
        prec = torch.as_tensor(state["prec"]).to(self.prec.device, torch.float32)
        _check_prior_values(mean, prec)
        self.mean.copy_(mean)
        self.prec.copy_(prec)

    def row(self, field):
        """Field `field`'s prior as the kernels read it: [2, d + 1] fp32, mean | precision."""
        if isinstance(field, bool) or not isinstance(field, int) or not 0 <= field < self.F:
            raise ValueError(f"field must be an int in [0, {self.F})")
        return torch.stack([self.mean[field], self.prec[field]]).contiguous()

    def validate(self):
        """ValueError unless every value is finite and every precision > 0 (before any kernel reads them)."""
        _check_prior_values(self.mean, self.prec)
        return self


def _check_prior_values(mean, prec):
    if not bool(torch.isfinite(mean).all()) or not bool(torch.isfinite(prec).all()):
        raise ValueError("priors: mean and prec must be finite")
    if not bool((prec > 0).all()):
        raise ValueError("priors: prec must be > 0 (a prior precision is what makes each system positive definite)")


def check_priors(model, priors):
    """Validate a priors= argument (no kernel runs): None, or a GroupPriors of the model's F and d with finite values
    and prec > 0.  Returns it."""
    if priors is None:
        return None
    if not isinstance(priors, GroupPriors):
        raise ValueError("priors must be a sweep.GroupPriors or None")
    if priors.F != model.F or priors.d != model.d:
        raise ValueError(f"priors are for F = {priors.F}, d = {priors.d}; the model has F = {model.F}, d = {model.d}")
    return priors.validate()


def _prior_row(model, priors, field):
    return None if priors is None else priors.row(int(field)).to(model.device)


def check_prec_bounds(prec_min, prec_max):
    lo, hi = float(prec_min), float(prec_max)
    if not (math.isfinite(lo) and math.isfinite(hi) and 0.0 < lo <= hi):
        raise ValueError("prec_min and prec_max must be finite with 0 < prec_min <= prec_max")
    f32 = torch.tensor([lo, hi], dtype=torch.float64).float()
    if float(f32[0]) <= 0.0 or not math.isfinite(float(f32[1])):
        raise ValueError("prec_min and prec_max must be representable in fp32 (the prior tables are fp32)")
    return lo, hi


def resolve_split_rows(split_rows, d):
    """The row count above which an entity is split: None (never), "auto" = 4 (d + 1), or an integer; at least d + 1, so
    that a split entity is always solved in the primal form."""
    if split_rows is None:
        return None
    if isinstance(split_rows, str):
        if split_rows != "auto":
            raise ValueError('split_rows must be None, "auto" or an integer >= 0')
        return 4 * (d + 1)
    if isinstance(split_rows, bool) or not isinstance(split_rows, int) or split_rows < 0:
        raise ValueError('split_rows must be None, "auto" or an integer >= 0')
    return max(split_rows, d + 1)


def check_chunk_rows(chunk_rows):
    if isinstance(chunk_rows, bool) or not isinstance(chunk_rows, int) or chunk_rows < 1:
        raise ValueError("chunk_rows must be an integer >= 1")
    return chunk_rows


def chunk_table(first, counts, chunk_rows):
    """The chunk table of entities whose rows start at first [E] and number counts [E] (numpy int64): (chunk_ptr [E + 1],
    chunks [n_chunks, 3] = (entity number, first row, rows)), an entity's chunks consecutive and in row order."""
    first, counts = np.asarray(first, np.int64), np.asarray(counts, np.int64)
    nch = (counts + chunk_rows - 1) // chunk_rows
    ptr = np.zeros(counts.size + 1, np.int64)
    np.cumsum(nch, out=ptr[1:])
    ent = np.repeat(np.arange(counts.size, dtype=np.int64), nch)
    k = np.arange(int(ptr[-1]), dtype=np.int64) - ptr[ent]
    rows = np.minimum(chunk_rows, counts[ent] - k * chunk_rows)
    return ptr, np.stack([ent, first[ent] + k * chunk_rows, rows], 1).reshape(-1, 3)


class SweepPlan:
    """Everything about one (X, y, field) that an exact solve needs and that does not depend on the parameters: the rows
    sorted (stably) by (split or not, folded id), so that the light entities come first with a contiguous row_ptr and the
    heavy ones after; the partner tuples and each row's tuple; the heavy entities' chunk table, cut in groups whose
    workspace stays under max_workspace_bytes.  Building it reads the row counts back once; running it reads nothing
    back.  x, y: as foldin.check_args_exact returns them.  The plan does not depend on the likelihood but for the size
    of a group: bound=True sizes the groups by the workspace of the split bound rounds (run_bound) instead of the split
    exact solve's (run)."""

    def __init__(self, model, x, y, field, split_rows=None, chunk_rows=2048, max_workspace_bytes=MAX_WORKSPACE_BYTES,
                 lds_dim=-1, bound=False, split_bytes=None):
        # split_bytes(n_chunks, n_heavy, n_ops, d, lds_dim): another split form's workspace (ImplicitPlan)
        self.field, self.d, self.lds_dim = int(field), model.d, int(lds_dim)
        self.threshold = resolve_split_rows(split_rows, model.d)
        self.chunk_rows = check_chunk_rows(chunk_rows)
        dev = x.device
        lo, hi = foldin.field_range(model, field)
        col = x[:, field]
        if self.threshold is None or x.shape[0] == 0:
            key = col
        else:
            per_id = torch.bincount(col - lo, minlength=hi - lo)
            key = col + (per_id[col - lo] > self.threshold).to(torch.int64) * model.T      # (heavy ids sort last)
        order = torch.sort(key, stable=True).indices
        self.order = order                                    # (what else is per row follows it: ImplicitPlan's weights)
        xs, self.ys = x[order].contiguous(), y[order].contiguous()
        self.ents, counts = torch.unique_consecutive(xs[:, field], return_counts=True)
        self.ents = self.ents.contiguous()
        self.E = self.ents.numel()
        self.ptr = torch.zeros(self.E + 1, dtype=torch.int64, device=dev)
        torch.cumsum(counts, 0, out=self.ptr[1:])
        self.counts = counts
        self.op_x, self.row_op = foldin.partner_tuples(xs, field) if self.E else (None, None)
        self.asc = torch.sort(self.ents).indices              # the entities in ascending order, as fold_in returns them
        self.n_light, self.groups = self.E, []
        if self.threshold is None or self.E == 0:
            return
        cnt = counts.cpu().numpy()                            # (the one readback)
        heavy = cnt > self.threshold
        self.n_light = int(self.E - heavy.sum())
        assert not heavy[:self.n_light].any()
        if self.n_light == self.E:
            return
        first = np.concatenate([[0], np.cumsum(cnt)])[:-1]
        n_ops, nch = self.op_x.shape[0], (cnt + self.chunk_rows - 1) // self.chunk_rows
        if split_bytes is not None:
            wsb = split_bytes
        elif bound:
            n_rows, bsb = int(x.shape[0]), _lib.load().vfm_foldin_bound_split_workspace_bytes
            wsb = lambda n_chunks, n_heavy, n_ops, d, lds_dim: bsb(n_chunks, n_heavy, n_rows, n_ops, d, lds_dim)
        else:
            wsb = _lib.load().vfm_foldin_split_workspace_bytes
        g0, chunks = self.n_light, 0
        bounds = []
        for g in range(self.n_light, self.E):                 # greedy: a group takes entities while its workspace fits
            if g > g0 and wsb(chunks + int(nch[g]), g + 1 - g0, n_ops, self.d, self.lds_dim) > max_workspace_bytes:
                bounds.append((g0, g))
                g0, chunks = g, 0
            chunks += int(nch[g])
        bounds.append((g0, self.E))
        for a, b in bounds:
            cptr, tab = chunk_table(first[a:b], cnt[a:b], self.chunk_rows)
            self.groups.append((a, b, torch.from_numpy(cptr).to(dev), torch.from_numpy(np.ascontiguousarray(tab)).to(dev)))

    def _solve(self, model, kl_weight, light, split, lik, rows=(), mid=(), tail=()):
        """One pass over the plan: the light entities in one call, then a call per group of heavy ones.  light, split:
        the form's (workspace-size op, solve op) pairs; lik: the light op's likelihood; rows: what the size ops take
        between the entity counts and n_ops; mid: what the solve ops take behind the loss (the prior); tail: behind
        kl_weight (the bound's n_iters and reset).  Returns (entities [E] ascending, loss [E], rows [E])."""
        dev = model.device
        loss = torch.empty(self.E, dtype=torch.float32, device=dev)
        if self.E == 0:
            return self.ents, loss, self.counts
        model._fresh_params()
        data = (self.ys, self.op_x, self.row_op, *model._views(model._flat))
        opts = (foldin._link_flags(model), self.lds_dim, float(kl_weight), *tail)

        def workspace(size, *counts):
            n = size(*counts, *rows, self.op_x.shape[0], self.d, self.lds_dim)
            return torch.empty(max(n, 1), dtype=torch.uint8, device=dev)

        if self.n_light:
            nl = self.n_light
            light[1](self.ents[:nl], self.ptr[:nl + 1], *data, workspace(light[0], nl), loss[:nl], *mid, self.field,
                     foldin.OBJECTIVES["closed_form"], lik, *opts)
        for a, b, cptr, tab in self.groups:
            split[1](self.ents[a:b], cptr, tab, *data, workspace(split[0], tab.shape[0], b - a), loss[a:b], *mid,
                     self.field, *opts)
        model.params_changed()              # (rows written outside the step kernels: derived caches are stale)
        return self.ents[self.asc], loss[self.asc], self.counts[self.asc]

    def run(self, model, kl_weight, prior=None):
        """Write the exact optimum of every entity of the plan into the model's tables.  prior: None (N(0, 1), the parent
        entry points) or the folded field's [2, d + 1] fp32 mean | precision on the device (include/vfm_prior.h).
        Returns (entities [E] ascending, loss [E], rows [E])."""
        o = _lib.ops()
        light, split, mid = ((o.foldin_solve, o.foldin_solve_split, ()) if prior is None else
                             (o.foldin_solve_prior, o.foldin_solve_split_prior, (prior,)))
        return self._solve(model, kl_weight, (o.foldin_solve_workspace_bytes, light),
                           (o.foldin_split_workspace_bytes, split), _lib.LIK_NORMAL, mid=mid)

    def run_bound(self, model, kl_weight, n_iters, reset=False, prior=None):
        """n_iters rounds of the bound's two block minimisers for every entity of the plan, written into the model's
        tables: the light entities by vfm_foldin_bound_f32, the heavy ones by vfm_foldin_bound_split_f32.  prior: None
        (N(0, 1), the parent entry points) or the folded field's [2, d + 1] fp32 mean | precision on the device
        (include/vfm_bound_prior.h).  Returns (entities [E] ascending, loss [E] = B_e, rows [E])."""
        o = _lib.ops()
        light, split, mid = ((o.foldin_bound, o.foldin_bound_split, ()) if prior is None else
                             (o.foldin_bound_prior, o.foldin_bound_split_prior, (prior,)))
        return self._solve(model, kl_weight,
                           (o.foldin_bound_workspace_bytes, lambda *a: light(*a, foldin.MODE_FIT)),
                           (o.foldin_bound_split_workspace_bytes, split), _lib.LIK_BERNOULLI,
                           rows=(self.ys.numel(),), mid=mid, tail=(int(n_iters), int(bool(reset))))


def _run_split(model, x, y, field, split_rows, chunk_rows, max_workspace_bytes, lds_dim, bound, run):
    """The body of the two split entry points over checked rows: the plan's own arguments checked, the plan, run(plan)."""
    resolve_split_rows(split_rows, model.d)
    check_chunk_rows(chunk_rows)
    foldin._check_lds_dim(lds_dim)
    if int(max_workspace_bytes) < 0:
        raise ValueError("max_workspace_bytes must be >= 0")
    ops._need_cuda(model._flat, "the model's parameters")
    return run(SweepPlan(model, x, y, field, split_rows, chunk_rows, int(max_workspace_bytes), lds_dim, bound=bound))


def run_bound_split(model, X, y, field=0, kl_weight=1.0, n_iters=8, reset=False, split_rows="auto", chunk_rows=2048,
                    max_workspace_bytes=MAX_WORKSPACE_BYTES, lds_dim=-1, priors=None):
    """foldin.run_bound with the entities of more than max(split_rows, d + 1) rows run by the split path; the same
    output contract: (entities [E] ascending, loss [E] = B_e, rows [E])."""
    x, y = foldin.check_args_bound(model, X, y, field, kl_weight, n_iters)
    check_priors(model, priors)
    return _run_split(model, x, y, field, split_rows, chunk_rows, max_workspace_bytes, lds_dim, True,
                      lambda plan: plan.run_bound(model, kl_weight, n_iters, reset, _prior_row(model, priors, field)))


def run_exact_split(model, X, y, field=0, kl_weight=1.0, split_rows="auto", chunk_rows=2048,
                    max_workspace_bytes=MAX_WORKSPACE_BYTES, lds_dim=-1, priors=None):
    """foldin.run_exact with the entities of more than max(split_rows, d + 1) rows solved by the split path."""
    x, y = foldin.check_args_exact(model, X, y, field, kl_weight)
    check_priors(model, priors)
    return _run_split(model, x, y, field, split_rows, chunk_rows, max_workspace_bytes, lds_dim, False,
                      lambda plan: plan.run(model, kl_weight, _prior_row(model, priors, field)))


# ---------------------------------------------------------------------------------------------------------------------
# the objective and the scalars
# ---------------------------------------------------------------------------------------------------------------------
def _link64(s, link):
    s = s.double()
    return s.abs() if link == "abs" else torch.nn.functional.softplus(s)


def _inv_link64(v, link):
    return v if link == "abs" else torch.log(torch.expm1(v))


def _kl64(mu, sg):
    return 0.5 * (sg * sg + mu * mu - 1.0) - torch.log(sg)


def _kl64_prior(mu, sg, m, lam):
    """KL(N(mu, sg^2) || N(m, 1 / lam)) = 1/2 (lam sg^2 + lam (mu - m)^2 - 1 - log(lam sg^2))."""
    v = lam * sg * sg
    return 0.5 * (v + lam * (mu - m) ** 2 - 1.0 - torch.log(v))


def _add_kl64_rows(kl, e, b, d, link):
    """kl plus the N(0, 1) KL of the table rows e [n, 2d], b [n, 2]: the factors' sum, then the weights'.  Two sums
    added in this order: the objectives' fp64 bits depend on it."""
    kl = kl + _kl64(e[:, :d].double(), _link64(e[:, d:], link)).sum()
    return kl + _kl64(b[:, 0].double(), _link64(b[:, 1], link)).sum()


def _add_kl64_rows_prior(kl, e, b, d, link, m, lam):
    """_add_kl64_rows with the KL to N(m, 1 / lam), m and lam [n, d + 1] (column 0: the weight), taken as the kernels take
    it: KL(N(mu, sg^2) || N(m, 1 / lam)) = KL(N(sqrt(lam) (mu - m), lam sg^2) || N(0, 1)).  At m = 0, lam = 1 every
    operation is _add_kl64_rows', so the objective's fp64 bits are those of priors=None."""
    sl = torch.sqrt(lam)
    kl = kl + _kl64(sl[:, 1:] * (e[:, :d].double() - m[:, 1:]), sl[:, 1:] * _link64(e[:, d:], link)).sum()
    return kl + _kl64(sl[:, 0] * (b[:, 0].double() - m[:, 0]), sl[:, 0] * _link64(b[:, 1], link)).sum()


def _field_of(model, ids):
    """The field of each id (ids within [0, T))."""
    edges = torch.tensor(np.cumsum(model.field_sizes)[:-1].tolist(), dtype=torch.int64, device=ids.device)
    return torch.bucketize(ids, edges, right=True)


def _theta64(model, ids):
    """(mu [n, d + 1], sigma [n, d + 1]) in fp64 of the table rows `ids`, column 0 the first-order weight."""
    d = model.d
    ent, bia, _ = model._views(model._flat)
    e, b = ent[ids], bia[ids]
    mu = torch.cat([b[:, :1], e[:, :d]], 1).double()
    sg = _link64(torch.cat([b[:, 1:], e[:, d:]], 1), model.link)
    return mu, sg


def _moments64(model, x):
    ent, bia, scal = model._views(model._flat)
    m, v, _ = rank.predictive_moments(x, ent, bia, scal, model.link)
    return m.double(), v.double()


def objective_terms(model, x, y, seen, kl_weight, priors=None):
    """J as a 0-dim fp64 tensor on the device: the rows' expected negative log likelihood from the predictive_moments
    kernel's fp32 moments, the KL of the entities `seen` (distinct ids) and of the global bias from the tables.  priors:
    the entities' KL is to their field's N(mean, 1 / prec); the global bias keeps N(0, 1)."""
    ent, bia, scal = model._views(model._flat)
    prec = _link64(scal[0], model.link)
    n = x.shape[0]
    J = torch.zeros((), dtype=torch.float64, device=x.device)
    if n:
        m, v = _moments64(model, x)
        J = J + 0.5 * prec * ((y.double() - m) ** 2 + v).sum() + n * (LOG_2PI_HALF - 0.5 * torch.log(prec))
    kl = _kl64(scal[1].double(), _link64(scal[2], model.link))
    if seen.numel() and priors is not None:
        f = _field_of(model, seen)
        mu, sg = _theta64(model, seen)
        kl = kl + _kl64_prior(mu, sg, priors.mean.to(x.device).double()[f], priors.prec.to(x.device).double()[f]).sum()
    elif seen.numel():
        kl = _add_kl64_rows(kl, ent[seen], bia[seen], model.d, model.link)
    return J + float(kl_weight) * kl


def prior_block64(mu, sg, m_old, learn_mean, prec_min, prec_max):
    """The exact minimiser of J over one field's prior, from its seen entities' mu, sigma [n, d + 1] (fp64):
    m* = mean_e mu (learn_mean; else m_old), 1 / lam* = mean_e (sigma^2 + (mu - m*)^2), lam* clamped to
    [prec_min, prec_max] (KL is unimodal in 1 / lam: the clamped value is the constrained minimiser).  Returns
    (m* [d + 1], lam* [d + 1], the number of coordinates at which a clamp binds)."""
    m = mu.mean(0) if learn_mean else m_old
    lam = 1.0 / (sg * sg + (mu - m) ** 2).mean(0)
    return m, lam.clamp(prec_min, prec_max), ((lam < prec_min) | (lam > prec_max)).sum()


def update_prior(model, priors, field, seen_f, learn_mean=True, prec_min=1e-4, prec_max=1e4):
    """Field `field`'s prior block, written into `priors` in place: prior_block64 in torch fp64 on the device from the
    table rows of seen_f (the field's ids that occur in X), rounded to fp32 when stored.  No readback.  Returns the
    0-dim int64 count of coordinates clamped (None when the field has no seen entity: nothing is written)."""
    if seen_f.numel() == 0:
        return None
    mu, sg = _theta64(model, seen_f)
    m, lam, n_clamped = prior_block64(mu, sg, priors.mean[field].to(mu.device).double(), learn_mean, prec_min, prec_max)
    priors.mean[field] = m.float().to(priors.mean.device)
    priors.prec[field] = lam.float().to(priors.prec.device)
    return n_clamped


def update_scalars(model, x, y, kl_weight):
    """The exact block minimisers of J over the scalars, written in place: first the global bias (mean and scale
    jointly), then the precision from the moments recomputed after it.  No readback."""
    n = x.shape[0]
    if n == 0:
        return
    scal = model._views(model._flat)[2]
    kl = float(kl_weight)
    yd = y.double()
    prec = _link64(scal[0], model.link)
    m, _ = _moments64(model, x)
    m0 = scal[1].double()
    den = kl + prec * n
    new_m0 = prec * (yd - (m - m0)).sum() / den
    new_s0 = _inv_link64(torch.sqrt(kl / den), model.link)
    scal[1:3] = torch.stack([new_m0, new_s0]).float()
    m, v = _moments64(model, x)
    new_prec = n / ((yd - m) ** 2 + v).sum()
    scal[0:1] = _inv_link64(new_prec, model.link).float().reshape(1)


_FIT_MODEL = {"reg": "fit_exact needs a 'reg' model (Gaussian likelihood): the closed form its blocks solve has none for "
                     "'class'; use fit",
              "class": "fit_bound needs a 'class' model (Bernoulli likelihood): a 'reg' model's blocks have their exact "
                       "optimum; use fit_exact"}


def check_fit_args(model, X, y, kind, check_field, n_sweeps, fields, split_rows, chunk_rows, tol):
    """Validate a fit_exact (kind 'reg') or fit_bound ('class') call (no GPU needed); check_field(f) -> (x, y): the
    fold-in's own check of the rows with field f folded, kl_weight (and n_iters) with it.  Returns (x, y, fields)."""
    if model.output != kind:
        raise ValueError(_FIT_MODEL[kind])
    if isinstance(n_sweeps, bool) or not isinstance(n_sweeps, int) or n_sweeps < 0:
        raise ValueError("n_sweeps must be an integer >= 0")
    if fields is None:
        fields = tuple(range(model.F))
    else:
        fields = tuple(fields)
        for f in fields:
            if isinstance(f, bool) or not isinstance(f, int) or not 0 <= f < model.F:
                raise ValueError(f"fields must hold ints in [0, {model.F})")
    resolve_split_rows(split_rows, model.d)
    check_chunk_rows(chunk_rows)
    if tol is not None and not float(tol) >= 0.0:
        raise ValueError("tol must be None or >= 0")
    x = yy = None
    for f in range(model.F):                                  # (every column is some block's or a partner of one)
        x, yy = check_field(f)
    return x, yy, fields


def _check_fit_exact(model, X, y, n_sweeps, kl_weight, fields, split_rows, chunk_rows, tol):
    return check_fit_args(model, X, y, "reg", lambda f: foldin.check_args_exact(model, X, y, f, kl_weight), n_sweeps,
                          fields, split_rows, chunk_rows, tol)


def _check_fit_bound(model, X, y, n_sweeps, kl_weight, n_iters, fields, split_rows, chunk_rows, tol):
    return check_fit_args(model, X, y, "class", lambda f: foldin.check_args_bound(model, X, y, f, kl_weight, n_iters),
                          n_sweeps, fields, split_rows, chunk_rows, tol)


def _sweeps(model, fields, n_sweeps, tol, on_step, objective, run_block, after_block=None, after_sweep=None, tag=None):
    """The sweep loop of fit and fit_bound: per sweep run_block(f) for every field, after_block(f) behind each where
    given (the prior's update, on_step's ("prior", f)), then after_sweep() where given (the scalars' blocks, on_step's
    `tag`), then objective(); it stops at the tol rule.  Returns {"objective", "sweeps", "ms"}."""
    values = [float(objective())]
    events = []
    for sweep in range(n_sweeps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for f in fields:
            run_block(f)
            if on_step is not None:
                on_step(sweep, f)
            if after_block is not None:
                after_block(f)
                if on_step is not None:
                    on_step(sweep, ("prior", f))
        if after_sweep is not None:
            after_sweep()
            if on_step is not None:
                on_step(sweep, tag)
        t1.record()
        events.append((t0, t1))
        values.append(float(objective()))
        if tol is not None and values[-2] - values[-1] <= float(tol) * abs(values[-2]):
            break
    model.params_changed()
    torch.cuda.synchronize(model.device)
    return {"objective": values, "sweeps": len(events), "ms": [a.elapsed_time(b) for a, b in events]}


def exact_objective(model, X, y, kl_weight=1.0, priors=None):
    x, y, _ = _check_fit_exact(model, X, y, 0, kl_weight, None, None, 1, None)
    check_priors(model, priors)
    ops._need_cuda(model._flat, "the model's parameters")
    model._fresh_params()
    return float(objective_terms(model, x, y, torch.unique(x), kl_weight, priors))


def fit(model, X, y, n_sweeps=10, kl_weight=1.0, fields=None, update_scalars_=True, split_rows="auto", chunk_rows=2048,
        on_step=None, tol=None, max_workspace_bytes=MAX_WORKSPACE_BYTES, priors=None, learn_priors=False,
        learn_mean=True, prec_min=1e-4, prec_max=1e4):
    x, y, fields = _check_fit_exact(model, X, y, n_sweeps, kl_weight, fields, split_rows, chunk_rows, tol)
    check_priors(model, priors)
    prec_min, prec_max = check_prec_bounds(prec_min, prec_max)
    ops._need_cuda(model._flat, "the model's parameters")
    if learn_priors and priors is None:
        priors = GroupPriors(model.F, model.d, model.device)          # (created at N(0, 1), returned under "priors")
    model._fresh_params()
    seen = torch.unique(x)
    plans = {f: SweepPlan(model, x, y, f, split_rows, chunk_rows, max_workspace_bytes) for f in dict.fromkeys(fields)}
    seen_f = {f: plans[f].ents[plans[f].asc] for f in plans} if learn_priors else {}
    clamped = {f: torch.zeros((), dtype=torch.int64, device=x.device) for f in plans} if learn_priors else {}

    def learn_prior(f):
        n_clamped = update_prior(model, priors, f, seen_f[f], learn_mean, prec_min, prec_max)
        if n_clamped is not None:
            clamped[f] += n_clamped

    out = _sweeps(model, fields, n_sweeps, tol, on_step, lambda: objective_terms(model, x, y, seen, kl_weight, priors),
                  lambda f: plans[f].run(model, kl_weight, _prior_row(model, priors, f)),
                  learn_prior if learn_priors else None,
                  (lambda: update_scalars(model, x, y, kl_weight)) if update_scalars_ else None, "scalars")
    if priors is not None:
        out["priors"] = priors
    if learn_priors:
        out["clamped"] = {f: int(n) for f, n in clamped.items()}
    return out


# ---------------------------------------------------------------------------------------------------------------------
# 'class' models: the bound's objective, the global bias' block and the sweeps ("Bound sweeps")
# ---------------------------------------------------------------------------------------------------------------------
def _xi64(m, v):
    return torch.sqrt(torch.clamp(m * m + v, min=0.0))


def _jj_weight64(xi):
    """w = tanh(xi / 2) / (2 xi), 1/4 - xi^2 / 48 below 1e-3: the kernels' rule."""
    small = xi < 1e-3
    safe = torch.where(small, torch.ones_like(xi), xi)
    return torch.where(small, 0.25 - xi * xi / 48.0, torch.tanh(0.5 * safe) / (2.0 * safe))


def bound_objective_terms(model, x, y, seen, kl_weight, priors=None):
    """J of fit_bound as a 0-dim fp64 tensor on the device: the rows' collapsed bound terms
    -(y - 1/2) E f + xi / 2 + log1p(e^-xi), xi = sqrt((E f)^2 + Var f), from the predictive_moments kernel's fp32
    moments, the KL of the entities `seen` (distinct ids) and of the global bias from the tables.  priors: the
    entities' KL is to their field's N(mean, 1 / prec) (objective_terms' branch, in the standardised form that gives
    the bits of priors=None at the standard prior); the global bias keeps N(0, 1)."""
    ent, bia, scal = model._views(model._flat)
    J = torch.zeros((), dtype=torch.float64, device=x.device)
    if x.shape[0]:
        m, v = _moments64(model, x)
        xi = _xi64(m, v)
        J = J + (-(y.double() - 0.5) * m + 0.5 * xi + torch.log1p(torch.exp(-xi))).sum()
    kl = _kl64(scal[1].double(), _link64(scal[2], model.link))
    if seen.numel() and priors is not None:
        f = _field_of(model, seen)
        kl = _add_kl64_rows_prior(kl, ent[seen], bia[seen], model.d, model.link, priors.mean.to(x.device).double()[f],
                                  priors.prec.to(x.device).double()[f])
    elif seen.numel():
        kl = _add_kl64_rows(kl, ent[seen], bia[seen], model.d, model.link)
    return J + float(kl_weight) * kl


def update_bias_bound(model, x, y, kl_weight):
    """The exact block minimiser of the bound over the global bias (mean and scale jointly) at xi of the current
    posterior, written in place: m0 = sum_r ((y_r - 1/2) - w_r (E f_r - m0_old)) / (kl + sum_r w_r),
    s0^2 = kl / (kl + sum_r w_r).  scalars[0] is left alone.  No readback."""
    if x.shape[0] == 0:
        return
    scal = model._views(model._flat)[2]
    kl = float(kl_weight)
    m, v = _moments64(model, x)
    w = _jj_weight64(_xi64(m, v))
    den = kl + w.sum()
    new_m0 = ((y.double() - 0.5) - w * (m - scal[1].double())).sum() / den
    new_s0 = _inv_link64(torch.sqrt(kl / den), model.link)
    scal[1:3] = torch.stack([new_m0, new_s0]).float()


def bound_objective(model, X, y, kl_weight=1.0, priors=None):
    x, y, _ = _check_fit_bound(model, X, y, 0, kl_weight, 1, None, None, 1, None)
    check_priors(model, priors)
    ops._need_cuda(model._flat, "the model's parameters")
    model._fresh_params()
    return float(bound_objective_terms(model, x, y, torch.unique(x), kl_weight, priors))


def fit_bound(model, X, y, n_sweeps=10, kl_weight=1.0, n_iters=8, fields=None, update_bias=True, split_rows="auto",
              chunk_rows=2048, on_step=None, tol=None, max_workspace_bytes=MAX_WORKSPACE_BYTES, priors=None,
              learn_priors=False, learn_mean=True, prec_min=1e-4, prec_max=1e4):
    x, y, fields = _check_fit_bound(model, X, y, n_sweeps, kl_weight, n_iters, fields, split_rows, chunk_rows, tol)
    check_priors(model, priors)
    prec_min, prec_max = check_prec_bounds(prec_min, prec_max)
    ops._need_cuda(model._flat, "the model's parameters")
    if learn_priors and priors is None:
        priors = GroupPriors(model.F, model.d, model.device)          # (created at N(0, 1), returned under "priors")
    model._fresh_params()
    seen = torch.unique(x)
    plans = {f: SweepPlan(model, x, y, f, split_rows, chunk_rows, max_workspace_bytes, bound=True)
             for f in dict.fromkeys(fields)}
    seen_f = {f: plans[f].ents[plans[f].asc] for f in plans} if learn_priors else {}
    clamped = {f: torch.zeros((), dtype=torch.int64, device=x.device) for f in plans} if learn_priors else {}

    def learn_prior(f):
        n_clamped = update_prior(model, priors, f, seen_f[f], learn_mean, prec_min, prec_max)
        if n_clamped is not None:
            clamped[f] += n_clamped

    out = _sweeps(model, fields, n_sweeps, tol, on_step,
                  lambda: bound_objective_terms(model, x, y, seen, kl_weight, priors),
                  # (from the current rows: B = J at the start)
                  lambda f: plans[f].run_bound(model, kl_weight, n_iters, False, _prior_row(model, priors, f)),
                  learn_prior if learn_priors else None,
                  (lambda: update_bias_bound(model, x, y, kl_weight)) if update_bias else None, "bias")
    if priors is not None:
        out["priors"] = priors
    if learn_priors:
        out["clamped"] = {f: int(n) for f, n in clamped.items()}
    return out


# ---------------------------------------------------------------------------------------------------------------------
# implicit feedback: every (user, item) pair is a row ("Implicit sweeps"; include/vfm_implicit.h)
# ---------------------------------------------------------------------------------------------------------------------
def hkv_weights(counts, w0, alpha, log_eps=None):
    """The confidence of Hu, Koren & Volinsky as weights= of the implicit calls: w0 (1 + alpha counts), or with log_eps
    w0 (1 + alpha log1p(counts / log_eps)), in fp32 (w0 rounded to fp32 first, as the calls round it, so that a count of
    0 weighs exactly w0).  counts: non-negative play counts, dwell times, quantities, one per observed pair.  A
    (user, item) pair that occurs twice stays an error of the implicit calls: adding up the counts of repeated pairs
    is the caller's job.  ValueError for a negative or non-finite count, alpha < 0 and log_eps <= 0."""
    c = torch.as_tensor(counts).to(torch.float64)
    alpha = float(alpha)
    w0 = float(torch.tensor(float(w0), dtype=torch.float32))
    if not (math.isfinite(w0) and w0 > 0.0):
        raise ValueError("w0 must be > 0 and finite")
    if not (math.isfinite(alpha) and alpha >= 0.0):
        raise ValueError("alpha must be >= 0 and finite")
    if c.numel() and not (bool(torch.isfinite(c).all()) and float(c.min()) >= 0.0):
        raise ValueError("counts must be >= 0 and finite")
    if log_eps is not None:
        log_eps = float(log_eps)
        if not (math.isfinite(log_eps) and log_eps > 0.0):
            raise ValueError("log_eps must be > 0 and finite")
        c = torch.log1p(c / log_eps)
    return (w0 * (1.0 + alpha * c)).float()          # (>= w0: rounding to fp32 is monotone and w0 is an fp32 value)


def _check_weights(weights, n_rows, w0, w1):
    """weights= of an implicit call: a 1-D floating tensor of one weight per row of X, each finite and >= w0 once
    rounded to fp32, and no w1 beside it."""
    w = weights if isinstance(weights, torch.Tensor) else torch.as_tensor(weights)
    if w.dim() != 1 or not w.dtype.is_floating_point or w.shape[0] != n_rows:
        raise ValueError(f"weights must be a 1-D floating tensor with one weight per row of X ({n_rows})")
    if w1 != 1.0:
        raise ValueError("weights and w1 are two sources of an observed pair's weight: give one of them")
    w = w.detach().float()
    if w.numel() and not bool(torch.isfinite(w).all()):
        raise ValueError("weights must be finite (in fp32)")
    if w.numel() and float(w.min()) < w0:
        raise ValueError("weights must be >= w0 (in fp32): an observed pair weighs at least what an unobserved one does")


def _row_weights(model, weights):
    """Checked weights= as the kernels take them: [R] fp32 on the model's device, in the order of X's rows."""
    return None if weights is None else torch.as_tensor(weights).detach().to(model.device, torch.float32).contiguous()


def check_implicit_args(model, X, y, w0, w1, kl_weight, weights=None):
    """Validate the rows and weights of an implicit call (no GPU needed): a two-field 'reg' model, kl_weight > 0, finite
    weights with w1 >= w0 > 0, ids in their fields, distinct (user, item) pairs.  y None: all ones.  weights: None, or a
    1-D floating tensor with a weight per row of X, finite and >= w0 in fp32, given with w1 left at 1.0 (_check_weights;
    _row_weights moves it to the device).  Returns (x [R, 2] int64, y [R] fp32, w0, w1) on the model's device."""
    if model.output != "reg":
        raise ValueError("the implicit solves need a 'reg' model (Gaussian likelihood): the closed form they solve has none "
                         "for 'class'")
    if model.F != 2:
        raise ValueError(f"the implicit solves need a two-field model (F = 2), not F = {model.F}")
    foldin._check_kl_positive(kl_weight)
    w0, w1 = (float(torch.tensor(float(w), dtype=torch.float32)) for w in (w0, w1))     # (the kernels take them in fp32)
    if not (math.isfinite(w0) and math.isfinite(w1)):
        raise ValueError("w0 and w1 must be finite")
    if not w0 > 0.0:
        raise ValueError("w0 must be > 0: it is the weight of every unobserved pair")
    if weights is None and w1 < w0:
        raise ValueError("w1 must be >= w0: an observed pair weighs at least what an unobserved one does")
    if y is None:
        n_rows = torch.as_tensor(X).shape[0] if torch.as_tensor(X).dim() else 0
        y = torch.ones(n_rows, dtype=torch.float32)
    x, y, _ = foldin.check_args(model, X, y, 0, "closed_form", 1, 0, 0.0, kl_weight)
    if weights is not None:
        _check_weights(weights, x.shape[0], w0, w1)
    if x.shape[0]:
        key = x[:, 0] * model.T + x[:, 1]
        if int(torch.unique(key).numel()) != x.shape[0]:
            raise ValueError("duplicate (user, item) pairs: every pair is one row of the implicit objective")
    return x, y, w0, w1


def _check_entities(model, entities, field):
    """entities= of fold_in_implicit: None, or distinct integer ids of the field's range.  Returns them sorted, on the
    model's device."""
    lo, hi = foldin.field_range(model, field)
    if entities is None:
        return None
    e = torch.as_tensor(entities)
    if e.numel() == 0:
        e = e.to(torch.int64).reshape(-1)
    if e.dtype.is_floating_point or e.dtype == torch.bool or e.dim() != 1:
        raise ValueError("entities must be a 1-D sequence of integer ids")
    e = e.to(model.device, torch.int64)
    if e.numel() and (int(e.min()) < lo or int(e.max()) >= hi):
        raise ValueError(f"entities must lie in the field's range [{lo}, {hi})")
    e = torch.sort(e).values
    if e.numel() > 1 and bool((e[1:] == e[:-1]).any()):
        raise ValueError("entities must be distinct")
    return e.contiguous()


def implicit_base(model, lo, hi, chunk_rows):
    """The base block [vfm_implicit_base_doubles(d)] fp64 of the id range [lo, hi) at the current tables
    (vfm_implicit_base_f32): its bits depend on the range, chunk_rows and d alone."""
    o = _lib.ops()
    out = torch.empty(o.implicit_base_doubles(model.d), dtype=torch.float64, device=model.device)
    ws = torch.empty(o.implicit_base_workspace_bytes(hi - lo, int(chunk_rows), model.d), dtype=torch.uint8,
                     device=model.device)
    o.implicit_base(*model._views(model._flat), ws, out, lo, hi - lo, int(chunk_rows), foldin._link_flags(model))
    return out


class ImplicitPlan:
    """What one (X, y, field) of an implicit solve needs and that does not depend on the parameters: a SweepPlan of the
    observed rows (its sort, its chunk table and its max_workspace_bytes grouping, the groups sized by
    vfm_implicit_solve_workspace_bytes), each row's partner id, and the entities without observed rows.  entities: None
    (the field's whole id range) or sorted distinct ids; rows of other entities are left out.  weights: None, or [R]
    fp32 beside y; it goes through the entities= filter and into the plan's row order as y does (self.ws)."""

    def __init__(self, model, x, y, field, entities=None, split_rows="auto", chunk_rows=2048,
                 max_workspace_bytes=MAX_WORKSPACE_BYTES, lds_dim=-1, weights=None):
        dev = x.device
        self.field, self.d, self.lds_dim = int(field), model.d, int(lds_dim)
        self.chunk_rows = check_chunk_rows(chunk_rows)
        lo, hi = foldin.field_range(model, field)
        self.partner_range = foldin.field_range(model, 1 - field)
        if entities is None:
            entities = torch.arange(lo, hi, dtype=torch.int64, device=dev)
        else:
            keep = torch.isin(x[:, field], entities)
            x, y = x[keep].contiguous(), y[keep].contiguous()
            weights = None if weights is None else weights[keep]
        size = _lib.load().vfm_implicit_solve_workspace_bytes
        self.obs = SweepPlan(model, x, y, field, split_rows, chunk_rows, max_workspace_bytes, lds_dim,
                             split_bytes=lambda n_chunks, n_heavy, n_ops, d, lds: size(n_heavy, n_chunks, d, lds))
        p = self.obs
        self.partner = (p.op_x[:, 1 - field][p.row_op].contiguous() if p.E else
                        torch.zeros(0, dtype=torch.int64, device=dev))
        self.ys = p.ys if p.E else torch.zeros(0, dtype=torch.float32, device=dev)
        self.ws = None if weights is None else weights[p.order].contiguous()
        self.empty = entities[~torch.isin(entities, p.ents)].contiguous()
        self.ents = torch.cat([p.ents, self.empty])
        self.counts = torch.cat([p.counts, torch.zeros_like(self.empty)])
        self.asc = torch.sort(self.ents).indices
        self.E = self.ents.numel()

    def base(self, model):
        """The partner field's base block [vfm_implicit_base_doubles(d)] fp64 at the current tables."""
        return implicit_base(model, *self.partner_range, self.chunk_rows)

    def run(self, model, kl_weight, w0, w1, prior=None, weights=None):
        """Write the optimum of every entity of the plan into the model's tables: the base of the partner field, then
        the entities with few observed rows in one call, a call per group of heavy ones, and the entities without
        rows.  prior: the folded field's [2, d + 1] mean | precision on the device (GroupPriors.row); every one of the
        calls then solves under it (vfm_foldin_solve_implicit_prior_f32, include/vfm_implicit_prior.h); None: the
        parent call itself.  weights: what the plan was built with, None or the rows' weights; the plan holds them in
        its own row order (self.ws) and every one of the calls is then vfm_foldin_solve_implicit_weights_f32
        (include/vfm_implicit_weights.h), which has no w1.  Returns (entities [E] ascending, loss [E], rows [E])."""
        if (weights is None) != (self.ws is None):
            raise ValueError("weights belong to the plan: build the ImplicitPlan with the weights= that run() is given")
        dev, p = model.device, self.obs
        loss = torch.empty(self.E, dtype=torch.float32, device=dev)
        if self.E == 0:
            return self.ents, loss, self.counts
        model._fresh_params()
        o = _lib.ops()
        base = self.base(model)
        lo, hi = self.partner_range
        tables = model._views(model._flat)
        opts = (lo, hi - lo, foldin._link_flags(model), self.lds_dim, float(kl_weight), float(w0), float(w1))

        def solve(ents, row_ptr, cptr, tab, out):
            n = o.implicit_solve_workspace_bytes(ents.numel(), 0 if tab is None else tab.shape[0], self.d, self.lds_dim)
            ws = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
            a = (ents, row_ptr, cptr, tab, self.ys, self.partner, base, *tables, ws, out)
            if self.ws is not None:
                o.foldin_solve_implicit_weights(*a, prior, self.ws, *opts[:-1])
            elif prior is None:
                o.foldin_solve_implicit(*a, *opts)
            else:
                o.foldin_solve_implicit_prior(*a, prior, *opts)

        if p.n_light:
            nl = p.n_light
            solve(p.ents[:nl], p.ptr[:nl + 1], None, None, loss[:nl])
        for a, b, cptr, tab in p.groups:
            solve(p.ents[a:b], None, cptr, tab, loss[a:b])
        if self.empty.numel():
            n0 = self.empty.numel()
            solve(self.empty, torch.zeros(n0 + 1, dtype=torch.int64, device=dev), None, None, loss[p.E:])
        model.params_changed()
        return self.ents[self.asc], loss[self.asc], self.counts[self.asc]


def run_implicit(model, X, y, field, w0, w1=1.0, kl_weight=1.0, entities=None, split_rows="auto", chunk_rows=2048,
                 max_workspace_bytes=MAX_WORKSPACE_BYTES, lds_dim=-1, priors=None, weights=None):
    """VFM.fold_in_implicit: (entities [E] ascending, loss [E], rows [E]).  priors: under the folded field's prior.
    weights: a weight per row of X in place of w1."""
    x, y, w0, w1 = check_implicit_args(model, X, y, w0, w1, kl_weight, weights)
    check_priors(model, priors)
    if isinstance(field, bool) or not isinstance(field, int) or not 0 <= field < 2:
        raise ValueError("field must be 0 or 1")
    entities = _check_entities(model, entities, field)
    resolve_split_rows(split_rows, model.d)
    check_chunk_rows(chunk_rows)
    foldin._check_lds_dim(lds_dim)
    if int(max_workspace_bytes) < 0:
        raise ValueError("max_workspace_bytes must be >= 0")
    ops._need_cuda(model._flat, "the model's parameters")
    weights = _row_weights(model, weights)
    plan = ImplicitPlan(model, x, y, field, entities, split_rows, chunk_rows, int(max_workspace_bytes), lds_dim, weights)
    return plan.run(model, kl_weight, w0, w1, _prior_row(model, priors, field), weights)


def implicit_sums(model, x, y, w0, w1, weights=None):
    """The three weighted sums over ALL (user, item) pairs that J_imp and its scalar blocks need, as 0-dim fp64 tensors on
    the device: W = sum w, S1 = sum w (y - (E pred - m0)), S2 = sum w ((y - E pred)^2 + Var pred).  The all-pairs parts
    are closed forms of the two fields' Grams and first moments (E pred_ui = p_u . q_i with p_u = (1, mu_w,u, mu_u) and
    q_i = (m0 + mu_w,i, 1, mu_i), so sum_ui (E pred)^2 = <sum_u p p^T, sum_i q q^T>), O((N + M) d^2) in torch fp64 from
    the tables; the observed rows correct them with the predictive_moments kernel's per-row moments.  weights ([R] on
    the device, in x's row order): row r weighs weights[r] in place of w1, so W = w0 N M + sum_r (w_r - w0)."""
    ent, bia, scal = model._views(model._flat)
    d, link = model.d, model.link
    N, M = model.field_sizes
    m0, s0 = scal[1].double(), _link64(scal[2], link)
    one = lambda n: torch.ones(n, 1, dtype=torch.float64, device=ent.device)
    mu_u, mu_i = ent[:N, :d].double(), ent[N:N + M, :d].double()
    su2, si2 = _link64(ent[:N, d:], link) ** 2, _link64(ent[N:N + M, d:], link) ** 2
    P = torch.cat([one(N), bia[:N, :1].double(), mu_u], 1)
    Q = torch.cat([m0 + bia[N:N + M, :1].double(), one(M), mu_i], 1)
    sum_m2 = ((P.T @ P) * (Q.T @ Q)).sum()
    sum_m = P.sum(0) @ Q.sum(0)
    sum_v = (N * M * s0 * s0 + M * (_link64(bia[:N, 1], link) ** 2).sum() + N * (_link64(bia[N:N + M, 1], link) ** 2).sum()
             + (mu_u * mu_u).sum(0) @ si2.sum(0) + su2.sum(0) @ (si2 + mu_i * mu_i).sum(0))
    n = x.shape[0]
    if weights is None:
        W = torch.tensor(w0 * N * M + (w1 - w0) * n, dtype=torch.float64, device=ent.device)
    else:
        w1 = weights.double()
        W = w0 * N * M + (w1 - w0).sum()
    S1 = -w0 * (sum_m - N * M * m0)
    S2 = w0 * (sum_m2 + sum_v)
    if n:
        m, v = _moments64(model, x)
        yd = y.double()
        S1 = S1 + (w1 * (yd - (m - m0)) + w0 * (m - m0)).sum()
        S2 = S2 + (w1 * ((yd - m) ** 2 + v) - w0 * (m * m + v)).sum()
    return W, S1, S2


def _field_ids(model, field):
    """Every id of `field`, seen in X or not, on the model's device."""
    lo, hi = foldin.field_range(model, field)
    return torch.arange(lo, hi, dtype=torch.int64, device=model.device)


def implicit_objective_terms(model, x, y, w0, w1, kl_weight, priors=None, weights=None):
    """J_imp as a 0-dim fp64 tensor on the device: the weighted expected negative log likelihood of every pair
    (implicit_sums) plus kl_weight times the KL to N(0, 1) of every entity of both fields and of the global bias.
    priors: every entity's KL -- observed or not: its w0 rows are in the likelihood -- is to its field's
    N(mean, 1 / prec); the global bias keeps N(0, 1).  weights: a weight per observed row in place of w1."""
    ent, bia, scal = model._views(model._flat)
    prec = _link64(scal[0], model.link)
    W, _, S2 = implicit_sums(model, x, y, w0, w1, weights)
    kl = _kl64(scal[1].double(), _link64(scal[2], model.link))
    if priors is None:
        kl = _add_kl64_rows(kl, ent, bia, model.d, model.link)
    else:
        for f in (0, 1):
            mu, sg = _theta64(model, _field_ids(model, f))
            kl = kl + _kl64_prior(mu, sg, priors.mean[f].to(mu.device).double(), priors.prec[f].to(mu.device).double()).sum()
    return 0.5 * prec * S2 + W * (LOG_2PI_HALF - 0.5 * torch.log(prec)) + float(kl_weight) * kl


def update_scalars_implicit(model, x, y, w0, w1, kl_weight, weights=None):
    """The exact block minimisers of J_imp over the scalars, written in place: the global bias (mean and scale jointly),
    then the precision from the sums recomputed after it.  No readback."""
    scal = model._views(model._flat)[2]
    kl = float(kl_weight)
    prec = _link64(scal[0], model.link)
    W, S1, _ = implicit_sums(model, x, y, w0, w1, weights)
    den = kl + prec * W
    scal[1:3] = torch.stack([prec * S1 / den, _inv_link64(torch.sqrt(kl / den), model.link)]).float()
    W, _, S2 = implicit_sums(model, x, y, w0, w1, weights)
    scal[0:1] = _inv_link64(W / S2, model.link).float().reshape(1)


def implicit_objective(model, X, y, w0, w1=1.0, kl_weight=1.0, priors=None, weights=None):
    x, y, w0, w1 = check_implicit_args(model, X, y, w0, w1, kl_weight, weights)
    check_priors(model, priors)
    ops._need_cuda(model._flat, "the model's parameters")
    model._fresh_params()
    return float(implicit_objective_terms(model, x, y, w0, w1, kl_weight, priors, _row_weights(model, weights)))


def fit_implicit(model, X, y=None, n_sweeps=10, w0=None, w1=1.0, kl_weight=1.0, update_scalars_=True, split_rows="auto",
                 chunk_rows=2048, on_step=None, tol=None, max_workspace_bytes=MAX_WORKSPACE_BYTES, priors=None,
                 learn_priors=False, learn_mean=True, prec_min=1e-4, prec_max=1e4, weights=None):
    x, y, w0, w1 = check_implicit_args(model, X, y, w0, w1, kl_weight, weights)
    check_fit_args(model, x, y, "reg", lambda f: (x, y), n_sweeps, None, split_rows, chunk_rows, tol)
    check_priors(model, priors)
    prec_min, prec_max = check_prec_bounds(prec_min, prec_max)
    ops._need_cuda(model._flat, "the model's parameters")
    if learn_priors and priors is None:
        priors = GroupPriors(model.F, model.d, model.device)          # (created at N(0, 1), returned under "priors")
    model._fresh_params()
    weights = _row_weights(model, weights)
    plans = {f: ImplicitPlan(model, x, y, f, None, split_rows, chunk_rows, max_workspace_bytes, weights=weights)
             for f in (0, 1)}
    # the prior block is over the field's WHOLE id range: in J_imp every entity is in the KL, observed or not
    all_f = {f: _field_ids(model, f) for f in (0, 1)} if learn_priors else {}
    clamped = {f: torch.zeros((), dtype=torch.int64, device=x.device) for f in all_f}

    def learn_prior(f):
        clamped[f] += update_prior(model, priors, f, all_f[f], learn_mean, prec_min, prec_max)

    out = _sweeps(model, (0, 1), n_sweeps, tol, on_step,
                  lambda: implicit_objective_terms(model, x, y, w0, w1, kl_weight, priors, weights),
                  lambda f: plans[f].run(model, kl_weight, w0, w1, _prior_row(model, priors, f), weights),
                  learn_prior if learn_priors else None,
                  (lambda: update_scalars_implicit(model, x, y, w0, w1, kl_weight, weights)) if update_scalars_ else None,
                  "scalars")
    if priors is not None:
        out["priors"] = priors
    if learn_priors:
        out["clamped"] = {f: int(n) for f, n in clamped.items()}
    return out

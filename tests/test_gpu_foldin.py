"""GPU: fold-in (include/vfm_foldin.h) -- the objective and its gradient against fp64 autograd of the restatement in
test_foldin_cpu.py (both objectives, both links, two and three fields, several d), the Adam trajectory against fp64
torch.optim.Adam, frozen means frozen (bitwise), determinism and independence of the other folded entities, the lazy /
look-ahead step forms, the ML-20M shape with a 5,000-row entity, and the cold-start use on a planted model."""

import numpy as np
import pytest
import torch

from golden_util import rel_err
from test_foldin_cpu import objective_fp64

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _model(field_sizes, d, output="reg", link="abs", seed=0, scale=0.5, rng_seed=0):
    from vae_amd.model import VFM
    torch.manual_seed(seed)
    m = VFM(field_sizes=list(field_sizes), embedding_size=d, output=output, link=link, device=DEV, rng_seed=rng_seed)
    g = torch.Generator().manual_seed(seed)
    m.entity_params.weight.data.copy_(torch.randn(m.T, 2 * d, generator=g) * scale)
    m.bias_params.weight.data.copy_(torch.randn(m.T, 2, generator=g) * scale)
    m._flat[m._off_scal: m._off_scal + 3] = torch.tensor([1.3, 0.2, 0.3], device=DEV)
    return m


def _rows(m, field, n_ent, R, seed, output="reg"):
    """R rows whose folded column holds n_ent distinct ids of field `field`, the partners uniform in their fields."""
    g = torch.Generator().manual_seed(seed)
    lo = sum(m.field_sizes[:field])
    ids = lo + torch.randperm(m.field_sizes[field], generator=g)[:n_ent]
    cols = []
    for f, n in enumerate(m.field_sizes):
        base = sum(m.field_sizes[:f])
        cols.append(ids[torch.randint(0, n_ent, (R,), generator=g)] if f == field
                    else base + torch.randint(0, n, (R,), generator=g))
    X = torch.stack(cols, 1)
    y = (torch.randn(R, generator=g) + 3.0) if output == "reg" else (torch.rand(R, generator=g) < 0.4).float()
    return X.to(DEV), y.to(DEV)


def _eps(m, seed, t, S):
    from vae_amd import ops
    spec = ops.Spec(T=m.T, F=m.F, d=m.d, group_hi=m.group_hi, group_n=m.group_n, likelihood=0, n_samples=1,
                    link=m.link)
    return [tuple(a.cpu() for a in ops.philox_eps(spec, seed, t * S + s, DEV)) for s in range(S)]


def _theta(m, ents, grad=True):
    d = m.d
    ent = m.entity_params.weight.detach().double().cpu()
    bia = m.bias_params.weight.detach().double().cpu()
    e = ents.cpu()
    th = [ent[e, :d].clone(), ent[e, d:].clone(), bia[e, 0].clone(), bia[e, 1].clone()]
    for t in th:
        t.requires_grad_(grad)
    return th


def _oracle(m, X, y, field, objective, theta, ents, eps=None, kl_weight=1.0):
    return objective_fp64(m.entity_params.weight.detach().cpu(), m.bias_params.weight.detach().cpu(), m._scalars().cpu(),
                          X.cpu(), y.cpu(), field, (ents.cpu(), *theta), m.link, m.output, objective, eps, kl_weight)


CASES = [  # objective, output, link, field sizes, folded field, d, n_samples
    ("closed_form", "reg", "abs", (40, 30), 0, 5, 1),
    ("closed_form", "reg", "softplus", (20, 30, 25), 1, 8, 1),
    ("closed_form", "reg", "abs", (20, 30, 25), 2, 128, 1),
    ("closed_form", "reg", "softplus", (40, 30), 1, 20, 1),
    ("sampled", "reg", "abs", (40, 30), 0, 20, 1),
    ("sampled", "reg", "softplus", (20, 30, 25), 0, 8, 2),
    ("sampled", "class", "softplus", (40, 30), 1, 5, 3),
    ("sampled", "class", "abs", (20, 30, 25), 1, 128, 1),
]


@pytest.mark.parametrize("objective,output,link,sizes,field,d,S", CASES)
def test_objective_and_gradient_match_fp64_autograd(objective, output, link, sizes, field, d, S):
    m = _model(sizes, d, output, link, seed=d + field)
    X, y = _rows(m, field, 7, 60, seed=d, output=output)
    loss, grads = m.fold_in_objective(X, y, field=field, objective=objective, n_samples=S, seed=5, step=2,
                                      kl_weight=0.7)
    ents = grads["entities"]
    assert torch.equal(ents, torch.unique(X[:, field]))
    th = _theta(m, ents)
    eps = _eps(m, 5, 2, S) if objective == "sampled" else None
    L = _oracle(m, X, y, field, objective, th, ents, eps, kl_weight=0.7)
    L.sum().backward()
    assert rel_err(loss.cpu().numpy(), L.detach().numpy()) <= 1e-5
    ge = torch.cat([th[0].grad, th[1].grad], 1).numpy()
    gb = torch.stack([th[2].grad, th[3].grad], 1).numpy()
    assert rel_err(grads["entity"].cpu().numpy(), ge) <= 1e-5
    assert rel_err(grads["bias"].cpu().numpy(), gb) <= 1e-5


# d = 512: k_foldin <64, 8> (vfm_foldin.hip shape_of), LDS cap 5 rows per entity
@pytest.mark.parametrize("objective,output,link,sizes,field,d,S", [CASES[1], CASES[4], CASES[6],
                                                                   ("closed_form", "reg", "abs", (20, 30, 25), 2, 512, 1)])
def test_trajectory_matches_fp64_adam(objective, output, link, sizes, field, d, S):
    m = _model(sizes, d, output, link, seed=3)
    X, y = _rows(m, field, 5, 40, seed=9, output=output)
    ents = torch.unique(X[:, field])
    th = _theta(m, ents)
    opt = torch.optim.Adam(th, lr=0.01)
    for t in range(50):
        opt.zero_grad()
        eps = _eps(m, 4, t, S) if objective == "sampled" else None
        _oracle(m, X, y, field, objective, th, ents, eps).sum().backward()
        opt.step()
    out = m.fold_in(X, y, field=field, n_steps=50, lr=0.01, objective=objective, n_samples=S, seed=4)
    with torch.no_grad():
        L = _oracle(m, X, y, field, objective, th, ents, _eps(m, 4, 50, S) if objective == "sampled" else None)
    e = ents.cpu()
    ent, bia = m.entity_params.weight.detach().cpu(), m.bias_params.weight.detach().cpu()
    d_ = m.d
    assert rel_err(ent[e, :d_].numpy(), th[0].detach().numpy()) <= 1e-4
    assert rel_err(ent[e, d_:].numpy(), th[1].detach().numpy()) <= 1e-4
    assert rel_err(bia[e].numpy(), torch.stack([th[2], th[3]], 1).detach().numpy()) <= 1e-4
    assert rel_err(out["loss"].cpu().numpy(), L.numpy()) <= 1e-4
    assert out["rows"].tolist() == [int((X[:, field] == int(v)).sum()) for v in e]


def _trained(lazy=None, lookahead=False, seed=1):
    """A small 'reg' model after a few training steps (Adam state; rows may lag in the lazy / look-ahead forms)."""
    from vae_amd.model import VFM
    torch.manual_seed(seed)
    m = VFM(300, 200, embedding_size=16, output="reg", device=DEV, rng_seed=2)
    m.pipeline = False
    g = torch.Generator().manual_seed(seed)
    X = torch.stack([torch.randint(0, 300, (1200,), generator=g), 300 + torch.randint(0, 200, (1200,), generator=g)], 1)
    y = torch.randint(1, 6, (1200,), generator=g).float()
    X, y = X.to(DEV), y.to(DEV)
    m.set_training_data(X)
    m.lr = 0.05
    if lazy is not None:
        m.lazy_adam = lazy
        m.lazy_min_params = 0
    m.lookahead = lookahead
    plans = [m.plan(X[i * 40:(i + 1) * 40], y[i * 40:(i + 1) * 40]) for i in range(30)]
    for s in range(12):
        m.train_step(plans[s % 30], next_plan=plans[(s + 1) % 30] if lookahead else None)
    return m, plans


def _fold_rows(m, seed=4, n_ent=6):
    g = torch.Generator().manual_seed(seed)
    users = torch.randperm(300, generator=g)[:n_ent]
    X = torch.stack([users[torch.randint(0, n_ent, (50,), generator=g)], 300 + torch.randint(0, 200, (50,), generator=g)], 1)
    return X.to(DEV), (torch.randint(1, 6, (50,), generator=g).float()).to(DEV)


def test_frozen_means_frozen():
    m, _ = _trained()
    m.save_weights()
    before = {k: getattr(m, k).clone() for k in ("_flat", "_adam_m", "_adam_v", "_last_flat", "_mean_flat")}
    t_before = m._adam_t
    X, y = _fold_rows(m)
    out = m.fold_in(X, y, n_steps=30, lr=0.05)
    ents = out["entities"]
    changed = torch.zeros(m._n_flat, dtype=torch.bool, device=DEV)
    for e in ents.tolist():
        changed[e * 2 * m.d:(e + 1) * 2 * m.d] = True
        changed[m._off_bias + 2 * e: m._off_bias + 2 * e + 2] = True
    assert torch.equal(m._flat[~changed], before["_flat"][~changed])
    assert not torch.equal(m._flat[changed], before["_flat"][changed])
    for k in ("_adam_m", "_adam_v", "_last_flat", "_mean_flat"):
        assert torch.equal(getattr(m, k), before[k]), k
    assert m._adam_t == t_before
    assert torch.isfinite(out["loss"]).all()


@pytest.mark.parametrize("objective", ["closed_form", "sampled"])
def test_deterministic_and_independent_of_the_other_entities(objective):
    from vae_amd import foldin
    m, _ = _trained()
    X, y = _fold_rows(m, n_ent=3)
    start = m._flat.clone()
    outs = []
    for _ in range(2):
        m._flat.copy_(start)
        outs.append((m.fold_in(X, y, n_steps=25, objective=objective, n_samples=2), m._flat.clone()))
    assert torch.equal(outs[0][0]["loss"], outs[1][0]["loss"]) and torch.equal(outs[0][1], outs[1][1])
    together = outs[0][1]
    alone = start.clone()
    for i, e in enumerate(outs[0][0]["entities"].tolist()):
        m._flat.copy_(start)
        sel = X[:, 0] == e
        o = m.fold_in(X[sel], y[sel], n_steps=25, objective=objective, n_samples=2)
        assert torch.equal(o["loss"], outs[0][0]["loss"][i:i + 1])
        rows = slice(e * 2 * m.d, (e + 1) * 2 * m.d)
        alone[rows] = m._flat[rows]
        alone[m._off_bias + 2 * e: m._off_bias + 2 * e + 2] = m._flat[m._off_bias + 2 * e: m._off_bias + 2 * e + 2]
    assert torch.equal(alone, together)
    if objective == "closed_form":                    # rows streamed from the operand table = rows staged in LDS
        m._flat.copy_(start)
        _, loss, _, _ = foldin.run(m, X, y, n_steps=25, lr=0.05, lds_rows=0)
        assert torch.equal(loss, outs[0][0]["loss"]) and torch.equal(m._flat, together)


@pytest.mark.parametrize("form", ["lazy", "lookahead"])
def test_step_forms(form):
    kw = dict(lazy=True) if form == "lazy" else dict(lookahead=True)
    a, pa = _trained(**kw)
    b, _ = _trained(**kw)
    c, pc = _trained(**kw)
    assert a._lazy_dirty and b._lazy_dirty                 # rows lag behind the last step
    X, y = _fold_rows(a)
    oa = a.fold_in(X, y, n_steps=20)
    b.sync_lazy()
    ob = b.fold_in(X, y, n_steps=20)
    assert torch.equal(a._flat, b._flat) and torch.equal(oa["loss"], ob["loss"])
    # the next train_step equals the one after a direct write of those rows + params_changed()
    c.sync_lazy()
    ents = oa["entities"]
    c.entity_params.weight.data[ents] = a.entity_params.weight.data[ents]
    c.bias_params.weight.data[ents] = a.bias_params.weight.data[ents]
    c.params_changed()
    assert torch.equal(a._flat, c._flat)
    for s in range(3):
        la, _ = a.train_step(pa[(12 + s) % 30], next_plan=pa[(13 + s) % 30] if form == "lookahead" else None)
        lc, _ = c.train_step(pc[(12 + s) % 30], next_plan=pc[(13 + s) % 30] if form == "lookahead" else None)
        assert torch.equal(la, lc)
    a.sync_lazy()
    c.sync_lazy()
    assert torch.equal(a._flat, c._flat) and torch.equal(a._adam_m, c._adam_m) and torch.equal(a._adam_v, c._adam_v)


def test_ml20m_shape_20k_entities_with_a_heavy_one():
    from vae_amd.model import VFM
    N, M, d = 138_493, 26_744, 128
    torch.manual_seed(0)
    m = VFM(N, M, d, output="reg", device=DEV)
    with torch.no_grad():
        m._flat.mul_(0.3)
        m._flat[m._off_scal: m._off_scal + 3] = torch.tensor([1.5, 3.5, 0.2], device=DEV)
    g = torch.Generator(device=DEV).manual_seed(1)
    users = torch.randperm(N, device=DEV, generator=g)[:20_000]
    n = torch.full((20_000,), 20, device=DEV, dtype=torch.int64)
    n[7] = 5000
    u = torch.repeat_interleave(users, n)
    X = torch.stack([u, N + torch.randint(0, M, (u.numel(),), device=DEV, generator=g)], 1)
    y = torch.randint(1, 6, (u.numel(),), device=DEV, generator=g).float()
    loss, grads = m.fold_in_objective(X, y)
    ents = grads["entities"]
    assert ents.numel() == 20_000
    heavy = int(users[7])
    pick = torch.cat([torch.tensor([heavy], device=DEV), ents[torch.randperm(20_000, device=DEV, generator=g)[:15]]])
    pick = torch.unique(pick)
    pos = torch.searchsorted(ents, pick)
    sel = torch.isin(X[:, 0], pick)
    th = _theta(m, pick)
    L = _oracle(m, X[sel], y[sel], 0, "closed_form", th, pick)
    L.sum().backward()
    assert rel_err(loss[pos].cpu().numpy(), L.detach().numpy()) <= 1e-5
    assert rel_err(grads["entity"][pos].cpu().numpy(), torch.cat([th[0].grad, th[1].grad], 1).numpy()) <= 1e-4
    assert rel_err(grads["bias"][pos].cpu().numpy(), torch.stack([th[2].grad, th[3].grad], 1).numpy()) <= 1e-4
    # the sub-problem alone gives the same bits as inside the 20,000-entity call
    l2, g2 = m.fold_in_objective(X[sel], y[sel])
    assert torch.equal(l2, loss[pos]) and torch.equal(g2["entity"], grads["entity"][pos])
    out = m.fold_in(X, y, n_steps=20, lr=0.01)
    assert torch.isfinite(out["loss"]).all() and float((out["loss"] < loss).float().mean()) > 0.99


def test_cold_start_user_on_a_planted_model():
    from vae_amd.model import VFM
    N, M, d = 50, 400, 8
    torch.manual_seed(0)
    m = VFM(N, M, d, output="reg", device=DEV)
    g = torch.Generator().manual_seed(2)
    mu = torch.randn(N + M, d, generator=g)
    ent = torch.cat([mu, torch.full((N + M, d), 0.05)], 1)
    bia = torch.stack([torch.randn(N + M, generator=g) * 0.1, torch.full((N + M,), 0.05)], 1)
    m.entity_params.weight.data.copy_(ent)
    m.bias_params.weight.data.copy_(bia)
    m._flat[m._off_scal: m._off_scal + 3] = torch.tensor([4.0, 0.0, 0.05], device=DEV)   # noise sd 0.5
    u = 17
    items = N + torch.randperm(M, generator=g)
    seen, held = items[:60], items[60:]
    truth = lambda it: (mu[u] * mu[it]).sum(1) + bia[u, 0] + bia[it, 0]
    X = torch.stack([torch.full_like(seen, u), seen], 1).to(DEV)
    y = (truth(seen) + 0.5 * torch.randn(60, generator=g)).to(DEV)
    l0 = m.fold_in(X, y, n_steps=0, reset=True)["loss"]            # the prior start
    prior_pred, _ = m.predictive_moments(torch.stack([torch.full_like(held, u), held], 1).to(DEV))
    l1 = m.fold_in(X, y, n_steps=300, lr=0.05, reset=True)["loss"]
    assert float(l1) < 0.5 * float(l0)
    pred, _ = m.predictive_moments(torch.stack([torch.full_like(held, u), held], 1).to(DEV))
    t = truth(held).numpy()
    c_fold = np.corrcoef(pred.cpu().numpy(), t)[0, 1]
    c_prior = np.corrcoef(prior_pred.cpu().numpy(), t)[0, 1]
    assert c_fold > 0.8 and c_fold > c_prior + 0.3, (c_fold, c_prior)
    # reset=True twice gives the same bits: the start does not depend on the row's current values
    l2 = m.fold_in(X, y, n_steps=300, lr=0.05, reset=True)["loss"]
    assert torch.equal(l1, l2)


def test_empty_fold_in_does_nothing():
    m = _model((10, 12), 8)
    before = m._flat.clone()
    out = m.fold_in(torch.zeros(0, 2, dtype=torch.int64), torch.zeros(0))
    assert out["entities"].numel() == 0 and out["loss"].numel() == 0
    assert torch.equal(m._flat, before)

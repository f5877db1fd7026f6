"""CPU: fold-in (include/vfm_foldin.h) -- an fp64 torch restatement of the per-entity objective L_e for both objectives
(the GPU tests differentiate it with autograd), its closed form against a large Monte Carlo of the sampled form, and
the argument checks of VFM.fold_in / fold_in_objective, which raise before anything needs a GPU."""
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LOG_2PI_HALF = 0.5 * math.log(2 * math.pi)


def link_t(s, link):
    return s.abs() if link == "abs" else torch.nn.functional.softplus(s)


def kl_t(mu, sg):
    return 0.5 * (sg * sg + mu * mu - 1.0) - torch.log(sg)


def objective_fp64(ent, bia, scal, x, y, field, theta, link="abs", output="reg", objective="closed_form", eps=None,
                   kl_weight=1.0):
    """fp64 L_e [E] of the folded entities.

    ent [T, 2d], bia [T, 2], scal [3]: the frozen tables (the folded entities' rows in them are not read).
    x [R, F] int64, y [R]; theta = (entities [E] ascending, mu [E, d], s [E, d], mu_w [E], s_w [E]) -- the factors being
    fitted (tensors that may require grad).  objective "closed_form": E[nll] in closed form ('reg');  "sampled": the mean
    over the draws in eps = [(eps_entity [T, d], eps_bias [T], eps_global [1]), ...] (one triple per draw).
    """
    ents, mu, s, mw, sw = theta
    ent, bia, scal = ent.double(), bia.double(), scal.double()
    y = y.double()
    d = ent.shape[1] // 2
    F = x.shape[1]
    idx = torch.searchsorted(ents, x[:, field].contiguous())             # entity index of each row
    sg, sgw = link_t(s, link), link_t(sw, link)
    prec = link_t(scal[0], link)
    m0, sg0 = scal[1], link_t(scal[2], link)
    Q = [f for f in range(F) if f != field]
    if objective == "closed_form":
        mq = torch.stack([ent[x[:, q], :d] for q in Q]) if Q else torch.zeros(1, x.shape[0], d, dtype=torch.float64)
        sq2 = (torch.stack([link_t(ent[x[:, q], d:], link) for q in Q]) ** 2 if Q
               else torch.zeros(1, x.shape[0], d, dtype=torch.float64))
        M, A = mq.sum(0), sq2.sum(0)
        C = 2.0 * (sq2 * (M[None] - mq)).sum(0)
        pm = 0.5 * (M ** 2 - (mq ** 2).sum(0)).sum(1)
        pv = (0.5 * (A ** 2 - (sq2 ** 2).sum(0)) + (sq2 * (M[None] - mq) ** 2).sum(0)).sum(1)
        cm = m0 + sum(bia[x[:, q], 0] for q in Q) + pm
        cv = sg0 ** 2 + sum(link_t(bia[x[:, q], 1], link) ** 2 for q in Q) + pv
        mu_r, sg_r = mu[idx], sg[idx]
        Ep = cm + mw[idx] + (mu_r * M).sum(1)
        Vp = cv + sgw[idx] ** 2 + (mu_r ** 2 * A + sg_r ** 2 * (A + M ** 2) + mu_r * C).sum(1)
        nll = 0.5 * prec * ((y - Ep) ** 2 + Vp) - 0.5 * torch.log(prec) + LOG_2PI_HALF
    else:
        ee = torch.stack([e[0] for e in eps]).double()                 # [S, T, d]
        eb = torch.stack([e[1] for e in eps]).double()                 # [S, T]
        eg = torch.stack([e[2].reshape(-1)[0] for e in eps]).double()  # [S]
        zsum = torch.zeros(len(eps), x.shape[0], d, dtype=torch.float64)
        zsq = torch.zeros_like(zsum)
        pred = (m0 + sg0 * eg)[:, None].expand(-1, x.shape[0])
        for f in range(F):
            e = x[:, f]
            if f == field:
                z = mu[idx] + sg[idx] * ee[:, e]
                w = mw[idx] + sgw[idx] * eb[:, e]
            else:
                z = ent[e, :d] + link_t(ent[e, d:], link) * ee[:, e]
                w = bia[e, 0] + link_t(bia[e, 1], link) * eb[:, e]
            zsum, zsq, pred = zsum + z, zsq + z * z, pred + w
        pred = pred + 0.5 * (zsum ** 2 - zsq).sum(2)
        if output == "reg":
            nll = 0.5 * prec * (y - pred) ** 2 - 0.5 * torch.log(prec) + LOG_2PI_HALF
        else:
            nll = torch.nn.functional.softplus(pred) - y * pred
        nll = nll.mean(0)
    L = torch.zeros(ents.numel(), dtype=torch.float64).index_add(0, idx, nll)
    kl = kl_t(mu, sg).sum(1) + kl_t(mw, sgw)
    return L + kl_weight * kl


def _tables(T, d, seed):
    g = torch.Generator().manual_seed(seed)
    ent = torch.randn(T, 2 * d, generator=g, dtype=torch.float64) * 0.6
    bia = torch.randn(T, 2, generator=g, dtype=torch.float64) * 0.5
    scal = torch.tensor([1.3, 0.2, 0.4], dtype=torch.float64)
    return ent, bia, scal


@pytest.mark.parametrize("F", [2, 3])
@pytest.mark.parametrize("link", ["abs", "softplus"])
def test_closed_form_matches_monte_carlo(F, link):
    d, n_per, n_mc = 4, 3, 40_000
    sizes = [5] * F
    T = sum(sizes)
    ent, bia, scal = _tables(T, d, 11 + F)
    g = torch.Generator().manual_seed(5)
    field = 1
    lo = 5 * field
    R = 12
    x = torch.stack([torch.randint(5 * f, 5 * f + 5, (R,), generator=g) for f in range(F)], 1)
    x[:, field] = lo + torch.arange(R) % n_per
    y = torch.randn(R, generator=g, dtype=torch.float64) + 1.0
    ents = torch.unique(x[:, field])
    theta = (ents, ent[ents, :d].clone(), ent[ents, d:].clone(), bia[ents, 0].clone(), bia[ents, 1].clone())
    cf = objective_fp64(ent, bia, scal, x, y, field, theta, link, "reg", "closed_form")
    # Monte Carlo: n_mc independent draws of every random variable through the sampled restatement, in 40 batches; the
    # spread of the batch means gives the standard error
    means = []
    for _ in range(40):
        n = n_mc // 40
        draws = [(torch.randn(T, d, generator=g, dtype=torch.float64), torch.randn(T, generator=g, dtype=torch.float64),
                  torch.randn(1, generator=g, dtype=torch.float64)) for _ in range(n)]
        means.append(objective_fp64(ent, bia, scal, x, y, field, theta, link, "reg", "sampled", draws))
    means = torch.stack(means)
    mc, sd = means.mean(0), means.std(0) / math.sqrt(means.shape[0])
    assert torch.all((mc - cf).abs() < 5 * sd), (mc, cf, sd)


def test_sampled_restatement_is_the_mean_over_draws():
    d, T = 3, 10
    ent, bia, scal = _tables(T, d, 3)
    x = torch.tensor([[0, 5], [1, 6], [0, 7]])
    y = torch.tensor([1.0, 0.0, 1.0], dtype=torch.float64)
    ents = torch.tensor([0, 1])
    theta = (ents, ent[ents, :d], ent[ents, d:], bia[ents, 0], bia[ents, 1])
    g = torch.Generator().manual_seed(1)
    eps = [(torch.randn(T, d, generator=g), torch.randn(T, generator=g), torch.randn(1, generator=g)) for _ in range(3)]
    both = objective_fp64(ent, bia, scal, x, y, 0, theta, "abs", "class", "sampled", eps)
    each = [objective_fp64(ent, bia, scal, x, y, 0, theta, "abs", "class", "sampled", [e]) for e in eps]
    assert torch.allclose(both, sum(each) / 3, rtol=1e-12, atol=1e-12)


# ---------------------------------------------------------------------------------------------------------------------
# argument checks: ValueError before anything runs on a GPU
# ---------------------------------------------------------------------------------------------------------------------
def _cpu_model(output="reg", **kw):
    from vae_amd.model import VFM
    return VFM(field_sizes=kw.pop("field_sizes", [6, 4]), embedding_size=kw.pop("d", 4), output=output, device="cpu",
               **kw)


@pytest.mark.parametrize("call", ["fold_in", "fold_in_objective"])
def test_argument_checks_raise_value_error(call):
    m = _cpu_model()
    fn = getattr(m, call)
    X = torch.tensor([[0, 6], [1, 7], [0, 9]])
    y = torch.tensor([1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="field"):
        fn(X, y, field=2)
    with pytest.raises(ValueError, match="field"):
        fn(X, y, field=-1)
    with pytest.raises(ValueError, match="range"):
        fn(torch.tensor([[6, 7]]), torch.tensor([1.0]), field=0)          # a field-1 id in the folded column
    with pytest.raises(ValueError, match="range"):
        fn(torch.tensor([[7, 1]]), torch.tensor([1.0]), field=1)          # a field-0 id folded as field 1
    with pytest.raises(ValueError, match="lie in"):
        fn(torch.tensor([[0, 10]]), torch.tensor([1.0]), field=0)         # partner id past T
    with pytest.raises(ValueError, match="length|one value"):
        fn(X, y[:2])
    with pytest.raises(ValueError, match="n_samples"):
        fn(X, y, objective="sampled", n_samples=0)
    with pytest.raises(ValueError, match="n_samples"):
        fn(X, y, objective="sampled", n_samples=5)
    with pytest.raises(ValueError, match="objective"):
        fn(X, y, objective="exact")
    with pytest.raises(ValueError, match=r"\[R, 2\]"):
        fn(torch.tensor([0, 1]), torch.tensor([1.0, 2.0]))
    mc = _cpu_model("class")
    with pytest.raises(ValueError, match="closed-form"):
        getattr(mc, call)(X, torch.tensor([1.0, 0.0, 1.0]), objective="closed_form")


def test_fold_in_step_checks():
    m = _cpu_model()
    X, y = torch.tensor([[0, 6]]), torch.tensor([1.0])
    with pytest.raises(ValueError, match="n_steps"):
        m.fold_in(X, y, n_steps=-1)
    with pytest.raises(ValueError, match="lr"):
        m.fold_in(X, y, lr=-0.1)
    with pytest.raises(ValueError, match="kl_weight"):
        m.fold_in(X, y, kl_weight=-1.0)


def test_three_fields_ranges():
    m = _cpu_model(field_sizes=[3, 4, 5])
    with pytest.raises(ValueError, match=r"\[3, 7\)"):
        m.fold_in(torch.tensor([[0, 2, 8]]), torch.tensor([1.0]), field=1)
    with pytest.raises(ValueError, match="frozen"):
        m.fold_in(torch.tensor([[0, 3, 4]]), torch.tensor([1.0]), field=1)    # partner column holds a field-1 id


def test_cpu_model_fails_loudly():
    from vae_amd._lib import VfmLibraryError
    m = _cpu_model()
    X, y = torch.tensor([[0, 6], [1, 7]]), torch.tensor([1.0, 2.0])
    with pytest.raises(VfmLibraryError, match="MI355X"):
        m.fold_in(X, y)
    with pytest.raises(VfmLibraryError, match="MI355X"):
        m.fold_in_objective(X, y)


def test_row_lists_and_partner_tuples():
    from vae_amd.foldin import partner_tuples, row_lists
    x = torch.tensor([[3, 10], [1, 11], [3, 12], [1, 10], [2, 11], [3, 10]])
    y = torch.arange(6, dtype=torch.float32)
    xs, ys, ents, ptr, rows = row_lists(x, y, 0)
    assert ents.tolist() == [1, 2, 3] and ptr.tolist() == [0, 2, 3, 6] and rows.tolist() == [2, 1, 3]
    assert ys.tolist() == [1.0, 3.0, 4.0, 0.0, 2.0, 5.0]                      # stable: the rows' order kept per entity
    op_x, row_op = partner_tuples(xs, 0)
    assert op_x[:, 1].tolist() == [10, 11, 12]
    assert op_x[row_op, 1].tolist() == xs[:, 1].tolist()
    x3 = torch.tensor([[0, 5, 9], [1, 5, 9], [0, 6, 9]])
    op3, ro3 = partner_tuples(x3, 0)
    assert op3.shape[0] == 2 and torch.equal(op3[ro3][:, 1:], x3[:, 1:])

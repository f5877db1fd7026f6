"""GPU: the fused variant step (include/vfm_variant_step.h, vae_amd/csrc_var/vfm_variant_step.hip) -- variant_forward +
variant_adam_step against fp64 (tests/variant_step_reference.py: oracle.variant_elbo's autograd gradients, then
adam_restatement.step_fp64 from a planted state, bounds derived from the tolerance test_variants_vs_oracle grants the
gradients; tests/test_variant_step_cpu.py shows that reference rejecting wrong steps).  The step kernels restate the
backward of csrc/vfm_variants.hip; the fp64 comparison is what ties the two copies together.

Every figure is printed as `VSTEP <case> <tensor> <quantity> error/bound <ratio>` before it is asserted.

Measured on an MI355X, worst error / bound over the 17 cases of test 1 (past the grid cap, test 3, in brackets):
  tensor    m'               v'               update           share left out
  entity    0.0009 (< 0.01)  0.117 (0.108)    0.332 (0.399)    0.0196 (four fresh rows of 204)
  bias      0.0009 (0.014)   0.116 (0.097)    0.351 (0.396)    0.0196
  scalars   0.0054 (0.001)   0.197 (0.199)    0.430 (0.332)    0
  priors    0.0005 (0.0003)  0.078 (0.064)    0.239 (0.201)    0
(the update's bound is dominated by one ulp of the stored parameter; the gradient term is far from filled).  All 24 tests
of the file run in 8 s."""
import os
import re

import numpy as np
import pytest
import torch

import adam_restatement as R
import variant_step_reference as V
from golden_util import ROOT

pytestmark = pytest.mark.gpu

SRC = os.path.join(ROOT, "vae_amd", "csrc_var", "vfm_variant_step.hip")
BLOCK = 256


# ------------------------------------------------------------------------------ launch arithmetic, read from the source
def read_launch_arithmetic():
    """(workgroup cap, {W: [(LPE, CPL), ...]}) from the text of the step's translation unit."""
    text = open(SRC).read()
    cap = [int(m) for m in re.findall(r"constexpr\s+int\s+VSTEP_BLOCKS\s*=\s*(\d+)\s*;", text)]
    assert len(cap) == 1
    shapes = {}
    for w in (8, 1):
        line = re.search(r"#define\s+VFM_FOR_VSTEP_SHAPES%d\(X\)(.*)" % w, text).group(1)
        shapes[w] = [(int(a), int(b)) for ww, a, b in re.findall(r"X\((\d+),\s*(\d+),\s*(\d+)\)", line) if int(ww) == w]
    assert "const int l = d <= 4 ? 4 : d <= 16 ? 16 : 64;" in text and "while (l < D8 && l < 64) l <<= 1;" in text
    return cap[0], shapes


def unit_of(d, shapes):
    """Lane groups (table rows in flight) per workgroup: vstep_shape, restated and checked against the instantiated list."""
    if d % 8 == 0:
        D8, l = d >> 3, 1
        while l < D8 and l < 64:
            l <<= 1
        shape, w = (l, (D8 + l - 1) // l), 8
    else:
        l = 4 if d <= 4 else 16 if d <= 16 else 64
        c = (d + l - 1) // l
        shape, w = (l, c if c <= 2 else 4 if c <= 4 else 16), 1
    assert shape in shapes[w], (d, shape)
    return BLOCK // shape[0]


# ------------------------------------------------------------------------------------------------------ running one step
def upload(pb, dev):
    from vae_amd import ops, _lib
    case = pb["case"]
    spec = ops.Spec(T=pb["T"], F=pb["F"], d=pb["d"], group_hi=tuple(int(v) for v in pb["hi"]), group_n=tuple(float(v) for v in pb["gn"]),
                    nb_train=pb["nb_train"], likelihood=_lib.LIK_NORMAL if case.output == "reg" else _lib.LIK_BERNOULLI)
    inv_occ = ops.inv_occ_from_counts(torch.tensor(pb["nb_occ"], device=dev))
    x_t = torch.tensor(pb["x"], device=dev).to(torch.int32 if case.id32 else torch.int64).contiguous()
    plan = ops.BatchPlan(spec, x_t, torch.tensor(pb["y"], device=dev), inv_occ)
    assert plan.id_bits == (32 if case.id32 else 64)
    v_t = torch.tensor(pb["vals"], device=dev) if case.values else None
    return spec, inv_occ, plan, v_t


def eps_of(pb, spec, dev):
    """(eps tables for the kernels or None, eps for the oracle or None): Philox eps of the case's (seed, step) either way."""
    from vae_amd import ops
    if pb["case"].objective != "sampled":
        return None, None
    ee, eb, eg = ops.philox_eps(spec, seed=pb["seed"], step=pb["step"], device=dev)
    host = (eg.cpu().numpy(), eb.cpu().numpy(), ee.cpu().numpy())
    return ((ee, eb, eg) if pb["case"].eps_table else None), host


def device_state(pb, planted, dev):
    """Fresh device copies of the four tensors and their planted moments."""
    from vae_amd.variants import VariantMoments
    P = V.params_of(pb)
    t = {n: (None if P[n] is None else torch.tensor(P[n], device=dev)) for n in V.TENSORS}
    mo = VariantMoments(t["entity"], t["bias"], t["scalars"], t["priors"])
    for n in V.TENSORS:
        if planted[n] is not None:
            getattr(mo, "m_" + n).copy_(torch.tensor(planted[n][0], device=dev))
            getattr(mo, "v_" + n).copy_(torch.tensor(planted[n][1], device=dev))
    return t, mo


def run_step(pb, plan, inv_occ, v_t, eps_dev, t, mo, lr=R.LR):
    from vae_amd.variants import variant_forward, variant_adam_step
    case = pb["case"]
    st = variant_forward(plan, case.objective, t["entity"], t["bias"], t["scalars"], inv_occ, priors=t["priors"], values=v_t,
                         eps=eps_dev, seed=pb["seed"], step=pb["step"])
    variant_adam_step(plan, st, t["entity"], t["bias"], t["scalars"], t["priors"], inv_occ, mo, lr, case.t,
                      betas=(R.B1, R.B2), eps=R.EPS)
    return st


def collect(t, mo):
    return {n: (None if t[n] is None else tuple(a.cpu().numpy() for a in (t[n], getattr(mo, "m_" + n), getattr(mo, "v_" + n))))
            for n in V.TENSORS}


def check(pb, ref, planted, got):
    want = V.reference_step(pb, ref, planted)
    rows, bad = V.compare(pb, ref, planted, want, got)
    for n, q, worst, left in rows:
        print("VSTEP %-44s %-8s %-7s error/bound %.4f  left out %.4f" % (pb["case"].id, n, q, worst, left))
    assert not bad, (pb["case"].id, bad)


# ------------------------------------------------------------------------- 1. one teacher-forced step from a live state
@pytest.mark.parametrize("case", V.CASES, ids=lambda c: c.id)
def test_one_step_from_a_live_state_against_fp64(case):
    dev = torch.device("cuda:0")
    pb = V.build_problem(case)
    spec, inv_occ, plan, v_t = upload(pb, dev)
    eps_dev, eps_host = eps_of(pb, spec, dev)
    ref = V.oracle_grads(pb, eps_host)
    planted = V.plant(pb, ref)
    t, mo = device_state(pb, planted, dev)
    st = run_step(pb, plan, inv_occ, v_t, eps_dev, t, mo)
    assert abs(st["loss3"][0].item() - ref["loss"]) / abs(ref["loss"]) < 1e-4        # (the forward the step was fed by)
    assert int(plan.status.item()) == 0
    check(pb, ref, planted, collect(t, mo))


# ------------------------------------------------------------------------------------------------------ 2. reproducible
@pytest.mark.parametrize("d", [8, 5])
def test_the_step_is_reproducible_bit_for_bit(d):
    """Priors on, T large enough that several workgroups share an id group: the partial rows of the prior gradients are
    summed in a fixed order, so the same step from the same buffers twice gives the same bits in every output."""
    from vae_amd import ops, _lib
    from vae_amd.variants import variant_forward, variant_adam_step, VariantMoments, priors_len
    dev = torch.device("cuda:0")
    cap, shapes = read_launch_arithmetic()
    unit = unit_of(d, shapes)
    sizes = [5 * unit + 3, 7 * unit + 1, 2 * unit + 5]                       # 15 workgroups, boundaries inside workgroups
    T, F, B = sum(sizes), 3, 6000
    g = np.random.default_rng(11)
    off = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    x = np.stack([off[f] + np.minimum(g.zipf(1.3, B) - 1, sizes[f] - 1) for f in range(F)], 1)
    spec = ops.Spec(T=T, F=F, d=d, group_hi=tuple(int(v) for v in np.cumsum(sizes)), group_n=tuple(float(s) for s in sizes),
                    nb_train=7 * B, likelihood=_lib.LIK_NORMAL)
    inv_occ = ops.inv_occ_from_counts(torch.tensor(np.bincount(x.reshape(-1), minlength=T) + 1, device=dev))
    plan = ops.BatchPlan(spec, torch.tensor(x, device=dev), torch.tensor(g.integers(1, 6, B).astype(np.float32), device=dev), inv_occ)
    tg = torch.Generator(device="cpu").manual_seed(3)
    rnd = lambda *s: torch.randn(*s, generator=tg)
    base = {"entity": 0.4 * rnd(T, 2 * d), "bias": 0.5 * rnd(T, 2), "scalars": torch.tensor([0.8, 0.3, -0.6]),
            "priors": torch.cat([torch.tensor([0.1, -1.1]), 0.3 * rnd(F), 1.0 + 0.2 * torch.rand(F, generator=tg), 0.2 * rnd(F * d),
                                 (1.0 + 0.2 * torch.rand(F * d, generator=tg)) * torch.sign(rnd(F * d))])}
    assert base["priors"].numel() == priors_len(F, d)
    mom = {n: (0.1 * rnd(*base[n].shape), 0.5 + torch.rand(*base[n].shape, generator=tg)) for n in base}
    vals = torch.tensor(g.uniform(0.3, 2.0, (B, F)).astype(np.float32), device=dev)

    def once():
        t = {n: base[n].clone().to(dev) for n in base}
        mo = VariantMoments(t["entity"], t["bias"], t["scalars"], t["priors"])
        for n in base:
            getattr(mo, "m_" + n).copy_(mom[n][0])
            getattr(mo, "v_" + n).copy_(mom[n][1])
        st = variant_forward(plan, "sampled", t["entity"], t["bias"], t["scalars"], inv_occ, priors=t["priors"], values=vals, seed=9, step=4)
        variant_adam_step(plan, st, t["entity"], t["bias"], t["scalars"], t["priors"], inv_occ, mo, 0.01, 7)
        return [t[n] for n in base] + [getattr(mo, k) for k in mo.NAMES]

    a, b = once(), once()
    assert all(torch.isfinite(u).all() for u in a)
    for i, (u, w) in enumerate(zip(a, b)):
        assert torch.equal(u, w), i
    assert not torch.equal(a[3], base["priors"].to(dev)) and not torch.equal(a[0], base["entity"].to(dev))


# ---------------------------------------------------------------------------------------------- 3. past the grid cap
@pytest.mark.parametrize("d,objective,values,id32", [(8, "sampled", True, True), (5, "closed_form", False, False)])
def test_past_the_grid_cap_against_fp64(d, objective, values, id32):
    """B = T = 2 cap unit + unit + 3 (cap and unit read from the source): every workgroup's entity range holds two or three
    rows per lane group, the last workgroup a ragged one; Zipf-tailed lists; priors on; the oracle in row chunks."""
    import test_gpu_variant_scale as S
    dev = torch.device("cuda:0")
    cap, shapes = read_launch_arithmetic()
    unit = unit_of(d, shapes)
    n = 2 * cap * unit + unit + 3
    B = T = n
    F = 2 if d == 8 else 3
    epb = -(-(-(-T // cap)) // unit) * unit
    assert epb == 3 * unit and -(-T // unit) > cap
    s0 = (T // epb // 3) * epb + unit // 2 + 1                                # a group boundary inside a workgroup's range
    sizes = (s0, T - s0) if F == 2 else (s0, 3, T - s0 - 3)
    case = V.StepCase(d, F, B, 57, objective, True, values, "reg", id32, False)
    scase = S.ScaleCase(d, objective, True, values, id32)
    g = np.random.default_rng(600 + d)
    x, _ = S.make_batch(g, sizes, B)
    cnt = np.bincount(x.reshape(-1), minlength=T)
    assert (cnt == 0).sum() > 1000 and cnt.max() >= 200
    se = 0.5
    P = {"alpha": np.array([0.9], np.float32), "global_bias_mean": np.array([0.4], np.float32),
         "global_bias_scale": np.array([-0.7], np.float32), "bias_params": (0.6 * g.standard_normal((T, 2))).astype(np.float32),
         "entity_params": (se * g.standard_normal((T, 2 * d))).astype(np.float32)}
    G = F
    pri = np.concatenate([[0.1, -1.2], 0.3 * g.standard_normal(G), g.uniform(0.6, 1.5, G) * g.choice([-1, 1], G),
                          se * 0.6 * g.standard_normal(G * d), g.uniform(0.6, 1.5, G * d) * g.choice([-1, 1], G * d)]).astype(np.float32)
    pb = dict(case=case, B=B, T=T, F=F, d=d, sizes=sizes, hi=np.cumsum(sizes), gn=np.array(sizes, np.float64), x=x,
              y=g.integers(1, 6, B).astype(np.float32), nb_occ=cnt + g.integers(1, 4, T), P=P, pri=pri,
              vals=g.uniform(0.3, 2.0, (B, F)).astype(np.float32) if values else None, nb_train=7 * B, seed=12345, step=678,
              rng=np.random.default_rng(5))
    spec, inv_occ, plan, v_t = upload(pb, dev)
    eps_dev, eps_host = eps_of(pb, spec, dev)
    o = S.oracle_eval(dict(pb, case=scase), eps_host)
    ref = {"entity": o["g_entity"], "bias": o["g_bias"], "scalars": o["g_scalars"], "priors": o["g_priors"], "pred": o["pred"],
           "loss": o["loss"]}
    planted = V.plant(pb, ref)
    t, mo = device_state(pb, planted, dev)
    st = run_step(pb, plan, inv_occ, v_t, eps_dev, t, mo)
    assert abs(st["loss3"][0].item() - ref["loss"]) / abs(ref["loss"]) < 1e-4
    assert int(plan.status.item()) == 0
    check(pb, ref, planted, collect(t, mo))


# ---------------------------------------------------------------------------------------------- 4. corrupted index
@pytest.mark.parametrize("d", [16, 5])
def test_a_corrupted_index_is_clamped_and_counted(d):
    """One out-of-range row number and one bad span: the entries are clamped (row 0 / an empty list), never followed, and
    counted in vfm_index_t.status; every output stays finite."""
    from vae_amd.variants import variant_forward, variant_adam_step
    dev = torch.device("cuda:0")
    case = V.StepCase(d, 2, 500, 2, "closed_form", True, True)
    pb = V.build_problem(case, seed=1)
    spec, inv_occ, plan, v_t = upload(pb, dev)
    P = V.params_of(pb)
    t = {n: torch.tensor(P[n], device=dev) for n in V.TENSORS}
    from vae_amd.variants import VariantMoments
    mo = VariantMoments(t["entity"], t["bias"], t["scalars"], t["priors"])
    st = variant_forward(plan, "closed_form", t["entity"], t["bias"], t["scalars"], inv_occ, priors=t["priors"], values=v_t)
    assert int(plan.status.item()) == 0
    ptr = plan.occ_ptr.cpu().numpy()
    e_bad = int(np.flatnonzero(np.diff(ptr) > 0)[3])                          # an entity with a non-empty list
    e_span = int(np.flatnonzero(np.diff(ptr) > 0)[9])
    plan.occ_rows[int(ptr[e_bad])] = pb["B"] + 5                              # a row number outside the batch
    plan.occ_ptr[e_span + 1] = -7                                             # entity e_span: end < beg; e_span + 1: beg < 0
    variant_adam_step(plan, st, t["entity"], t["bias"], t["scalars"], t["priors"], inv_occ, mo, 0.01, 2)
    torch.cuda.synchronize()
    assert int(plan.status.item()) >= 3                                       # (the positions kernel counts them too)
    for n in V.TENSORS:
        assert torch.isfinite(t[n]).all() and torch.isfinite(getattr(mo, "m_" + n)).all(), n
    from vae_amd import _lib
    with pytest.raises(_lib.VfmLibraryError):
        plan.check_status()


# ---------------------------------------------------------------------------------------------------- 5. public path
def test_fused_fit_learns_and_keeps_the_named_parameters_current():
    from vae_amd.variants import VFMClosedForm, variant_forward
    from vae_amd.data import synthetic_triples
    dev = torch.device("cuda:0")
    X, y = synthetic_triples([60, 40], 4000, seed=2)
    torch.manual_seed(0)
    m = VFMClosedForm([60, 40], 4, alpha_0=1.0)
    torch.manual_seed(0)
    m0 = VFMClosedForm([60, 40], 4, alpha_0=1.0)
    hist = m.fit(X, y, n_epochs=8, batch_size=1000, lr=0.05, fused=True)
    assert np.isfinite(hist).all() and hist[-1] < 0.8 * hist[0], hist
    # the first recorded batch loss is the unfused model's first batch loss (same init, same forward kernel)
    m0.set_training_data(torch.as_tensor(X))
    first, _, _ = m0.elbo(plan=m0.plan(torch.as_tensor(X)[:1000], torch.as_tensor(y, dtype=torch.float32)[:1000]))
    assert m.batch_losses[0][0].item() == first.item()
    # the named parameters are the flat buffers
    s = m.step_state()
    assert s.t == 8 * 4 and not s.dirty
    assert torch.equal(torch.cat([m.alpha, m.mean_global_bias, m.scale_global_bias]).detach(), s.scalars)
    assert torch.equal(m.priors_flat().detach(), s.priors)
    assert not torch.equal(s.scalars.cpu(), torch.cat([m0.alpha, m0.mean_global_bias, m0.scale_global_bias]).detach().cpu())
    plan = m.plan(torch.as_tensor(X)[:500], None)
    want = variant_forward(plan, "closed_form", m.entity_params.data, m.bias_params.data, s.scalars, None, train=False)["pred"]
    assert torch.equal(m(torch.as_tensor(X)[:500]), want)
    # checkpoint -> a fresh model -> one more step: the same bits as the original continuing
    state = m.training_state_dict()
    m2 = VFMClosedForm([60, 40], 4, alpha_0=1.0)
    m2.load_training_state_dict(state)
    m2.set_training_data(torch.as_tensor(X))
    assert torch.equal(m2.inv_occ, m.inv_occ) and m2.step_state().t == s.t
    Xb, yb = torch.as_tensor(X)[1000:2000], torch.as_tensor(y, dtype=torch.float32)[1000:2000]
    l1 = m.train_step(m.plan(Xb, yb), 0.05)
    l2 = m2.train_step(m2.plan(Xb, yb), 0.05)
    assert torch.equal(l1, l2)
    m.sync_parameters()
    m2.sync_parameters()
    sd1, sd2 = m.state_dict(), m2.state_dict()
    for k in sd1:
        assert torch.equal(sd1[k], sd2[k]), k
    for k in m.step_state().moments.NAMES:
        assert torch.equal(getattr(m.step_state().moments, k), getattr(m2.step_state().moments, k)), k

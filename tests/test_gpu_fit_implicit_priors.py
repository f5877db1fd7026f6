"""GPU: the implicit-feedback solve under a learnt field prior (include/vfm_implicit_prior.h:
VFM.fold_in_implicit(priors=), implicit_objective(priors=), fit_implicit(priors=, learn_priors=True)) against the fp64
reference of tests/implicit_prior_reference.py, which solves every entity from its dense row set under the prior.

Cases and bounds: those of tests/test_gpu_fit_implicit.py, unchanged (CHUNK = 16, W0 = f32(0.15), W1 = 1.25,
KLW = f32(0.7)).  Rows written by a solve: per element |got - ref| <= 2^-23 |ref| + 4 (d + 1) 2^-52 cond(H) max|ref|
(solve_reference.elementwise_ok / solve_abs_term) after asserting cond(H) <= 1e3 on the reference's own matrix, the
scales with solve_reference.scale_abs_term over 2 n_dense.  Losses and J_imp: 1e-5 relative.  J_imp after a block:
J_after <= J_before + 1e-9 |J_before|.  The prior block, computed by torch in fp64 and rounded once: 2^-23 |ref|
(elementwise_ok with no absolute term).  The priors are drawn with prior_reference.draw_priors(2, d, seed,
prec_lo_for(d)): means in [-0.5, 0.5], precisions in [0.25, 16].

Sensitivity: in every solve case the fp64 optimum under N(0, 1) misses the bound against the prior reference for every
entity (asserted on the CPU side of _check), so a kernel that ignores the prior cannot pass.

Every test here fails on the parent of this feature: the priors= arguments and the entry point do not exist there.

Measured on an MI355X: worst elementwise ratio of the solve under a prior 0.496 over d = 1, 8, 9, 33, 128, 134, 135, both
links and both fields, and the five catalog sizes (1 = at the bound; the reference itself rounded to fp32 gives at most
0.5), of the field blocks of three fit_implicit(learn_priors=True) sweeps 0.498 and of their prior blocks 0.484; losses
within 6.4e-8 and J_imp within 4.5e-9 relative; worst cond(H) 11.8 (a catalog of 16), 5.6 over the solve cases."""
import numpy as np
import pytest
import torch

import implicit_prior_reference as IPR
import implicit_reference as IR
import prior_reference as P
import solve_reference as R
from test_gpu_fit_implicit import CHUNK, KLW, W0, W1, _case, _counts, _model_of, _rows_of, _tables_of, _written

pytestmark = pytest.mark.gpu
DEV = "cuda"
LINKS = ["abs", "softplus"]


def _priors_of(d, seed, standard=False):
    from vae_amd import sweep
    pr = sweep.GroupPriors(2, d, DEV)
    if not standard:
        mean, prec = P.draw_priors(2, d, seed, P.prec_lo_for(d))
        pr.load_state_dict({"mean": mean.float(), "prec": prec.float()})
    return pr


def _row64(pr, field):
    return pr.mean[field].cpu().double(), pr.prec[field].cpu().double()


def _fold(c, m, pr, field=None, **kw):
    """pr None: the call without priors= (the methods take a GroupPriors or nothing)."""
    kw.setdefault("chunk_rows", CHUNK)
    if pr is not None:
        kw["priors"] = pr
    return m.fold_in_implicit(c["x"].to(DEV), c["y"].to(DEV), c["field"] if field is None else field, w0=W0, w1=W1,
                              kl_weight=KLW, **kw)


def _check(tab, c, m, out, pr, what, field=None):
    """The rows of out["entities"] written into m against implicit_solve_fp64_prior from the tables `tab` per element,
    out["loss"] against entity_loss_fp64_prior at the written rows, and -- sensitivity -- the fp64 optimum under N(0, 1)
    against the same reference: it misses the bound for every entity.  Returns (worst ratio, worst loss error)."""
    field = c["field"] if field is None else field
    ent, bia, scal = tab
    N, M, d, link = c["N"], c["M"], c["d"], c["link"]
    pm, pl = _row64(pr, field)
    ids = out["entities"].cpu()
    sol = IPR.implicit_solve_fp64_prior(ent, bia, scal, c["x"], c["y"], field, N, M, link, W0, W1, KLW, pm, pl, entities=ids)
    std = IR.implicit_solve_fp64(ent, bia, scal, c["x"], c["y"], field, N, M, link, W0, W1, KLW, entities=ids)
    assert float(sol["cond"].max()) <= 1e3, sol["cond"]
    theta, s = _written(m, ids)
    n_dense = M if field == 0 else N
    rs, rs_std = IR.inv_link_t(sol["sigma"], link), IR.inv_link_t(std["sigma"], link)
    worst, worst_l = 0.0, 0.0
    for i, e in enumerate(ids.tolist()):
        rt = sol["theta"][i].numpy()
        abs_t, abs_s = R.solve_abs_term(d, float(sol["cond"][i]), rt), R.scale_abs_term(2 * n_dense, rs[i].numpy())
        ok_t, w_t = R.elementwise_ok(theta[i], rt, abs_t)
        ok_s, w_s = R.elementwise_ok(s[i], rs[i].numpy(), abs_s)
        assert ok_t and ok_s, (what, e, int(out["rows"][i]), w_t, w_s)
        worst = max(worst, w_t, w_s)
        miss_t = not R.elementwise_ok(std["theta"][i], rt, abs_t)[0]
        miss_s = not R.elementwise_ok(rs_std[i], rs[i].numpy(), abs_s)[0]
        assert miss_t and miss_s, (what, e, "the N(0, 1) optimum is within the bound: the case does not see the prior")
        L = float(IPR.entity_loss_fp64_prior(ent, bia, scal, c["x"], c["y"], field, N, M, link, W0, W1, KLW, e,
                                             theta[i], IR.link_t(s[i], link), pm, pl))
        err = abs(float(out["loss"][i]) - L) / abs(L)
        assert err <= 1e-5, (what, e, float(out["loss"][i]), L)
        worst_l = max(worst_l, err)
    print(f"IMPLICIT-PRIOR {what} {link} d={d} field={field}: worst ratio {worst:.3f}, loss rel_err {worst_l:.2e}, "
          f"worst cond {float(sol['cond'].max()):.1f}")
    return worst, worst_l


# ---------------------------------------------------------------------------------------------------------------------
# the solve against implicit_solve_fp64_prior
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("d", [1, 8, 9, 33, 128])
def test_prior_solve_matches_fp64(d, link, field):
    from vae_amd import sweep
    split = sweep.resolve_split_rows(20, d)                                # (max(20, d + 1))
    counts = _counts(d, split)
    c = _case(len(counts) + 1, CHUNK * 40 + 5, d, link, counts, seed=500 + d, field=field)
    m, pr = _model_of(c), _priors_of(d, 31 + d)
    tab = _tables_of(m)
    out = _fold(c, m, pr, split_rows=20)
    assert out["rows"].tolist() == counts + [0] and out["entities"].numel() == len(counts) + 1
    _check(tab, c, m, out, pr, "solve")


@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("d", [R.LDS - 1, R.LDS])
def test_lds_rule_under_the_prior(d, link):
    """d + 1 = LDS: the triangle in LDS with the prior's 2 (d + 1) doubles beside it; d + 1 = LDS + 1: the slab."""
    counts = [0, d + 2, CHUNK * (d // CHUNK + 2) + 1]
    c = _case(4, 200, d, link, counts, seed=600 + d)
    m, pr = _model_of(c), _priors_of(d, 41 + d)
    tab = _tables_of(m)
    assert R.has_slabs(d) == (d == R.LDS)
    out = _fold(c, m, pr, split_rows=d + 3)                                # the second in its workgroup, the third in chunks
    _check(tab, c, m, out, pr, "lds/slab")


@pytest.mark.parametrize("n_partner", [1, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5])
def test_catalog_sizes_under_the_prior(n_partner):
    """A small catalog has a small base: the prior dominates the system."""
    d = 8
    counts = sorted({0, 1, min(n_partner, d + 1), n_partner})
    for link, field in (("abs", 0), ("softplus", 1)):
        c = _case(len(counts), n_partner, d, link, counts, seed=700 + n_partner, field=field)
        m, pr = _model_of(c), _priors_of(d, 51 + n_partner)
        tab = _tables_of(m)
        out = _fold(c, m, pr, split_rows=0)
        _check(tab, c, m, out, pr, f"catalog {n_partner}")


# ---------------------------------------------------------------------------------------------------------------------
# bits: the standard prior is the parent, an entity's bytes do not depend on the call
# ---------------------------------------------------------------------------------------------------------------------
def _mixed_case():
    """test_gpu_fit_implicit._mixed's case on a model of its own: 60 entities of 0 .. 11 observed rows and three heavy
    ones (100, 61 and 47 rows), d = 8, softplus."""
    counts = [g % 12 for g in range(60)]
    counts[17], counts[40], counts[41] = 100, 61, 47
    c = _case(60, 130, 8, "softplus", counts, seed=55)
    m = _model_of(c)
    return c, m, m._flat.clone()


@pytest.mark.parametrize("link", LINKS)
def test_standard_prior_is_the_parent_bit_for_bit(link):
    counts = [0, 1, 5, 9, 10, 21, 40, 100, 61]                             # no rows, the row-list form, the chunk form
    c = _case(len(counts) + 1, 130, 8, link, counts, seed=56)
    m = _model_of(c)
    start = m._flat.clone()
    std = _priors_of(8, 0, standard=True)
    for kw in (dict(split_rows=20), dict(split_rows=None), dict(split_rows=0, chunk_rows=7)):
        m._flat.copy_(start)
        parent = _fold(c, m, None, **kw)
        flat = m._flat.clone()
        m._flat.copy_(start)
        got = _fold(c, m, std, **kw)
        assert parent["rows"].tolist() == counts + [0]
        assert torch.equal(m._flat, flat) and torch.equal(got["loss"], parent["loss"]), kw
        assert torch.equal(got["entities"], parent["entities"]) and not torch.equal(flat, start)
    X, y = c["x"].to(DEV), c["y"].to(DEV)
    m._flat.copy_(start)
    a = m.fit_implicit(X, y, 2, w0=W0, w1=W1, kl_weight=KLW, split_rows=20, chunk_rows=CHUNK)
    flat = m._flat.clone()
    m._flat.copy_(start)
    b = m.fit_implicit(X, y, 2, w0=W0, w1=W1, kl_weight=KLW, split_rows=20, chunk_rows=CHUNK, priors=std)
    assert torch.equal(m._flat, flat) and "priors" not in a and b["priors"] is std and "clamped" not in b
    for Ja, Jb in zip(a["objective"], b["objective"]):
        assert abs(Ja - Jb) <= 1e-12 * abs(Ja)
    # learn_priors=True without priors= starts at N(0, 1): its first block is the parent's first block
    first = {}
    m._flat.copy_(start)
    m.fit_implicit(X, y, 1, w0=W0, w1=W1, kl_weight=KLW, split_rows=20, chunk_rows=CHUNK,
                   on_step=lambda s, w: first.setdefault("parent", m._flat.clone()))
    m._flat.copy_(start)
    out = m.fit_implicit(X, y, 1, w0=W0, w1=W1, kl_weight=KLW, split_rows=20, chunk_rows=CHUNK, learn_priors=True,
                         on_step=lambda s, w: first.setdefault("learnt", m._flat.clone()))
    assert torch.equal(first["parent"], first["learnt"])
    assert out["priors"].F == 2 and out["priors"].d == 8 and set(out["clamped"]) == {0, 1}
    assert not torch.equal(out["priors"].prec, torch.ones_like(out["priors"].prec))


def test_bits_under_a_prior_do_not_depend_on_the_call():
    c, m, start = _mixed_case()
    pr = _priors_of(8, 77)
    kw = dict(split_rows=20)
    out = _fold(c, m, pr, **kw)
    flat = m._flat.clone()
    assert out["rows"].tolist() == c["counts"]
    m._flat.copy_(start)
    again = _fold(c, m, pr, **kw)                                          # repeated calls
    assert torch.equal(m._flat, flat) and torch.equal(again["loss"], out["loss"])
    m._flat.copy_(start)
    parent = _fold(c, m, None, **kw)                                       # ... and the prior is read
    assert not torch.equal(m._flat, flat) and not torch.equal(parent["loss"], out["loss"])
    # groups: a workspace cap that holds one heavy entity's chunks at a time
    from vae_amd import _lib, sweep
    one = _lib.load().vfm_implicit_solve_prior_workspace_bytes(1, 6, 8, -1)   # (7, 4 and 3 chunks: no two fit together)
    x, y, _, _ = sweep.check_implicit_args(m, c["x"].to(DEV), c["y"].to(DEV), W0, W1, KLW)
    plan = sweep.ImplicitPlan(m, x, y, 0, None, 20, CHUNK, one)
    assert len(plan.obs.groups) == 3 and plan.obs.n_light == 52 and plan.empty.numel() == 5
    m._flat.copy_(start)
    grouped = _fold(c, m, pr, max_workspace_bytes=one, **kw)
    assert torch.equal(m._flat, flat) and torch.equal(grouped["loss"], out["loss"])
    # alone: a heavy entity, a light one, one without rows
    for e in (17, 40, 5, 0, 59):
        m._flat.copy_(start)
        alone = _fold(c, m, pr, entities=[e], **kw)
        assert alone["entities"].tolist() == [e] and alone["rows"].tolist() == [c["counts"][e]]
        assert torch.equal(alone["loss"], out["loss"][e:e + 1]), e
        assert torch.equal(_rows_of(m, m._flat, e), _rows_of(m, flat, e)), e
        other = (e + 1) % 60
        assert torch.equal(_rows_of(m, m._flat, other), _rows_of(m, start, other))       # nothing else is written


# ---------------------------------------------------------------------------------------------------------------------
# the objective and the sweeps
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("link", LINKS)
def test_implicit_objective_under_priors_matches_fp64(link):
    c = _case(30, 50, 9, link, [0, 1, 7, 50, 20, 33], seed=900)
    m, pr = _model_of(c), _priors_of(9, 61)
    mean, prec = pr.mean.cpu().double(), pr.prec.cpu().double()
    for klw in (1.0, KLW):
        J = m.implicit_objective(c["x"].to(DEV), c["y"].to(DEV), w0=W0, w1=W1, kl_weight=klw, priors=pr)
        ref = float(IPR.gram_J_prior(c["ent"], c["bia"], c["scal"], c["x"], c["y"], c["N"], c["M"], link, W0, W1, klw,
                                     mean, prec))
        brute = float(IPR.brute_J_prior(c["ent"], c["bia"], c["scal"], c["x"], c["y"], c["N"], c["M"], link, W0, W1, klw,
                                        mean, prec))
        plain = m.implicit_objective(c["x"].to(DEV), c["y"].to(DEV), w0=W0, w1=W1, kl_weight=klw)
        print(f"IMPLICIT-PRIOR objective {link} kl {klw}: rel_err {abs(J - ref) / abs(ref):.2e}")
        assert abs(ref - brute) <= 1e-10 * abs(brute)
        assert abs(J - ref) <= 1e-5 * abs(ref), (J, ref)
        assert abs(plain - ref) > 1e-3 * abs(ref)                          # the priors are in J


@pytest.mark.parametrize("link", LINKS)
def test_three_sweeps_block_by_block_learning_priors(link):
    counts = [0, 1, 5, 30, 12, 21, 40, 3, 0, 17]
    c = _case(12, 45, 5, link, counts, seed=1000)
    N, M, d = c["N"], c["M"], c["d"]
    m, pr = _model_of(c), _priors_of(5, 71)
    X, y = c["x"].to(DEV), c["y"].to(DEV)
    args = (c["x"], c["y"], N, M, link, W0, W1)
    pri = lambda: (pr.mean.cpu().double().clone(), pr.prec.cpu().double().clone())
    state = {"tab": _tables_of(m), "pri": pri(), "J": [], "whats": [], "worst": 0.0, "worst_p": 0.0}
    state["J"].append(float(IPR.gram_J_prior(*state["tab"], *args, KLW, *state["pri"])))

    def on_step(sweep, what):
        before, (mean0, prec0) = state["tab"], state["pri"]
        now, (mean1, prec1) = _tables_of(m), pri()
        state["whats"].append((sweep, what))
        if what == "scalars":
            s1 = IR.bias_block_fp64(before[0], before[1], before[2].double(), *args, KLW)
            s2 = IR.precision_block_fp64(before[0], before[1], s1, *args)
            assert torch.equal(now[0], before[0]) and torch.equal(now[1], before[1])
            assert torch.allclose(now[2].double(), s2, rtol=1e-5, atol=1e-7), (now[2], s2)
            assert torch.equal(mean1, mean0) and torch.equal(prec1, prec0)
        elif isinstance(what, tuple):
            f = what[1]
            assert what[0] == "prior" and all(torch.equal(a, b) for a, b in zip(now, before))
            rm, rl, _ = IPR.prior_block_fp64(now[0], now[1], f, N, M, link, mean0[f])       # over the field's whole range
            ok_m, w_m = R.elementwise_ok(mean1[f], rm.numpy(), 0.0)
            ok_l, w_l = R.elementwise_ok(prec1[f], rl.numpy(), 0.0)
            assert ok_m and ok_l, (sweep, what, w_m, w_l)
            state["worst_p"] = max(state["worst_p"], w_m, w_l)
            assert torch.equal(mean1[1 - f], mean0[1 - f]) and torch.equal(prec1[1 - f], prec0[1 - f])
        else:
            lo, hi = (0, N) if what == 0 else (N, N + M)
            ids = torch.arange(lo, hi)
            sol = IPR.implicit_solve_fp64_prior(*before, c["x"], c["y"], what, N, M, link, W0, W1, KLW, mean0[what],
                                                prec0[what])
            assert float(sol["cond"].max()) <= 1e3
            theta, s = _written(m, ids)
            rs = IR.inv_link_t(sol["sigma"], link)
            for i in range(ids.numel()):
                rt = sol["theta"][i].numpy()
                ok_t, w_t = R.elementwise_ok(theta[i], rt, R.solve_abs_term(d, float(sol["cond"][i]), rt))
                ok_s, w_s = R.elementwise_ok(s[i], rs[i].numpy(), R.scale_abs_term(2 * (hi - lo + N + M), rs[i].numpy()))
                assert ok_t and ok_s, (sweep, what, i, w_t, w_s)
                state["worst"] = max(state["worst"], w_t, w_s)
            olo, ohi = (N, N + M) if what == 0 else (0, N)
            assert torch.equal(now[0][olo:ohi], before[0][olo:ohi]) and torch.equal(now[2], before[2])
            assert torch.equal(mean1, mean0) and torch.equal(prec1, prec0)
        J = float(IPR.gram_J_prior(*now, *args, KLW, mean1, prec1))
        got = m.implicit_objective(X, y, w0=W0, w1=W1, kl_weight=KLW, priors=pr)
        assert abs(got - J) <= 1e-5 * abs(J), (sweep, what, got, J)
        assert J <= state["J"][-1] + 1e-9 * abs(state["J"][-1]), (sweep, what, J, state["J"][-1])
        state["J"].append(J)
        state["tab"], state["pri"] = now, (mean1, prec1)

    out = m.fit_implicit(X, y, 3, w0=W0, w1=W1, kl_weight=KLW, split_rows=9, chunk_rows=CHUNK, on_step=on_step, priors=pr,
                         learn_priors=True)
    assert state["whats"] == [(s, w) for s in range(3) for w in (0, ("prior", 0), 1, ("prior", 1), "scalars")]
    assert out["sweeps"] == 3 and len(out["objective"]) == 4 and out["priors"] is pr and out["clamped"] == {0: 0, 1: 0}
    for k, J in enumerate(out["objective"]):
        ref = state["J"][5 * k]
        assert abs(J - ref) <= 1e-5 * abs(ref), (k, J, ref)
    assert state["J"][-1] < state["J"][0]
    print(f"IMPLICIT-PRIOR sweeps {link}: worst ratio {state['worst']:.3f}, prior blocks {state['worst_p']:.3f}, "
          f"J {state['J'][0]:.4f} -> {state['J'][-1]:.4f}")


def test_learn_mean_false_and_the_clamp_count():
    counts = [0, 1, 5, 30, 12, 21, 40, 3, 0, 17]
    c = _case(12, 45, 5, "softplus", counts, seed=1001)
    N, M, link = c["N"], c["M"], c["link"]
    m, pr = _model_of(c), _priors_of(5, 81)
    X, y = c["x"].to(DEV), c["y"].to(DEV)
    mean0 = pr.mean.clone()
    lo_b, hi_b = 3.0, 4.0
    ref = {0: 0, 1: 0}

    def on_step(sweep, what):
        if isinstance(what, tuple):
            f = what[1]
            ent, bia, _ = _tables_of(m)
            _, clamped, free = IPR.prior_block_fp64(ent, bia, f, N, M, link, mean0[f].cpu(), learn_mean=False,
                                                    prec_min=lo_b, prec_max=hi_b)
            assert float(((free - lo_b).abs().min())) > 1e-6 and float(((free - hi_b).abs().min())) > 1e-6     # no tie
            ref[f] += int(((free < lo_b) | (free > hi_b)).sum())
            ok, _ = R.elementwise_ok(pr.prec[f].cpu(), clamped.numpy(), 0.0)
            assert ok, (sweep, what)

    out = m.fit_implicit(X, y, 2, w0=W0, w1=W1, kl_weight=KLW, split_rows=9, chunk_rows=CHUNK, on_step=on_step, priors=pr,
                         learn_priors=True, learn_mean=False, prec_min=lo_b, prec_max=hi_b)
    assert torch.equal(pr.mean, mean0)                                     # the means are kept
    assert out["clamped"] == ref and sum(ref.values()) > 0, (out["clamped"], ref)
    assert float(pr.prec.min()) >= lo_b and float(pr.prec.max()) <= hi_b
    Js = out["objective"]
    assert all(b <= a + 1e-9 * abs(a) for a, b in zip(Js, Js[1:]))


# ---------------------------------------------------------------------------------------------------------------------
# guards and E = 0 (supplied out-of-range ids only)
# ---------------------------------------------------------------------------------------------------------------------
def test_guards_and_an_empty_call_under_a_prior():
    from vae_amd import _lib
    c = _case(6, 40, 8, "abs", [3, 12, 0, 30], seed=1100)
    m, pr = _model_of(c), _priors_of(8, 91)
    o = _lib.ops()
    d, N, M, T = 8, c["N"], c["M"], c["N"] + c["M"]
    tables = m._views(m._flat)
    prior = pr.row(0)
    base = torch.empty(o.implicit_base_doubles(d), dtype=torch.float64, device=DEV)
    ws = torch.empty(o.implicit_base_workspace_bytes(M, CHUNK, d), dtype=torch.uint8, device=DEV)
    o.implicit_base(*tables, ws, base, N, M, CHUNK, 0)
    order = torch.sort(c["x"][:, 0], stable=True).indices
    xs, ys = c["x"][order], c["y"][order].to(DEV)
    partner = xs[:, 1].clone()
    partner[4] = T + 7                                                     # a row of entity 1: outside the table
    partner[20] = 2                                                        # a row of entity 3: inside it, outside the range
    ents = torch.tensor([0, 1, 2, 3, -1, T], device=DEV)
    ptr = torch.tensor([0, 3, 15, 15, 45, 45, 45], device=DEV)
    start = m._flat.clone()

    def solve(ents, row_ptr, cptr, tab, n_chunks):
        loss = torch.full((ents.numel(),), 7.0, device=DEV)
        w = torch.empty(max(o.implicit_solve_workspace_bytes(ents.numel(), n_chunks, d, -1), 1), dtype=torch.uint8, device=DEV)
        o.foldin_solve_implicit_prior(ents, row_ptr, cptr, tab, ys, partner.to(DEV), base, *tables, w, loss, prior, N, M, 0,
                                      -1, KLW, W0, W1)
        torch.cuda.synchronize()
        return loss

    def verify(loss):
        flat = m._flat
        assert bool(torch.isnan(loss[4])) and bool(torch.isnan(loss[5]))   # ids outside the table: NaN, nothing written
        for g in (1, 3):
            row = _rows_of(m, flat, g)
            assert bool(torch.isnan(row[:2 * d]).all()) and bool(torch.isnan(row[2 * d])) and bool(torch.isnan(loss[g])), g
            assert bool(torch.isfinite(row[2 * d + 1])), g                 # s_w is a function of the counts and the prior
        for g in (0, 2):
            assert bool(torch.isfinite(_rows_of(m, flat, g)).all()) and bool(torch.isfinite(loss[g])), g
        assert torch.equal(flat[4 * 2 * d:N * 2 * d], start[4 * 2 * d:N * 2 * d])
        assert torch.equal(flat[N * 2 * d:T * 2 * d], start[N * 2 * d:T * 2 * d])

    verify(solve(ents, ptr, None, None, 0))                                # the row-list form
    m._flat.copy_(start)
    cptr = torch.tensor([0, 1, 2, 2, 4, 4, 4], device=DEV)                 # the chunk form; the last chunk runs past R
    tab = torch.tensor([[0, 0, 3], [1, 3, 12], [3, 15, 16], [3, 31, 1 << 40]], device=DEV)
    verify(solve(ents, None, cptr, tab, 4))
    m._flat.copy_(start)
    # E = 0: nothing is launched, nothing is written
    none = torch.zeros(0, dtype=torch.int64, device=DEV)
    loss = solve(none, torch.zeros(1, dtype=torch.int64, device=DEV), None, None, 0)
    assert loss.numel() == 0 and torch.equal(m._flat, start)
    out = m.fold_in_implicit(c["x"].to(DEV), c["y"].to(DEV), 0, w0=W0, entities=[], priors=pr)
    assert out["entities"].numel() == 0 and out["loss"].numel() == 0 and torch.equal(m._flat, start)
    # a prior of the wrong shape never reaches the library
    with pytest.raises(RuntimeError, match="prior must be"):
        o.foldin_solve_implicit_prior(ents, ptr, None, None, ys, partner.to(DEV), base, *tables,
                                      torch.empty(1, dtype=torch.uint8, device=DEV), torch.empty(6, device=DEV),
                                      prior[:, :d].contiguous(), N, M, 0, -1, KLW, W0, W1)

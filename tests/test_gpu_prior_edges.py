"""GPU: the PRIOR instances of solve_body, bound_body, the two split solvers and the design score over the priors' own
range -- precisions at the ends of the learner's clamp [1e-4, 1e4], means in [-3, 3] -- and at the solver's widths.  The
cases and their references come from tests/prior_edges.py; tests/test_prior_edges_cpu.py checks the conditions on the
inputs and that every case of parts 2, 3 and 5 rejects four planted mistakes.

  2. exact solves over the range against mpmath (optimum_mp_prior): d = 8 and 64, both links, F = 2 and 3, n = 1, d / 2
     with duplicated rows, d, d + 1 and one split entity, unsplit and split.  Means: 2^-23 |ref| + 8 e_ref, e_ref the
     distance of the kernel-order fp64 restatement from mpmath; scales: scale_abs_term_wide; loss: 1e-5 of
     entity_objective_prior at the written rows, per entity.
  3. bound solves over the range against bound_rounds_fp64_prior: d = 8 and 33, both links, BR.GPU_ITERS, unsplit and
     split, by test_gpu_fit_bound_priors._check with n_iters solve_abs_term(d, cond_max, ref) <= 2^-23 max|ref| in the
     place of cond <= 1e3.
  4. widths and storage under drawn priors (cond <= 1e3, computed on the CPU): the parent's width_case (d = 300) and
     largest_dual_case (d = 512), past_cap_case, bitwise_case under a mixed prior (lds_dim -1 / 0 / 3 and block 0's three
     entities alone, bit for bit), and one wide bound case (d = 300).
  5. sessions under a prior along the rows the GPU session asked.  Wide: elicit_field_exact / _design / _bound at
     d = 33, 129 and LDS, reset on and off, drawn priors, every posterior against solve_fp64_prior /
     bound_rounds_fp64_prior with test_gpu_elicit_priors' criteria and caps (78.4 and 1e3).  One respondent has a long
     history: d - 2 rows at d = 33 (its system goes dual, largest dual, primal); LDS - 3 rows and 4 rounds at d = 129,
     where the primal system of 130 fits LDS and nothing crosses; LDS - 2 rows and 4 rounds at d = LDS
     (solve_reference.session_cases' pattern), where the system leaves LDS for the slab in round 2.  Range: d = 8, reset
     on, the three mixed priors and flat, 3 rounds; round 0 scored at foldin.prior_theta bit for bit, each fold against
     optimum_mp_prior by part 2's criterion, the bound session by part 3's.  And the design scores under all kinds of
     prior at d = 5, 20 and 128 against design_scores_prior, 2^-23 |ref|.

Measured on an MI355X (the printed PEDGE lines; 1 = at the bound, the reference rounded to fp32 gives at most 0.5):
  exact, per (d, kind) over links, F, n, unsplit and split: largest cond / e_ref / kernel_error = max |got - ref| of the
  fp32 result / ratio of the means / of the scales / loss rel
    8  flat   1.7e5  5.1e-11  2.0e-7  0.478  0.471  9.0e-8      64  flat   1.4e6  2.7e-9   7.7e-7  0.484  0.484  1.6e-7
    8  sharp  1.0    1.1e-15  1.2e-7  0.477  0.427  1.1e-7      64  sharp  1.1    3.1e-15  1.2e-7  0.484  0.433  1.2e-7
    8  mixed  1.8e5  8.8e-11  2.2e-7  0.493  0.477  1.2e-7      64  mixed  1.4e6  2.1e-9   7.0e-7  0.488  0.486  1.1e-7
    8  far    19     8.9e-15  1.0e-7  0.458  0.477  9.6e-8      64  far    140    1.6e-13  1.2e-7  0.476  0.486  8.9e-8
  bound, per (d, kind) over links, rounds and reset, unsplit = split: cond_max / worst ratio / rows / loss
    8  flat 2.0e4 0.481 4.6e-8 7.4e-8; sharp 2.7 0.483 5.2e-8 3.6e-8; mixed 4.3e5 0.495 5.1e-8 6.7e-8; far 5.7 0.467
    5.6e-8 6.5e-8;  33  flat 5.5e4 0.495 4.2e-8 9.1e-8; sharp 3.4 0.490 5.2e-8 7.1e-8; mixed 2.8e5 0.490 5.7e-8 6.9e-8;
    far 8.3 0.490 5.1e-8 5.6e-8
  widths: d = 300 0.473 (abs, cond_max 108.5, loss 3.9e-7) / 0.490 (softplus, 126.8, 4.1e-7); d = 512 0.475 (132.4,
    4.5e-7) / 0.475 (155.2, 5.6e-7); past the grid cap at d = 135 0.497 (14.2, 1.6e-7); the 16 entities of the bitwise
    case under mixed1 0.431 (cond up to 930, 8.7e-8); the wide bound case 0.498 / 0.487, rows 4.3e-8, loss 6.6e-8
  design scores, 18 (case, kind) pairs: at most 0.498 of 2^-23 |ref|
  wide sessions, cond_max / worst ratio / loss rel, reset on | off (the exact and design posteriors do not depend on it):
    d = 33   exact 40.3 0.478 6.1e-8;  design 21.4 0.492 9.6e-8;  bound 6.4 0.475 1.9e-7 | 0.493 1.0e-7
    d = 129  exact 23.7 0.485 | 0.486 9.7e-8;  design 66.9 0.492 6.0e-8;  bound 5.4 0.489 | 0.464 9.0e-8
    d = 135  exact 26.9 0.489 1.0e-7;  design 63.7 0.492 1.1e-7;  bound 5.1 0.486 1.1e-7
    (the long respondent's systems at d = 135: (134, lds), (135, lds), (136, slab), (136, slab))
  range sessions, exact | design: cond_max / e_ref / kernel_error / ratio of the means / of the scales / loss rel
    mixed0  1.5e5 1.4e-11 1.2e-7 0.490 0.412 1.2e-7 | 1.3e5 1.7e-11 2.1e-7 0.424 0.434 9.0e-8
    mixed1  967   2.6e-15 1.2e-7 0.464 0.469 8.5e-8 | 2.2e3 1.3e-15 1.1e-7 0.378 0.452 7.5e-8
    mixed2  585   8.9e-16 1.1e-7 0.443 0.410 9.6e-8 | 1.7e3 1.3e-15 1.2e-7 0.497 0.464 8.2e-8
    flat    1.5e5 2.0e-11 6.9e-8 0.476 0.447 6.9e-8 | 1.3e5 1.6e-11 9.3e-8 0.444 0.456 9.6e-8
    bound: mixed0 1.4e5 0.461 8.6e-7; mixed1 1.9e4 0.485 6.9e-8; mixed2 9.4e3 0.490 1.1e-7; flat 3.3e3 0.465 1.1e-6
    round 0 of all twelve at foldin.prior_theta bit for bit
The kernels' error is fp32 rounding in every case: nothing here exposed a fault in a PRIOR instance."""
import numpy as np
import pytest
import torch

import bound_prior_reference as BP
import bound_reference as BR
import design_restatement as DR
import elicit_priors_cases as EC
import prior_edges as E
import prior_reference as P
import solve_reference as R
from golden_util import rel_err
from test_gpu_solve_edges import _model_of, _written

pytestmark = pytest.mark.gpu
DEV = "cuda"
LINKS = ["abs", "softplus"]


def _priors(F, d, mean, prec):
    from vae_amd import sweep
    pr = sweep.GroupPriors(F, d, DEV)
    pr.load_state_dict({"mean": mean.float(), "prec": prec.float()})
    return pr


# ---------------------------------------------------------------------------------------------------------------------
# 2. exact solves over the range, against mpmath
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [2, 3])
@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("d", E.RANGE_DS)
def test_exact_solves_over_the_range_against_mpmath(d, link, F):
    bad = []
    for kind in E.exact_range_kinds(d, link, F):
        c, (pm, pl), refs = E.exact_range_references(d, link, F, kind)
        m = _model_of(c)
        start = m._flat.clone()
        pr = _priors(F, d, *E.edge_priors(F, d, kind))
        for how, kw in (("unsplit", {}), ("split", dict(split_rows=0, chunk_rows=E.CHUNK))):
            m._flat.copy_(start)
            out = m.fold_in_exact(c["X"].to(DEV), c["y"].to(DEV), field=0, kl_weight=c["kl_weight"], priors=pr, **kw)
            assert torch.equal(out["entities"].cpu(), c["ids"]) and out["rows"].tolist() == c["counts"]
            theta, s = _written(m, c["ids"])
            loss = out["loss"].cpu().double().numpy()
            for k, r in enumerate(refs):
                ok, w_t, w_s = E.exact_criterion(r, theta[k], s[k])
                err = float(np.abs(theta[k].double().numpy() - r["ref"]["theta"]).max())
                L = E.reference_objective(c, k, theta[k].double().numpy(), s[k].double().numpy(), pm, pl)
                el = abs(loss[k] - L) / abs(L)
                print(f"PEDGE exact d={d} {link} F={F} {kind} {how} n={r['n']}: cond {r['ref']['cond']:.3e} e_ref "
                      f"{r['e_ref']:.3e} kernel_error {err:.3e} ratio theta {w_t:.3f} scales {w_s:.3f} loss rel {el:.2e}")
                if not (ok and el <= 1e-5):
                    bad.append((kind, how, r["n"], w_t, w_s, el))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------
# 3. bound solves over the range
# ---------------------------------------------------------------------------------------------------------------------
def _check_bound(c, m, loss, pm, pl, n_iters, reset, what):
    """test_gpu_fit_bound_priors._check with its cond <= 1e3 replaced by prior_edges.bound_tight."""
    from test_gpu_foldin_bound import _written as written
    ids, d, f = c["ids"], c["d"], c["field"]
    theta, s = written(m, ids)
    worst, cmax, Bref, rt, rs = 0.0, 0.0, [], [], []
    for k in range(len(c["counts"])):
        r = BP.case_rounds_prior(c, k, n_iters, reset, pm, pl)
        cond = float(r["cond"].max())
        assert r["n"] == c["counts"][k] and E.bound_tight(d, n_iters, cond, r["theta"][-1]), (what, cond)
        ok, w = E.bound_criterion(d, n_iters, r, theta[k], s[k])
        assert ok, (what, n_iters, reset, r["n"], w)
        worst, cmax = max(worst, w), max(cmax, cond)
        rt.append(r["theta"][-1])
        rs.append(r["s"][-1])
        Bref.append(BP.bound_objective_fp64_prior(c["ent"], c["bia"], c["scal"], c["X"], c["y"], f, c["link"],
                                                  c["kl_weight"], int(ids[k]), theta[k], s[k], pm, pl))
    e_rows = max(rel_err(theta.numpy(), np.array(rt)), rel_err(s.numpy(), np.array(rs)))
    e_loss = rel_err(loss.cpu().numpy(), np.array(Bref))
    print(f"PEDGE bound {what} d={d} {c['link']} n_iters={n_iters} reset={int(reset)}: cond_max {cmax:.3e} worst ratio "
          f"{worst:.3f} rows {e_rows:.2e} loss {e_loss:.2e}")
    assert e_rows <= 1e-4 and e_loss <= 1e-5, (e_rows, e_loss)
    return worst


@pytest.mark.parametrize("kind", E.KINDS)
@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("d", E.BOUND_DS)
def test_bound_solves_over_the_range(d, link, kind):
    from test_gpu_foldin_bound import _model_of as model_of
    c = E.bound_range_case(d, link)
    mean, prec = E.edge_priors(3, d, kind)
    m, pr = model_of(c), _priors(3, d, mean, prec)
    start = m._flat.clone()
    for how, kw in (("unsplit", {}), ("split", dict(split_rows=0, chunk_rows=E.CHUNK))):
        for n_iters, reset in BR.GPU_ITERS:
            m._flat.copy_(start)
            out = m.fold_in_bound(c["X"].to(DEV), c["y"].to(DEV), field=0, kl_weight=c["kl_weight"], n_iters=n_iters,
                                  reset=reset, priors=pr, **kw)
            assert torch.equal(out["entities"].cpu(), c["ids"]) and out["rows"].tolist() == c["counts"]
            _check_bound(c, m, out["loss"], mean[0], prec[0], n_iters, reset, f"{kind} {how}")


# ---------------------------------------------------------------------------------------------------------------------
# 4. widths and storage under a prior
# ---------------------------------------------------------------------------------------------------------------------
def _check_exact(c, m, loss, pm, pl, what, which=None, cap=E.WIDTH_COND):
    """test_gpu_solve_edges._check against solve_fp64_prior and entity_objective_prior."""
    which = list(range(len(c["counts"]))) if which is None else list(which)
    ids = c["ids"][which]
    field, link, klw, d = c["field"], c["link"], c["kl_weight"], c["d"]
    sel = torch.isin(c["X"][:, field], ids)
    X, y = c["X"][sel], c["y"][sel]
    sol = P.solve_fp64_prior(c["ent"], c["bia"], c["scal"], X, y, field, link, klw, pm, pl)
    assert torch.equal(sol["entities"], ids)
    cond = sol["cond"].tolist()
    assert cap is None or max(cond) <= cap, max(cond)
    theta, s = _written(m, ids)
    worst = 0.0
    for i, k in enumerate(which):
        n = c["counts"][k]
        rt = np.concatenate([[float(sol["mu_w"][i])], sol["mu"][i].numpy()])
        rs = np.concatenate([[float(sol["s_w"][i])], sol["s"][i].numpy()])
        ok_t, w_t = R.elementwise_ok(theta[i], rt, R.solve_abs_term(d, cond[i], rt))
        ok_s, w_s = R.elementwise_ok(s[i], rs, R.scale_abs_term(n, rs))
        if len(which) <= 16:
            print(f"PEDGE {what} {link} d={d} n={n} {'dual' if n <= d else 'primal'} {R.storage(n, d)} cond "
                  f"{cond[i]:.1f}: worst ratio theta {w_t:.3f} scales {w_s:.3f}")
        assert ok_t and ok_s, (what, n, w_t, w_s)
        worst = max(worst, w_t, w_s)
    th = (ids, theta[:, 1:].double(), s[:, 1:].double(), theta[:, 0].double(), s[:, 0].double())
    L = P.entity_objective_prior(c["ent"], c["bia"], c["scal"], X, y.double(), field, th, link, klw, pm, pl)
    el = rel_err(loss.cpu()[which].numpy(), L.numpy())
    print(f"PEDGE {what} {link} d={d}: worst ratio {worst:.3f}, cond_max {max(cond):.1f}, loss rel_err {el:.2e}")
    assert el <= 1e-5, el
    return worst


def _run_exact(c, m, pr, lds_dim=-1, X=None, y=None):
    from vae_amd import foldin
    X, y = (c["X"], c["y"]) if X is None else (X, y)
    return foldin.run_exact(m, X.to(DEV), y.to(DEV), c["field"], c["kl_weight"], lds_dim=lds_dim, priors=pr)


@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("name", ["width", "largest_dual"])
def test_storage_and_width_edges_under_a_prior(name, link):
    c = (R.width_case if name == "width" else R.largest_dual_case)(link)
    mean, prec = E.width_priors(c, name)
    m, pr = _model_of(c), _priors(len(c["sizes"]), c["d"], mean, prec)
    ents, loss, rows = _run_exact(c, m, pr)
    assert torch.equal(ents.cpu(), c["ids"]) and rows.tolist() == c["counts"]
    assert {R.storage(n, c["d"]) for n in c["counts"]} == ({"lds", "slab"} if c["d"] == 300 else {"slab"})
    f = c["field"]
    _check_exact(c, m, loss, mean[f], prec[f], name)


def test_past_the_slab_grid_cap_under_a_prior():
    c = R.past_cap_case()
    mean, prec = E.width_priors(c, "past_cap")
    m, pr = _model_of(c), _priors(2, c["d"], mean, prec)
    ents, loss, rows = _run_exact(c, m, pr)
    assert ents.numel() == R.SLABS + 5 and rows.tolist() == c["counts"]
    _check_exact(c, m, loss, mean[0], prec[0], "past_cap")


def test_past_the_slab_grid_cap_bitwise_under_a_mixed_prior():
    c = R.bitwise_case()
    mean, prec = E.edge_priors(3, R.BITWISE_D, E.BITWISE_KIND)
    m, pr = _model_of(c), _priors(3, R.BITWISE_D, mean, prec)
    start = m._flat.clone()
    E_ = len(c["counts"])
    runs = {}
    for ld in R.BITWISE_LDS_DIMS:
        m._flat.copy_(start)
        ents, loss, rows = _run_exact(c, m, pr, ld)
        assert ents.numel() == E_ and rows.tolist() == c["counts"]
        runs[ld] = (m._flat.clone(), loss.clone())
    first = runs[R.BITWISE_LDS_DIMS[0]]
    assert bool(torch.isfinite(first[1]).all()) and not torch.equal(first[0], start)
    for ld in R.BITWISE_LDS_DIMS[1:]:
        assert torch.equal(runs[ld][0], first[0]) and torch.equal(runs[ld][1], first[1]), ld
    d, off = m.d, m._off_bias
    for g in (0, R.SLABS, 2 * R.SLABS):                      # block 0's three entities, each alone
        e = int(c["ids"][g])
        sel = c["X"][:, c["field"]] == e
        for ld in R.BITWISE_LDS_DIMS:
            m._flat.copy_(start)
            _, loss, rows = _run_exact(c, m, pr, ld, c["X"][sel], c["y"][sel])
            assert rows.tolist() == [c["counts"][g]]
            assert torch.equal(loss, first[1][g:g + 1]), (g, ld)
            assert torch.equal(m._flat[e * 2 * d:(e + 1) * 2 * d], first[0][e * 2 * d:(e + 1) * 2 * d]), (g, ld)
            assert torch.equal(m._flat[off + 2 * e: off + 2 * e + 2], first[0][off + 2 * e: off + 2 * e + 2]), (g, ld)
    m._flat.copy_(first[0])
    _check_exact(c, m, first[1], mean[0], prec[0], "bitwise", R.bitwise_sample(E_))


@pytest.mark.parametrize("link", LINKS)
def test_wide_bound_solve_under_a_prior(link):
    from test_gpu_fit_bound_priors import _check
    from test_gpu_foldin_bound import _model_of as model_of
    c = E.bound_wide_case(link)
    mean, prec = E.width_priors(c, "bound_wide")
    m, pr = model_of(c), _priors(3, 300, mean, prec)
    out = m.fold_in_bound(c["X"].to(DEV), c["y"].to(DEV), field=1, kl_weight=c["kl_weight"], n_iters=2, reset=True, priors=pr)
    assert out["rows"].tolist() == c["counts"]
    worst, e_rows, e_loss = _check(c, m, out["loss"], pr, 2, True, "wide")
    print(f"PEDGE bound wide d=300 {link}: worst ratio {worst:.3f} rows {e_rows:.2e} loss {e_loss:.2e}")


# ---------------------------------------------------------------------------------------------------------------------
# 5. the design scores under every kind of prior
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d5_abs", "d20_softplus", "d128_softplus"])
def test_design_scores_over_the_range(name):
    from test_gpu_foldin import _model
    c, ref = DR.build(name)
    m = _model(c["sizes"], c["d"], "reg", c["link"], seed=1)
    m.entity_params.weight.data.copy_(c["ent"])
    m.bias_params.weight.data.copy_(c["bia"])
    m._flat[m._off_scal: m._off_scal + 3] = c["scal"].to(DEV)
    m.params_changed()
    g = {k: (c[k].to(DEV) if c[k] is not None else None) for k in ("pool", "hist_x", "hist_y", "targets")}
    hist = (g["hist_x"], g["hist_y"]) if g["hist_x"].shape[0] else None
    f = c["field"]
    pk, kl = DR.prec_kl(c["scal"], c["link"], c["klw"])
    for kind in E.KINDS:
        mean, prec = E.edge_priors(len(c["sizes"]), c["d"], kind)
        got = m.design_scores_field(g["pool"], f, targets=g["targets"], history=hist, kl_weight=c["klw"],
                                    priors=_priors(len(c["sizes"]), c["d"], mean, prec)).cpu()
        worst = 0.0
        for e, r in ref.items():
            pm, hm = c["pool"][:, f] == e, c["hist_x"][:, f] == e
            Mp, Ap = DR.operands(c["ent"], c["bia"], c["scal"], c["pool"][pm].numpy(), f, c["link"])
            Mh, Ah = DR.operands(c["ent"], c["bia"], c["scal"], c["hist_x"][hm].numpy(), f, c["link"])
            want = EC.design_scores_prior(DR.walk_S(Mh, Ah), r["W"], int(hm.sum()), Mp, Ap, kl, pk, prec[f].numpy())
            err = np.abs(got[pm].double().numpy() - want)
            worst = max(worst, float((err / (R.EPS32 * np.abs(want))).max()))
        print(f"PEDGE design {name} {kind}: worst |got - ref| / (2^-23 |ref|) = {worst:.3f}")
        assert worst <= 1.0, (kind, worst)


# ---------------------------------------------------------------------------------------------------------------------
# 5. sessions under a prior beyond d = 5, against fp64 / mpmath along the rows the session asked
# ---------------------------------------------------------------------------------------------------------------------
def _session(c, name, reset, **kw):
    from test_gpu_elicit_priors import _planted, _run
    m, priors = _planted(c)
    pool, y_pool, hx, hy = (c[k].to(DEV) for k in ("pool", "y_pool", "hist_x", "hist_y"))
    out = _run(name, m, pool, y_pool, c["Q"], c["field"], "variance", (hx, hy), reset, priors, n_iters=c["n_iters"],
               return_theta=True, **kw)
    assert bool((out["rows"] >= 0).all())                   # every pool row was asked
    return m, priors, out


def _split_theta(got, d):
    return torch.cat([got[2 * d:2 * d + 1], got[:d]]), torch.cat([got[2 * d + 1:], got[d:2 * d]])


def _exact_loss_ref(c, x, y, e, gt, gs):
    f = c["field"]
    th = (torch.tensor([e]), gt[None, 1:].double(), gs[None, 1:].double(), gt[:1].double(), gs[:1].double())
    return float(P.entity_objective_prior(c["ent"], c["bia"], c["scal"], x, y.double(), f, th, c["link"], R.f32(c["klw"]),
                                          c["mean"][f], c["prec"][f])[0])


def _bound_session_check(c, out, reset, what, tight):
    """test_gpu_elicit_priors.test_bound_posteriors_against_fp64_along_the_sessions_rows for case c; tight: part 3's
    condition in the place of cond <= COND_BOUND."""
    f, d = c["field"], c["d"]
    rows, theta, loss = out["rows"].cpu(), out["theta"].cpu(), out["loss"].cpu()
    worst = cmax = lmax = 0.0
    for u, e in enumerate(out["entities"].tolist()):
        start = E.session_start(c, e, reset)
        for q in range(c["Q"]):
            x, y = EC.rows_of(c, e, rows[u, :q + 1])
            r = EC.bound_fold(c, x, y, e, start)
            cond = float(r["cond"].max())
            if tight:
                assert E.bound_tight(d, c["n_iters"], cond, r["theta"][-1]), (e, q, cond)
            else:
                assert cond <= EC.COND_BOUND, (e, q, cond)
            gt, gs = _split_theta(theta[u, q], d)
            ok, w = E.bound_criterion(d, c["n_iters"], r, gt, gs)
            assert ok, (what, e, q, w)
            want = BP.bound_objective_fp64_prior(c["ent"], c["bia"], c["scal"], x, y, f, c["link"], c["klw"], e, gt, gs,
                                                 c["mean"][f], c["prec"][f])
            el = abs(float(loss[u, q]) - want) / abs(want)
            assert el <= 1e-5, (what, e, q, float(loss[u, q]), want)
            worst, cmax, lmax = max(worst, w), max(cmax, cond), max(lmax, el)
            start = EC.start_of_row(c, gt[:1].numpy(), gt[1:].numpy(), gs[:1].numpy(), gs[1:].numpy())
    print(f"PEDGE session {what}: cond_max {cmax:.3e} worst ratio {worst:.3f} loss rel {lmax:.2e}")


@pytest.mark.parametrize("reset", [True, False])
@pytest.mark.parametrize("name", E.SESSION_NAMES)
@pytest.mark.parametrize("d", E.WIDE_DS)
def test_wide_sessions_against_fp64_along_the_sessions_rows(d, name, reset):
    c = E.session_case(name, d)
    m, priors, out = _session(c, name, reset)
    what = f"wide {name} d={d} reset={int(reset)}"
    u_long = out["entities"].tolist().index(c["long"])
    print(f"PEDGE session {what}: systems of the long respondent {R.session_systems(d, c['H'], c['Q'])}")
    if name == "bound":
        return _bound_session_check(c, out, reset, what, tight=False)
    rows, theta, loss = out["rows"].cpu(), out["theta"].cpu(), out["loss"].cpu()
    worst = cmax = lmax = 0.0
    for u, e in enumerate(out["entities"].tolist()):
        for q in range(c["Q"]):
            x, y = EC.rows_of(c, e, rows[u, :q + 1])
            rt, rs, cond, n = E.session_reference_fp64(c, x, y)
            assert cond <= EC.COND_EXACT, (e, q, cond)
            assert u != u_long or n == c["H"] + q + 1
            gt, gs = _split_theta(theta[u, q], d)
            ok, w = E.wide_criterion(d, rt, rs, cond, n, gt, gs)
            assert ok, (what, e, q, w)
            want = _exact_loss_ref(c, x, y, e, gt, gs)
            el = abs(float(loss[u, q]) - want) / abs(want)
            assert el <= 1e-5, (what, e, q, float(loss[u, q]), want)
            worst, cmax, lmax = max(worst, w), max(cmax, cond), max(lmax, el)
    print(f"PEDGE session {what}: cond_max {cmax:.1f} worst ratio {worst:.3f} loss rel {lmax:.2e}")


@pytest.mark.parametrize("kind", E.RANGE_KINDS)
@pytest.mark.parametrize("name", E.SESSION_NAMES)
def test_range_sessions_against_mpmath_along_the_sessions_rows(name, kind):
    from test_gpu_elicit import _same_bits
    from test_gpu_elicit_priors import _write_prior_rows
    d = E.RANGE_D
    c = E.session_case(name, d, kind)
    m, priors, out = _session(c, name, True, return_moments=True)
    what = f"range {name} {kind}"
    if name == "bound":
        _bound_session_check(c, out, True, what, tight=True)
    else:
        rows, theta, loss = out["rows"].cpu(), out["theta"].cpu(), out["loss"].cpu()
        worst_t = worst_s = cmax = emax = kmax = lmax = 0.0
        for u, e in enumerate(out["entities"].tolist()):
            for q in range(c["Q"]):
                x, y = EC.rows_of(c, e, rows[u, :q + 1])
                r = E.session_reference_mp(c, x, y, e)
                gt, gs = _split_theta(theta[u, q], d)
                ok, w_t, w_s = E.exact_criterion(r, gt, gs)
                assert ok, (what, e, q, w_t, w_s)
                want = _exact_loss_ref(c, x, y, e, gt, gs)
                el = abs(float(loss[u, q]) - want) / abs(want)
                assert el <= 1e-5, (what, e, q, float(loss[u, q]), want)
                worst_t, worst_s, lmax = max(worst_t, w_t), max(worst_s, w_s), max(lmax, el)
                cmax, emax = max(cmax, r["ref"]["cond"]), max(emax, r["e_ref"])
                kmax = max(kmax, float(np.abs(gt.double().numpy() - r["ref"]["theta"]).max()))
        print(f"PEDGE session {what}: cond_max {cmax:.3e} e_ref {emax:.3e} kernel_error {kmax:.3e} ratio theta "
              f"{worst_t:.3f} scales {worst_s:.3f} loss rel {lmax:.2e}")
    # round 0 was scored at foldin.prior_theta, bit for bit
    pool = c["pool"].to(DEV)
    _write_prior_rows(m, torch.unique(pool[:, c["field"]]), priors, c["field"])
    mean, var, _ = m.field_moments(pool, c["field"])
    assert _same_bits(out["logit_mean"][0], mean) and _same_bits(out["logit_var"][0], var)

"""CPU: the references and the input conditions of tests/test_gpu_prior_edges.py (the PRIOR instances of the solvers over
the priors' own range [1e-4, 1e4] and at the solver's widths), from tests/prior_edges.py.

  - edge_priors is what its docstring says: fp32 values, the range's ends, three rotations of mixed, distinct means;
  - optimum_mp_prior at (0, 1) is optimum_mp to the last digit kept; solve_fp64_prior's two forms and the kernel-order
    restatements agree with it within e_ref's order;
  - every exact case of the range: |L_e| >= 1 at the reference optimum; the restatement rounded once to fp32 passes the
    case's criterion with worst ratio <= 0.5; under the mixed prior each of the four planted mistakes
    (prior_edges.MISTAKES) fails it, for every entity;
  - every bound case of the range: n_iters solve_abs_term(d, cond_max, ref) <= 2^-23 max|ref| (printed BCOND: cond up to
    4.3e5 against the caps 1.5e7 / 1.9e6 at d = 8 and 3.9e6 / 4.9e5 at d = 33 for 1 / 8 rounds), and under the mixed
    prior the four mistakes fail test_gpu_fit_bound_priors._check's elementwise criterion;
  - the sessions of part 5: the wide cases (d = 33, 129, LDS) keep every matrix a session could factor under
    elicit_priors_cases' caps (printed SCOND) and the respondent with the long history meets the edges its d is there for;
    the range cases (d = 8) meet part 3's condition (bound) in every order; along the pool order and its reverse every fold
    of every session case passes its criterion with the restatement rounded to fp32 at <= 0.5 and, under a mixed prior,
    fails it with each of the four mistakes;
  - the width cases under their drawn priors keep every factored matrix under cond 1e3 (printed WCOND)."""
import numpy as np
import pytest
import torch

import bound_prior_reference as BP
import bound_reference as BR
import elicit_priors_cases as EC
import prior_edges as E
import prior_reference as P
import solve_reference as R

LINKS = ["abs", "softplus"]


# ---------------------------------------------------------------------------------------------------------------------
# 1. the priors
# ---------------------------------------------------------------------------------------------------------------------
def test_edge_priors():
    for F, d in ((2, 8), (3, 64)):
        weight = set()
        for kind in E.KINDS:
            mean, prec = E.edge_priors(F, d, kind)
            assert mean.shape == prec.shape == (F, d + 1) and mean.dtype == prec.dtype == torch.float64
            assert torch.equal(mean, mean.float().double()) and torch.equal(prec, prec.float().double())
            assert float(mean.abs().max()) <= 3.0 and float(mean.max()) > 1.0 and float(mean.min()) < -1.0
            assert all(torch.unique(mean[f]).numel() == d + 1 for f in range(F))         # distinct per coordinate
            assert float(prec.min()) >= E.LAM_LO and float(prec.max()) <= E.LAM_HI
            if kind in E.MIXED:
                weight.add(float(prec[0, 0]))
                assert sorted(torch.unique(prec).tolist()) == [E.LAM_LO, 1.0, E.LAM_HI]
                assert bool((prec[:, 1:] != prec[:, :-1]).all())                         # neighbours differ
            else:
                assert torch.unique(prec).tolist() == [dict(flat=E.LAM_LO, sharp=E.LAM_HI, far=1.0)[kind]]
        assert weight == {E.LAM_LO, 1.0, E.LAM_HI}                                       # the weight takes each value once
    assert torch.equal(E.edge_priors(2, 8, "mixed")[1], E.edge_priors(2, 8, "mixed0")[1])


# ---------------------------------------------------------------------------------------------------------------------
# 2. the references
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("F", [2, 3])
def test_optimum_mp_prior_at_the_standard_prior_is_optimum_mp(F, link):
    c = E.exact_range_case(8, link, F)
    for k in range(len(c["counts"])):
        a = R.optimum_mp(*E._args(c, k))
        b = E.optimum_mp_prior(*E._args(c, k), np.zeros(9), np.ones(9))
        assert a["n"] == b["n"] and np.array_equal(a["theta"], b["theta"]) and np.array_equal(a["s"], b["s"])


@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("d", E.RANGE_DS)
def test_fp64_forms_agree_with_mpmath_within_e_refs_order(d, link):
    """solve_fp64_prior (LAPACK, both forms) and the two kernel-order restatements against optimum_mp_prior: each within
    64 eps64 cond max|ref| of it, the order of e_ref (YARDSTICK of test_solve_edges_cpu: 0.18 to 2.3 eps64 cond
    max|ref|), cond the condition number of the matrix that form factors."""
    F, kind = 3, [k for k in E.exact_range_kinds(d, link, 3) if k in E.MIXED][0]
    c, (m, lam), refs = E.exact_range_references(d, link, F, kind)
    sols = {form: P.solve_fp64_prior(c["ent"], c["bia"], c["scal"], c["X"], c["y"], 0, link, c["kl_weight"], m, lam, form)
            for form in ("primal", "dual")}
    for k, r in enumerate(refs):
        ref, n = r["ref"], r["n"]
        top = float(np.abs(ref["theta"]).max())
        s = E.system64_prior(*E._args(c, k), m, lam)
        U = np.concatenate([np.ones((n, 1)), s["M"]], 1)
        cond = {"primal": float(np.linalg.cond(np.diag(s["D"]) + s["prec"] * (U.T @ U))),
                "dual": float(np.linalg.cond(np.eye(n) / s["prec"] + (U / s["D"]) @ U.T))}
        for form, sol in sols.items():
            th = np.concatenate([[float(sol["mu_w"][k])], sol["mu"][k].numpy()])
            sc = np.concatenate([[float(sol["s_w"][k])], sol["s"][k].numpy()])
            err = float(np.abs(th - ref["theta"]).max())
            # (the dual form subtracts D^-1 b and D^-1 U^T z, each up to max(D^-1 b) / max|ref| times their difference)
            amp = max(1.0, float(np.abs(s["b"] / s["D"]).max()) / top) if form == "dual" else 1.0
            assert err <= 64 * R.EPS64 * cond[form] * amp * top, (form, n, err)
            assert R.elementwise_ok(sc.astype(np.float32), ref["s"], E.scale_abs_term_wide(n, ref["s"]))[0]
        kform = "dual" if n <= d else "primal"
        amp = max(1.0, float(np.abs(s["b"] / s["D"]).max()) / top) if kform == "dual" else 1.0
        print(f"EREF d={d} {link} {kind} n={n} {kform}: cond {cond[kform]:.3e} e_ref {r['e_ref']:.3e} "
              f"e_ref / (eps64 cond max|ref|) {r['e_ref'] / (R.EPS64 * cond[kform] * top):.3f}")
        assert abs(cond[kform] - ref["cond"]) <= 1e-6 * ref["cond"]
        assert r["e_ref"] <= 64 * R.EPS64 * cond[kform] * amp * top


def test_scale_abs_term_wide_is_the_derivation():
    """g(sigma) = sigma / (1 - exp(-sigma)) against the two bounds the docstring uses, over [0.01, 100]; the term is
    never below scale_abs_term."""
    sg = np.exp(np.linspace(np.log(0.01), np.log(100.0), 2001))
    g = sg / -np.expm1(-sg)
    s = np.log(np.expm1(sg))
    assert (g[sg <= 1.0] <= 1.6).all() and (g >= 1.0).all()
    assert (g[sg > 1.0] <= 2.46 * np.maximum(1.0, np.abs(s[sg > 1.0]))).all()
    assert (g <= 2.46 * np.maximum(1.0, np.abs(s))).all()
    for n in (0, 1, 9, 81, 4000):
        for ref in ([0.3], [-4.6], [100.0]):
            assert E.scale_abs_term_wide(n, ref) >= R.scale_abs_term(n, ref)
            assert 2.46 * (n / 2 + 4.5) + 2 <= 1.25 * n + 14


# ---------------------------------------------------------------------------------------------------------------------
# 2 / 6. the exact cases of the range: conditions on the inputs, and the cases discriminate
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [2, 3])
@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("d", E.RANGE_DS)
def test_exact_range_cases(d, link, F):
    kinds = E.exact_range_kinds(d, link, F)
    assert set(kinds) >= {"flat", "sharp", "far"} and any(k in E.MIXED for k in kinds)
    for kind in kinds:
        c, (m, lam), refs = E.exact_range_references(d, link, F, kind)
        assert c["counts"] == [1, d // 2, d, d + 1, E.CHUNK * (d // E.CHUNK + 2) + 1] and c["kl_weight"] != 1.0
        assert [int((c["X"][:, 0] == e).sum()) for e in c["ids"]] == c["counts"]
        half = c["X"][c["X"][:, 0] == int(c["ids"][1])]
        assert bool((torch.unique(half, dim=0, return_counts=True)[1] % 2 == 0).all())   # every other row a duplicate
        for k, r in enumerate(refs):
            ref, n = r["ref"], r["n"]
            L = E.reference_objective(c, k, ref["theta"], ref["s"], m, lam)
            assert abs(L) >= 1.0, (kind, n, L)
            assert 0.009 <= ref["sigma"].min() and ref["sigma"].max() <= 100.0    # (scale_abs_term_wide's range)
            th, s = r["restated"]
            ok, w_t, w_s = E.exact_criterion(r, th.astype(np.float32), s.astype(np.float32))
            assert ok and max(w_t, w_s) <= 0.5, (kind, n, w_t, w_s)
            caught = []
            if kind in E.MIXED:
                for mistake in E.MISTAKES:
                    th2, s2 = E.restatement_fp64_prior(*E._args(c, k), m, lam, mistake)
                    bad, v_t, v_s = E.exact_criterion(r, th2.astype(np.float32), s2.astype(np.float32))
                    assert not bad, (kind, n, mistake, v_t, v_s)
                    caught.append(max(v_t, v_s))
            print(f"ECASE d={d} {link} F={F} {kind} n={n}: cond {ref['cond']:.3e} e_ref {r['e_ref']:.3e} L_e {L:.1f} sigma "
                  f"[{ref['sigma'].min():.3g}, {ref['sigma'].max():.3g}] restated ratio {max(w_t, w_s):.3f}"
                  + (f" mistakes' ratios {min(caught):.1e} .. {max(caught):.1e}" if caught else ""))


# ---------------------------------------------------------------------------------------------------------------------
# 3 / 6. the bound cases of the range
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("d", E.BOUND_DS)
def test_bound_range_cases(d, link):
    c = E.bound_range_case(d, link)
    assert c["counts"] == BR.shape_counts(d) + [E.split_count(d)] and c["kl_weight"] != 1.0
    for kind in E.KINDS:
        mean, prec = E.edge_priors(3, d, kind)
        m, lam = mean[0].numpy(), prec[0].numpy()
        for n_iters, reset in BR.GPU_ITERS:
            worst = 0.0
            for k, n in enumerate(c["counts"]):
                r = BP.case_rounds_prior(c, k, n_iters, reset, m, lam)
                cond = float(r["cond"].max())
                worst = max(worst, cond)
                assert E.bound_tight(d, n_iters, cond, r["theta"][-1]), (kind, n_iters, reset, n, cond)
                assert cond <= E.bound_cond_cap(d, n_iters)
                th, s = E.bound_rounds_mistaken(c, k, n_iters, reset, m, lam, None)
                ok, w = E.bound_criterion(d, n_iters, r, th.astype(np.float32), s.astype(np.float32))
                assert ok and w <= 0.5, (kind, n_iters, reset, n, w)
                if kind in E.MIXED:
                    for mistake in E.MISTAKES:
                        th2, s2 = E.bound_rounds_mistaken(c, k, n_iters, reset, m, lam, mistake)
                        bad, v = E.bound_criterion(d, n_iters, r, th2.astype(np.float32), s2.astype(np.float32))
                        assert not bad, (kind, n_iters, reset, n, mistake, v)
            print(f"BCOND d={d} {link} {kind} n_iters={n_iters} reset={int(reset)}: cond_max {worst:.3e} (cap "
                  f"{E.bound_cond_cap(d, n_iters):.3e})")


# ---------------------------------------------------------------------------------------------------------------------
# 4. the width cases under their drawn priors
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("name", ["width", "largest_dual"])
def test_width_cases_stay_under_the_parents_cap(name, link):
    c = (R.width_case if name == "width" else R.largest_dual_case)(link)
    mean, prec = E.width_priors(c, name)
    f = c["field"]
    assert float(prec.min()) >= E.WIDTH_PREC_LO[name]
    cond = E.case_conds_prior(c, mean[f].numpy(), prec[f].numpy())
    print(f"WCOND {name} {link} prec_lo {E.WIDTH_PREC_LO[name]}: " + " ".join(f"n={n}:{v:.1f}" for n, v in zip(c["counts"], cond)))
    assert max(cond) <= E.WIDTH_COND


def test_past_cap_and_bitwise_cases_stay_under_the_parents_cap():
    c = R.past_cap_case()
    mean, prec = E.width_priors(c, "past_cap")
    cond = E.case_conds_prior(c, mean[0].numpy(), prec[0].numpy())
    c2 = R.bitwise_case()
    mean, prec = E.edge_priors(3, R.BITWISE_D, E.BITWISE_KIND)
    picks = R.bitwise_sample(len(c2["counts"]))
    cond2 = E.case_conds_prior(c2, mean[0].numpy(), prec[0].numpy(), picks)
    print(f"WCOND past_cap {max(cond):.1f}; bitwise under {E.BITWISE_KIND} (16 entities) {max(cond2):.3e}")
    assert len(cond) == R.SLABS + 5 and max(cond) <= E.WIDTH_COND and max(cond2) <= E.WIDTH_COND


@pytest.mark.parametrize("link", LINKS)
def test_bound_wide_case(link):
    c = E.bound_wide_case(link)
    assert c["counts"] == [R.FB - 1, R.FB + 1, 300, 301] and {R.storage(n, 300) for n in c["counts"]} == {"slab"}
    mean, prec = E.width_priors(c, "bound_wide")
    for k, n in enumerate(c["counts"]):
        r = BP.case_rounds_prior(c, k, 2, True, mean[1], prec[1])
        print(f"WCOND bound_wide {link} n={n}: cond_max {float(r['cond'].max()):.1f}")
        assert float(r["cond"].max()) <= 1e3


# ---------------------------------------------------------------------------------------------------------------------
# 5 / 6. the session cases
# ---------------------------------------------------------------------------------------------------------------------
def _respondents(c):
    return torch.unique(c["pool"][:, c["field"]]).tolist()


def _two_orders(c, e):
    o = E.pool_order(c, e)
    return [o, o[::-1]]


def _exact_fold_discriminates(c, x, y, e, criterion, mixed):
    """One fold of an exact or design session: the restatement rounded to fp32 passes `criterion` at <= 0.5 and (mixed)
    each planted mistake fails it."""
    m, lam = E.session_prior(c)
    a = E._args(E.session_view(c, x, y, e), 0)
    th, s = E.restatement_fp64_prior(*a, m, lam)
    ok, w = criterion(th.astype(np.float32), s.astype(np.float32))
    assert ok and w <= 0.5, (e, x.shape[0], w)
    if mixed:
        for mistake in E.MISTAKES:
            th2, s2 = E.restatement_fp64_prior(*a, m, lam, mistake)
            bad, v = criterion(th2.astype(np.float32), s2.astype(np.float32))
            assert not bad, (e, x.shape[0], mistake, v)


def _bound_session_discriminates(c, e, order, reset, mixed, tight):
    """The folds of a bound session of respondent e along `order`: cond by `tight` or COND_BOUND, the correct rounds
    rounded to fp32 at <= 0.5, each mistake planted in a fold (started where the reference stands) fails."""
    m, lam = E.session_prior(c)
    start = E.session_start(c, e, reset)
    worst = 0.0
    for q in range(c["Q"]):
        x, y = EC.rows_of(c, e, order[:q + 1])
        r = EC.bound_fold(c, x, y, e, start)
        cond = float(r["cond"].max())
        worst = max(worst, cond)
        if tight:
            assert E.bound_tight(c["d"], c["n_iters"], cond, r["theta"][-1]), (e, q, cond)
        else:
            assert cond <= EC.COND_BOUND, (e, q, cond)
        if mixed is not None:
            v = E.session_view(c, x, y, e)
            th, s = E.bound_rounds_mistaken(v, 0, c["n_iters"], False, m, lam, None, start=start)
            ok, w = E.bound_criterion(c["d"], c["n_iters"], r, th.astype(np.float32), s.astype(np.float32))
            assert ok and w <= 0.5, (e, q, w)
            for mistake in (E.MISTAKES if mixed else ()):
                th2, s2 = E.bound_rounds_mistaken(v, 0, c["n_iters"], False, m, lam, mistake, start=start)
                bad, w2 = E.bound_criterion(c["d"], c["n_iters"], r, th2.astype(np.float32), s2.astype(np.float32))
                assert not bad, (e, q, mistake, w2)
        # (the next fold reads the fp32 row)
        t32, s32 = r["theta"][-1].astype(np.float32), r["s"][-1].astype(np.float32)
        start = EC.start_of_row(c, t32[:1], t32[1:], s32[:1], s32[1:])
    return worst


@pytest.mark.parametrize("name", E.SESSION_NAMES)
@pytest.mark.parametrize("d", E.WIDE_DS)
def test_wide_session_cases(d, name):
    import itertools
    c = E.session_case(name, d)
    H, Q = c["H"], c["Q"]
    assert int((c["hist_x"][:, 0] == c["long"]).sum()) == H and c["pool"].shape[0] == 4 * Q
    systems = R.session_systems(d, H, Q)
    if d == R.LDS:                                           # the crossing from LDS to the slab mid-session
        assert [st for _, st in systems] == ["lds", "lds", "slab", "slab"] and systems[1][0] == R.LDS
    elif d == 129:                                           # (the primal system of 130 fits LDS: nothing crosses at this d)
        assert systems == [(130, "lds")] * 4 and H == R.LDS - 3
    else:
        assert [sz for sz, _ in systems] == [d - 1, d, d + 1]                 # dual, the largest dual, primal
    worst = 0.0
    for e in _respondents(c):
        if name == "bound":
            orders = EC.orders(c, e) if Q == 3 else _two_orders(c, e)
            for order in orders:
                for reset in (True, False):
                    worst = max(worst, _bound_session_discriminates(c, e, list(order), reset, None, False))
        else:                                                # the matrix depends on the set of rows asked, not their order
            idx = E.pool_order(c, e)
            for k in range(1, Q + 1):
                for sub in itertools.combinations(idx, k):
                    x, y = EC.rows_of(c, e, list(sub))
                    m, lam = E.session_prior(c)
                    cond = P.cond_of_the_factored_prior(*E._args(E.session_view(c, x, y, e), 0), m, lam)
                    worst = max(worst, cond)
                    assert cond <= EC.COND_EXACT, (e, sub, cond)
    print(f"SCOND wide {name} d={d}: systems {systems}, cond_max {worst:.1f}")
    # part 6: under a mixed prior, along the pool order
    cm = E.session_case(name, d, "mixed0")
    for e in _respondents(cm):
        order = E.pool_order(cm, e)
        if name == "bound":                                  # (the criterion carries each fold's own cond; no cap under mixed)
            _bound_mixed_wide(cm, e)
            continue
        for q in range(Q):
            x, y = EC.rows_of(cm, e, order[:q + 1])
            rt, rs, cond, n = E.session_reference_fp64(cm, x, y)
            _exact_fold_discriminates(cm, x, y, e, lambda t, s: E.wide_criterion(d, rt, rs, cond, n, t, s), True)


def _bound_mixed_wide(c, e):
    m, lam = E.session_prior(c)
    start = E.session_start(c, e, True)
    order = E.pool_order(c, e)
    for q in range(c["Q"]):
        x, y = EC.rows_of(c, e, order[:q + 1])
        r = EC.bound_fold(c, x, y, e, start)
        v = E.session_view(c, x, y, e)
        th, s = E.bound_rounds_mistaken(v, 0, c["n_iters"], False, m, lam, None, start=start)
        ok, w = E.bound_criterion(c["d"], c["n_iters"], r, th.astype(np.float32), s.astype(np.float32))
        assert ok and w <= 0.5, (e, q, w)
        for mistake in E.MISTAKES:
            th2, s2 = E.bound_rounds_mistaken(v, 0, c["n_iters"], False, m, lam, mistake, start=start)
            assert not E.bound_criterion(c["d"], c["n_iters"], r, th2.astype(np.float32), s2.astype(np.float32))[0], (e, q, mistake)
        t32, s32 = r["theta"][-1].astype(np.float32), r["s"][-1].astype(np.float32)
        start = EC.start_of_row(c, t32[:1], t32[1:], s32[:1], s32[1:])


@pytest.mark.parametrize("kind", E.RANGE_KINDS)
@pytest.mark.parametrize("name", E.SESSION_NAMES)
def test_range_session_cases(name, kind):
    c = E.session_case(name, E.RANGE_D, kind)
    assert c["Q"] == E.RANGE_Q and [sz for sz, _ in R.session_systems(8, c["H"], 3)] == [7, 8, 9] and c["klw"] != 1.0
    mixed = kind in E.MIXED
    worst = 0.0
    for e in _respondents(c):
        if name == "bound":
            for order in EC.orders(c, e):
                worst = max(worst, _bound_session_discriminates(c, e, list(order), True, None, True))
            _bound_session_discriminates(c, e, E.pool_order(c, e), True, mixed, True)
            continue
        for order in _two_orders(c, e):
            for q in range(c["Q"]):
                x, y = EC.rows_of(c, e, order[:q + 1])
                r = E.session_reference_mp(c, x, y, e)
                worst = max(worst, r["ref"]["cond"])
                v = E.session_view(c, x, y, e)
                m, lam = E.session_prior(c)
                L = E.reference_objective(v, 0, r["ref"]["theta"], r["ref"]["s"], m, lam)
                assert abs(L) >= 1.0, (e, q, L)

                def criterion(t, s, r=r):
                    ok, w_t, w_s = E.exact_criterion(r, t, s)
                    return ok, max(w_t, w_s)

                _exact_fold_discriminates(c, x, y, e, criterion, mixed)
    print(f"SCOND range {name} {kind}: cond_max {worst:.3e}")

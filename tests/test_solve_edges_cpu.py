"""CPU: the references and the input conditions of tests/test_gpu_solve_edges.py (solve_body at its own edges).

  - optimum_mp (mpmath, 50 digits) agrees with test_foldin_exact_cpu.solve_fp64 in both forms to 1e-10;
  - elementwise_ok rejects planted wrong answers that the suite's rel_err <= 1e-4 accepts: one small coordinate 4 fp32
    ulps off, a duplicated row counted once, D_0 taken with the A sum of coordinate 1, the scales from SA instead of SB;
  - the row counts of every GPU case, derived from the constants parsed out of include/vfm_foldin.h and
    vfm_foldin_body.hpp, hit the edges they are named after, and move when the constants do;
  - the well-conditioned cases have cond <= 1e3 of the matrix the kernel factors (cond(K) for a dual entity);
  - the conditioning cases have cond(K) in [1e6, 1e8] and a reference that stays within the cap by itself:
    2^-23 + 8 e_ref / max|ref| <= 1e-6, e_ref = max |dual_fp64_in_kernel_order - optimum_mp|.

Printed per conditioning case: YARDSTICK e_ref / (eps64 cond(K) max|ref|) -- 0.18 to 2.3 for the entities with n >= 2 on
the committed seeds.  At n = 1, K is 1 x 1 (cond(K) = 1) and e_ref is still 2e-11 to 3e-10: D^-1 b and D^-1 U^T z are each
about prec / kl_weight times their difference, a cancellation of the Woodbury form that cond(K) does not show."""
import os
import shutil

import numpy as np
import pytest
import torch

import solve_reference as R
from golden_util import rel_err
from test_foldin_exact_cpu import _problem, solve_fp64


# ---------------------------------------------------------------------------------------------------------------------
# the references
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("link", ["abs", "softplus"])
@pytest.mark.parametrize("F,d", [(2, 3), (3, 3), (2, 12), (3, 12)])
def test_optimum_mp_agrees_with_solve_fp64(F, d, link):
    ent, bia, scal, x, y, field = _problem(F, d, 20 + F + d)
    ent, bia, scal, y = ent.float(), bia.float(), scal.float(), y.float()      # the tables a kernel would read
    klw = R.f32(0.7)
    sols = {form: solve_fp64(ent, bia, scal, x, y, field, link, klw, form=form) for form in ("primal", "dual")}
    seen = set()
    for i, e in enumerate(sols["primal"]["entities"].tolist()):
        ref = R.optimum_mp(ent, bia, scal, x, y, field, link, klw, e)
        seen.add("dual" if ref["n"] <= d else "primal")
        for form, sol in sols.items():
            th = np.concatenate([[float(sol["mu_w"][i])], sol["mu"][i].numpy()])
            s = np.concatenate([[float(sol["s_w"][i])], sol["s"][i].numpy()])
            assert rel_err(th, ref["theta"]) <= 1e-10, (form, e)
            assert rel_err(s, ref["s"]) <= 1e-10, (form, e)
        assert abs(ref["cond_H"] - float(sols["primal"]["cond"][i])) <= 1e-6 * ref["cond_H"]
        assert (ref["cond_K"] is None) == (ref["n"] > d)
        if ref["n"] <= d:                                    # the restatement of the kernel's dual path, same optimum
            assert rel_err(R.dual_fp64_in_kernel_order(ent, bia, scal, x, y, field, link, klw, e), ref["theta"]) <= 1e-10
    assert seen == ({"primal"} if d == 3 else {"dual"})


def test_elementwise_ok_is_the_stated_bound():
    ref = np.array([1.0, -2.0, 1e-3, 0.0])
    ok, worst = R.elementwise_ok(ref.astype(np.float32), ref, 0.0)
    assert ok and worst <= 0.5                               # a rounding to nearest is half the bound at most
    ok, worst = R.elementwise_ok(np.float32(1.0) + np.float32(2.0 ** -23), np.array(1.0), 0.0)
    assert ok and worst == 1.0                              # exactly at the bound
    assert not R.elementwise_ok(np.float32(1.0) + np.float32(2.0 ** -22), np.array(1.0), 0.0)[0]
    assert R.elementwise_ok(np.float32(1.0) + np.float32(2.0 ** -22), np.array(1.0), 2.0 ** -23)[0]
    assert not R.elementwise_ok(np.float32(1e-30), np.array(0.0), 0.0)[0]      # a zero of the reference is a zero
    assert not R.elementwise_ok(np.float32("nan"), np.array(1.0), 1.0)[0]
    assert R.solve_abs_term(512, 1e3, np.array([-2.0, 1.0])) == 4 * 513 * 2.0 ** -52 * 1e3 * 2.0
    assert R.solve_abs_term(512, 1e3, np.ones(1)) <= 5e-10


# ---------------------------------------------------------------------------------------------------------------------
# the reference rejects wrong answers that rel_err <= 1e-4 accepts
# ---------------------------------------------------------------------------------------------------------------------
def _optimum_np(c, entity, variant=None):
    """(theta, s, cond, n) of one entity in numpy fp64, or the same with one planted mistake."""
    X, y = c["X"], c["y"]
    if variant == "duplicates_counted_once":
        sel = (X[:, c["field"]] == entity).numpy()
        _, first = np.unique(X.numpy()[sel], axis=0, return_index=True)
        keep = np.sort(np.nonzero(sel)[0][first])
        assert keep.size == sel.sum() - 1                   # (the case has exactly one repeated row)
        X, y = X[keep], y[keep]
    s = R.system64(c["ent"], c["bia"], c["scal"], X, y, c["field"], c["link"], c["kl_weight"], entity)
    n, d, prec, kl, D = s["n"], s["d"], s["prec"], s["kl"], s["D"].copy()
    if variant == "d0_with_the_a_sum_of_coordinate_1":
        D[0] = D[1]
    U = np.concatenate([np.ones((n, 1)), s["M"]], 1)
    H = np.diag(D) + prec * (U.T @ U)
    theta = np.linalg.solve(H, s["b"])
    SB = (s["D"] - kl) / prec if variant == "scales_from_sa" else s["SB"]
    sg = np.sqrt(kl / (kl + prec * SB))
    return theta, (sg if c["link"] == "abs" else np.log(np.expm1(sg))), float(np.linalg.cond(H)), n


def _heavy_case():
    """One entity of 40,000 distinct rows and one repeated row, d = 3, the partners' scales 3e-3: one row in 40,000 and
    A = 2e-5 beside n move the optimum by less than 1e-4 and by much more than an fp32 rounding."""
    n = 40_000
    sizes = (1, 300, 300)
    ent, bia, scal = R.tables(sizes, 3, seed=3)
    ent[:, 3:] = 3e-3
    g = torch.Generator().manual_seed(4)
    pick = torch.randperm(300 * 300, generator=g)[:n - 1]
    X = torch.stack([torch.zeros(n - 1, dtype=torch.int64), 1 + pick // 300, 301 + pick % 300], 1)
    X = torch.cat([X, X[:1]])
    y = torch.randn(n, generator=g) + 3.0
    return dict(sizes=sizes, field=0, d=3, link="abs", kl_weight=1.0, ent=ent, bia=bia, scal=scal, X=X, y=y)


def _small_case(kl_weight):
    c = R.case((6, 40, 30), 0, 12, "abs", [9, 20], seed=13, kl_weight=kl_weight)
    return c, int(c["ids"][1])


PLANTED = {  # mistake: (case, entity)
    "duplicates_counted_once": lambda: (_heavy_case(), 0),
    "d0_with_the_a_sum_of_coordinate_1": lambda: (_heavy_case(), 0),
    # (a prior 1e6 times the default: sigma = 1 - 1e-5, so SA for SB moves it by about 1e-5)
    "scales_from_sa": lambda: _small_case(1e6),
}


@pytest.mark.parametrize("mistake", list(PLANTED) + ["one_small_coordinate_4_ulps_off"])
def test_elementwise_ok_rejects_what_rel_err_accepts(mistake):
    if mistake == "one_small_coordinate_4_ulps_off":
        c, e = _small_case(1.0)
        theta, s, cond, n = _optimum_np(c, e)
        wrong_t, wrong_s = theta.astype(np.float32), s.astype(np.float32)
        i = int(np.argmin(np.abs(theta)))
        assert 0 < abs(theta[i]) < 0.2 * np.abs(theta).max()
        for _ in range(4):
            wrong_t[i] = np.nextafter(wrong_t[i], np.float32(np.inf))
    else:
        c, e = PLANTED[mistake]()
        theta, s, cond, n = _optimum_np(c, e)
        wrong_t, wrong_s = (v.astype(np.float32) for v in _optimum_np(c, e, mistake)[:2])
    assert cond <= 1e3
    ta, sa = R.solve_abs_term(c["d"], cond, theta), R.scale_abs_term(n, s)
    # the correct answer rounded to fp32 passes both metrics
    assert R.elementwise_ok(theta.astype(np.float32), theta, ta)[0] and R.elementwise_ok(s.astype(np.float32), s, sa)[0]
    old = max(rel_err(wrong_t, theta), rel_err(wrong_s, s))
    ok_t, worst_t = R.elementwise_ok(wrong_t, theta, ta)
    ok_s, worst_s = R.elementwise_ok(wrong_s, s, sa)
    print(f"PLANTED {mistake}: rel_err {old:.2e} (accepted at 1e-4); elementwise worst ratio theta {worst_t:.1f} "
          f"scales {worst_s:.1f} (rejected above 1)")
    assert old <= 1e-4
    assert not (ok_t and ok_s)


# ---------------------------------------------------------------------------------------------------------------------
# the cases of the GPU tests: their row counts are the edges, and move with the constants
# ---------------------------------------------------------------------------------------------------------------------
def test_constants_are_the_librarys():
    from vae_amd import _lib
    assert (R.LDS, R.SLABS) == (_lib.FOLDIN_SOLVE_LDS_DIM, _lib.FOLDIN_SOLVE_SLABS)
    assert R.FB % 64 == 0


def test_row_counts_hit_the_named_edges():
    L, S, B = R.LDS, R.SLABS, R.FB
    # 3.1: both storages in one launch, the block exactly filled (m + 1 = FB rows with the right-hand side), the
    # right-hand side wrapping to thread 0 (m = FB), two rows per thread, the last dual and the first primal
    d = 300
    w = R.width_counts(d)
    assert w == [1, L - 1, L, L + 1, B - 1, B, B + 1, d - 1, d, d + 1]
    assert L + 1 < B - 1 and B + 1 < d - 1                   # (distinct edges at this d)
    assert [R.storage(n, d) for n in w] == ["lds"] * 3 + ["slab"] * 7
    assert [R.solve_dim(n, d) for n in w] == w[:-1] + [d + 1]
    assert R.width_case("abs")["X"].shape[0] == sum(w) and 1800 <= sum(w) <= 2400
    d = 512
    assert R.largest_dual_counts(d) == [B + 1, 511, 512, 513]
    assert [R.solve_dim(n, d) for n in R.largest_dual_counts(d)] == [B + 1, 511, 512, 513]
    assert R.tri(512) == 131_328 or B != 256                 # (the pairs of phase B at the largest dual)
    # 3.2: the rule d + 1 > cap_dim flips between these two d
    lo, hi = R.slab_rule_ds()
    assert hi == lo + 1 and not R.has_slabs(lo) and R.has_slabs(hi)
    assert all(R.storage(n, lo) == "lds" for n in R.slab_rule_counts(lo))
    assert [R.storage(n, hi) for n in R.slab_rule_counts(hi)] == ["lds", "lds", "slab", "slab"]
    pc = R.past_cap_counts(hi)
    assert len(pc) == S + 5 and len(set(pc)) == 5
    for b in range(5):                                       # block b: entities b and SLABS + b, of different storages
        assert R.storage(pc[b], hi) != R.storage(pc[S + b], hi), b
    # 3.3
    bc = R.bitwise_counts()
    assert len(bc) == 2 * S + 37 and sorted(set(bc)) == list(range(1, 13))
    assert {R.solve_dim(n, R.BITWISE_D) for n in bc} == {1, 2, 3, 4, 5, 6}
    assert {R.storage(n, R.BITWISE_D, 3) for n in bc} == {"lds", "slab"} and R.has_slabs(R.BITWISE_D, 3)
    assert not R.has_slabs(R.BITWISE_D, -1) and {R.storage(n, R.BITWISE_D, 0) for n in bc} == {"slab"}
    mixed = [R.storage(bc[g], R.BITWISE_D, 3) for g in (0, S, 2 * S)]          # block 0's three trips
    assert mixed == ["lds", "slab", "slab"] or len(set(mixed)) == 2
    picks = R.bitwise_sample(len(bc))
    assert len(picks) == 16 and {0, S, 2 * S} <= set(picks)
    # 3.4
    sc = R.session_cases()
    assert sc == [(200, L - 2, 5), (300, B - 2, 4), (L - 1, L - 3, 4), (L, L - 2, 4)]
    assert R.session_systems(*sc[0]) == [(L - 1, "lds"), (L, "lds"), (L + 1, "slab"), (L + 2, "slab"), (L + 3, "slab")]
    assert [m for m, _ in R.session_systems(*sc[1])] == [B - 1, B, B + 1, B + 2]
    assert R.session_systems(*sc[2]) == [(L - 2, "lds"), (L - 1, "lds"), (L, "lds"), (L, "lds")]     # dual, dual, primal
    assert R.session_systems(*sc[3]) == [(L - 1, "lds"), (L, "lds"), (L + 1, "slab"), (L + 1, "slab")]
    # 3.5
    assert [R.kcond_counts(d) for d in R.KCOND_DS] == [[1, 4, 8, 9], [1, 32, 64, 65]]


def test_the_issues_literal_edges_at_todays_constants():
    if (R.LDS, R.SLABS, R.FB) != (135, 256, 256):
        pytest.skip("the constants moved: test_row_counts_hit_the_named_edges checks the derived lists")
    assert R.width_counts(300) == [1, 134, 135, 136, 255, 256, 257, 299, 300, 301]
    assert R.slab_rule_ds() == (134, 135)
    assert len(R.bitwise_counts()) == 549
    assert R.session_cases() == [(200, 133, 5), (300, 254, 4), (134, 132, 4), (135, 133, 4)]


def test_the_cases_move_with_the_constants(tmp_path):
    """VFM_FOLDIN_SOLVE_LDS_DIM changed in a scratch copy of the two files: the derived lists follow."""
    for rel in ("include/vfm_foldin.h", "vae_amd/csrc_rank/vfm_foldin_body.hpp"):
        os.makedirs(tmp_path / os.path.dirname(rel), exist_ok=True)
        shutil.copy(os.path.join(R.ROOT, rel), tmp_path / rel)
    hdr = tmp_path / "include" / "vfm_foldin.h"
    hdr.write_text(hdr.read_text().replace(f"VFM_FOLDIN_SOLVE_LDS_DIM {R.LDS}", "VFM_FOLDIN_SOLVE_LDS_DIM 100")
                   .replace(f"VFM_FOLDIN_SOLVE_SLABS {R.SLABS}", "VFM_FOLDIN_SOLVE_SLABS 64"))
    body = tmp_path / "vae_amd" / "csrc_rank" / "vfm_foldin_body.hpp"
    body.write_text(body.read_text().replace(f"constexpr int FB = {R.FB};", "constexpr int FB = 128;"))
    lds, slabs, fb = R.read_solver_constants(str(tmp_path))
    assert (lds, slabs, fb) == (100, 64, 128)
    assert R.width_counts(300, lds, fb) == [1, 99, 100, 101, 127, 128, 129, 299, 300, 301]
    assert R.slab_rule_ds(lds) == (99, 100)
    assert len(R.bitwise_counts(slabs)) == 165
    assert R.session_cases(lds, fb)[0] == (200, 98, 5)
    pc = R.past_cap_counts(100, slabs, lds)
    assert len(pc) == 69 and all(R.storage(pc[b], 100, lds=lds) != R.storage(pc[64 + b], 100, lds=lds) for b in range(5))


# ---------------------------------------------------------------------------------------------------------------------
# the conditions on the inputs
# ---------------------------------------------------------------------------------------------------------------------
WELL = [("width", R.width_case, None), ("largest_dual", R.largest_dual_case, None),
        ("slab_rule_lo", lambda link: R.slab_rule_case(R.slab_rule_ds()[0], link), None),
        ("slab_rule_hi", lambda link: R.slab_rule_case(R.slab_rule_ds()[1], link), None)]


@pytest.mark.parametrize("link", ["abs", "softplus"])
@pytest.mark.parametrize("name,build,which", WELL, ids=[w[0] for w in WELL])
def test_well_conditioned_cases(name, build, which, link):
    c = build(link)
    assert torch.unique(c["X"][:, c["field"]]).tolist() == c["ids"].tolist()
    assert [int((c["X"][:, c["field"]] == e).sum()) for e in c["ids"]] == c["counts"]
    cond = R.case_conds(c, which)
    print(f"COND {name} {link}: " + " ".join(f"n={n}:{v:.1f}" for n, v in zip(c["counts"], cond)))
    assert max(cond) <= 1e3, cond


def test_well_conditioned_past_the_caps():
    c = R.past_cap_case()
    cond = R.case_conds(c)
    assert len(cond) == R.SLABS + 5 and max(cond) <= 1e3, max(cond)
    c = R.bitwise_case()
    picks = R.bitwise_sample(len(c["counts"]))
    cond = R.case_conds(c, picks)
    print(f"COND past_cap / bitwise: {max(R.case_conds(R.past_cap_case(), range(5))):.1f} {max(cond):.1f}")
    assert max(cond) <= 1e3, cond


@pytest.mark.parametrize("link", ["abs", "softplus"])
@pytest.mark.parametrize("d", R.KCOND_DS)
def test_conditioning_cases(d, link):
    c, refs = R.kcond_references(d, link)
    prec = float(R._link64(c["scal"].numpy()[0], link))
    assert 49.0 <= prec <= 51.0 and c["kl_weight"] == R.f32(1e-4)
    sig = R._link64(c["ent"][:, d:].numpy(), link)
    assert 0.99e-3 <= sig.min() <= 2e-3 and 1.5 <= sig.max() <= 2.01          # the partners' scales span 1e-3 .. 2
    X = c["X"]
    half = X[X[:, 0] == int(c["ids"][1])]
    assert bool((torch.unique(half, dim=0, return_counts=True)[1] % 2 == 0).all())     # every other row a duplicate
    for r in refs:
        ref, n = r["ref"], r["n"]
        top = float(np.abs(ref["theta"]).max())
        if n > d:                                            # the primal control: bounded with cond(H), whatever it is
            assert ref["cond_K"] is None and np.isfinite(ref["cond_H"])
            print(f"YARDSTICK d={d} {link} n={n} primal control: cond(H) {ref['cond_H']:.3e}")
            continue
        yard = r["e_ref"] / (R.EPS64 * ref["cond_K"] * top)
        print(f"YARDSTICK d={d} {link} n={n}: cond(H) {ref['cond_H']:.3e} cond(K) {ref['cond_K']:.3e} e_ref "
              f"{r['e_ref']:.3e} max|ref| {top:.3e} e_ref / (eps64 cond(K) max|ref|) {yard:.3f}")
        if n >= 2:                                           # (n = 1: K is 1 x 1, its condition number is 1)
            assert 1e6 <= ref["cond_K"] <= 1e8, ref["cond_K"]
        else:
            assert ref["cond_K"] == 1.0
        assert R.EPS32 + 8.0 * r["e_ref"] / top <= 1e-6      # the reference alone stays within the cap

"""CPU: the references and the input conditions of tests/test_gpu_implicit_edges.py (the implicit solves at their own
edges; the cases come from tests/implicit_edges.py).

  - implicit_edges.reference (the partner field built once) gives what implicit_reference, implicit_prior_reference and
    implicit_weights_reference give, for every form, at d = 9;
  - every case meets the conditions under which its GPU test means something -- the trips of the coordinate loops and of
    the tile walk, the slab rule, the calls that pass the slab grid cap, the chunk counts past the 2^20 cap, cond(H) --
    each an expression in the constants parsed from the sources;
  - for every case the fp64 reference rounded to fp32 and passed through the GPU tests' own comparison has a worst ratio
    <= 0.5: a case whose reference does not pass its own bound is wrong;
  - the conditioning cases: cond(H) in [1e5, 1e7] and the torch fp64 solve agrees with the mpmath optimum to well inside
    the bound (printed: IMPEDGE-CPU cond).

Printed on the committed seeds, IMPEDGE-CPU cond d link form n: cond(H) 1.3e5 .. 5.9e5; |fp64 - mpmath| is 5e-12 ..
8e-10, at most 6e-3 of the fp64 term of the bound (the assertion asks for 5e-2)."""
import numpy as np
import pytest
import torch

import implicit_edges as IE
import implicit_reference as IR
import solve_reference as R

LINKS = list(IE.LINKS)
FORMS = list(IE.FORMS)


def _tab(c):
    return c["ent"], c["bia"], c["scal"]


def _rounded_passes(c, form, ids, what, field=None, cond_range=(0.0, 1e3)):
    """The reference of the entities ids rounded to fp32 through compare(): the worst ratio must be <= 0.5."""
    sol, _ = IE.reference(form, _tab(c), c, ids, field)
    worst, bad = IE.compare(c, sol, *IE.rounded(sol, c["link"]), field, cond_range)
    print(f"IMPEDGE-CPU {what} {c['link']} d={c['d']} {form}: rounded reference worst ratio {worst:.3f}, worst cond "
          f"{float(sol['cond'].max()):.3g}")
    assert not bad and worst <= 0.5, (what, worst, bad)
    return sol


def _counts_of(c):
    f = c["field"]
    lo = 0 if f == 0 else c["N"]
    n = c["N"] if f == 0 else c["M"]
    return torch.bincount(c["x"][:, f] - lo, minlength=n).tolist()


# ---------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("link,field", [("abs", 0), ("softplus", 1)])
def test_batched_reference_is_the_existing_one(link, field, form):
    c = IE.sign_case(link, field)
    assert c["d"] == 9
    ids = IE.folded_ids(c)
    a, loss_a = IE.reference(form, _tab(c), c, ids)
    b, loss_b = IE.existing_reference(form, _tab(c), c, ids)
    for k in ("theta", "sigma", "cond"):
        assert torch.allclose(a[k], b[k], rtol=1e-12, atol=1e-14), k
    for i in (0, 3, len(ids) - 2):
        e = int(ids[i])
        la, lb = loss_a(e, a["theta"][i], a["sigma"][i]), loss_b(e, a["theta"][i], a["sigma"][i])
        assert abs(la - lb) <= 1e-12 * abs(lb), (e, la, lb)
    # the forms are four problems: neither the prior nor the weights drop out
    plain, _ = IE.reference("plain", _tab(c), c, ids)
    if form != "plain":
        assert not torch.allclose(a["theta"], plain["theta"], rtol=1e-3)


def test_constants():
    from vae_amd import _lib
    assert (IE.LDS, IE.SLABS) == (_lib.FOLDIN_SOLVE_LDS_DIM, _lib.FOLDIN_SOLVE_SLABS)
    assert IE.GRID_CAP == 1 << 20 and IE.FB % 64 == 0
    assert IE.W0 == R.f32(IE.W0) and IE.KLW == R.f32(IE.KLW) and IE.W1 == R.f32(IE.W1) and IE.COND_KL == R.f32(1e-4)
    w = IE.width_case(300, "abs")["w"]
    assert w.dtype == torch.float32 and float(w.min()) == IE.W0 and float(w.max()) <= IE.RATIO * IE.W0


# ---------------------------------------------------------------------------------------------------------------------
# 1. width
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("d", IE.WIDTH_DS)
def test_width_cases(d, link, form):
    c = IE.width_case(d, link)
    counts = IE.width_counts(d)
    assert _counts_of(c) == counts and c["M"] == IE.width_partners(d) and max(counts) <= c["M"]
    assert d + 1 > IE.FB and IE.trips(d + 1) >= 2                           # the coordinate loops take another trip
    assert R.has_slabs(d)
    assert IE.tiles(d) > IE.FB and IE.trips(IE.tiles(d)) >= 2              # a thread owns more than one tile
    if IE.FB == 256:                                                        # (at today's FB: 3 trips and 33 tiles at d = 512)
        assert (IE.trips(d + 1), IE.trips(IE.tiles(d))) == ((3, 33) if d == 512 else (2, 12))
    assert IE.trips(R.tri(d + 1)) > 1                                       # ... and phase B more than one element
    thr = IE.threshold(IE.width_split(d), d)
    forms = ["chunks" if n > thr else "rows" for n in counts]
    assert forms == ["rows"] * 5 + ["chunks"] and counts[4] == d + 2 > d + 1
    assert counts[2] < IE.FB < counts[3]
    _rounded_passes(c, form, IE.folded_ids(c), "width")


# ---------------------------------------------------------------------------------------------------------------------
# 2. the slab rule past its grid cap
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_past_cap_case(form):
    c = IE.past_cap_case()
    S = IE.SLABS
    counts = _counts_of(c)
    assert counts == IE.past_cap_counts() and c["d"] == IE.LDS and c["link"] == "abs" and c["M"] == 48
    assert R.has_slabs(c["d"]) and not R.has_slabs(c["d"] - 1)
    seen = [g for g, n in enumerate(counts) if n]
    assert seen == list(range(5)) + list(range(S, S + 5))
    empty = len(counts) - len(seen)
    assert empty == S + 5 > S                                # the empty call: blocks 0 .. 4 solve twice
    assert max(counts) <= IE.threshold(0, c["d"])            # (no entity can be split: the catalog is below d + 1)
    ids = seen + [5, S + 5, len(counts) - 1]
    _rounded_passes(c, form, ids, "past_cap")


# ---------------------------------------------------------------------------------------------------------------------
# 3. past the slab grid cap, bitwise
# ---------------------------------------------------------------------------------------------------------------------
def test_bitwise_case():
    c = IE.bitwise_case()
    S, d = IE.SLABS, IE.BITWISE_D
    counts = _counts_of(c)
    assert counts == IE.bitwise_counts() and c["link"] == "softplus" and c["M"] == IE.BITWISE_PARTNERS
    light, heavy, empty = IE.bitwise_calls(counts)
    assert len(light) == 2 * S + 37 and len(heavy) == 2 * S + 1 and len(empty) == S + 5
    assert sorted({counts[g] for g in light}) == list(range(1, 12))
    assert [counts[heavy[k * S]] for k in range(3)] == list(IE.BITWISE_HEAVY)  # block 0's three trips of the chunk call
    assert min(counts[g] for g in heavy) > IE.threshold(IE.BITWISE_SPLIT, d) and max(counts) <= c["M"]
    assert IE.BITWISE_LDS_DIMS == (-1, 0, 3) and not R.has_slabs(d, -1)
    for ld in (0, 3):
        assert R.has_slabs(d, ld)
        for call in (light, heavy, empty):
            assert len(call) > S                             # every call loops
        assert len(light) > 2 * S and len(heavy) > 2 * S     # ... block 0 of these two three times
    picks = IE.bitwise_sample(c)
    assert len(picks) == 16 and {light[0], light[S], light[2 * S], heavy[0], heavy[S], heavy[2 * S], empty[0],
                                 empty[S]} <= set(picks)
    for form in FORMS:
        _rounded_passes(c, form, picks, "bitwise")
    # the raw entry: bad ids in the second trip of blocks 0 and 1, the third trip behind them
    assert 2 * S + 3 <= len(light)
    p, y, w, ptr = IE.row_lists(c, light[:2 * S + 3])
    assert ptr.tolist() == np.concatenate([[0], np.cumsum([counts[g] for g in light[:2 * S + 3]])]).tolist()
    assert p.numel() == y.numel() == w.numel() == int(ptr[-1]) and int(p.min()) >= c["N"]


# ---------------------------------------------------------------------------------------------------------------------
# 4. the 2^20 caps
# ---------------------------------------------------------------------------------------------------------------------
def test_cap_case():
    c = IE.cap_case()
    n, E, k = IE.cap_partners(), IE.CAP_ENTITIES, IE.cap_rows_per_entity()
    assert c["d"] == 1 and c["link"] == "abs" and c["M"] == n == IE.GRID_CAP + 3
    assert n > IE.GRID_CAP                                   # k_implicit_base at chunk_rows = 1: a chunk per id
    assert E * k == c["x"].shape[0] > IE.GRID_CAP            # k_implicit_chunks: a chunk per row
    assert _counts_of(c) == [k] * E
    key = c["x"][:, 0] * (c["N"] + c["M"]) + c["x"][:, 1]
    assert torch.unique(key).numel() == key.numel()          # distinct pairs
    assert int(c["x"][:, 1].min()) >= E and int(c["x"][:, 1].max()) < E + n
    ids = IE.folded_ids(c)
    for form in IE.CAP_FORMS:
        _rounded_passes(c, form, ids, "cap")
    base, mag = IE.base_fp64(c)
    assert base.shape == (10,) and base[0] == n and base[5] == n and base[3] == 0.0
    # against implicit_reference's partners: the triangle, sum A, sum (A + M^2), sum t u, sum q
    _, u, A, cm, cv = IR._partners(*_tab(c), 0, c["N"], c["M"], "abs")
    ref = torch.cat([(u.T @ u)[torch.tril_indices(2, 2)[0], torch.tril_indices(2, 2)[1]], A.sum(0),
                     torch.tensor([float(n)]), (A + u * u).sum(0)[1:], -(cm[:, None] * u).sum(0),
                     (cm * cm + cv).sum().reshape(1)]).numpy()
    assert np.all(np.abs(base - ref) <= 4 * n * R.EPS64 * mag)


# ---------------------------------------------------------------------------------------------------------------------
# 5. conditioning
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", IE.COND_FORMS)
@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("d", IE.COND_DS)
def test_conditioning_cases(d, link, form):
    c, sol = IE.cond_references(d, link, form)
    N, n = c["N"], c["M"]
    assert c["klw"] == IE.COND_KL and _counts_of(c) == IE.cond_counts(d)
    thr = IE.threshold(IE.cond_split(d), d)
    assert [k > thr for k in IE.cond_counts(d)] == [False, False, False, True]
    sig = R._link64(np.concatenate([c["ent"][N:N + n, d:].numpy(), c["bia"][N:N + n, 1:].numpy()], 1), link)
    assert 4e-4 <= sig.min() and sig.max() <= 3e-3           # sigma about 1e-3
    raw = c["ent"][N:N + n, d:]
    assert (bool((raw < 0).any()) and bool((raw > 0).any())) if link == "abs" else (-7 <= float(raw.min()) and float(raw.max()) <= -6)
    sv = torch.linalg.svdvals(c["ent"][N:N + n, :d].double())
    assert float(sv[d // 2 - 1]) > 30 * float(sv[d // 2])    # the means sit near a subspace of rank d / 2
    lo, hi = IE.COND_RANGE
    assert lo <= float(sol["cond"].min()) and float(sol["cond"].max()) <= hi, sol["cond"]
    # the fp64 term of the bound stays within about ten fp32 ulps at the ceiling
    assert 4 * (d + 1) * R.EPS64 * hi <= 10 * R.EPS32
    # torch fp64 against mpmath: well inside the bound
    for i, e in enumerate(sol["ids"].tolist()):
        rt = sol["theta"][i].numpy()
        term = R.solve_abs_term(d, float(sol["cond"][i]), rt)
        err = float(np.abs(sol["fp64"][i].numpy() - rt).max())
        bound = float((R.EPS32 * np.abs(rt) + term).min())
        print(f"IMPEDGE-CPU cond d={d} {link} {form} n={c['counts'][i]}: cond(H) {float(sol['cond'][i]):.3e} "
              f"|fp64 - mpmath| {err:.2e} fp64 term {term:.2e} smallest bound {bound:.2e}")
        assert err <= 0.05 * term and err <= 0.05 * bound, (e, err, term, bound)
        es = float(np.abs(IR.inv_link_t(sol["fp64_sigma"][i], link).numpy() - sol["s"][i].numpy()).max())
        assert es <= 0.05 * R.scale_abs_term(2 * n, sol["s"][i].numpy())
    worst, bad = IE.compare(c, sol, *IE.rounded(sol, link), None, IE.COND_RANGE)
    print(f"IMPEDGE-CPU cond d={d} {link} {form}: rounded reference worst ratio {worst:.3f}")
    assert not bad and worst <= 0.5


# ---------------------------------------------------------------------------------------------------------------------
# 6. signed and small raw scales
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("field", [0, 1])
def test_signed_scales_case(field, form):
    c = IE.sign_case("abs", field)
    f = IE.flipped(c)
    d = c["d"]
    for a, b in ((c["ent"][:, d:], f["ent"][:, d:]), (c["bia"][:, 1], f["bia"][:, 1])):
        assert torch.equal(a.abs(), b.abs()) and int((a != b).sum()) == a.numel() // 2 and bool((b < 0).any())
    assert torch.equal(c["ent"][:, :d], f["ent"][:, :d]) and torch.equal(c["bia"][:, 0], f["bia"][:, 0])
    assert float(f["scal"][0]) == -float(c["scal"][0]) < 0 and float(f["scal"][2]) == -float(c["scal"][2]) < 0
    assert float(f["scal"][1]) == float(c["scal"][1])
    ids = IE.folded_ids(c)
    a = _rounded_passes(f, form, ids, "signed")
    b, _ = IE.reference(form, _tab(c), c, ids)
    assert torch.equal(a["theta"], b["theta"]) and torch.equal(a["sigma"], b["sigma"])     # |s| alone enters
    # a closed form with s where it needs |s| is far outside the bound: the precision's sign flips the whole solve
    wrong = dict(f, link="softplus")                         # (any link that is not even in s)
    w, _ = IE.reference(form, _tab(wrong), wrong, ids)
    assert not torch.allclose(w["theta"], b["theta"], rtol=1e-2)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("field", [0, 1])
def test_small_scales_case(field, form):
    c = IE.small_scale_case(field)
    d = c["d"]
    lo, hi = IE.SOFTPLUS_RAW_RANGE
    raw = torch.cat([c["ent"][:, d:].reshape(-1), c["bia"][:, 1]])
    assert lo <= float(raw.min()) < lo + 0.1 and hi - 0.1 < float(raw.max()) <= hi and float(c["scal"][2]) == IE.SOFTPLUS_S0
    assert _counts_of(c)[:len(c["counts"])] == IE.sign_counts()
    _rounded_passes(c, form, IE.folded_ids(c), "small")

"""GPU: the implicit-feedback solves (vae_amd/csrc_rank/vfm_implicit.hip: k_implicit_base, k_implicit_base_sum,
k_implicit_chunks, k_implicit_solve in its four forms -- plain, prior, weights, prior with weights) at their own edges.
The cases and their references come from tests/implicit_edges.py, every edge an expression in the constants parsed from
the sources (LDS, SLABS, FB, the 2^20 grid cap); tests/test_implicit_edges_cpu.py checks the conditions on the inputs
and that every reference rounded to fp32 passes its own bound at a ratio <= 0.5.

  1. width: d = 300 and d = 512 (the coordinate loops take 2 and 3 trips, a thread walks 12 and 33 tiles, the slabs are
     up to 1 MB), both links, the four forms, entities of 0, 1, FB - 1, FB + 1, d + 2 rows and one in chunk form
  2. the slab rule past its grid cap at d = LDS: the call of the SLABS + 5 entities without rows, blocks 0 .. 4 solve
     twice; every entity against fp64, the entities without rows equal bit for bit
  3. past the slab grid cap through lds_dim at d = 5: the light, the heavy-group and the empty call each of more than
     SLABS entities, lds_dim -1 / 0 / 3 bit for bit, block 0's three entities of the light and of the chunk-form call
     alone bit for bit, 16 entities against fp64; the raw entry with bad ids in the second trip of blocks 0 and 1
  4. the 2^20 grid caps of k_implicit_base and k_implicit_chunks: 2^20 + 3 partners at chunk_rows = 1, 64 entities of
     16,385 rows, a row per chunk
  5. conditioning: cond(H) 1.3e5 .. 5.9e5 against mpmath at 50 digits
  6. signed raw scales under abs (bit for bit the unsigned tables) and raw scales in [-8, 3] under softplus

Bounds.  Rows written by a solve: per element |got - ref| <= 2^-23 |ref| + 4 (d + 1) 2^-52 cond(H) max|ref|
(implicit_edges.compare: solve_reference.elementwise_ok / solve_abs_term), the raw scales with scale_abs_term over
2 n_dense, after asserting cond(H) <= 1e3 on the reference's matrix -- in 5. after asserting cond(H) in [1e5, 1e7]
instead, the same bound with the case's own cond(H).  Losses: 1e-5 relative against the row-by-row fp64 loss at the
written rows.  The base block: 4 n 2^-52 relative to the sum of the absolute terms of each element.

Two of the cases as they were first drawn up could not meet their own conditions, and are built to meet them: with
SLABS + 5 entities of which ten have rows the empty call of 2. has SLABS - 5 entities, so it has SLABS + 15 here (and
its catalog of 48 is below d + 1, so no entity of it can be split: the chunk form at a slab d is in 1.); one population
of 2 SLABS + 37 entities with three heavy ones gives 3. a heavy call of 3 and an empty call of 46 entities, so each of
the three calls has a run of ids of its own here (implicit_edges.bitwise_counts).

Measured on an MI355X, worst elementwise ratio per case (the printed IMPEDGE lines; 1 = at the bound, the reference
itself rounded to fp32 gives at most 0.5), plain / prior / weights / prior with weights:
  width d = 300   abs 0.484 / 0.497 / 0.485 / 0.493   softplus 0.491 / 0.478 / 0.496 / 0.490   cond(H) <= 6.5
  width d = 512   abs 0.497 / 0.496 / 0.489 / 0.496   softplus 0.475 / 0.488 / 0.479 / 0.495   cond(H) <= 7.4
  past_cap d = 135 (271 entities)   0.487 / 0.490 / 0.478 / 0.493   cond(H) <= 17.2
  bitwise d = 5 (16 of 1323 entities)   0.463 / 0.440 / 0.495 / 0.470; the third trip behind the bad ids 0.335 / 0.438 /
  0.411 / 0.331
  cap d = 1 (64 entities, 1,048,640 chunks)   plain 0.431, weights 0.465; the base block 3.1e-4 of its bound
  signed abs d = 9   field 0: 0.460 / 0.470 / 0.479 / 0.454   field 1: 0.480 / 0.468 / 0.491 / 0.484, bit for bit the
  unsigned tables (rows, losses, one sweep of fit_implicit and J_imp)
  small softplus d = 9   field 0: 0.488 / 0.454 / 0.488 / 0.451   field 1: 0.491 / 0.466 / 0.491 / 0.488
Losses 1.7e-8 .. 6.3e-8 relative in every case above against the 1e-5 bound.  The printed IMPEDGE cond lines (d link
form, n = 0 / 3 / d + 2 / chunk form: cond(H), kernel_error = max |got - ref| of the fp32 result, ratio):
  8 abs plain        1.5e5 / 1.7e5 / 2.2e5 / 3.2e5   7.4e-8 / 3.1e-7 / 4.6e-7 / 4.6e-7   0.30 / 0.35 / 0.33 / 0.35
  8 abs weights      1.5e5 / 1.8e5 / 2.2e5 / 3.2e5   7.4e-8 / 3.3e-7 / 4.7e-7 / 2.3e-7   0.30 / 0.33 / 0.26 / 0.21
  8 softplus plain   1.3e5 / 1.5e5 / 1.8e5 / 2.3e5   4.8e-8 / 1.5e-6 / 8.4e-7 / 2.7e-7   0.30 / 0.41 / 0.42 / 0.29
  8 softplus weights 1.3e5 / 1.5e5 / 1.7e5 / 2.2e5   4.8e-8 / 8.6e-7 / 4.7e-7 / 6.7e-7   0.30 / 0.34 / 0.28 / 0.40
  64 abs plain       2.6e5 / 2.9e5 / 5.3e5 / 5.6e5   1.7e-7 / 6.3e-7 / 9.4e-7 / 8.8e-7   0.28 / 0.28 / 0.32 / 0.18
  64 abs weights     2.6e5 / 2.9e5 / 5.7e5 / 5.9e5   1.7e-7 / 4.0e-7 / 1.3e-6 / 9.2e-7   0.28 / 0.27 / 0.26 / 0.26
  64 softplus plain  2.0e5 / 2.1e5 / 3.1e5 / 3.1e5   2.3e-7 / 2.1e-7 / 4.7e-7 / 9.3e-7   0.38 / 0.30 / 0.30 / 0.39
  64 softplus weights 2.0e5 / 2.0e5 / 3.3e5 / 3.3e5  2.3e-7 / 2.3e-7 / 9.0e-7 / 6.9e-7   0.38 / 0.35 / 0.32 / 0.33
  (worst ratio with the scales 0.38 .. 0.46; the loss taken from the system within 3.6e-8 .. 5.6e-8 of the row-by-row loss)
The kernels' error is fp32 rounding in every case: nothing here exposed a fault in the implicit solves."""
import numpy as np
import pytest
import torch

import implicit_edges as IE
import implicit_reference as IR
import solve_reference as R
from implicit_edges import CHUNK, KLW, W0, W1
from test_gpu_fit_implicit import _model_of, _rows_of

pytestmark = pytest.mark.gpu
DEV = "cuda"
LINKS = list(IE.LINKS)
FORMS = list(IE.FORMS)


def _priors_of(c):
    from vae_amd import sweep
    pr = sweep.GroupPriors(2, c["d"], DEV)
    pr.load_state_dict({"mean": c["prior"][0].float(), "prec": c["prior"][1].float()})
    return pr


def _form_kw(c, form):
    """What a call of `form` takes beside the rows: w1 or the weights, and the priors."""
    kw = {"weights": c["w"].to(DEV)} if "weights" in form else {"w1": W1}
    if "prior" in form:
        kw["priors"] = _priors_of(c)
    return kw


def _run(c, m, form, split_rows, lds_dim=-1, entities=None):
    """sweep.run_implicit of the case: (entities, loss, rows)."""
    from vae_amd import sweep
    kw = _form_kw(c, form)
    return sweep.run_implicit(m, c["x"].to(DEV), c["y"].to(DEV), c["field"], W0, kw.pop("w1", 1.0), c.get("klw", KLW),
                              entities=entities, split_rows=split_rows, chunk_rows=CHUNK, lds_dim=lds_dim,
                              priors=kw.get("priors"), weights=kw.get("weights"))


def _tables_cpu(tables):
    return tuple(t.detach().cpu().clone() for t in tables)


def _written(tables, ids):
    """(theta [E, d + 1] = (mu_w, mu), s [E, d + 1] = (s_w, s)) of the rows ids of the device tables, fp32 on the CPU."""
    d = tables[0].shape[1] // 2
    ent, bia = tables[0].detach()[ids.to(DEV)].cpu(), tables[1].detach()[ids.to(DEV)].cpu()
    return torch.cat([bia[:, :1], ent[:, :d]], 1), torch.cat([bia[:, 1:], ent[:, d:]], 1)


def _check(c, tab, tables, form, ids, loss, what, sol=None, cond_range=(0.0, 1e3)):
    """The rows ids of the device tables against the fp64 solve from the tables `tab` (or sol) per element, loss [len(ids)]
    against the row-by-row fp64 loss at the written rows.  Prints the IMPEDGE line; returns (worst ratio, worst loss
    error)."""
    ids = torch.as_tensor(ids, dtype=torch.int64)
    ref = IE.Reference(tab, c, form)
    sol = ref.solve(ids) if sol is None else sol
    theta, s = _written(tables, ids)
    worst, bad = IE.compare(c, sol, theta, s, None, cond_range)
    worst_l = 0.0
    loss = loss.detach().cpu()
    for i, e in enumerate(ids.tolist()):
        L = ref.loss(e, theta[i], IR.link_t(s[i], c["link"]))
        worst_l = max(worst_l, abs(float(loss[i]) - L) / abs(L))
    print(f"IMPEDGE {what} {c['link']} d={c['d']} {form}: worst ratio {worst:.3f}, loss rel_err {worst_l:.2e}, worst "
          f"cond {float(sol['cond'].max()):.3g}")
    assert not bad, (what, form, bad)
    assert worst_l <= 1e-5, (what, form, worst_l)
    return worst, worst_l


# ---------------------------------------------------------------------------------------------------------------------
# 1. width: d = 300 and d = 512
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("d", IE.WIDTH_DS)
def test_width(d, link, form):
    c = IE.width_case(d, link)
    assert d + 1 > IE.FB and R.has_slabs(d) and IE.tiles(d) > IE.FB
    m = _model_of(c)
    tables = m._views(m._flat)
    tab = _tables_cpu(tables)
    ents, loss, rows = _run(c, m, form, IE.width_split(d))              # one launch chain: light, the chunk group, empty
    assert rows.tolist() == IE.width_counts(d) and ents.tolist() == IE.folded_ids(c).tolist()
    _check(c, tab, tables, form, ents.cpu(), loss, "width")


# ---------------------------------------------------------------------------------------------------------------------
# 2. the slab rule past its grid cap, at a real slab d
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_the_slab_rule_past_its_grid_cap(form):
    c = IE.past_cap_case()
    S, d = IE.SLABS, c["d"]
    m = _model_of(c)
    tables = m._views(m._flat)
    tab = _tables_cpu(tables)
    start = m._flat.clone()
    ents, loss, rows = _run(c, m, form, d + 3)
    assert rows.tolist() == c["counts"] and R.has_slabs(d)
    empty = [g for g, n in enumerate(c["counts"]) if n == 0]
    assert len(empty) > S                                                # blocks 0 .. 4 of the empty call solve twice
    _check(c, tab, tables, form, ents.cpu(), loss, "past_cap")
    # the entities without rows solve one system: one loss and one row, bit for bit, whichever block and trip
    first = _rows_of(m, m._flat, empty[0])
    assert not torch.equal(first, _rows_of(m, start, empty[0]))
    for g in empty:
        assert torch.equal(loss[g], loss[empty[0]]), g
        assert torch.equal(_rows_of(m, m._flat, g), first), g


# ---------------------------------------------------------------------------------------------------------------------
# 3. past the slab grid cap, bitwise, through lds_dim
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_past_the_slab_grid_cap_bitwise(form):
    from vae_amd import sweep
    c = IE.bitwise_case()
    S, d, split = IE.SLABS, c["d"], IE.BITWISE_SPLIT
    light, heavy, empty = IE.bitwise_calls(c["counts"])
    m = _model_of(c)
    tables = m._views(m._flat)
    tab = _tables_cpu(tables)
    start = m._flat.clone()
    kw = _form_kw(c, form)
    x, y, _, _ = sweep.check_implicit_args(m, c["x"].to(DEV), c["y"].to(DEV), W0, kw.get("w1", 1.0), KLW, kw.get("weights"))
    runs = {}
    for ld in IE.BITWISE_LDS_DIMS:
        plan = sweep.ImplicitPlan(m, x, y, 0, None, split, CHUNK, sweep.MAX_WORKSPACE_BYTES, ld, kw.get("weights"))
        calls = [plan.obs.n_light] + [b - a for a, b, _, _ in plan.obs.groups] + [plan.empty.numel()]
        assert calls == [len(light), len(heavy), len(empty)]             # the three calls the plan makes
        if ld >= 0:
            assert R.has_slabs(d, ld) and min(calls) > S                 # ... each capped at SLABS blocks: each loops
        else:
            assert not R.has_slabs(d, ld)
        m._flat.copy_(start)
        ents, loss, rows = _run(c, m, form, split, ld)
        assert rows.tolist() == c["counts"]
        runs[ld] = (m._flat.clone(), loss.clone())
    first = runs[IE.BITWISE_LDS_DIMS[0]]
    assert bool(torch.isfinite(first[1]).all()) and not torch.equal(first[0], start)
    for ld in IE.BITWISE_LDS_DIMS[1:]:
        assert torch.equal(runs[ld][0], first[0]) and torch.equal(runs[ld][1], first[1]), ld
    # block 0's three entities of the light call (the row-list form) and of the heavy call (the chunk form), each alone
    for call in (light, heavy):
        for g in (call[0], call[S], call[2 * S]):
            for ld in (-1, 0):
                m._flat.copy_(start)
                ents, loss, rows = _run(c, m, form, split, ld, entities=[g])
                assert ents.tolist() == [g] and rows.tolist() == [c["counts"][g]]
                assert torch.equal(loss, first[1][g:g + 1]), (g, ld)
                assert torch.equal(_rows_of(m, m._flat, g), _rows_of(m, first[0], g)), (g, ld)
    m._flat.copy_(first[0])
    picks = IE.bitwise_sample(c)
    _check(c, tab, tables, form, picks, first[1][picks], "bitwise")


def _raw_solve(c, tables, form, base, ents, row_ptr, cptr, chunks, ys, partner, wts, lds_dim, klw=KLW):
    """One raw call of the form's op: loss [E] (7.0 where nothing is written)."""
    from vae_amd import _lib
    o = _lib.ops()
    d, N, M = c["d"], c["N"], c["M"]
    loss = torch.full((ents.numel(),), 7.0, device=DEV)
    n_chunks = 0 if chunks is None else chunks.shape[0]
    ws = torch.empty(max(o.implicit_solve_workspace_bytes(ents.numel(), n_chunks, d, lds_dim), 1), dtype=torch.uint8, device=DEV)
    a = (ents, row_ptr, cptr, chunks, ys, partner, base, *tables, ws, loss)
    flags = _lib._gen.VFM_FLAG_LINK_SOFTPLUS if c["link"] == "softplus" else 0
    opts = (N, M, flags, lds_dim, klw, W0)
    prior = _priors_of(c).row(0) if "prior" in form else None
    if "weights" in form:
        o.foldin_solve_implicit_weights(*a, prior, wts, *opts)
    elif form == "prior":
        o.foldin_solve_implicit_prior(*a, prior, *opts, W1)
    else:
        o.foldin_solve_implicit(*a, *opts, W1)
    torch.cuda.synchronize()
    return loss


def _base_of(c, tables, chunk_rows):
    from vae_amd import _lib
    o = _lib.ops()
    base = torch.empty(o.implicit_base_doubles(c["d"]), dtype=torch.float64, device=DEV)
    ws = torch.empty(o.implicit_base_workspace_bytes(c["M"], chunk_rows, c["d"]), dtype=torch.uint8, device=DEV)
    flags = _lib._gen.VFM_FLAG_LINK_SOFTPLUS if c["link"] == "softplus" else 0
    o.implicit_base(*tables, ws, base, c["N"], c["M"], chunk_rows, flags)
    torch.cuda.synchronize()
    return base


@pytest.mark.parametrize("form", FORMS)
def test_bad_ids_in_the_second_trip_of_the_raw_entry(form):
    """2 SLABS + 3 entities in one raw row-list call with lds_dim = 0 (slabs: the grid is SLABS), -1 at position SLABS
    and T at SLABS + 1: blocks 0 and 1 skip their second entity and still solve their third."""
    c = IE.bitwise_case()
    S, T = IE.SLABS, c["N"] + c["M"]
    good = IE.bitwise_calls(c["counts"])[0][:2 * S + 3]
    m = _model_of(c)
    tables = m._views(m._flat)
    tab = _tables_cpu(tables)
    start = m._flat.clone()
    base = _base_of(c, tables, CHUNK)
    assert R.has_slabs(c["d"], 0) and len(good) > 2 * S + 2

    def call(ids, ents):
        partner, ys, wts, ptr = (t.to(DEV) for t in IE.row_lists(c, ids))
        m._flat.copy_(start)
        loss = _raw_solve(c, tables, form, base, ents.to(DEV), ptr, None, None, ys, partner, wts, 0)
        return loss, m._flat.clone()

    ents = torch.tensor(good)
    ents[S], ents[S + 1] = -1, T
    loss, flat = call(good, ents)                                        # (the bad ids keep the rows of the ids they replace)
    rest = good[:S] + good[S + 2:]
    loss0, flat0 = call(rest, torch.tensor(rest))                        # the call without the two
    assert bool(torch.isnan(loss[S])) and bool(torch.isnan(loss[S + 1]))
    for g in (good[S], good[S + 1]):
        assert torch.equal(_rows_of(m, flat, g), _rows_of(m, start, g))  # nothing is written for them
    assert torch.equal(torch.cat([loss[:S], loss[S + 2:]]), loss0) and bool(torch.isfinite(loss0).all())
    assert torch.equal(flat, flat0) and not torch.equal(flat, start)
    third = [good[2 * S], good[2 * S + 1]]                               # the same blocks' third trip
    m._flat.copy_(flat)
    _check(c, tab, tables, form, third, loss[2 * S:2 * S + 2], "bad_ids")
    m._flat.copy_(start)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the 2^20 caps of the base and the chunk pass
# ---------------------------------------------------------------------------------------------------------------------
def test_the_grid_caps_of_the_base_and_the_chunk_pass():
    from vae_amd import sweep
    c = IE.cap_case()
    n, E, k = c["M"], c["N"], IE.cap_rows_per_entity()
    assert n > IE.GRID_CAP and E * k > IE.GRID_CAP                       # a chunk per id, a chunk per row: both past the cap
    tab = (c["ent"], c["bia"], c["scal"])
    tables = tuple(t.to(DEV).contiguous() for t in tab)
    start = tuple(t.clone() for t in tables)
    base = _base_of(c, tables, 1)
    ref, mag = IE.base_fp64(c)
    err = np.abs(base.cpu().numpy() - ref)
    bound = 4 * n * R.EPS64 * mag
    print(f"IMPEDGE cap base: worst |got - ref| / bound {float((err / np.where(bound > 0, bound, 1.0)).max()):.2e}")
    assert np.all(err <= bound), (err, bound)
    first = np.arange(E, dtype=np.int64) * k                             # (the rows are entity-major as drawn)
    assert c["x"][:, 0].tolist() == np.repeat(np.arange(E), k).tolist()
    cptr, chunks = sweep.chunk_table(first, np.full(E, k, np.int64), 1)
    assert chunks.shape[0] == E * k > IE.GRID_CAP
    cptr, chunks = torch.from_numpy(cptr).to(DEV), torch.from_numpy(np.ascontiguousarray(chunks)).to(DEV)
    partner, ys, wts = c["x"][:, 1].contiguous().to(DEV), c["y"].to(DEV), c["w"].to(DEV)
    ids = IE.folded_ids(c)
    for form in IE.CAP_FORMS:
        for t, s in zip(tables, start):
            t.copy_(s)
        loss = _raw_solve(c, tables, form, base, ids.to(DEV), None, cptr, chunks, ys, partner, wts, -1)
        _check(c, tab, tables, form, ids, loss, "cap")


# ---------------------------------------------------------------------------------------------------------------------
# 5. conditioning, against mpmath
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", IE.COND_FORMS)
@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("d", IE.COND_DS)
def test_conditioning(d, link, form):
    c, sol = IE.cond_references(d, link, form)
    lo, hi = IE.COND_RANGE
    assert lo <= float(sol["cond"].min()) and float(sol["cond"].max()) <= hi, sol["cond"]
    m = _model_of(c)
    tables = m._views(m._flat)
    tab = _tables_cpu(tables)
    ents, loss, rows = _run(c, m, form, IE.cond_split(d))
    assert rows.tolist() == IE.cond_counts(d) and bool(torch.isfinite(loss).all())
    theta, _ = _written(tables, ents.cpu())
    for i, n in enumerate(rows.tolist()):
        rt = sol["theta"][i].numpy()
        err = float(np.abs(theta[i].double().numpy() - rt).max())
        _, w = R.elementwise_ok(theta[i], rt, R.solve_abs_term(d, float(sol["cond"][i]), rt))
        print(f"IMPEDGE cond d={d} {link} {form} n={n}: cond(H) {float(sol['cond'][i]):.3e} kernel_error {err:.3e} "
              f"ratio {w:.3f}")
    _check(c, tab, tables, form, ents.cpu(), loss, "cond", sol=sol, cond_range=IE.COND_RANGE)


# ---------------------------------------------------------------------------------------------------------------------
# 6. signed and small raw scales
# ---------------------------------------------------------------------------------------------------------------------
def _brute_J(c, form, tab):
    import implicit_prior_reference as IPR
    import implicit_weights_reference as IWR
    a = (*tab, c["x"], c["y"])
    g = (c["N"], c["M"], c["link"])
    if "weights" in form:
        return float(IWR.brute_J(*a, c["w"], *g, W0, KLW, c["prior"] if "prior" in form else None))
    if form == "prior":
        return float(IPR.brute_J_prior(*a, *g, W0, W1, KLW, *c["prior"]))
    return float(IR.brute_J(*a, *g, W0, W1, KLW))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("field", [0, 1])
def test_signed_raw_scales_under_abs(field, form):
    c = IE.sign_case("abs", field)
    f = IE.flipped(c)
    X, y = c["x"].to(DEV), c["y"].to(DEV)
    res = {}
    for name, case in (("unsigned", c), ("signed", f)):
        m = _model_of(case)
        tables = m._views(m._flat)
        tab = _tables_cpu(tables)
        kw = _form_kw(case, form)
        J = m.implicit_objective(X, y, w0=W0, kl_weight=KLW, **kw)
        ref = _brute_J(case, form, tab)
        assert abs(J - ref) <= 1e-5 * abs(ref), (name, J, ref)
        start = m._flat.clone()
        ents, loss, rows = _run(case, m, form, 20)
        assert rows.tolist() == c["counts"] + [0]
        fold = (torch.stack([_rows_of(m, m._flat, int(e)) for e in ents]), loss.clone())
        if name == "signed":
            _check(case, tab, tables, form, ents.cpu(), loss, "signed")
        m._flat.copy_(start)
        fit = m.fit_implicit(X, y, 1, w0=W0, kl_weight=KLW, split_rows=20, chunk_rows=CHUNK, **kw)
        res[name] = (fold, m._flat.clone(), fit["objective"], J, start)
    a, b = res["unsigned"], res["signed"]
    assert not torch.equal(a[4], b[4])                                   # (the tables differ: the signs)
    assert torch.equal(a[0][0], b[0][0]) and torch.equal(a[0][1], b[0][1])     # the rows written and the losses
    assert torch.equal(a[1], b[1]) and a[2] == b[2]                      # one sweep: every parameter and J_imp
    assert a[3] == b[3]
    print(f"IMPEDGE signed abs d={c['d']} field={field} {form}: bit for bit the unsigned tables")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("field", [0, 1])
def test_small_and_negative_raw_scales_under_softplus(field, form):
    c = IE.small_scale_case(field)
    m = _model_of(c)
    tables = m._views(m._flat)
    tab = _tables_cpu(tables)
    ents, loss, rows = _run(c, m, form, 20)
    assert rows.tolist() == c["counts"] + [0]
    _check(c, tab, tables, form, ents.cpu(), loss, f"small field={field}")

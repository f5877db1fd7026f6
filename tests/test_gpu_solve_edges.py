"""GPU: solve_body (vae_amd/csrc_rank/vfm_foldin_solve_body.hpp) at its own edges, through k_foldin_solve
(VFM.fold_in_exact, vfm_foldin_solve_f32) and k_elicit_solve (VFM.elicit_field_exact).  The cases and their references
come from tests/solve_reference.py, every edge an expression in the constants parsed from the sources (LDS =
VFM_FOLDIN_SOLVE_LDS_DIM, SLABS = VFM_FOLDIN_SOLVE_SLABS, FB); tests/test_solve_edges_cpu.py checks the conditions on
the inputs.

  1. storage and width edges in one launch: d = 300, n in {1, LDS - 1, LDS, LDS + 1, FB - 1, FB, FB + 1, d - 1, d,
     d + 1}, and d = 512, n in {FB + 1, 511, 512, 513}; both links
  2. the slab rule between d = LDS - 1 and d = LDS: the workspace, n in {d - 1, d, d + 1, d + 40}, and SLABS + 5
     entities at d = LDS, where blocks 0-4 take a second entity of the other storage
  3. fold-in past the slab grid cap: 2 SLABS + 37 entities at d = 5, lds_dim -1 / 0 / 3 bit for bit, block 0's three
     entities alone bit for bit, 16 entities against fp64
  4. sessions whose system crosses LDS, FB and the dual / primal rule at the largest LDS system, bitwise against the
     composition
  5. the conditioning of the dual path (cond(K) 2e6 .. 3e7) against mpmath
  6. the guards of the raw entry

Bounds.  Well-conditioned cases (cond <= 1e3 of the matrix the kernel factors, asserted): per element
|got - ref| <= 2^-23 |ref| + 4 (d + 1) 2^-52 cond max|ref| against solve_fp64 (elementwise_ok, solve_abs_term); the
loss against objective_fp64 at the written rows at test_gpu_foldin_exact.py's 1e-5.  Conditioning cases, dual entities:
2^-23 |ref| + 8 e_ref against optimum_mp, e_ref the distance of the fp64 restatement of the dual path from optimum_mp.

Measured on an MI355X, worst elementwise ratio per case (1 = at the bound; the reference itself rounded to fp32 gives
at most 0.5) -- the printed EDGE lines: width d = 300 0.483 (abs) / 0.485 (softplus), d = 512 0.492 / 0.470; slab rule
d = 134 0.479 / 0.476, d = 135 0.467 / 0.465; past the grid cap at d = 135 0.497; the 16 entities of the bitwise case
0.441; losses 6e-8 .. 6e-7 against the 1e-5 bound; the loss of an empty range 0.0 under both links.  The printed KCOND
lines (d link n: cond(K), e_ref, kernel_error = max |got - ref| of the fp32 result, ratio):
  8 abs       1 / 4 / 8:    1 / 2.0e6 / 4.0e6   2.4e-11 / 6.7e-10 / 1.7e-9   4.2e-8 / 6.1e-8 / 9.5e-8   0.33 / 0.17 / 0.30
  8 softplus  1 / 4 / 8:    1 / 2.0e6 / 4.0e6   2.4e-10 / 1.3e-9 / 4.6e-10   5.0e-8 / 8.1e-8 / 8.3e-8   0.33 / 0.27 / 0.25
  64 abs      1 / 32 / 64:  1 / 1.6e7 / 3.2e7   3.0e-10 / 1.5e-8 / 2.8e-8    7.7e-8 / 3.0e-8 / 9.1e-8   0.31 / 0.07 / 0.16
  64 softplus 1 / 32 / 64:  1 / 1.6e7 / 3.2e7   4.2e-11 / 1.5e-8 / 1.0e-8    2.0e-8 / 1.0e-7 / 7.9e-8   0.36 / 0.23 / 0.20
  primal controls (n = d + 1, cond(H) about 10): 0.36, 0.30, 0.43, 0.44
The kernel's error is fp32 rounding in every case: nothing here exposed a fault in the solver."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import solve_reference as R
import test_gpu_foldin as G
from golden_util import rel_err
from test_foldin_cpu import objective_fp64
from test_foldin_exact_cpu import solve_fp64

pytestmark = pytest.mark.gpu
DEV = "cuda"
LINKS = ["abs", "softplus"]


def _model_of(c):
    """A model holding the tables of a solve_reference case."""
    from vae_amd.model import VFM
    torch.manual_seed(0)
    m = VFM(field_sizes=list(c["sizes"]), embedding_size=c["d"], output="reg", link=c["link"], device=DEV)
    m.entity_params.weight.data.copy_(c["ent"])
    m.bias_params.weight.data.copy_(c["bia"])
    m._flat[m._off_scal: m._off_scal + 3] = c["scal"].to(DEV)
    return m


def _written(m, ids):
    """(theta [E, d + 1] = (mu_w, mu), s [E, d + 1] = (s_w, s)) of the rows ids, fp32 on the CPU."""
    d = m.d
    ent = m.entity_params.weight.detach()[ids.to(DEV)].cpu()
    bia = m.bias_params.weight.detach()[ids.to(DEV)].cpu()
    return torch.cat([bia[:, :1], ent[:, :d]], 1), torch.cat([bia[:, 1:], ent[:, d:]], 1)


def _check(c, m, loss, what, which=None):
    """The written rows of the entities number `which` of case c (default: all) against solve_fp64 per element, the
    returned loss against objective_fp64 at the written rows.  Returns the worst elementwise ratio."""
    which = list(range(len(c["counts"]))) if which is None else list(which)
    ids = c["ids"][which]
    field, link, klw, d = c["field"], c["link"], c["kl_weight"], c["d"]
    sel = torch.isin(c["X"][:, field], ids)
    X, y = c["X"][sel], c["y"][sel]
    sol = solve_fp64(c["ent"], c["bia"], c["scal"], X, y, field, link, klw)
    assert torch.equal(sol["entities"], ids)
    cond = R.case_conds(c, which)
    assert max(cond) <= 1e3, cond                            # (the condition on the inputs, of K for a dual entity)
    theta, s = _written(m, ids)
    worst = 0.0
    for i, k in enumerate(which):
        n = c["counts"][k]
        rt = np.concatenate([[float(sol["mu_w"][i])], sol["mu"][i].numpy()])
        rs = np.concatenate([[float(sol["s_w"][i])], sol["s"][i].numpy()])
        ok_t, w_t = R.elementwise_ok(theta[i], rt, R.solve_abs_term(d, cond[i], rt))
        ok_s, w_s = R.elementwise_ok(s[i], rs, R.scale_abs_term(n, rs))
        if len(which) <= 16:
            print(f"EDGE {what} {link} d={d} n={n} {'dual' if n <= d else 'primal'} {R.storage(n, d)} cond "
                  f"{cond[i]:.1f}: worst ratio theta {w_t:.3f} scales {w_s:.3f}")
        assert ok_t and ok_s, (what, n, w_t, w_s)
        worst = max(worst, w_t, w_s)
    th = (ids, theta[:, 1:].double(), s[:, 1:].double(), theta[:, 0].double(), s[:, 0].double())
    L = objective_fp64(c["ent"], c["bia"], c["scal"], X, y.double(), field, th, link, "reg", "closed_form", None, klw)
    el = rel_err(loss.cpu()[which].numpy(), L.numpy())
    print(f"EDGE {what} {link} d={d}: worst ratio {worst:.3f}, loss rel_err {el:.2e}")
    assert el <= 1e-5, el
    return worst


def _fold(c, m, lds_dim=-1, X=None, y=None):
    from vae_amd import foldin
    X, y = (c["X"], c["y"]) if X is None else (X, y)
    return foldin.run_exact(m, X.to(DEV), y.to(DEV), c["field"], c["kl_weight"], lds_dim=lds_dim)


# ---------------------------------------------------------------------------------------------------------------------
# 1. storage and width edges in one launch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("build", [R.width_case, R.largest_dual_case], ids=["d300", "d512"])
def test_storage_and_width_edges_in_one_launch(build, link):
    c = build(link)
    m = _model_of(c)
    ents, loss, rows = _fold(c, m)
    assert torch.equal(ents.cpu(), c["ids"]) and rows.tolist() == c["counts"]
    assert {R.storage(n, c["d"]) for n in c["counts"]} == ({"lds", "slab"} if c["d"] == 300 else {"slab"})
    _check(c, m, loss, "width")


# ---------------------------------------------------------------------------------------------------------------------
# 2. the slab rule between d = LDS - 1 and d = LDS
# ---------------------------------------------------------------------------------------------------------------------
def test_the_slab_rule_in_the_workspace():
    from vae_amd import _lib
    wsb = _lib.load().vfm_foldin_solve_workspace_bytes
    lo, hi = R.slab_rule_ds()
    ru = lambda v: (v + 255) // 256 * 256
    for E in (3, R.SLABS, R.SLABS + 5):
        assert wsb(E, 40, lo, -1) == wsb(0, 40, lo, -1) > 0                    # no slab term
        assert wsb(E, 40, hi, -1) - wsb(0, 40, hi, -1) == min(E, R.SLABS) * ru(R.tri(hi + 1) * 8)


@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("side", ["lo", "hi"])
def test_the_slab_rule(side, link):
    d = R.slab_rule_ds()[side == "hi"]
    c = R.slab_rule_case(d, link)
    m = _model_of(c)
    ents, loss, rows = _fold(c, m)
    assert rows.tolist() == [d - 1, d, d + 1, d + 40]
    _check(c, m, loss, f"slab_rule_{side}")


def test_the_slab_rule_past_the_grid_cap():
    c = R.past_cap_case()
    m = _model_of(c)
    ents, loss, rows = _fold(c, m)
    assert ents.numel() == R.SLABS + 5 and rows.tolist() == c["counts"]
    for b in range(5):
        assert R.storage(c["counts"][b], c["d"]) != R.storage(c["counts"][R.SLABS + b], c["d"])
    _check(c, m, loss, "past_cap")


# ---------------------------------------------------------------------------------------------------------------------
# 3. fold-in past the slab grid cap, bitwise
# ---------------------------------------------------------------------------------------------------------------------
def test_past_the_slab_grid_cap_bitwise():
    c = R.bitwise_case()
    m = _model_of(c)
    start = m._flat.clone()
    E = len(c["counts"])
    runs = {}
    for ld in R.BITWISE_LDS_DIMS:
        m._flat.copy_(start)
        ents, loss, rows = _fold(c, m, ld)
        assert ents.numel() == E and rows.tolist() == c["counts"]
        runs[ld] = (m._flat.clone(), loss.clone())
    first = runs[R.BITWISE_LDS_DIMS[0]]
    assert bool(torch.isfinite(first[1]).all()) and not torch.equal(first[0], start)
    for ld in R.BITWISE_LDS_DIMS[1:]:
        assert torch.equal(runs[ld][0], first[0]) and torch.equal(runs[ld][1], first[1]), ld
    # block 0's three entities (one per trip of its loop when the grid is capped), each alone
    d, off = m.d, m._off_bias
    for g in (0, R.SLABS, 2 * R.SLABS):
        e = int(c["ids"][g])
        sel = c["X"][:, c["field"]] == e
        for ld in R.BITWISE_LDS_DIMS:
            m._flat.copy_(start)
            _, loss, rows = _fold(c, m, ld, c["X"][sel], c["y"][sel])
            assert rows.tolist() == [c["counts"][g]]
            assert torch.equal(loss, first[1][g:g + 1]), (g, ld)
            assert torch.equal(m._flat[e * 2 * d:(e + 1) * 2 * d], first[0][e * 2 * d:(e + 1) * 2 * d]), (g, ld)
            assert torch.equal(m._flat[off + 2 * e: off + 2 * e + 2], first[0][off + 2 * e: off + 2 * e + 2]), (g, ld)
    m._flat.copy_(first[0])
    _check(c, m, first[1], "bitwise", R.bitwise_sample(E))


# ---------------------------------------------------------------------------------------------------------------------
# 4. sessions across the same edges, bitwise against the composition
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.session_cases())))
def test_sessions_across_the_edges(i):
    from test_gpu_elicit_exact import A3, _against_the_composition
    from test_gpu_elicit_field import _problem
    d, n_hist, Q = R.session_cases()[i]
    m = G._model(A3, d, "reg", LINKS[i % 2], seed=d + 1, rng_seed=3)
    pool, y_pool, hx, hy = _problem(m, 0, 3, [Q + 3, 5, 3], [n_hist, 0, 3], seed=d)
    ents, counts = torch.unique(hx[:, 0], return_counts=True)
    assert int(counts.max()) == n_hist                       # the respondent whose system crosses the edge
    out = _against_the_composition(m, pool, y_pool, Q, 0, "variance", (hx, hy), False)
    u = int(torch.searchsorted(out["entities"], ents[counts.argmax()]))
    assert int((out["rows"][u] < 0).sum()) == 0             # every round folded: n ran from n_hist + 1 to n_hist + Q
    assert bool(torch.isfinite(out["loss"][u]).all())
    print(f"EDGE session d={d}: systems {R.session_systems(d, n_hist, Q)}")


# ---------------------------------------------------------------------------------------------------------------------
# 5. the conditioning of the dual path, against mpmath
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("d", R.KCOND_DS)
def test_conditioning_of_the_dual_path(d, link):
    c, refs = R.kcond_references(d, link)
    m = _model_of(c)
    ents, loss, rows = _fold(c, m)
    assert rows.tolist() == c["counts"] and bool(torch.isfinite(loss).all())
    theta, s = _written(m, c["ids"])
    bad = []
    for i, r in enumerate(refs):
        ref, n = r["ref"], r["n"]
        err = float(np.abs(theta[i].double().numpy() - ref["theta"]).max())
        if n <= d:
            ok, w = R.elementwise_ok(theta[i], ref["theta"], 8.0 * r["e_ref"])
            print(f"KCOND d={d} {link} n={n} dual: cond(K) {ref['cond_K']:.3e} e_ref {r['e_ref']:.3e} kernel_error "
                  f"{err:.3e} ratio {w:.3f}")
        else:
            ok, w = R.elementwise_ok(theta[i], ref["theta"], R.solve_abs_term(d, ref["cond_H"], ref["theta"]))
            print(f"KCOND d={d} {link} n={n} primal control: cond(H) {ref['cond_H']:.3e} kernel_error {err:.3e} "
                  f"ratio {w:.3f}")
        ok_s, w_s = R.elementwise_ok(s[i], ref["s"], R.scale_abs_term(n, ref["s"]))
        if not (ok and ok_s):
            bad.append((n, w, w_s))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------
# 6. the guards of the raw entry
# ---------------------------------------------------------------------------------------------------------------------
class _Raw:
    """vfm_foldin_solve_f32 on the row lists of a small case, field by field as test_raw_abi_rejects_before_launching
    fills the struct; every call starts from the same table and returns (rc, table, loss)."""

    def __init__(self, link):
        from vae_amd import _lib, foldin
        self._lib, self.lib = _lib, _lib.load()
        self.c = c = R.case((40, 30), 0, 5, link, [3, 9, 14, 6, 11, 8], seed=91)
        self.m = m = _model_of(c)
        self.start = m._flat.clone()
        xs, self.ys, self.ents, self.ptr, _ = foldin.row_lists(c["X"].to(DEV), c["y"].to(DEV), 0)
        self.op_x, self.row_op = foldin.partner_tuples(xs, 0)
        self.flags = _lib._gen.VFM_FLAG_LINK_SOFTPLUS if link == "softplus" else 0

    def __call__(self, ents, ptr, ys, op_x, row_op, **kw):
        _lib, lib, m = self._lib, self.lib, self.m
        m._flat.copy_(self.start)
        E, n_ops = ents.numel(), op_x.shape[0]
        args = dict(E=E, R=ys.numel(), T=m.T, n_ops=n_ops, F=2, d=m.d, col=0, objective=_lib.OBJ_CLOSED_FORM,
                    likelihood=_lib.LIK_NORMAL, flags=self.flags, lds_dim=-1, kl_weight=1.0)
        args.update(kw)
        need = lib.vfm_foldin_solve_workspace_bytes(max(args["E"], 1), max(args["n_ops"], 1), m.d, args["lds_dim"])
        ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
        loss = torch.full((max(E, 1),), -7.0, device=DEV)
        ent, bia, scal = m._views(m._flat)
        keep = [t.contiguous() for t in (ents, ptr, ys, op_x, row_op)]
        args.update(entities=keep[0].data_ptr(), row_ptr=keep[1].data_ptr(), y=keep[2].data_ptr(),
                    op_x=keep[3].data_ptr(), row_op=keep[4].data_ptr(), entity_params=ent.data_ptr(),
                    bias_params=bia.data_ptr(), scalars=scal.data_ptr(), out_loss=loss.data_ptr(),
                    workspace=ws.data_ptr(), workspace_bytes=need)
        p = _lib.FoldinSolve()
        for k, v in args.items():
            setattr(p, k, v)
        rc = lib.vfm_foldin_solve_f32(C.byref(p), C.c_void_p(_lib.raw_stream(torch.device(DEV))))
        torch.cuda.synchronize()
        self.untouched = bool((loss == -7.0).all()) and not bool(ws.any())     # (what a call that launches nothing leaves)
        return rc, m._flat.clone(), loss[:E].clone()

    def rows_of(self, flat, e):
        d, off = self.m.d, self.m._off_bias
        return flat[e * 2 * d:(e + 1) * 2 * d], flat[off + 2 * e: off + 2 * e + 2]


@functools.lru_cache(maxsize=None)
def _raw(link):
    r = _Raw(link)
    rc, flat, loss = r(r.ents, r.ptr, r.ys, r.op_x, r.row_op)
    assert rc == 0 and bool(torch.isfinite(loss).all()) and not torch.equal(flat, r.start)
    return r, flat, loss


@pytest.mark.parametrize("link", LINKS)
def test_guard_entity_ids_outside_the_table(link):
    """One entity id < 0 and one >= T, each with rows of its own: a NaN loss, nothing written, the others bit for bit."""
    r, flat0, loss0 = _raw(link)
    E, Rr = r.ents.numel(), r.ys.numel()
    ents = torch.cat([torch.tensor([-3], device=DEV), r.ents, torch.tensor([r.m.T + 2], device=DEV)])
    ys = torch.cat([r.ys[:2], r.ys, r.ys[:3]])
    row_op = torch.cat([r.row_op[:2], r.row_op, r.row_op[:3]])
    ptr = torch.cat([torch.tensor([0], device=DEV), r.ptr + 2, torch.tensor([Rr + 5], device=DEV)])
    rc, flat, loss = r(ents, ptr, ys, r.op_x, row_op)
    assert rc == 0
    assert bool(torch.isnan(loss[0])) and bool(torch.isnan(loss[-1]))
    assert torch.equal(loss[1:-1], loss0)
    assert torch.equal(flat, flat0)                          # the real entities as without the ghosts, nothing else


@pytest.mark.parametrize("link", LINKS)
def test_guard_partner_ids_outside_the_table(link):
    """One operand with a partner id >= T and one with a negative id, each on one row: exactly the two entities that own
    those rows come back NaN (table row, first-order mean and loss), the others bit for bit.  (s_w is written finite:
    sigma_w^2 = kl / (kl + prec n) has no partner in it.)"""
    r, flat0, loss0 = _raw(link)
    n_ops = r.op_x.shape[0]
    op_x = torch.cat([r.op_x, torch.tensor([[0, r.m.T + 5], [0, -2]], device=DEV)])
    row_op = r.row_op.clone()
    hit = (1, 4)
    row_op[int(r.ptr[1]) + 2] = n_ops
    row_op[int(r.ptr[4])] = n_ops + 1
    rc, flat, loss = r(r.ents, r.ptr, r.ys, op_x, row_op)
    assert rc == 0
    for g, e in enumerate(r.ents.tolist()):
        row, bias = r.rows_of(flat, e)
        if g in hit:
            assert bool(torch.isnan(row).all()) and bool(torch.isnan(bias[0])) and bool(torch.isnan(loss[g])), g
            assert bool(torch.isnan(bias[1])) or torch.equal(bias[1], r.rows_of(flat0, e)[1][1]), g
        else:
            row0, bias0 = r.rows_of(flat0, e)
            assert torch.equal(row, row0) and torch.equal(bias, bias0) and torch.equal(loss[g], loss0[g]), g
    changed = flat != flat0
    own = torch.zeros_like(changed)
    for g in hit:
        e = int(r.ents[g])
        own[e * 2 * r.m.d:(e + 1) * 2 * r.m.d] = True
        own[r.m._off_bias + 2 * e: r.m._off_bias + 2 * e + 2] = True
    assert not bool((changed & ~own).any())


@pytest.mark.parametrize("link", LINKS)
def test_guard_row_ptr_is_clamped_and_an_empty_range_gives_the_prior(link):
    """row_ptr[0] < 0 and row_ptr[E] > R change nothing; with a decreasing pair every entity is solved on its clamped
    range [min(max(ptr[g], 0), R), min(max(ptr[g + 1], that), R)): bit for bit what a launch of that entity alone on
    that range writes.  The empty range: mu = 0, s = link^-1(1), loss = 0."""
    r, flat0, loss0 = _raw(link)
    E, Rr, d = r.ents.numel(), r.ys.numel(), r.m.d
    ptr = r.ptr.clone()
    ptr[0], ptr[E] = -5, Rr + 7
    rc, flat, loss = r(r.ents, ptr, r.ys, r.op_x, r.row_op)
    assert rc == 0 and torch.equal(flat, flat0) and torch.equal(loss, loss0)
    ptr[3] = ptr[2] - 2                                      # entity 2: empty; entity 3: from two rows of entity 1 on
    rc, flat, loss = r(r.ents, ptr, r.ys, r.op_x, r.row_op)
    assert rc == 0
    for g, e in enumerate(r.ents.tolist()):
        lo = min(max(int(ptr[g]), 0), Rr)
        hi = min(max(int(ptr[g + 1]), lo), Rr)
        assert (hi - lo == 0) == (g == 2)
        rc1, flat1, loss1 = r(r.ents[g:g + 1], torch.tensor([lo, hi], device=DEV), r.ys, r.op_x, r.row_op)
        assert rc1 == 0
        for a, b in zip(r.rows_of(flat, e), r.rows_of(flat1, e)):
            assert torch.equal(a, b), g
        assert torch.equal(loss[g:g + 1], loss1), g
    assert not torch.equal(r.rows_of(flat, int(r.ents[3]))[0], r.rows_of(flat0, int(r.ents[3]))[0])
    row, bias = r.rows_of(flat, int(r.ents[2]))
    prior = 1.0 if link == "abs" else math.log(math.expm1(1.0))
    assert bool((row[:d] == 0).all()) and float(bias[0]) == 0.0
    assert R.elementwise_ok(torch.cat([row[d:], bias[1:]]).cpu(), np.full(d + 1, prior), 0.0)[0]
    # L_e of no rows at the prior: the d + 1 KL terms, each zero to a few fp32 roundings of sigma = 1
    print(f"EDGE empty range {link}: loss {float(loss[2]):.3e}")
    assert abs(float(loss[2])) <= (d + 1) * 4 * R.EPS32
    empty_loss = loss[2:3].clone()
    # no rows at all: every entity at the prior
    rc, flat, loss = r(r.ents, torch.zeros(E + 1, dtype=torch.int64, device=DEV), r.ys[:0], r.op_x, r.row_op[:0])
    assert rc == 0
    for e in r.ents.tolist():
        for a, b in zip(r.rows_of(flat, e), (row, bias)):
            assert torch.equal(a, b)
    assert torch.equal(loss, empty_loss.expand(E))


def test_guard_nothing_to_do_writes_nothing():
    """E = 0, with rows and without: 0, and neither the table nor the loss nor the workspace is written."""
    r, _, _ = _raw("abs")
    for kw in (dict(E=0), dict(E=0, R=0), dict(E=0, R=0, n_ops=0)):
        rc, flat, _ = r(r.ents[:0], r.ptr[:1], r.ys, r.op_x, r.row_op, **kw)
        assert rc == 0 and torch.equal(flat, r.start) and r.untouched, kw

"""GPU: one sweep over the compiled shape buckets of every kernel family at the wide and ragged embedding sizes the
public API accepts (training d <= 1024, fold-in d <= 512, ranking d <= 4096) -- each against the project's fp64
oracles.  Next to each d list: the instantiation each d selects, worked out from the host selection code named there."""
import dataclasses
import math

import numpy as np
import pytest
import torch

from golden_util import rel_err
from oracle import vfm_oracle as O
from test_gpu_shapes import _random_problem, _run_gpu, _check
from test_gpu_rank import _model as _rank_model, oracle as rank_oracle, check_ranking, _excluded_mask, _tables_np
from test_gpu_rank import _exclusions as _rank_exclusions
from test_gpu_rank_eval import check_against_oracle, draw_positives, _exclusions
from test_rank_cpu import closed_form

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ------------------------------------------------------------------------------------------------ training step
# vfm_abi.hip pick_shape -> k_fwd / k_bwd / k_heavy <LPE, CPL, VEC>: d % 4 == 0: C = d/4 chunks of 4, LPE = pow2 >= C
# (4..64), CPL = ceil(C/LPE) rounded up to 1, 2, 4; else VEC = 1: (8,1) to d = 8, (64,1) to 64, (64,4) to 256.
# vfm_fwd2.hip dispatch_fwd2 (F = 2, 20 <= d <= 512, d % 4 == 0) -> k_fwd2 <LPE = pow2 >= ceil(C/2), FULL = d == 8 LPE>.
# d -> (LPE, CPL, VEC), filled chunks of LPE*CPL | k_fwd2:
# 2:(8,1,1) | -   66:(64,4,1) | -   255:(64,4,1) | -
# 260:(64,2,4) 65/128 | <64,false>   300:(64,2,4) 75/128 | <64,false>   508:(64,2,4) 127/128 | <64,false>
# 516:(64,4,4) 129/256 (ceil(C/64) = 3 -> 4) | -   600:(64,4,4) 150/256 | -   768:(64,4,4) 192/256 (4th chunk empty) | -
# 1020:(64,4,4) 255/256 | -
WIDE_D = [2, 66, 255, 260, 300, 508, 516, 600, 768, 1020]


def _wide_case(d, output, id_dtype):
    B = 300 if d <= 256 else 96
    args = _random_problem([37, 29], d, B, output, seed=d)
    _check(*args[:6], args[6], output, id_dtype)


@pytest.mark.parametrize("id_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("output", ["reg", "class"])
@pytest.mark.parametrize("d", WIDE_D)
def test_table_eps_F2_wide_and_ragged(d, output, id_dtype):
    _wide_case(d, output, id_dtype)


@pytest.mark.parametrize("id_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("output", ["reg", "class"])
@pytest.mark.parametrize("d", [v for v in WIDE_D if v <= 512])
def test_table_eps_F2_wide_and_ragged_row_parallel_forward(d, output, id_dtype, monkeypatch):
    """The same sizes with k_fwd forced (VFM_FWD_KERNEL=1) where k_fwd2 would run."""
    monkeypatch.setenv("VFM_FWD_KERNEL", "1")
    _wide_case(d, output, id_dtype)


# Philox eps.  F = 2, S = 1: k_fwd2 (above); 300 -> <64,false>, 512 -> <64,true>.
# F = 3: vfm_fwdg.hip (use_fwdg: F != 2, 16 <= d <= 512, d % 4 == 0, Philox) -> k_fwdg <LPE = pow2 >= ceil(C/2), FULL>:
#   300 -> <64,false>, 512 -> <64,true>.
# F = 2, S = 2..4: vfm_fwd2m.hip, the same rule -> k_fwd2m <64,false> at 300.
# softplus link: the general kernels k_fwd / k_bwd: 300 -> (64,2,4), 1020 -> (64,4,4).
PHILOX_CASES = [  # F, d, S, link, output
    (2, 300, 1, "abs", "reg"), (2, 512, 1, "abs", "class"),
    (3, 300, 1, "abs", "class"), (3, 512, 1, "abs", "reg"),
    (2, 300, 2, "abs", "reg"), (2, 300, 4, "abs", "class"),
    (2, 300, 1, "softplus", "class"), (2, 1020, 1, "softplus", "reg"),
]


@pytest.mark.parametrize("F,d,S,link,output", PHILOX_CASES)
def test_philox_eps_wide_against_oracle(F, d, S, link, output):
    """Forward, loss and gradients with the kernels' own draws, the eps tables dumped by philox_eps fed to the oracle
    (as tests/fuzz_parity.py does)."""
    from vae_amd import ops
    dev = torch.device(DEV)
    spec, P, x, y, nb_occ, _, group_hi = _random_problem([23 + 5 * f for f in range(F)], d, 160, output, seed=d + F + S)
    spec = dataclasses.replace(spec, n_samples=S, link=link)
    ent, bia = torch.tensor(P["entity_params"], device=dev), torch.tensor(P["bias_params"], device=dev)
    scal = torch.tensor(np.concatenate([P["alpha"], P["global_bias_mean"], P["global_bias_scale"]]), device=dev)
    inv_occ = ops.inv_occ_from_counts(torch.tensor(nb_occ, device=dev))
    plan = ops.BatchPlan(spec, torch.tensor(x, device=dev), torch.tensor(y, device=dev), inv_occ)
    st = ops.elbo_forward(plan, ent, bia, scal, inv_occ, seed=77, step=5)
    loss3 = ops.elbo_finalize(st, scal)
    g_ent, g_bias, _ = ops.elbo_backward(plan, st, ent, bia, scal, inv_occ, torch.ones(1, device=dev))
    ee, eb, eg = (t.cpu().numpy() for t in ops.philox_eps(spec, seed=77, step=5, device=dev))
    r = O.rowwise_elbo(P, x, y.astype(np.float64), nb_occ, np.array(group_hi), np.array(spec.group_n), spec.nb_train,
                       eg, eb, ee, output, link=link)
    # the tolerances of test_randomised_configurations_against_oracle
    assert abs(loss3[0].item() - r["loss"]) / abs(r["loss"]) < 2e-5
    assert rel_err(st.pred.cpu().numpy(), r["pred"]) < 5e-5
    assert rel_err(g_ent.cpu().numpy(), r["g_entity_params"]) < 1e-4
    assert rel_err(g_bias.cpu().numpy(), r["g_bias_params"]) < 1e-4


# fused backward + Adam (k_bwd): 300 -> (64,2,4) 75/128 chunks, 1020 -> (64,4,4) 255/256; forward k_fwd2 <64,false>
# at (F = 2, 300), k_fwd elsewhere (table eps)
@pytest.mark.parametrize("F,d,output,id_dtype", [(2, 300, "reg", torch.int32), (2, 1020, "class", torch.int64),
                                                 (3, 300, "class", torch.int64), (3, 1020, "reg", torch.int32)])
def test_fused_backward_adam_wide_against_oracle(F, d, output, id_dtype):
    from vae_amd import ops
    dev = torch.device(DEV)
    spec, P, x, y, nb_occ, eps, group_hi = _random_problem([31 + 3 * f for f in range(F)], d, 120, output, seed=d + F)
    plan, _, _, _ = _run_gpu(spec, P, x, y, nb_occ, eps, id_dtype)
    r = O.rowwise_elbo(P, x, y.astype(np.float64), nb_occ, group_hi, spec.group_n, spec.nb_train,
                       eps[0], eps[1], eps[2], output)
    ent = torch.tensor(P["entity_params"], device=dev); bia = torch.tensor(P["bias_params"], device=dev)
    scal = torch.tensor(np.concatenate([P["alpha"], P["global_bias_mean"], P["global_bias_scale"]]), device=dev)
    inv_occ = ops.inv_occ_from_counts(torch.tensor(nb_occ, device=dev))
    e = (torch.tensor(eps[2], device=dev), torch.tensor(eps[1], device=dev), torch.tensor(eps[0], device=dev))
    mv = [(torch.zeros_like(ent), torch.zeros_like(bia), torch.zeros(3, device=dev)) for _ in range(2)]
    st = ops.elbo_forward(plan, ent, bia, scal, inv_occ, eps=e)
    l3 = torch.empty(3, device=dev)
    ops.elbo_backward_adam(plan, st, ent, bia, scal, inv_occ, mv[0], mv[1], 0.01, 1, loss_out=l3)
    pe = P["entity_params"].astype(np.float64).copy()
    O.adam_step(pe, r["g_entity_params"], np.zeros_like(pe), np.zeros_like(pe), 1, 0.01)
    assert rel_err(ent.cpu().numpy(), pe) < 1e-5
    assert abs(l3[0].item() - r["loss"]) / abs(r["loss"]) < 2e-5


# pick_shape refuses: 257 (d % 4 != 0 above 256), 1028 (C = 257: ceil(C/64) = 5 chunks per lane)
@pytest.mark.parametrize("d", [257, 1028])
def test_unsupported_embedding_sizes_are_refused(d):
    args = _random_problem([11, 13], d, 20, "reg", seed=d)
    with pytest.raises(RuntimeError, match="embedding size d not supported"):
        _run_gpu(*args[:6])


# ------------------------------------------------------------------------------------------------ objective variants
# vfm_variants.hip: d % 8 == 0 -> var_shape: D8 = d/8, LPE = pow2 >= D8 capped at 64, CPL = ceil(D8/LPE)
# (k_var_fwd8 / k_var_bwd8 <LPE, CPL>); d % 8 != 0 -> the scalar pair k_var_fwd / k_var_bwd.
# d -> shape: 264: (64,1) 33/64 lanes   512: (64,1) full   1024: (64,2) full   300: scalar
VARIANT_D = [264, 512, 1024, 300]


@pytest.mark.parametrize("objective", ["sampled", "closed_form"])
@pytest.mark.parametrize("d", VARIANT_D)
def test_variants_wide_shapes_vs_oracle(d, objective):
    """Both objectives, priors and values on and off, F in {1, 3}, against oracle.variant_elbo (fp64 autograd) with
    the tolerances of test_variants_vs_oracle."""
    from test_gpu_objectives import _random_problem as _var_problem
    from vae_amd import ops
    from vae_amd.variants import variant_forward, variant_backward, priors_len
    dev = torch.device(DEV)
    g = np.random.default_rng(d + (objective == "sampled"))
    for F in (1, 3):
        for use_pri, use_val in ((False, False), (True, True), (True, False), (False, True)):
            B = 40
            output = "reg" if objective == "closed_form" or use_pri == use_val else "class"
            sizes, T, x, y, nb_occ, P, hi, gn, spec = _var_problem(g, F, d, B, output)
            G = F
            pri_np = None
            if use_pri:
                pri_np = np.concatenate([[g.normal() * 0.3, g.uniform(0.6, 1.5) * g.choice([-1, 1])], 0.3 * g.standard_normal(G),
                                         g.uniform(0.6, 1.5, G), 0.3 * g.standard_normal(G * d),
                                         g.uniform(0.6, 1.5, G * d) * g.choice([-1, 1], G * d)]).astype(np.float32)
                assert pri_np.size == priors_len(G, d)
            vals = g.uniform(0.3, 2.0, (B, F)).astype(np.float32) if use_val else None
            ent, bia = torch.tensor(P["entity_params"], device=dev), torch.tensor(P["bias_params"], device=dev)
            scal = torch.tensor(np.concatenate([P["alpha"], P["global_bias_mean"], P["global_bias_scale"]]), device=dev)
            inv_occ = ops.inv_occ_from_counts(torch.tensor(nb_occ, device=dev))
            plan = ops.BatchPlan(spec, torch.tensor(x, device=dev), torch.tensor(y, device=dev), inv_occ)
            pri = torch.tensor(pri_np, device=dev) if use_pri else None
            v_t = torch.tensor(vals, device=dev) if use_val else None
            st = variant_forward(plan, objective, ent, bia, scal, inv_occ, priors=pri, values=v_t, seed=11, step=3)
            g_ent, g_bias, g_sc, g_pr = variant_backward(plan, st, ent, bia, scal, inv_occ, torch.ones(1, device=dev))
            ee, eb, eg = (t.cpu().numpy().astype(np.float64) for t in ops.philox_eps(spec, seed=11, step=3, device=dev))
            leaf = lambda a_: torch.tensor(np.asarray(a_, np.float64), requires_grad=True)
            Pt = {k: leaf(v) for k, v in P.items()}
            prt = None
            if use_pri:
                flat = leaf(pri_np)
                prt = {"global": (flat[0], flat[1]), "bias": (flat[2:2 + G], flat[2 + G:2 + 2 * G]),
                       "entity": (flat[2 + 2 * G:2 + 2 * G + G * d], flat[2 + 2 * G + G * d:])}
            r = O.variant_elbo(Pt, x, y, nb_occ, hi, gn, spec.nb_train, objective, priors=prt, values=vals,
                               eps=(eg, eb, ee), output=output)
            r["loss"].backward()
            cfg = dict(F=F, d=d, objective=objective, output=output, priors=use_pri, values=use_val)
            assert abs(st["loss3"][0].item() - r["loss"].item()) / abs(r["loss"].item()) < 1e-4, cfg
            assert rel_err(st["pred"].cpu().numpy(), r["pred"].detach().numpy()) < 2e-4, cfg
            tol = 0.2 if F == 1 and objective == "sampled" else 5e-4      # (F = 1 sampled: pure cancellation)
            assert rel_err(g_ent.cpu().numpy(), Pt["entity_params"].grad.numpy()) < tol, cfg
            assert rel_err(g_bias.cpu().numpy(), Pt["bias_params"].grad.numpy()) < 5e-4, cfg
            want_sc = np.array([0.0 if Pt[k].grad is None else Pt[k].grad.numpy()[0]
                                for k in ("alpha", "global_bias_mean", "global_bias_scale")])
            mag = np.abs(r["pred"].detach().numpy()).sum() * spec.nb_train / B + 1.0
            assert np.all(np.abs(g_sc.cpu().numpy() - want_sc) <= 5e-4 * np.abs(want_sc) + 2e-4 * mag), cfg
            if use_pri:
                assert rel_err(g_pr.cpu().numpy(), flat.grad.numpy()) < 1e-3, cfg


# ------------------------------------------------------------------------------------------------ fold-in
# vfm_foldin.hip shape_of: W = 8 / 16 / 32 / 64 lanes for d <= 8 / 16 / 32 / above, CPL = ceil(d/W) rounded up to
# 1, 2, 4, 8 -> k_foldin <W, CPL>; closed form: rows staged in LDS per entity, cap = 12288 / (256/W) / (W*CPL + 1).
# d -> (W, CPL) cap: 1:(8,1) 42   9:(16,1) 45   16:(16,1) 45   33:(64,1) 47   64:(64,1) 47   65:(64,2) 23
# 129:(64,4) 11   256:(64,4) 11   257:(64,8) 5   512:(64,8) 5
FOLD_D = [1, 9, 16, 33, 64, 65, 129, 256, 257, 512]
FOLD_CASES = [("closed_form", "reg", "abs"), ("closed_form", "reg", "softplus"), ("sampled", "class", "abs"),
              ("sampled", "class", "softplus")]


@pytest.mark.parametrize("objective,output,link", FOLD_CASES)
@pytest.mark.parametrize("d", FOLD_D)
def test_foldin_every_shape_vs_fp64(d, objective, output, link):
    """Objective and gradient against fp64 autograd of objective_fp64; one entity has 60 rows, more than any shape's
    LDS cap, so the streamed rows are part of the comparison; then rows all streamed (lds_rows = 0) == staged, bitwise."""
    from test_gpu_foldin import _model as _fold_model, _rows, _theta, _oracle
    from vae_amd import foldin
    i = FOLD_D.index(d)
    F = (2, 3)[i % 2] if objective == "closed_form" else (1, 2, 3)[i % 3]
    S = 1 if objective == "closed_form" else 1 + i % 3
    field = i % F
    m = _fold_model((40, 30, 25)[:F], d, output, link, seed=d + field)
    X, y = _rows(m, field, 6, 40, seed=d, output=output)
    Xh, yh = _rows(m, field, 1, 60, seed=d + 1, output=output)       # one entity with 60 rows (caps: 5 ... 47)
    X, y = torch.cat([X, Xh]), torch.cat([y, yh])
    loss, grads = m.fold_in_objective(X, y, field=field, objective=objective, n_samples=S, seed=5, step=2,
                                      kl_weight=0.7)
    ents = grads["entities"]
    assert torch.equal(ents, torch.unique(X[:, field]))
    assert int((X[:, field] == Xh[0, field]).sum()) >= 60
    th = _theta(m, ents)
    eps = _eps_any_d(m, 5, 2, S) if objective == "sampled" else None
    L = _oracle(m, X, y, field, objective, th, ents, eps, kl_weight=0.7)
    L.sum().backward()
    assert rel_err(loss.cpu().numpy(), L.detach().numpy()) <= 1e-5
    ge = torch.cat([th[0].grad, th[1].grad], 1).numpy()
    gb = torch.stack([th[2].grad, th[3].grad], 1).numpy()
    assert rel_err(grads["entity"].cpu().numpy(), ge) <= 1e-5
    assert rel_err(grads["bias"].cpu().numpy(), gb) <= 1e-5
    _, l0, _, g0 = foldin.run(m, X, y, field, objective, S, 5, 0.7, mode=foldin.MODE_OBJECTIVE, t0=2, lds_rows=0)
    assert torch.equal(l0, loss)
    assert torch.equal(g0, torch.cat([grads["entity"], grads["bias"]], 1))


def _eps_any_d(m, seed, t, S):
    """test_gpu_foldin._eps at any d: the Philox draws are keyed on (entity, block of 8 coordinates), not on d, so the
    tables of d' = 8 ceil(d/8) cut to d columns are those of d (philox_eps takes the training sizes only, and d = 257
    is not one of them)."""
    from vae_amd import ops
    d8 = -(-m.d // 8) * 8
    spec = ops.Spec(T=m.T, F=m.F, d=d8, group_hi=m.group_hi, group_n=m.group_n, likelihood=0, n_samples=1, link=m.link)
    out = []
    for s in range(S):
        ee, eb, eg = (a.cpu() for a in ops.philox_eps(spec, seed, t * S + s, DEV))
        out.append((ee[:, :m.d].contiguous(), eb, eg))
    return out


def test_foldin_refuses_d_above_512():
    from test_gpu_foldin import _model as _fold_model, _rows
    m = _fold_model((40, 30), 513)
    X, y = _rows(m, 0, 3, 12, seed=1)
    with pytest.raises(ValueError, match="512"):
        m.fold_in_objective(X, y)
    with pytest.raises(ValueError, match="512"):
        m.fold_in(X, y, n_steps=2, lr=0.01)


# ------------------------------------------------------------------------------------------------ ranking
# vfm_rank_tile.hpp: mean GEMM depth KA = ceil(d/16)*16, variance GEMM depth KB = ceil(2d/16)*16 (zero padded),
# 256-user x 64-item tiles, KR = 16 register list.
# d -> (KA, KB): 1:(16,16) 2:(16,16) 16:(16,32) 17:(32,48) 256:(256,512) 1024:(1024,2048)
RANK_D = [1, 2, 16, 17, 256, 1024]
STRATEGIES = ["top", "variance", "mean", "random"]


@pytest.mark.parametrize("link", ["abs", "softplus"])
@pytest.mark.parametrize("d", RANK_D)
def test_rank_items_every_padding(d, link):
    """rank_items against the fp64 oracle (check_ranking, tie-aware) for every strategy: 200 items = 4 item tiles
    (the last 8 wide), candidate sets of 1 / 63 / 64 / 65 items, k = 16 / 17 / 128, n_splits above the tile count."""
    N, M = 300, 200
    m = _rank_model(N, M, d, output="class", link=link, seed=d)
    rng = np.random.default_rng(d + (link == "abs"))
    all_items = np.arange(N, N + M, dtype=np.int64)
    for si, strategy in enumerate(STRATEGIES):
        users = np.sort(rng.choice(N - 1, 40, replace=False)).astype(np.int64)
        S_all, M_all, V_all = rank_oracle(m, users, all_items, strategy, seed=9)
        scale = np.abs(S_all).max() + 1
        tol = 0.0 if strategy == "random" else 3e-6 * scale * (1 + d / 16)
        tol_mv = (3e-6 * (np.abs(M_all).max() + 1) * (1 + d / 16), 3e-6 * (np.abs(V_all).max() + 1) * (1 + d / 16))
        ex = _rank_exclusions(users, all_items, rng)
        sub = rng.choice(all_items, (1, 63, 64, 65)[si], replace=False)
        for items, exclude, k, n_splits in ((None, ex, 17, 0), (None, None, 16, 7), (sub, ex, 16, 5),
                                            (sub, None, 128, 64)):
            cand = all_items if items is None else np.sort(items)
            cols = cand - N
            excl = (_excluded_mask(users, cand, exclude) if exclude is not None
                    else np.zeros((len(users), len(cand)), bool))
            out = m.rank_items(torch.tensor(users), k=k, strategy=strategy,
                               items=None if items is None else torch.tensor(items),
                               exclude=None if exclude is None else torch.tensor(exclude), seed=9, n_splits=n_splits)
            check_ranking(out, cand, S_all[:, cols], M_all[:, cols], V_all[:, cols], excl, k, tol, tol_mv)


@pytest.mark.parametrize("U", [255, 256, 257])
def test_rank_user_tile_edges(U):
    """255 / 256 / 257 query users around the 256-user tile: rank_items against the fp64 oracle, rank_heldout against
    the exact ranks (d = 17: KA = 32, KB = 48)."""
    N, M, d = 300, 130, 17
    m = _rank_model(N, M, d, output="class", seed=U)
    rng = np.random.default_rng(U)
    users = np.arange(U, dtype=np.int64)
    all_items = np.arange(N, N + M, dtype=np.int64)
    ex = _exclusions(users, all_items, rng, 0.1)
    excl = _excluded_mask(users, all_items, ex)
    for strategy, k in (("top", 17), ("variance", 128)):
        S_all, M_all, V_all = rank_oracle(m, users, all_items, strategy)
        tol = 3e-6 * (np.abs(S_all).max() + 1) * (1 + d / 16)
        tol_mv = (3e-6 * (np.abs(M_all).max() + 1) * (1 + d / 16), 3e-6 * (np.abs(V_all).max() + 1) * (1 + d / 16))
        out = m.rank_items(torch.tensor(users), k=k, strategy=strategy, exclude=torch.tensor(ex))
        check_ranking(out, all_items, S_all, M_all, V_all, excl, k, tol, tol_mv)
        pos = draw_positives(users, all_items, ex, rng, mean=3.0)
        r = m.rank_heldout(torch.tensor(pos), exclude=torch.tensor(ex), strategy=strategy)
        check_against_oracle(m, r, all_items, pos, ex, strategy)


@pytest.mark.parametrize("link", ["abs", "softplus"])
@pytest.mark.parametrize("d", RANK_D)
def test_rank_heldout_every_padding(d, link):
    N, M = 300, 200
    m = _rank_model(N, M, d, output="class", link=link, seed=d + 1)
    rng = np.random.default_rng(d)
    users = np.sort(rng.choice(N, 24, replace=False)).astype(np.int64)
    all_items = np.arange(N, N + M, dtype=np.int64)
    ex = _exclusions(users, all_items, rng)
    for si, strategy in enumerate(STRATEGIES):
        sub = rng.choice(all_items, (1, 63, 64, 65)[si], replace=False)
        for items, exclude, n_splits in ((None, ex, 0), (sub, None, 7)):
            cand = all_items if items is None else np.sort(items)
            pos = draw_positives(users, cand, exclude, rng)
            r = m.rank_heldout(torch.tensor(pos), items=None if items is None else torch.tensor(items),
                               exclude=None if exclude is None else torch.tensor(exclude), strategy=strategy, seed=9,
                               n_splits=n_splits)
            check_against_oracle(m, r, cand, pos, exclude, strategy, seed=9)


# k_moments (F = 2 and general F): the same padded depths as above.  Error model: the fp32 dot products are fma chains
# whose rounding errors add like a random walk, so the error relative to the largest |value| grows like sqrt(d); the
# 2e-6 of test_moments_general_fields (which holds up to d = 128) is scaled by sqrt(d / 128) above d = 128.
@pytest.mark.parametrize("F,d", [(2, v) for v in RANK_D] + [(3, 1024)])
@pytest.mark.parametrize("link", ["abs", "softplus"])
def test_predictive_moments_every_padding(F, d, link):
    from vae_amd.model import VFM
    sizes = [40 + 7 * f for f in range(F)]
    torch.manual_seed(F * 100 + d)
    m = VFM(field_sizes=sizes, embedding_size=d, link=link, device=DEV)
    with torch.no_grad():
        m._flat.mul_(0.5)
    off = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    rng = np.random.default_rng(d)
    xn = (rng.integers(0, min(sizes), size=(700, F)) + off[None, :]).astype(np.int64)
    rm, rv = closed_form(*_tables_np(m), xn, link)
    tol = 2e-6 * max(1.0, math.sqrt(d / 128))
    for dt in (torch.int64, torch.int32):
        mean, var = m.predictive_moments(torch.tensor(xn, device=DEV).to(dt))
        assert np.abs(mean.cpu().numpy() - rm).max() <= tol * np.abs(rm).max()
        assert np.abs(var.cpu().numpy() - rv).max() <= tol * np.abs(rv).max()

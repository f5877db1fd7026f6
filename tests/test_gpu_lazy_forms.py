"""GPU: the look-ahead, row-list (lazy), staged and pipelined forms of the fused backward + Adam at EVERY lane-group shape
and configuration they accept, ONE step from a planted optimiser state against fp64 -- on the machinery of
tests/test_gpu_adam_state.py (_case: planted moments, lagging rows replayed in fp64, bounds from adam_restatement.bounds +
replay_bound; nothing here is fitted to what the kernels give) -- plus the two records these forms keep beside the tables:
the NEXT step's sample record written by k_bwd<PIPE>, and the packed first-order records (wrec).

d -> k_bwd <LPE, CPL, VEC> (pick_shape) -> cases of this file (LA look-ahead entry, listed + scan; LZ catch-up +
rows="touched"; ST acc + apply in two chunks and acc_rows + apply_rows; PI pipelined + next record; W wrec write-back):
  4, 8, 12   (4,1,4)    LA 4 8 12 | LZ 4, 8 (S = 2, MULTI instance with a row list)
  20         (8,1,4)    LA | PI plain, scaled, look-ahead form | W every entry
  64         (16,1,4)   LA (softplus; t = 40 and 127) | LZ (softplus, table eps) | ST (softplus, Bernoulli, F = 3)
  100, 128   (32,1,4)   LA (100: F = 5) | PI 128
  256        (64,1,4)   LA (softplus, Bernoulli) | LZ (S = 2, softplus)
  300, 512   (64,2,4)   LA 300 (F = 2 and F = 5, Bernoulli), 512 (softplus, F = 3), heavy lists 300 | ST 300 | PI 300, 512 |
                        W 300 every entry
  516, 768, 1020 (64,4,4)  LA all three (1020: F = 5, t = 40 and 127) | LZ 516, 1020 | ST 516
  5, 7       (8,1,1)    LA 5, 7 (softplus, Bernoulli, F = 3) | ST 7
  33         (64,1,1)   LA (F = 5, Bernoulli, int32 ids) | LZ
  130, 255   (64,4,1)   LA 130 (softplus), 255 (t = 40 and 127) | LZ 130
  16         (4,1,4)    LA heavy lists
Every look-ahead case forces S = 1 and Philox eps (the entry takes nothing else); the staged entries force S = 1
(single_sample_only in vfm_abi.hip); apply_adam_rows has no eps arguments, so its cases run Philox.  The lazy row-list
step DOES take S > 1: launch_bwd_t launches the MULTI instance with b.row_ids (no refusal in vfm_elbo_bwd_adam_f32), so
d = 8 and d = 256 run it with S = 2 and table eps.  Refused before any launch (asserted: VFM_E_UNSUPPORTED, the
message, tables / moments / last_step bitwise unchanged): look-ahead and pipelined with S = 2, pipelined with softplus,
pipelined with d % 4 != 0.

The next-step record (w, KL weighted, 0, 0 | z) of an entity of the next plan, against fp64 at the reference's updated
parameters p' (R.step_fp64) with the draws of philox_eps(step + 1), group_n / W(next plan) and 1 / occ:
  z, w     |dz| <= du_mu + |eps| du_s + 1/2 ulp(|mu| + |sigma eps|): du is _case's bound on p' (update + replay), the
           half ulp the single rounding of fmaf(sigma, eps, mu).
  KL       |dKL| <= cs io [ sum_k (|mu_k| du_mu_k + |sigma_k - 1 / sigma_k| du_s_k) + N_KL 2^-24 sum_k a_k ],
           a_k = (sigma_k^2 + mu_k^2 + 1) / 2 + |log sigma_k| over the d coordinates and the first-order pair;
           N_KL = 28 counted in vfm_bwd.hpp / vfm_common.hpp: kl_std_normal 8 (two squares, their sum, - 1, the hardware
           log2 at 1 ulp = 2, the constant LN2 and its product, the difference), the lane's serial sum of CPL VEC <= 8
           terms (d <= 512), lane 0's first-order term 1, group_sum over 64 lanes 6, and 5 for the weight (W summed from
           fp32 1 / occ, its cast to fp32, 1 / occ itself, cs io, the last product).
  Entries whose update bound is not asserted (adam_restatement.asserted: the fresh rows) carry no statement; at most 2 %.

Wrong kernels this file catches (each run once on an MI355X against a scratch build of the |.|-link fused-Adam unit; the
assertion that tripped, with the worst value / bound seen):
  (a) the replay applied to chunk 0 only when CPL > 1: the parameters of a next-only row's chunks 1.. stay `lag` steps
      behind -- `update` of the entity table, 4.2e5 bounds at d = 300 and 4.5e5 at d = 516, listed and scan (d = 20, CPL = 1, passes).
  (b) next-only rows stepped with this step's (a1, q2) for the whole lag: `update` of the entity table (and bias) at
      every size: 2.7e5 bounds at d = 5, 3.1e5 at d = 33 and d = 255 (the three VEC = 1 shapes), listed and scan.
  (c) cs_next from this plan's W: the weighted KL of every record is off by W / W_next - 1 (percents) --
      "next record KL", 1.1e4 bounds (plain, scaled) and 3.0e4 (look-ahead form) at d = 20.
  (d) the next record sampled from the parameters before the update: "next record z" (error lr-sized against a bound
      of 1e-7): 4.8e4 bounds at d = 20, all four forms.
  (e) the wrec write-back skipped for next-only rows: "wrec of the visited rows" of test_wrec_written_by_every_entry
      [lookahead], d = 20 and d = 300.

The lazy cases hand _case the tables their gradient was taken at (params_at_gradient: read back after the catch-up), and
the oracle's gradient is taken there: the fp32 replay may differ from the fp64 one by replay_bound -- granted to the update
-- and where the replay has carried a scale parameter to within 1e-5 of zero (d = 1020: one of 640,000) the 1 / sigma term
of the KL gradient turns that difference into 4 bounds of m' if the oracle stands at the fp64 replay instead.

Measured on an MI355X, worst error / bound (m', v', update; the file runs in 17 s):
  entry point (cases of this file)   form    entity                bias                  scalars
  look-ahead, listed and scan        scaled  0.021  0.380  0.471   0.019  0.365  0.476   0.015  0.214  0.433
  look-ahead, heavy lists            scaled  0.010  0.393  0.465   0.007  0.281  0.474   0.002  0.173  0.376
  lazy (catch-up + row list)         scaled  0.011  0.383  0.471   0.006  0.329  0.444   0.010  0.072  0.403
  lazy, S = 2                        scaled  0.008  0.388  0.463   0.006  0.305  0.463   0.000  0.054  0.085
  acc + apply, two chunks            plain   0.009  0.204  0.474   0.004  0.198  0.467   0.044  0.123  0.311
  acc + apply, two chunks            scaled  0.009  0.381  0.473   0.006  0.280  0.466   0.029  0.101  0.310
  acc_rows + apply_rows              scaled  0.008  0.362  0.453   0.006  0.316  0.466   0.012  0.114  0.380
  pipelined + next record            plain   0.006  0.204  0.470   0.003  0.184  0.471   0.027  0.195  0.436
  pipelined + next record            scaled  0.009  0.381  0.469   0.005  0.322  0.470   0.019  0.218  0.435
  pipelined look-ahead + record      scaled  0.008  0.358  0.459   0.005  0.293  0.460   0.004  0.154  0.280
  next record (z, w, KL)             pipelined plain 0.592 0.599 0.048, scaled 0.590 0.598 0.048, look-ahead form 0.611 0.558 0.042
  loss within 1.0e-7 of the oracle's; forwards fed with the record / with wrec: pred 2.4e-7, loss 5.4e-8
"""
import types

import numpy as np
import pytest
import torch

import adam_restatement as R
from golden_util import rel_err
from oracle import vfm_oracle as O
from test_gpu_adam_state import (ALL_D, COVER, DEV, EXTRA_COVER, I32, I64, LOSS_TOL, _case, _lookahead_lag, _period_start,
                                 _pipe_forward, _scaled_tab, build_problem)

pytestmark = pytest.mark.gpu
N_KL = 28
SENTINEL = np.float32(-3.0e33)

# ------------------------------------------------------------------------------------------------ the problems (numpy only)
LA_T = 40
LA_CASES = [(d, COVER[d], d) for d in ALL_D] + [(d, cfg, d + 1) for d, cfg in EXTRA_COVER]      # (d, configuration, seed)
LA_LONG = [1020, 255, 64]                 # t = 127: CPL = 4, wide VEC = 1, softplus
LAZY_D, LAZY_MULTI_D = [4, 33, 64, 130, 516, 1020], [8, 256]
STAGED_D = [7, 64, 300, 516]
PIPE_D = [20, 128, 300, 512]
WREC_D = [20, 300]


def _cover_kw(d, cfg, seed, S=1):
    return dict(F=cfg[0], d=d, output=cfg[3], link=cfg[2], S=S, seed=seed)


def _plain_kw(d):
    return dict(F=2, d=d, output="reg", seed=300 + d)          # the problems of the pipelined cases of test_gpu_adam_state.py


HEAVY_KW = dict(F=2, output="reg", seed=77, B=3000, sizes=[3000, 2500], skew=True)


def problems_of_lazy_forms():
    """(name, build_problem arguments, steps t at which a look-ahead next batch is drawn) of every planted problem of this
    file: tests/test_adam_state_cpu.py checks the excluded share of each, and the look-ahead split, without a GPU."""
    out = [("lookahead d=%d F=%d" % (d, cfg[0]), _cover_kw(d, cfg, seed), [LA_T] + ([127] if d in LA_LONG and cfg is COVER[d] else []))
           for d, cfg, seed in LA_CASES]
    out += [("lookahead heavy d=%d" % d, dict(HEAVY_KW, d=d), [LA_T]) for d in (16, 300)]
    out += [("lazy d=%d" % d, _cover_kw(d, COVER[d], 500 + d), []) for d in LAZY_D]
    out += [("lazy S=2 d=%d" % d, _cover_kw(d, COVER[d], 500 + d, S=2), []) for d in LAZY_MULTI_D]
    out += [("staged d=%d" % d, _cover_kw(d, COVER[d], 700 + d), []) for d in STAGED_D]
    out += [("record / wrec d=%d" % d, _plain_kw(d), [LA_T]) for d in sorted(set(PIPE_D + WREC_D))]
    return out


def lookahead_split(pb, t):
    """The next batch _case will draw for (pb, t) -- its own generator state -- and the split's row counts."""
    d = pb["spec"].d
    c = types.SimpleNamespace(spec=pb["spec"], touched=pb["touched"])
    nxt = {}
    _lookahead_lag(np.random.default_rng(1000 * t + d), c, pb, t, nxt)        # (asserts the 20-row minimums)
    return nxt


# ------------------------------------------------------------------------------------------------ 1. look-ahead entry
def _la_run(pb, t, nxt, listed, ids, wrec=None, after=None):
    def run(c):
        ops = c.ops
        plan2 = ops.BatchPlan(c.spec, torch.tensor(nxt["x"], device=c.dev).to(ids).contiguous(),
                              torch.tensor(pb["y"], device=c.dev), c.inv_occ)
        tab = torch.tensor(_scaled_tab(t, c.lr), device=c.dev)
        if wrec is not None:
            c.wrec = _build_wrec(c)
        c.forward()
        ops.elbo_backward_adam_lookahead(c.plan, c.st, plan2, c.ent, c.bia, c.scal, c.inv_occ, c.mv, c.vv, c.lr, t, c.l3,
                                         c.last_step, tab, listed=listed, wrec=getattr(c, "wrec", None))
        visited = c.touched | nxt["mask"]
        c.visited = visited
        last = c.last_step.cpu().numpy()
        assert (last[visited] == t).all()
        assert np.array_equal(last[~visited], c.last_np[~visited])
        k = (t - 1) % R.PERIOD + 1
        cst = R.scaled_consts(t, c.lr)             # the kernel leaves this step's (a1, q2) for later replays
        assert abs(tab[2 * k].item() - cst["a1"]) <= R.ulp32(cst["a1"]) and abs(tab[2 * k + 1].item() - cst["q2"]) <= R.ulp32(cst["q2"])
        if after is not None:
            after(c)
    return run


def _lookahead_case(pb, t, listed, ids=I64, tag="lookahead", **kw):
    nxt = {}

    def lag(rng, c):
        return _lookahead_lag(rng, c, pb, t, nxt)
    return _case("lookahead", pb, t, "scaled", eps="philox", ids=ids, lag=lag, run=_la_run(pb, t, nxt, listed, ids, **kw),
                 tag="%s:%s" % (tag, "listed" if listed else "scan")), nxt


@pytest.mark.parametrize("listed", [True, False])
@pytest.mark.parametrize("d,cfg,seed", LA_CASES, ids=["d%d-F%d" % (d, cfg[0]) for d, cfg, _ in LA_CASES])
def test_lookahead_every_bucket(d, cfg, seed, listed):
    """k_bwd<..., LA> at all 18 sizes with the covering set's F, link, likelihood and id width (S = 1, Philox): rows of
    this batch take the gradient step, rows only the next batch holds replay their lag (up to 39 steps) + this step's
    zero-gradient update, rows in neither stay bitwise, the table keeps this step's (a1, q2)."""
    _lookahead_case(build_problem(**_cover_kw(d, cfg, seed)), LA_T, listed, ids=cfg[5])


@pytest.mark.parametrize("listed", [True, False])
@pytest.mark.parametrize("d", LA_LONG)
def test_lookahead_long_lags(d, listed):
    """t = 127: lags up to 126 steps at CPL = 4 (1020), the wide VEC = 1 shape (255) and the softplus link (64)."""
    cfg = COVER[d]
    _lookahead_case(build_problem(**_cover_kw(d, cfg, d)), 127, listed, ids=cfg[5])


@pytest.mark.parametrize("d", [16, 300])
def test_lookahead_heavy_lists(d):
    """The skewed batch of test_heavy_lists_step under the look-ahead entry (listed): the pre-reduced long lists feed LA."""
    pb = build_problem(**dict(HEAVY_KW, d=d))

    def after(c):
        assert c.plan.heavy is not None and c.plan.heavy[0].numel() >= 4
    _lookahead_case(pb, LA_T, True, tag="lookahead-heavy", after=after)


# ------------------------------------------------------------------------------------------------ 2. lazy row list, stages
def _lazy_run(t, wrec=False):
    def run(c):
        ops, out = c.ops, torch.tensor(~c.touched, device=c.dev)
        lrs = [c.lr] * (t - _period_start(t))
        ids = c.plan.touched_ids()
        w = w0 = None
        if wrec:
            w = c.wrec = _build_wrec(c)
            w0 = w.clone()
        ops.adam_catchup(c.ent, c.bia, c.mv, c.vv, c.last_step, ids, lrs[:-1], upto=t - 1, mark=t, wrec=w)
        if wrec:               # the catch-up refreshed the records of ITS rows from the caught-up bias table
            _assert_wrec(c, w, w0, c.touched, "catch-up")
        # the step's gradient is taken at THESE parameters: the oracle's too (see _case: params_at_gradient)
        c.params_at_gradient = [c.ent.cpu().numpy(), c.bia.cpu().numpy()]
        e0, b0, m0, v0, l0 = c.ent.clone(), c.bia.clone(), c.mv[0].clone(), c.vv[0].clone(), c.last_step.clone()
        c.forward()
        ops.elbo_backward_adam(c.plan, c.st, c.ent, c.bia, c.scal, c.inv_occ, c.mv, c.vv, c.lr, t, loss_out=c.l3,
                               scaled_moments=True, rows="touched", wrec=w)
        assert torch.equal(c.ent[out], e0[out]) and torch.equal(c.bia[out], b0[out])
        assert torch.equal(c.mv[0][out], m0[out]) and torch.equal(c.vv[0][out], v0[out])
        assert torch.equal(c.last_step[out], l0[out]) and bool((c.last_step[~out] == t).all())
        assert np.array_equal(l0[out].cpu().numpy(), c.last_np[~c.touched])
        if wrec:
            _assert_wrec(c, w, w0, c.touched, "rows=touched")
        ops.adam_catchup(c.ent, c.bia, c.mv, c.vv, c.last_step, None, lrs, upto=t, mark=t, wrec=w)
        assert bool((c.last_step == t).all())
        c.visited = np.ones(c.spec.T, bool)
    return run


def _lazy_lag(t):
    def lag(rng, c):
        return rng.integers(_period_start(t), t, c.spec.T), np.zeros(c.spec.T, bool)
    return lag


@pytest.mark.parametrize("d", LAZY_D)
def test_lazy_row_list_uncovered_buckets(d):
    """vfm_adam_catchup_f32 + the rows="touched" step (the dense instance walking a row list) at one size per bucket the
    lazy entry had not met, with the covering set's F, link, likelihood, eps source and id width at S = 1."""
    cfg = COVER[d]
    pb = build_problem(**_cover_kw(d, cfg, 500 + d))
    _case("lazy", pb, LA_T, "scaled", eps=cfg[4], ids=cfg[5], lag=_lazy_lag(LA_T), run=_lazy_run(LA_T))


@pytest.mark.parametrize("d", LAZY_MULTI_D)
def test_lazy_row_list_two_samples(d):
    """S = 2 with a row list: launch(yes, no, no) of launch_bwd_t with b.row_ids -- the MULTI instance's per-sample walk
    over listed rows (table eps)."""
    cfg = COVER[d]
    pb = build_problem(**_cover_kw(d, cfg, 500 + d, S=2))
    _case("lazy-S2", pb, LA_T, "scaled", eps="table", ids=cfg[5], lag=_lazy_lag(LA_T), run=_lazy_run(LA_T))


def _two_chunks(c):
    ops, T, d = c.ops, c.spec.T, c.spec.d
    c.forward()
    c.l3.copy_(ops.elbo_finalize(c.st, c.scal))
    acc = torch.zeros(T * ops.exchange_record_len(d), device=c.dev)
    sums = torch.zeros(2, device=c.dev)
    mid = T // 2 + 1
    for lo, hi in ((0, mid), (mid, T)):
        ops.elbo_backward_acc(c.plan, c.st, acc, sums, lo, hi)
    for lo, hi in ((0, mid), (mid, T)):
        ops.elbo_apply_adam(c.plan, c.st, acc, sums, c.ent, c.bia, c.scal, c.inv_occ, c.mv, c.vv, c.lr, c.t, e_lo=lo,
                            e_hi=hi, scaled_moments=c.scaled)


def _rows_compact(wrec=False):
    def run(c):
        ops, d = c.ops, c.spec.d
        w = w0 = None
        if wrec:
            w = c.wrec = _build_wrec(c)
            w0 = w.clone()
        c.forward()
        c.l3.copy_(ops.elbo_finalize(c.st, c.scal))
        ids = c.plan.touched_ids()
        acc = torch.zeros(ids.numel() * ops.exchange_record_len(d), device=c.dev)
        sums = torch.zeros(2, device=c.dev)
        ops.elbo_backward_acc_rows(c.plan, c.st, ids, acc, sums)
        ops.elbo_apply_adam_rows(c.plan, c.st, acc, sums, ids, c.ent, c.bia, c.scal, c.inv_occ, c.mv, c.vv, c.lr, c.t,
                                 move_scalars=True, compact=True, wrec=w)
        c.visited = c.touched.copy()
    return run


def _keep_untouched(rng, c):
    return np.full(c.spec.T, c.t - 1, np.int64), ~c.touched


@pytest.mark.parametrize("form", ["plain", "scaled"])
@pytest.mark.parametrize("d", STAGED_D)
def test_staged_two_entity_chunks(d, form):
    """elbo_backward_acc + elbo_apply_adam over two entity chunks with the covering set's F, link, likelihood, eps source
    and id width (S = 1: the stages exchange single-sample statistics) -- VEC = 1 (7), softplus (7, 64), CPL = 2 and 4."""
    cfg = COVER[d]
    pb = build_problem(**_cover_kw(d, cfg, 700 + d))
    _case("acc+apply", pb, 57, form, eps=cfg[4], ids=cfg[5], run=_two_chunks)


@pytest.mark.parametrize("d", STAGED_D)
def test_staged_listed_rows_compact(d):
    """elbo_backward_acc_rows + elbo_apply_adam_rows with compact records (Philox: the entry takes no eps tables)."""
    cfg = COVER[d]
    pb = build_problem(**_cover_kw(d, cfg, 700 + d))
    _case("acc_rows+apply_rows", pb, 57, "scaled", eps="philox", ids=cfg[5], lag=_keep_untouched, run=_rows_compact())


REFUSALS = {
    "lookahead-S2": (dict(F=2, d=20, output="reg", S=2), ("vfm_elbo_bwd_adam_lookahead_f32", "n_samples")),
    "pipe-S2": (dict(F=2, d=20, output="reg", S=2), ("vfm_elbo_bwd_adam_pipe_f32", "n_samples")),
    "pipe-softplus": (dict(F=2, d=20, output="reg", link="softplus"), ("vfm_elbo_bwd_adam_pipe_f32", "|.| link")),
    "pipe-d6": (dict(F=2, d=6, output="reg"), ("vfm_elbo_bwd_adam_pipe_f32", "d % 4 == 0")),
}


@pytest.mark.parametrize("which", list(REFUSALS))
def test_refused_before_any_launch(which):
    """What the C ABI refuses (VFM_E_UNSUPPORTED = -2, a host-side return): nothing of the state moves."""
    from vae_amd import _lib, ops
    kw, words = REFUSALS[which]
    pb = build_problem(seed=900, **kw)
    spec, P, dev, t = pb["spec"], pb["P"], torch.device(DEV), LA_T
    T, d = spec.T, spec.d
    rng = np.random.default_rng(3)
    inv_occ = ops.inv_occ_from_counts(torch.tensor(pb["nb_occ"], device=dev))
    plan = ops.BatchPlan(spec, torch.tensor(pb["x"], device=dev), torch.tensor(pb["y"], device=dev), inv_occ)
    plan2 = ops.BatchPlan(spec, torch.tensor(pb["x"][::-1].copy(), device=dev), torch.tensor(pb["y"], device=dev), inv_occ)
    ent, bia = torch.tensor(P["entity_params"], device=dev), torch.tensor(P["bias_params"], device=dev)
    scal = torch.tensor(np.concatenate([P["alpha"], P["global_bias_mean"], P["global_bias_scale"]]), device=dev)
    mv = tuple(torch.tensor(rng.standard_normal(s).astype(np.float32), device=dev) for s in ((T, 2 * d), (T, 2), (3,)))
    vv = tuple(torch.tensor(rng.uniform(0.5, 2, s).astype(np.float32), device=dev) for s in ((T, 2 * d), (T, 2), (3,)))
    last = torch.full((T,), t - 1, dtype=torch.int32, device=dev)
    tab = torch.tensor(_scaled_tab(t, R.LR), device=dev)
    l3 = torch.zeros(3, device=dev)
    st = ops.elbo_forward(plan, ent, bia, scal, inv_occ, seed=77, step=1000 + t)
    state = [ent, bia, scal, last, tab, l3] + list(mv) + list(vv)
    before = [a.clone() for a in state]
    with pytest.raises(_lib.VfmLibraryError) as ei:
        if which.startswith("lookahead"):
            ops.elbo_backward_adam_lookahead(plan, st, plan2, ent, bia, scal, inv_occ, mv, vv, R.LR, t, l3, last, tab)
        else:
            zrec = torch.zeros(T, ops.record_len(d), device=dev)
            ops.elbo_backward_adam_pipe(plan, st, zrec, None, None, 1001 + t, ent, bia, scal, inv_occ, mv, vv, R.LR, t, l3)
    msg = str(ei.value)
    assert "code %d" % _lib._gen.VFM_E_UNSUPPORTED in msg and all(w in msg for w in words), msg
    torch.cuda.synchronize()
    for a, b in zip(state, before):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------ 3. the next-step record
def _kl_terms(mu, sg):
    return 0.5 * (sg * sg + mu * mu - 1.0) - np.log(sg), 0.5 * (sg * sg + mu * mu + 1.0) + np.abs(np.log(sg))


def _check_next_record(c, pb, x2, plan2, zrec_next, tag):
    """zrec_next after the step against fp64 at _case's reference p' (c.p_ref) and bound on p' (c.du)."""
    ops, spec = c.ops, c.spec
    T, d, next_step = spec.T, spec.d, c.step + 1
    in_next = np.zeros(T, bool)
    in_next[x2.reshape(-1)] = True
    got = zrec_next.cpu().numpy()
    assert (got[~in_next].view(np.uint32) == SENTINEL.view(np.uint32)).all(), "records outside the next plan"
    assert (got[in_next][:, 2:4].view(np.uint32) == 0).all(), "slots 2, 3"
    ee, eb, eg = (a.cpu().numpy().astype(np.float64) for a in ops.philox_eps(spec, seed=c.seed, step=next_step, device=c.dev))
    pe, pbi, due, dub = c.p_ref[0], c.p_ref[1], c.du[0], c.du[1]
    ok_e = c.ok[0][:, :d] & c.ok[0][:, d:] & in_next[:, None]
    ok_w = c.ok[1][:, 0] & c.ok[1][:, 1] & in_next
    ok_row = ok_w & (c.ok[0].all(axis=1))
    assert 1.0 - (ok_e | ~in_next[:, None]).mean() <= R.MAX_EXCLUDED and 1.0 - (ok_row | ~in_next).mean() <= R.MAX_EXCLUDED
    mu, sg, dmu, dsg = pe[:, :d], np.abs(pe[:, d:]), due[:, :d], due[:, d:]
    z_ref = mu + sg * ee
    dz = dmu + np.abs(ee) * dsg + 0.5 * R.ulp32(np.abs(mu) + dmu + (sg + dsg) * np.abs(ee))
    rz = float((np.abs(got[:, 4:4 + d] - z_ref) / dz)[ok_e].max())
    muw, sgw = pbi[:, 0], np.abs(pbi[:, 1])
    w_ref = muw + sgw * eb
    dw = dub[:, 0] + np.abs(eb) * dub[:, 1] + 0.5 * R.ulp32(np.abs(muw) + dub[:, 0] + (sgw + dub[:, 1]) * np.abs(eb))
    rw = float((np.abs(got[:, 0] - w_ref) / dw)[ok_w].max())
    kv, av = _kl_terms(mu, sg)
    kw_, aw = _kl_terms(muw, sgw)
    W2 = O.batch_norms(x2, pb["nb_occ"])
    grp = O.group_of(np.arange(T), pb["group_hi"])
    weight = (np.asarray(spec.group_n, np.float64) / W2)[grp] / pb["nb_occ"].astype(np.float64)
    kl_ref = (kv.sum(axis=1) + kw_) * weight
    with np.errstate(invalid="ignore"):
        prop = (np.abs(mu) * dmu + np.abs(sg - 1.0 / sg) * dsg).sum(axis=1) + np.abs(muw) * dub[:, 0] + np.abs(sgw - 1.0 / sgw) * dub[:, 1]
    dkl = weight * (prop + N_KL * R.U * (av.sum(axis=1) + aw))
    rk = float((np.abs(got[:, 1] - kl_ref) / dkl)[ok_row].max())
    print("LAZYFORMS next record %s d=%d  z %.3f  w %.3f  KL %.3f" % (tag, d, rz, rw, rk))
    assert rz <= 1.0, ("next record z", rz)
    assert rw <= 1.0, ("next record w", rw)
    assert rk <= 1.0, ("next record KL", rk)
    # ... bitwise what the stand-alone sampler writes from the updated tables
    again = torch.full_like(zrec_next, float(SENTINEL))
    ops.sample_records(plan2, c.ent, c.bia, c.inv_occ, again, c.seed, next_step)
    assert torch.equal(again.view(torch.int32), zrec_next.view(torch.int32)), "next record against vfm_sample_records_f32"
    # ... and consumed: the record forward of the next step against fp64 at p' with the next step's draws
    from vae_amd import _lib
    B = pb["B"]
    st2 = ops.elbo_forward_records(plan2, zrec_next, c.scal, c.seed, next_step, torch.empty(B, device=c.dev),
                                   torch.empty(B, device=c.dev), torch.empty(_lib.PARTIALS_LEN, dtype=torch.float64, device=c.dev))
    loss2 = float(ops.elbo_finalize(st2, c.scal)[0].item())
    ps = c.p_ref[2]
    Pd = {"entity_params": pe, "bias_params": pbi, "alpha": ps[0:1], "global_bias_mean": ps[1:2], "global_bias_scale": ps[2:3]}
    r = O.rowwise_elbo(Pd, x2, pb["y"].astype(np.float64), pb["nb_occ"], np.asarray(pb["group_hi"]), np.asarray(spec.group_n),
                       spec.nb_train, eg, eb, ee, pb["output"], want_grads=False, link=pb["link"])
    rp, rl = rel_err(st2.pred.cpu().numpy(), r["pred"]), abs(loss2 - r["loss"]) / abs(r["loss"])
    print("LAZYFORMS next forward %s d=%d  pred %.2e  loss %.2e" % (tag, d, rp, rl))
    assert rp < 1e-4 and rl < LOSS_TOL, (rp, rl)


def _pipe_run(pb, t, form, x2_of, look=None, wrec=False):
    """elbo_backward_adam_pipe with the next plan's records asked for; look: None, or (nxt, listed) for the look-ahead form."""
    def run(c):
        ops = c.ops
        x2 = x2_of(c)
        c.x2 = x2
        c.plan2 = ops.BatchPlan(c.spec, torch.tensor(x2, device=c.dev), torch.tensor(pb["y"], device=c.dev), c.inv_occ)
        c.zrec_next = torch.full((c.spec.T, ops.record_len(c.spec.d)), float(SENTINEL), device=c.dev)
        w = None
        if wrec:
            w = c.wrec = _build_wrec(c)
        _pipe_forward(c)
        kw = {}
        if look is not None:
            kw = dict(last_step=c.last_step, step_tab=torch.tensor(_scaled_tab(t, c.lr), device=c.dev), listed=look[1], la_next=c.plan2)
        ops.elbo_backward_adam_pipe(c.plan, c.st, c.zrec, c.zrec_next, c.plan2, c.step + 1, c.ent, c.bia, c.scal, c.inv_occ,
                                    c.mv, c.vv, c.lr, t, c.l3, scaled_moments=c.scaled, wrec=w, **kw)
        c.visited = np.ones(c.spec.T, bool)
        if look is not None:
            c.visited = c.touched | look[0]["mask"]
            last = c.last_step.cpu().numpy()
            assert (last[c.visited] == t).all() and np.array_equal(last[~c.visited], c.last_np[~c.visited])
    return run


def _fresh_batch(pb):
    """A next batch for the dense pipelined step (every row is visited: any batch over the same tables)."""
    def x2_of(c):
        hi = np.asarray(pb["group_hi"], np.int64)
        lo = np.concatenate([[0], hi[:-1]])
        g = np.random.default_rng(4242 + c.spec.d)
        return np.stack([g.integers(lo[f], hi[f], pb["B"]) for f in range(len(hi))], 1).astype(np.int64)
    return x2_of


@pytest.mark.parametrize("form", ["plain", "scaled"])
@pytest.mark.parametrize("d", PIPE_D)
def test_next_step_record(d, form):
    """k_bwd<PIPE>: the record of every entity of the next plan is (w, KL weighted, 0, 0 | z) at the UPDATED parameters with
    the next step's draws and the next plan's W; the others keep the sentinel; the next forward consumes it."""
    pb = build_problem(**_plain_kw(d))
    c = _case("pipe+record", pb, 57, form, eps="philox", run=_pipe_run(pb, 57, form, _fresh_batch(pb)))
    _check_next_record(c, pb, c.x2, c.plan2, c.zrec_next, "pipe:" + form)


@pytest.mark.parametrize("listed", [True, False])
@pytest.mark.parametrize("d", PIPE_D)
def test_next_step_record_lookahead_form(d, listed):
    """k_bwd<PIPE, LA> at t = 40: a row only the next batch holds is caught up AND has its record written in one launch."""
    pb = build_problem(**_plain_kw(d))
    nxt = {}

    def lag(rng, c):
        return _lookahead_lag(rng, c, pb, LA_T, nxt)
    c = _case("pipe-lookahead+record", pb, LA_T, "scaled", eps="philox", lag=lag,
              run=_pipe_run(pb, LA_T, "scaled", lambda c: nxt["x"], look=(nxt, listed)),
              tag="pipe-lookahead+record:" + ("listed" if listed else "scan"))
    _check_next_record(c, pb, nxt["x"], c.plan2, c.zrec_next, "pipe-lookahead:" + ("listed" if listed else "scan"))


# ------------------------------------------------------------------------------------------------ 4. packed first-order records
def _build_wrec(c):
    w = torch.full((c.spec.T, 4), float(SENTINEL), device=c.dev)
    c.ops.wrec_build(c.bia, c.inv_occ, w)
    c.wrec0 = w.clone()
    return w


def _assert_wrec(c, w, w0, visited, what):
    """Rows the step visited hold (bias'[e, 0], bias'[e, 1], 1 / occ[e], 0) bitwise; the others are as built."""
    v = torch.tensor(visited, device=c.dev)
    want = torch.cat([c.bia, c.inv_occ[:, None], torch.zeros_like(c.inv_occ)[:, None]], 1)
    assert torch.equal(w[v].view(torch.int32), want[v].view(torch.int32)), ("wrec of the visited rows", what)
    assert torch.equal(w[~v].view(torch.int32), w0[~v].view(torch.int32)), ("wrec of the other rows", what)


def _dense_wrec(c):
    c.wrec = _build_wrec(c)
    c.forward()
    c.ops.elbo_backward_adam(c.plan, c.st, c.ent, c.bia, c.scal, c.inv_occ, c.mv, c.vv, c.lr, c.t, loss_out=c.l3,
                             scaled_moments=c.scaled, wrec=c.wrec)
    c.visited = np.ones(c.spec.T, bool)


@pytest.mark.parametrize("entry", ["dense", "lazy", "lookahead", "pipe", "apply_rows"])
@pytest.mark.parametrize("d", WREC_D)
def test_wrec_written_by_every_entry(d, entry):
    """Every entry that takes `wrec` refreshes the records of the rows it updates, and of no other row ("lazy": the
    catch-up kernel, then the rows="touched" step, each checked on its own)."""
    pb = build_problem(**_plain_kw(d))
    if entry == "dense":
        c = _case("dense+wrec", pb, 57, "scaled", eps="philox", run=_dense_wrec)
    elif entry == "lazy":
        c = _case("lazy+wrec", pb, LA_T, "scaled", eps="philox", lag=_lazy_lag(LA_T), run=_lazy_run(LA_T, wrec=True))
    elif entry == "lookahead":
        c, _ = _lookahead_case(pb, LA_T, True, tag="lookahead+wrec", wrec=True)
    elif entry == "pipe":
        c = _case("pipe+wrec", pb, 57, "scaled", eps="philox", run=_pipe_run(pb, 57, "scaled", _fresh_batch(pb), wrec=True))
    else:
        c = _case("apply_rows+wrec", pb, 57, "scaled", eps="philox", lag=_keep_untouched, run=_rows_compact(wrec=True))
    assert c.visited.any()
    _assert_wrec(c, c.wrec, c.wrec0, c.visited, entry)


@pytest.mark.parametrize("planted", [False, True])
@pytest.mark.parametrize("F,d", [(2, 20), (3, 32)])
def test_forward_reads_the_packed_records(F, d, planted):
    """The training forward given `wrec` (k_fwd2 at F = 2, k_fwdg at F = 3) takes (mu_w, s_w) and 1 / occ from the record
    (vfm_fwd2.hpp load_ent): pred and loss against fp64.  planted: the record is built from ANOTHER bias table and other
    occurrence counts -- the forward must follow the record (a kernel that ignored it would give the unplanted result,
    which the test first shows to be far outside the tolerances)."""
    from vae_amd import ops
    pb = build_problem(F, d, "reg", seed=40 + d)
    spec, P, x, y, nb_occ, dev = pb["spec"], pb["P"], pb["x"], pb["y"], pb["nb_occ"], torch.device(DEV)
    g = np.random.default_rng(d)
    bias2, occ2 = P["bias_params"], nb_occ
    if planted:
        bias2 = (P["bias_params"] + 0.3 * g.standard_normal(P["bias_params"].shape)).astype(np.float32)
        occ2 = nb_occ + g.integers(1, 9, nb_occ.shape)
    inv_occ = ops.inv_occ_from_counts(torch.tensor(nb_occ, device=dev))
    ent, bia = torch.tensor(P["entity_params"], device=dev), torch.tensor(P["bias_params"], device=dev)
    scal = torch.tensor(np.concatenate([P["alpha"], P["global_bias_mean"], P["global_bias_scale"]]), device=dev)
    plan = ops.BatchPlan(spec, torch.tensor(x, device=dev), torch.tensor(y, device=dev), inv_occ)
    wrec = torch.empty(spec.T, 4, device=dev)
    ops.wrec_build(torch.tensor(bias2, device=dev), ops.inv_occ_from_counts(torch.tensor(occ2, device=dev)), wrec)
    st = ops.elbo_forward(plan, ent, bia, scal, inv_occ, seed=5, step=9, wrec=wrec)
    loss = float(ops.elbo_finalize(st, scal)[0].item())
    ee, eb, eg = (a.cpu().numpy() for a in ops.philox_eps(spec, seed=5, step=9, device=dev))

    def ref(bias, occ):        # (the normalisers W are the plan's: from the true counts)
        return O.rowwise_elbo(dict(P, bias_params=bias), x, y.astype(np.float64), occ, np.asarray(pb["group_hi"]),
                              np.asarray(spec.group_n), spec.nb_train, eg, eb, ee, "reg", W=O.batch_norms(x, nb_occ),
                              want_grads=False)
    r = ref(bias2, occ2)
    if planted:
        r0 = ref(P["bias_params"], nb_occ)
        assert rel_err(r0["pred"], r["pred"]) > 1e-2 and abs(r0["loss"] - r["loss"]) / abs(r["loss"]) > 100 * LOSS_TOL
    rp, rl = rel_err(st.pred.cpu().numpy(), r["pred"]), abs(loss - r["loss"]) / abs(r["loss"])
    print("LAZYFORMS forward with wrec F=%d d=%d planted=%s  pred %.2e  loss %.2e" % (F, d, planted, rp, rl))
    assert rp < 1e-4 and rl < LOSS_TOL, (rp, rl)

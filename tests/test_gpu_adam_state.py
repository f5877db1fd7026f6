"""GPU: the fused Adam of every backward entry point, ONE step from a planted (live) optimiser state, against fp64.

Every case plants plain moments "after t - 1 steps" (tests/adam_restatement.py: m ~ N(0, (0.3 G)^2), v in
[0.25, 4] G^2, a few fresh rows with m = v = 0), hands the kernel the buffers in the form it expects, runs one step with
lr = 0.01 and compares the entity table, the bias table and the three scalars -- new moments, update p' - p, loss --
with oracle.vfm_oracle.rowwise_elbo + adam_step in fp64.  The bounds are derived (adam_restatement.bounds) from the
gradient tolerance the suite already grants (1e-4 of the largest entry for the tables, the fuzz's summation bound for the
scalars) and from counted roundings; nothing here is fitted to what the kernels give.  F = 1 is left out: its embedding
gradient is cancellation noise (tests/fuzz_parity.py).  The lazy entry points start from rows that LAG (their parameters
are those of an earlier step): the reference replays the zero-gradient steps in fp64, and the gradient oracle is evaluated
at the fp64 caught-up parameters -- the kernels' fp32 replay differs from them by less than replay_bound, which moves the
gradient by far less than the granted tol_g.

d -> k_bwd <LPE, CPL, VEC> (pick_shape, vfm_abi.hip):
  4, 8, 12:(4,1,4)  20:(8,1,4)  64:(16,1,4)  100, 128:(32,1,4)  256:(64,1,4)      CPL = 1
  300, 512:(64,2,4)                                                                  CPL = 2
  516, 768, 1020:(64,4,4)                                                            CPL = 4
  5, 7:(8,1,1)  33:(64,1,1)  130, 255:(64,4,1)                                       VEC = 1
Philox eps, one sample, d % 4 == 0, d <= 256 and a table under 2 MiB: the dense step is the one-launch small-table kernel
(vfm_bwd_small.hpp) unless VFM_BWD_SMALL=0; table eps, S > 1 and every other d run k_bwd.

Wrong kernels this file catches (mutations of adam_update, its halves and the host's constants; by reading).  The
step-1-from-zero tests pass every one of them for the same reason: with m = v = 0 at t = 1 the update is -lr sign(g)
whatever decay, scale or bias correction multiplies the moments, only the entity table is compared, and an untouched row
does not move at all.
  1. b1 and b2 swapped in c1 / c2 (scaled form): m' gains 0.001 g / b2^k instead of 0.1 g / b1^k -- the m' assertion of
     every scaled case, first at d = 4, t = 57 (error ~0.1 G against a bound of 1e-5 G).
  2. k taken as t mod 128 instead of (t - 1) mod 128 + 1: at t = 57 the new moments come out scaled by b^56 where b^57
     is expected -- m' is off by 10 % at every scaled case; at t = 128 k = 0 never ends the period, so the "plain as
     stored" comparison of the t = 128 cases (d = 20, 128, 300, 1020) fails on every row.
  3. store_true not honoured for untouched rows: the t = 128 scaled cases compare the buffers AS STORED for all rows; an
     untouched row would still hold m / b1^127 (7e5 times too large).  First at d = 20, t = 128.
  4. The moments of chunk i read for chunk i + 1 at CPL = 2 or 4: m' and v' of the displaced coordinates are those of
     other coordinates (independent random plants: error of order G) -- the m' / v' assertions at d = 300, 512 (CPL = 2)
     and 516, 768, 1020 (CPL = 4), t = 57, both forms.
  5. q2 without 1 / sqrt(bc2): the denominator is sqrt(v') instead of sqrt(v') / sqrt(1 - b2^t); at t = 57 sqrt(bc2) =
     0.235, so every update is 4.2 times too large -- the update assertion of every scaled case, first d = 4, t = 57 (at
     t = 1000 it would be 1.26: the small t cases are the sharp ones, t = 2 at d = 20 gives a factor 22).
  6. A replay using this step's (a1, q2) for every replayed step: a row lagging n steps must move by
     sum_s a1_s m / (sqrt(v) q2_s + eps); with the constants of step t alone the sum differs by the drift of b1^k / bc1
     over the lag (tens of percent over 100 steps) -- the parameter assertion on the lagging rows of the lazy and
     look-ahead cases, first at d = 5, t = 40 (lags up to 39 steps).

Measured on an MI355X, worst error / bound over the cases of an entry point (m', v', update):
  entry point                    form    entity                bias                  scalars
  dense (every d, t)             plain   0.020  0.206  0.474   0.017  0.205  0.473   0.046  0.243  0.478
  dense (every d, t)             scaled  0.020  0.492  0.474   0.017  0.410  0.473   0.020  0.155  0.475
  small table, one launch        plain   0.006  0.204  0.455   0.004  0.202  0.471   0.003  0.195  0.436
  small table, one launch        scaled  0.009  0.381  0.454   0.005  0.298  0.470   0.003  0.218  0.435
  small table, three launches    as the one-launch rows, digit for digit
  heavy lists                    scaled  0.008  0.341  0.473   0.007  0.319  0.472   0.003  0.086  0.431
  lazy (catch-up + touched)      scaled  0.659  0.387  0.456   0.701  0.350  0.437   0.068  0.170  0.480
  look-ahead, listed and scan    scaled  0.009  0.361  0.458   0.008  0.354  0.459   0.013  0.264  0.308
  acc + apply, two chunks        plain   0.004  0.204  0.455   0.003  0.184  0.470   0.001  0.111  0.436
  acc + apply, two chunks        scaled  0.009  0.381  0.454   0.005  0.300  0.469   0.003  0.218  0.435
  acc_rows + apply_rows          scaled  0.009  0.381  0.452   0.005  0.300  0.469   0.003  0.218  0.435
  k_adam (flat)                  plain   m' 0.141  v' 0.250  update 0.498
  pipelined                      plain   0.006  0.204  0.457   0.003  0.184  0.471   0.003  0.195  0.436
  pipelined                      scaled  0.009  0.381  0.456   0.005  0.322  0.470   0.019  0.218  0.435
  pipelined, look-ahead form     scaled  0.008  0.358  0.458   0.005  0.262  0.456   0.002  0.154  0.280
The update sits at half its bound everywhere: that is the half ulp of the stored parameter, the bound's dominant term.
The lazy step's m' uses 0.7 of its bound: its gradient is taken at fp32 parameters that went through up to 126 replayed
steps, the oracle's at the fp64 replay.  The loss is within 1.2e-7 of the oracle's (lazy: 3.3e-6) against the 2e-5.
"""
import dataclasses

import numpy as np
import pytest
import torch

import adam_restatement as R
from oracle import vfm_oracle as O
from test_gpu_shapes import _random_problem

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOSS_TOL = 2e-5            # test_randomised_configurations_against_oracle


# ------------------------------------------------------------------------------------------------ problems (numpy only)
def table_sizes(F, B):
    """Field sizes around B: each column's B draws touch about half of its rows."""
    return [int(B * r) for r in (1.5, 1.25, 1.1, 1.4, 1.3)[:F]]


def batch_of(d):
    return 200 if d <= 256 else 96


def build_problem(F, d, output, link="abs", S=1, seed=0, B=None, sizes=None, skew=False):
    B = B or batch_of(d)
    sizes = sizes or table_sizes(F, B)
    spec, P, x, y, nb_occ, eps, group_hi = _random_problem(sizes, d, B, output, seed=seed)
    spec = dataclasses.replace(spec, n_samples=S, link=link)
    g = np.random.default_rng(seed + 17)
    if skew:                # the generator of test_gpu_shapes.test_skewed_batch_heavy_lists
        hot = g.random(B) < 0.7
        x[hot, 1] = sizes[0] + g.integers(0, 3, hot.sum())          # 3 items own 70 % of the rows
        x[g.random(B) < 0.3, 0] = 7                                  # one user owns 30 %
    T = spec.T
    eg, eb, ee = eps
    if S > 1:
        eg, eb, ee = (g.standard_normal(S).astype(np.float32), g.standard_normal((S, T)).astype(np.float32),
                      g.standard_normal((S, T, d)).astype(np.float32))
    touched = np.zeros(T, bool)
    touched[x.reshape(-1)] = True
    return dict(spec=spec, P=P, x=x, y=y, nb_occ=nb_occ, eps=(eg, eb, ee), group_hi=group_hi, output=output, link=link, S=S,
                B=B, touched=touched, rng=g)


# d -> (F, S, link, output, eps, ids): every value with every d class (VEC = 1; CPL = 1, 2, 4) at least once
I32, I64 = torch.int32, torch.int64
COVER = {
    5: (2, 1, "abs", "reg", "table", I32), 7: (3, 2, "softplus", "class", "philox", I64),
    33: (5, 1, "abs", "class", "philox", I32), 130: (2, 2, "softplus", "reg", "table", I64),
    255: (3, 1, "abs", "reg", "philox", I64),
    4: (2, 1, "abs", "reg", "table", I64), 8: (3, 2, "abs", "class", "philox", I32),
    12: (5, 1, "softplus", "reg", "table", I32), 20: (2, 1, "abs", "class", "philox", I64),
    64: (3, 1, "softplus", "class", "table", I64), 100: (5, 2, "abs", "reg", "philox", I32),
    128: (2, 1, "abs", "reg", "table", I32), 256: (2, 2, "softplus", "class", "philox", I64),
    300: (2, 1, "abs", "reg", "table", I32), 512: (3, 2, "softplus", "class", "philox", I64),
    516: (2, 1, "abs", "reg", "philox", I32), 768: (3, 2, "softplus", "class", "table", I64),
    1020: (5, 1, "abs", "reg", "table", I64),
}
EXTRA_COVER = [(300, (5, 1, "abs", "class", "philox", I64))]       # CPL = 2 has two sizes: F = 5 comes here
ALL_D = [4, 5, 7, 8, 12, 20, 33, 64, 100, 128, 130, 255, 256, 300, 512, 516, 768, 1020]
SWEEP_D, SWEEP_T = [20, 128, 300, 1020], [2, 127, 128, 129, 300]


def problems_of_gpu_cases():
    """(name, build_problem arguments) of every distinct planted problem below: tests/test_adam_state_cpu.py checks the
    excluded share of each without a GPU."""
    out = [("dense d=%d" % d, dict(F=c[0], d=d, output=c[3], link=c[2], S=c[1], seed=d)) for d, c in COVER.items()]
    out += [("dense extra d=%d" % d, dict(F=c[0], d=d, output=c[3], link=c[2], S=c[1], seed=d + 1)) for d, c in EXTRA_COVER]
    out += [("heavy d=%d" % d, dict(F=2, d=d, output="reg", seed=77, B=3000, sizes=[3000, 2500], skew=True)) for d in (16, 300)]
    out += [("philox F=2 d=%d" % d, dict(F=2, d=d, output="reg", seed=300 + d)) for d in (5, 12, 16, 20, 32, 128, 300)]
    return out


# ------------------------------------------------------------------------------------------------ the shared case
class Ctx:
    pass


def _case(entry, pb, t, form, eps="table", ids=I64, lag=None, run=None, tag=None):
    """One step `t` of entry point `run(c)` from a planted state.  pb: build_problem(); form: "plain" / "scaled";
    lag: None (every row is at step t - 1) or a function (rng, c) -> (last_step [T], keep [T] bool): rows that start at an
    earlier step (their moments are those of the common state, their parameters those of their own step) and rows the
    step must leave bitwise alone."""
    from vae_amd import ops
    dev = torch.device(DEV)
    spec, P, x, y, nb_occ = pb["spec"], pb["P"], pb["x"], pb["y"], pb["nb_occ"]
    T, d, S, output, link, touched = spec.T, spec.d, pb["S"], pb["output"], pb["link"], pb["touched"]
    scaled = form == "scaled"
    rng = np.random.default_rng(1000 * t + d)
    share = touched.mean()
    assert share >= 0.3 and 1 - share >= 0.3, share        # rows in the batch AND rows outside it
    c = Ctx()
    c.ops, c.pb, c.t, c.scaled, c.dev, c.spec, c.touched = ops, pb, t, scaled, dev, spec, touched
    c.inv_occ = ops.inv_occ_from_counts(torch.tensor(nb_occ, device=dev))
    c.plan = ops.BatchPlan(spec, torch.tensor(x, device=dev).to(ids).contiguous(), torch.tensor(y, device=dev), c.inv_occ)
    c.philox = eps == "philox"
    c.seed, c.step = 77, 1000 + t
    if c.philox:
        ee, eb, eg = (a.cpu().numpy() for a in ops.philox_eps(spec, seed=c.seed, step=c.step, device=dev))
        c.eps_t = None
    else:
        eg, eb, ee = pb["eps"]
        c.eps_t = tuple(torch.tensor(a, device=dev) for a in (ee, eb, eg))
    # rows that lag / rows to keep
    last = np.full(T, t - 1, np.int64)
    keep = np.zeros(T, bool)
    if lag is not None:
        last, keep = lag(rng, c)
    c.last_np = last
    fresh = R.fresh_rows(rng, touched)
    p_start = [P["entity_params"], P["bias_params"],
               np.concatenate([P["alpha"], P["global_bias_mean"], P["global_bias_scale"]])]
    c.ent, c.bia, c.scal = (torch.tensor(a, device=dev) for a in p_start)
    c.l3 = torch.zeros(3, device=dev)
    c.lr = R.LR

    # fp64: each lagging row's parameters brought to step t - 1 (its moments at ITS step are the common ones, undecayed)
    gap = (t - 1 - last).astype(np.float64)[:, None]

    def oracle(p64):
        Pd = {"entity_params": p64[0], "bias_params": p64[1], "alpha": p64[2][0:1], "global_bias_mean": p64[2][1:2],
              "global_bias_scale": p64[2][2:3]}
        return O.rowwise_elbo(Pd, x, y.astype(np.float64), nb_occ, np.asarray(pb["group_hi"]), np.asarray(spec.group_n),
                              spec.nb_train, eg, eb, ee, output, link=link)

    def grads(r):
        return [r["g_entity_params"], r["g_bias_params"],
                np.array([r["g_alpha"][0], r["g_global_bias_mean"][0], r["g_global_bias_scale"][0]])]

    sc_ok = slice(1, 3) if output == "class" else slice(0, 3)       # alpha: no gradient under Bernoulli (as the fuzz)
    # The scale G of the planted state is that of the gradient the step will see.  With lagging rows that gradient is
    # taken at the caught-up parameters, which depend on the planted state only through m / sqrt(v) -- not on G: plant
    # from the gradient at the start parameters, replay, and plant once more (same draws) from the gradient found there.
    r = oracle([a.astype(np.float64) for a in p_start])
    for _ in range(1 if lag is None else 2):
        gp, prng = grads(r), np.random.default_rng(1000 * t + d + 1)
        planted = [R.plant_state(prng, gp[0], t, fresh), R.plant_state(prng, gp[1], t, fresh), R.plant_state(prng, gp[2][sc_ok], t)]
        if output == "class":     # (the scalars' state has three entries whatever the likelihood)
            m3, v3 = planted[2]
            planted[2] = (np.concatenate([[np.float32(0)], m3]), np.concatenate([[np.float32(0)], v3]))
        m_pl = [np.asarray(a[0], np.float64) for a in planted]
        v_pl = [np.asarray(a[1], np.float64) for a in planted]
        before, moved, nrep = [], [], []
        for i in range(2):
            pb_, _, _, mv_, n_ = R.replay_fp64(p_start[i], m_pl[i] / R.B1 ** gap, v_pl[i] / R.B2 ** gap, last, t - 1, c.lr)
            before.append(pb_); moved.append(mv_); nrep.append(n_)
        before.append(p_start[2].astype(np.float64)); moved.append(np.zeros(3)); nrep.append(0)
        if lag is not None:
            r = oracle(before)          # the gradient at the fp64 caught-up parameters
    stored = [R.to_stored(m_pl[i], v_pl[i], t - 1, scaled) for i in range(3)]
    c.mv = tuple(torch.tensor(s[0], device=dev) for s in stored)
    c.vv = tuple(torch.tensor(s[1], device=dev) for s in stored)
    c.last_step = torch.tensor(last, device=dev, dtype=torch.int32)

    def forward():
        kw = dict(seed=c.seed, step=c.step) if c.philox else dict(eps=c.eps_t)
        c.st = ops.elbo_forward(c.plan, c.ent, c.bia, c.scal, c.inv_occ, **kw)
        return c.st
    c.forward = forward
    c.params_at_gradient = None
    run(c)
    torch.cuda.synchronize()
    if c.params_at_gradient is not None:
        # A run that caught its rows up itself hands over the (entity, bias) tables its gradient was taken at.  The fp32
        # replay may differ from the fp64 one by replay_bound (granted to the update below); where the replay has carried
        # a scale parameter close to zero, the 1 / sigma term of the KL gradient turns that difference into more than the
        # gradient's own grant, so the reference gradient is taken where the kernel's was.
        r = oracle([a.astype(np.float64) for a in c.params_at_gradient] + [before[2]])

    # reference: the gradient at the fp64 caught-up parameters, one Adam step, a zero-gradient one where the row is not
    # in the batch
    g64 = grads(r)
    tol = [R.TOL_TABLE, R.TOL_TABLE, None]
    G = [float(np.abs(g64[0]).max()), float(np.abs(g64[1]).max()), float(np.abs(g64[2][sc_ok]).max())]
    tol[2] = R.scalar_tolerances(r, P, y, eg, spec.nb_train, pb["B"], S, output, link) / G[2]
    loss = float(c.l3[0].item())
    print("ADAMSTATE %s %s d=%d t=%d loss rel %.2e" % (tag or entry, form, d, t, abs(loss - r["loss"]) / abs(r["loss"])))
    assert abs(loss - r["loss"]) / abs(r["loss"]) < LOSS_TOL
    got_p = [a.cpu().numpy() for a in (c.ent, c.bia, c.scal)]
    got_m = [a.cpu().numpy() for a in c.mv]
    got_v = [a.cpu().numpy() for a in c.vv]
    k_step = ((t - 1) % R.PERIOD + 1) if scaled else 0
    c.keep, c.p_ref, c.du, c.ok = keep, [], [], []     # for callers that go on from the fp64 step (its p', the bound on p')
    for i, kind in enumerate(("entity", "bias", "scalars")):
        rows = (~keep) if i < 2 else sc_ok
        kept = keep if i < 2 else (slice(0, 1) if output == "class" else slice(0, 0))
        # rows the step must not touch: parameters and stored moments bitwise
        assert np.array_equal(got_p[i][kept], p_start[i][kept]), kind
        assert np.array_equal(got_m[i][kept], stored[i][0][kept]) and np.array_equal(got_v[i][kept], stored[i][1][kept]), kind
        p_ref, m_ref, v_ref = R.step_fp64(before[i], g64[i], m_pl[i], v_pl[i], t, c.lr)
        m_got, v_got = R.to_plain(got_m[i], got_v[i], t, scaled)       # (t % 128 == 0: compared as stored)
        dm, dv, du = R.bounds(G[i], tol[i], before[i], m_ref, v_ref, t, c.lr, k_step)
        du = du + (R.replay_bound(before[i], moved[i], nrep[i]) if i < 2 else 0.0)
        em, ev = np.abs(m_got - m_ref) / dm, np.abs(v_got - v_ref) / dv
        ok = R.asserted(G[i], g64[i], v_ref, fresh if i < 2 else None)
        c.p_ref.append(p_ref); c.du.append(du); c.ok.append(ok)
        sel = np.zeros(ok.shape, bool)
        sel[rows] = True
        left_out = 1.0 - (ok | ~sel).mean()
        assert left_out <= R.MAX_EXCLUDED, (kind, left_out)
        eu = np.abs((got_p[i].astype(np.float64) - p_start[i]) - (p_ref - p_start[i])) / du
        rm, rv, ru = float(em[sel].max()), float(ev[sel].max()), float(eu[sel & ok].max())
        print("ADAMSTATE %s %s %s d=%d t=%d m %.3f v %.3f upd %.3f left out %.4f" % (tag or entry, form, kind, d, t, rm, rv, ru, left_out))
        assert rm <= 1.0, (kind, "m'", rm)
        assert rv <= 1.0, (kind, "v'", rv)
        assert ru <= 1.0, (kind, "update", ru)
        if i < 2:
            out = ~touched & ~keep
            if scaled and t % R.PERIOD != 0:       # rows without gradient: the stored moments are not rewritten
                assert np.array_equal(got_m[i][out], stored[i][0][out]) and np.array_equal(got_v[i][out], stored[i][1][out]), kind
            fo = fresh & ~touched                  # a row no batch has touched yet does not move
            assert fo.any() and np.array_equal(got_p[i][fo], p_start[i][fo]), kind
    return c


def _dense(c):
    c.forward()
    c.ops.elbo_backward_adam(c.plan, c.st, c.ent, c.bia, c.scal, c.inv_occ, c.mv, c.vv, c.lr, c.t, loss_out=c.l3,
                             scaled_moments=c.scaled)


def _cover_case(d, cfg, t, form, seed, tag="dense"):
    F, S, link, output, eps, ids = cfg
    pb = build_problem(F, d, output, link, S, seed=seed)
    _case("dense", pb, t, form, eps=eps, ids=ids, run=_dense, tag=tag)


# ------------------------------------------------------------------------------------------------ a. dense fused step
@pytest.mark.parametrize("form", ["plain", "scaled"])
@pytest.mark.parametrize("d", ALL_D)
def test_dense_step_every_shape_bucket(d, form):
    _cover_case(d, COVER[d], 57, form, seed=d)


@pytest.mark.parametrize("form", ["plain", "scaled"])
@pytest.mark.parametrize("d,cfg", EXTRA_COVER)
def test_dense_step_covering_extras(d, cfg, form):
    _cover_case(d, cfg, 57, form, seed=d + 1)


@pytest.mark.parametrize("form", ["plain", "scaled"])
@pytest.mark.parametrize("t", SWEEP_T)
@pytest.mark.parametrize("d", SWEEP_D)
def test_dense_step_period_positions(d, t, form):
    """t = 2 (bias corrections far from 1), 127 / 128 / 129 (last scaled step, the period's end: true moments written for
    EVERY row, first step of the next period) and 300 (third period)."""
    _cover_case(d, COVER[d], t, form, seed=d)


# ------------------------------------------------------------------------------------------------ b. small-table step
@pytest.mark.parametrize("small", ["one_launch", "three_launch"])
@pytest.mark.parametrize("form", ["plain", "scaled"])
@pytest.mark.parametrize("d", [5, 20, 128])
def test_small_table_step_and_three_launch_path(d, form, small, monkeypatch):
    """Philox eps, one sample: d = 20, 128 take the one-launch small-table kernel by default, VFM_BWD_SMALL=0 forces the
    three-launch path (d = 5: k_bwd either way) -- each against fp64."""
    if small == "three_launch":
        monkeypatch.setenv("VFM_BWD_SMALL", "0")
    pb = build_problem(2, d, "reg", seed=300 + d)
    _case("small", pb, 57, form, eps="philox", run=_dense, tag="small:" + small)


# ------------------------------------------------------------------------------------------------ c. heavy lists
@pytest.mark.parametrize("d", [16, 300])
def test_heavy_lists_step(d):
    pb = build_problem(2, d, "reg", seed=77, B=3000, sizes=[3000, 2500], skew=True)

    def run(c):
        assert c.plan.heavy is not None and c.plan.heavy[0].numel() >= 4
        _dense(c)
    _case("heavy", pb, 57, "scaled", run=run)


# ------------------------------------------------------------------------------------------------ e. lazy exact Adam
def _period_start(t):
    return ((t - 1) // R.PERIOD) * R.PERIOD


def _scaled_tab(t, lr):
    """(a1, q2) of the steps of t's period before t, as the look-ahead kernel's table holds them (restated in fp64)."""
    tab = np.zeros(2 * (R.PERIOD + 1), np.float32)
    ps = _period_start(t)
    for k in range(1, t - ps):
        cst = R.scaled_consts(ps + k, lr)
        tab[2 * k], tab[2 * k + 1] = cst["a1"], cst["q2"]
    return tab


@pytest.mark.parametrize("t", [40, 127])
@pytest.mark.parametrize("d", [5, 16, 128, 300])
def test_lazy_step_from_a_lagging_state(d, t):
    """vfm_adam_catchup_f32 on the batch's rows, the forward, the rows="touched" step; rows outside the batch are bitwise
    untouched and keep their last_step; then every row is caught up to t and the WHOLE table is compared with the fp64
    replay + step (lags up to t - 1 steps: 126 at t = 127)."""
    pb = build_problem(2, d, "reg", seed=300 + d)

    def lag(rng, c):
        return rng.integers(_period_start(t), t, c.spec.T), np.zeros(c.spec.T, bool)

    def run(c):
        ops, out = c.ops, torch.tensor(~c.touched, device=c.dev)
        lrs = [c.lr] * (t - _period_start(t))
        ids = c.plan.touched_ids()
        ops.adam_catchup(c.ent, c.bia, c.mv, c.vv, c.last_step, ids, lrs[:-1], upto=t - 1, mark=t)
        e0, b0, m0, v0, l0 = c.ent.clone(), c.bia.clone(), c.mv[0].clone(), c.vv[0].clone(), c.last_step.clone()
        c.forward()
        ops.elbo_backward_adam(c.plan, c.st, c.ent, c.bia, c.scal, c.inv_occ, c.mv, c.vv, c.lr, t, loss_out=c.l3,
                               scaled_moments=True, rows="touched")
        assert torch.equal(c.ent[out], e0[out]) and torch.equal(c.bia[out], b0[out])
        assert torch.equal(c.mv[0][out], m0[out]) and torch.equal(c.vv[0][out], v0[out])
        assert torch.equal(c.last_step[out], l0[out]) and bool((c.last_step[~out] == t).all())
        assert np.array_equal(l0[out].cpu().numpy(), c.last_np[~c.touched])
        ops.adam_catchup(c.ent, c.bia, c.mv, c.vv, c.last_step, None, lrs, upto=t, mark=t)
        assert bool((c.last_step == t).all())
    _case("lazy", pb, t, "scaled", eps="philox", lag=lag, run=run)


# ------------------------------------------------------------------------------------------------ f. look-ahead entry
def _lookahead_lag(rng, c, pb, t, nxt):
    """A next batch over the same tables (kept in nxt), lags for every row outside this batch, and the rows in neither.
    One column per field, drawn field by field (F = 2: the draws of the two-column form this grew from)."""
    T = c.spec.T
    hi = np.asarray(pb["group_hi"], np.int64)
    lo = np.concatenate([[0], hi[:-1]])
    x2 = np.stack([int(lo[f]) + rng.integers(0, int(hi[f] - lo[f]), pb["B"]) for f in range(len(hi))], 1).astype(np.int64)
    in_next = np.zeros(T, bool)
    in_next[x2.reshape(-1)] = True
    nxt["x"], nxt["mask"] = x2, in_next
    last = rng.integers(_period_start(t), t, T)
    last[c.touched] = t - 1                   # the rows of this batch were announced to the previous step: current
    keep = ~c.touched & ~in_next
    assert keep.sum() >= 20 and (in_next & ~c.touched).sum() >= 20
    return last, keep


@pytest.mark.parametrize("listed", [True, False])
@pytest.mark.parametrize("t", [40, 127])
@pytest.mark.parametrize("d", [5, 32, 128, 300])
def test_lookahead_step_from_a_lagging_state(d, t, listed):
    """Rows of this batch take the gradient step; rows only in the NEXT batch replay their lag and this step's
    zero-gradient update; rows in neither stay bitwise (parameters, moments, last_step)."""
    pb = build_problem(2, d, "reg", seed=300 + d)
    nxt = {}

    def lag(rng, c):
        return _lookahead_lag(rng, c, pb, t, nxt)

    def run(c):
        ops = c.ops
        y2 = torch.tensor(pb["y"], device=c.dev)
        plan2 = ops.BatchPlan(c.spec, torch.tensor(nxt["x"], device=c.dev), y2, c.inv_occ)
        tab = torch.tensor(_scaled_tab(t, c.lr), device=c.dev)
        c.forward()
        ops.elbo_backward_adam_lookahead(c.plan, c.st, plan2, c.ent, c.bia, c.scal, c.inv_occ, c.mv, c.vv, c.lr, t, c.l3,
                                         c.last_step, tab, listed=listed)
        visited = torch.tensor(c.touched | nxt["mask"], device=c.dev)
        assert bool((c.last_step[visited] == t).all())
        assert np.array_equal(c.last_step[~visited].cpu().numpy(), c.last_np[~(c.touched | nxt["mask"])])
        k = (t - 1) % R.PERIOD + 1
        cst = R.scaled_consts(t, c.lr)             # the kernel leaves this step's (a1, q2) for later replays
        assert abs(tab[2 * k].item() - cst["a1"]) <= R.ulp32(cst["a1"]) and abs(tab[2 * k + 1].item() - cst["q2"]) <= R.ulp32(cst["q2"])
    _case("lookahead", pb, t, "scaled", eps="philox", lag=lag, run=run, tag="lookahead:" + ("listed" if listed else "scan"))


# ------------------------------------------------------------------------------------------------ g. pipelined entry
def _pipe_forward(c):
    """The record forward of the pipelined step: this step's sample records from the tables, then the gather."""
    from vae_amd import _lib
    ops, B = c.ops, c.pb["B"]
    c.zrec = torch.zeros(c.spec.T, ops.record_len(c.spec.d), device=c.dev)
    ops.sample_records(c.plan, c.ent, c.bia, c.inv_occ, c.zrec, c.seed, c.step)
    c.st = ops.elbo_forward_records(c.plan, c.zrec, c.scal, c.seed, c.step, torch.empty(B, device=c.dev),
                                    torch.empty(B, device=c.dev), torch.empty(_lib.PARTIALS_LEN, dtype=torch.float64, device=c.dev))


@pytest.mark.parametrize("form", ["plain", "scaled"])
@pytest.mark.parametrize("d", [20, 128, 300])
def test_pipelined_step(d, form):
    """elbo_backward_adam_pipe (k_bwd<PIPE>: the walk gathers the other entity's sample record), every row visited."""
    pb = build_problem(2, d, "reg", seed=300 + d)

    def run(c):
        _pipe_forward(c)
        c.ops.elbo_backward_adam_pipe(c.plan, c.st, c.zrec, None, None, c.step + 1, c.ent, c.bia, c.scal, c.inv_occ, c.mv, c.vv,
                                      c.lr, c.t, c.l3, scaled_moments=c.scaled)
    _case("pipe", pb, 57, form, eps="philox", run=run)


@pytest.mark.parametrize("listed", [True, False])
@pytest.mark.parametrize("d", [20, 128, 300])
def test_pipelined_step_lookahead_form(d, listed):
    """k_bwd<PIPE, LA>: as the look-ahead entry -- gradient step on this batch's rows, lag + zero-gradient step on the
    rows only the next batch holds, the others bitwise -- with the samples gathered from records."""
    t = 40
    pb = build_problem(2, d, "reg", seed=300 + d)
    nxt = {}

    def lag(rng, c):
        last, keep = _lookahead_lag(rng, c, pb, t, nxt)
        return last, keep

    def run(c):
        ops = c.ops
        plan2 = ops.BatchPlan(c.spec, torch.tensor(nxt["x"], device=c.dev), torch.tensor(pb["y"], device=c.dev), c.inv_occ)
        tab = torch.tensor(_scaled_tab(t, c.lr), device=c.dev)
        _pipe_forward(c)
        ops.elbo_backward_adam_pipe(c.plan, c.st, c.zrec, None, None, c.step + 1, c.ent, c.bia, c.scal, c.inv_occ, c.mv, c.vv,
                                    c.lr, t, c.l3, scaled_moments=True, last_step=c.last_step, step_tab=tab, listed=listed,
                                    la_next=plan2)
        visited = c.touched | nxt["mask"]
        assert bool((c.last_step[torch.tensor(visited, device=c.dev)] == t).all())
        assert np.array_equal(c.last_step.cpu().numpy()[~visited], c.last_np[~visited])
    _case("pipe-lookahead", pb, t, "scaled", eps="philox", lag=lag, run=run, tag="pipe-lookahead:" + ("listed" if listed else "scan"))


# ------------------------------------------------------------------------------------------------ h. multi-rank stages
@pytest.mark.parametrize("form", ["plain", "scaled"])
@pytest.mark.parametrize("d", [12, 128])
def test_multi_rank_stages_two_entity_chunks(d, form):
    """elbo_backward_acc + elbo_apply_adam over two entity chunks (the chunk that ends at T moves the scalars)."""
    pb = build_problem(2, d, "reg", seed=300 + d)

    def run(c):
        ops, T = c.ops, c.spec.T
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
    _case("acc+apply", pb, 57, form, eps="philox", run=run)


@pytest.mark.parametrize("d", [12, 128])
def test_multi_rank_stages_listed_rows_compact(d):
    """elbo_backward_acc_rows + elbo_apply_adam_rows over the batch's rows with compact records: the listed rows and the
    scalars take the step, every other row stays bitwise."""
    pb = build_problem(2, d, "reg", seed=300 + d)

    def lag(rng, c):
        return np.full(c.spec.T, c.t - 1, np.int64), ~c.touched

    def run(c):
        ops = c.ops
        c.forward()
        c.l3.copy_(ops.elbo_finalize(c.st, c.scal))
        ids = c.plan.touched_ids()
        acc = torch.zeros(ids.numel() * ops.exchange_record_len(d), device=c.dev)
        sums = torch.zeros(2, device=c.dev)
        ops.elbo_backward_acc_rows(c.plan, c.st, ids, acc, sums)
        ops.elbo_apply_adam_rows(c.plan, c.st, acc, sums, ids, c.ent, c.bia, c.scal, c.inv_occ, c.mv, c.vv, c.lr, c.t,
                                 move_scalars=True, compact=True)
    _case("acc_rows+apply_rows", pb, 57, "scaled", eps="philox", lag=lag, run=run)


# ------------------------------------------------------------------------------------------------ i. small related checks
@pytest.mark.parametrize("n", [4096, 4097, 4098, 4099])
def test_flat_adam_kernel_from_a_planted_state(n):
    """ops.adam_step (k_adam): the vector body and every tail length; the gradient is handed over exactly (tol_g = 0)."""
    from vae_amd import ops
    rng = np.random.default_rng(n)
    t = 57
    g = (rng.standard_normal(n) * 0.3).astype(np.float32)
    p = (rng.standard_normal(n) * 0.5).astype(np.float32)
    m, v = R.plant_state(rng, g, t)
    n4 = (n + 3) // 4 * 4
    buf = [torch.zeros(n4, device=DEV) for _ in range(4)]
    for b_, a in zip(buf, (p, g, m, v)):
        b_[:n] = torch.tensor(a, device=DEV)
    ops.adam_step(buf[0][:n], buf[1][:n], buf[2][:n], buf[3][:n], R.LR, t)
    p_ref, m_ref, v_ref = R.step_fp64(p, g, m, v, t)
    G = float(np.abs(g).max())
    dm, dv, du = R.bounds(G, 0.0, p, m_ref, v_ref, t)
    got = [b_[:n].cpu().numpy().astype(np.float64) for b_ in buf]
    rm, rv = np.abs(got[2] - m_ref) / dm, np.abs(got[3] - v_ref) / dv
    ru = np.abs((got[0] - p) - (p_ref - p)) / du
    print("ADAMSTATE k_adam plain flat n=%d m %.3f v %.3f upd %.3f" % (n, rm.max(), rv.max(), ru.max()))
    assert rm.max() <= 1 and rv.max() <= 1 and ru.max() <= 1
    assert all(float(b_[n:].abs().sum()) == 0 for b_ in buf)          # nothing written past n


@pytest.mark.parametrize("steps", [1, 127, 128, 300])
def test_moments_rescale_against_the_host_conversion(steps):
    """ops.moments_rescale against to_stored / to_plain (fp64, one rounding): within 2 ulp per entry (the kernel multiplies
    by the rounded factor: half an ulp for the factor, half for the product, the grid moves by up to 2 under a scale that
    is no power of two), and bitwise unchanged at multiples of 128."""
    from vae_amd import ops
    rng = np.random.default_rng(steps)
    m, v = R.plant_state(rng, rng.standard_normal(1003), 2)
    for to_scaled in (True, False):
        tm, tv = torch.tensor(m, device=DEV), torch.tensor(v, device=DEV)
        ops.moments_rescale(tm, tv, steps, to_scaled=to_scaled)
        k = steps % R.PERIOD
        want_m = m.astype(np.float64) * (R.B1 ** -k if to_scaled else R.B1 ** k)
        want_v = v.astype(np.float64) * (R.B2 ** -k if to_scaled else R.B2 ** k)
        if to_scaled:
            assert np.array_equal(want_m.astype(np.float32), R.to_stored(m, v, steps, True)[0])
        else:
            assert np.array_equal(want_m, R.to_plain(m, v, steps, True)[0])
        gm, gv = tm.cpu().numpy(), tv.cpu().numpy()
        if k == 0:
            assert np.array_equal(gm, m) and np.array_equal(gv, v)
        assert np.all(np.abs(gm - want_m) <= 2 * R.ulp32(want_m)) and np.all(np.abs(gv - want_v) <= 2 * R.ulp32(want_v))

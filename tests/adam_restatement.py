"""Adam from a LIVE optimiser state, restated: helpers of tests/test_adam_state_cpu.py and tests/test_gpu_adam_state.py.
TEST INFRASTRUCTURE ONLY (numpy; no GPU, no vae_amd import).

One teacher-forced step from a planted state (m, v, t) has no trajectory amplification, so the fused kernels' optimiser
arithmetic can be held against fp64 with bounds DERIVED from the tolerance the suite already grants the gradient -- not
chosen to fit.  From a zero state at t = 1 every mistake in the moments' bookkeeping gives the same bits (the first Adam
step is -lr sign(g)); from a planted state it is an error of order 1.

The hyper-parameters are the fp32 values the C ABI receives (B1 = fp32(0.9), ...): the operation under test is Adam with
THOSE betas, and 1 - B1, 1 - B2 are then exact in fp32.

Stored forms.  Plain: the buffers hold m, v.  Scaled (VFM_FLAG_SCALED_MOMENTS): they hold m / B1^k, v / B2^k with
k = (Adam steps so far) mod 128; `to_stored` / `to_plain` convert in fp64 on the host (one rounding to fp32), on purpose
not through ops.moments_rescale, which is code under test.

Bounds (`bounds`), in units u = 2^-24 (half an ulp, relative) and ulp(x) = spacing of fp32 at |x|.  With dg the granted
absolute gradient error of an entry (tables: tol_g G, G = max |g| of the tensor) and |g| <= G:
  |dm'| <= (1 - B1) dg + c_m ulp(|m'| + G)
  |dv'| <= (1 - B2) (2 G dg + dg^2) + c_v ulp(|v'| + (1 - B2) G^2)
  |d(p' - p)| <= step/den dm' + step |m'| / (2 den^2 sqrt(v') sqrt(bc2)) dv' + c_u u |p' - p| + ulp(|p| + |p' - p|),
      den = sqrt(v') / sqrt(bc2) + eps        (first-order propagation through step m' / den)
counted from the kernels' operation sequences (adam_update in vae_amd/csrc/vfm_bwd.hpp, k_adam in vfm_adam.hpp):
  plain  m' = m + (g - m)(1 - B1): three roundings of at most half an ulp of an operand no larger than |m'| + G
         (|m| <= (|m'| + 0.1 G) / 0.9): c_m = 2.   v' = v B2 + ((1 - B2) g) g: the product v B2 and the sum round at
         the size of v', the two small products at 1e-3 of it: c_v = 2.
  scaled the handed-in buffer is m / B1^k rounded once (<= 1 ulp of m after scaling back: a scale that is no power of two
         moves the ulp grid by up to 2), c1 = fp32((1 - B1) / B1^k) (u of 0.1 G), one fma (1 ulp after scaling back), and
         at the end of a period the product with fp32(B1^k) (constant + product: 1 ulp): c_m = 4; the same count gives
         c_v = 4.
  update plain: fp32(step_size), step_size m', IEEE sqrt, fp32(bc2_sqrt), the division by it, + eps, the last division:
         7 u.  scaled: fp32(a1), a1 m, hardware sqrt (1 ulp = 2 u), fp32(q2), fma(r, q2, eps), hardware rcp (2 u): 8 u.
         c_u = 8 for both, and one ulp at |p| + |p' - p| for the rounding of the stored parameter -- the dominant term.
A replay of n zero-gradient steps (`replay_bound`) sums n such steps with dg = 0: the moments enter with their stored
rounding (u each, 1.5 u on the update), so (c_u + 2) u sum |updates| + n ulp(|p| + sum |updates|).

Where the statement holds (`asserted`): the update bound is relative in nature, so it is asserted on entries with
v' >= (0.1 G)^2 (and on fresh rows additionally |g| >= 1e-3 G); elsewhere eps and cancellation take over.  Planted second
moments are >= 0.25 G^2, so only FRESH rows (m = v = 0: no batch has touched them) can fall out, and `fresh_rows` plants so
few of them (two in the batch, two outside, tables of >= 200 rows) that at most 2 % of a tensor is left out.

CPU run (tests/test_adam_state_cpu.py, the gradient perturbed by the FULL tolerance, t = 2, 57, 127, 128, 129, 300,
1000), worst value / bound:
  entity   plain  m' 0.984  v' 0.875  update 0.980      scaled  m' 0.968  v' 0.874  update 0.961
  bias     plain  m' 0.988  v' 0.709  update 0.985      scaled  m' 0.977  v' 0.592  update 0.972
  scalars  plain  m' 1.000  v' 0.972  update 0.992      scaled  m' 0.999  v' 0.922  update 0.991
  (the gradient term fills the bound: the perturbation is the whole granted error; the roundings alone reach 0.5 of the
  update bound and 0.25 of v'), a replay of 126 steps 0.076 of replay_bound; with sqrt(bc2) dropped from the
  denominator the update is more than 10 bounds off at every t <= 300.
"""
import math

import numpy as np

from oracle import vfm_oracle as O

f4, f8 = np.float32, np.float64
B1, B2, EPS, LR = float(f4(0.9)), float(f4(0.999)), float(f4(1e-8)), float(f4(0.01))
PERIOD = 128
U = 2.0 ** -24
TOL_TABLE = 1e-4           # tests/test_gpu_shapes.py::test_randomised_configurations_against_oracle: 1e-4 of the largest entry
C_M = {False: 2.0, True: 4.0}
C_V = {False: 2.0, True: 4.0}
C_U = 8.0
MAX_EXCLUDED = 0.02


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, f8)).astype(f4)).astype(f8)


def fresh_rows(rng, touched):
    """Row mask of the fresh rows (m = v = 0) of a table whose rows `touched` (bool [T]) are in the batch: two rows of
    the batch and two outside it -- at most 2 % of a table of >= 200 rows."""
    touched = np.asarray(touched, bool)
    assert touched.size >= 200 and touched.sum() >= 2 and (~touched).sum() >= 2
    fresh = np.zeros(touched.size, bool)
    fresh[rng.choice(np.flatnonzero(touched), 2, replace=False)] = True
    fresh[rng.choice(np.flatnonzero(~touched), 2, replace=False)] = True
    return fresh


def plant_state(rng, g64, t, fresh=None):
    """Plain moments "after t - 1 steps" of one tensor with fp64 gradient g64: m ~ N(0, (0.3 G)^2), v = u G^2 with
    u ~ U[0.25, 4], G = max |g64|; both rounded to fp32.  fresh: bool mask over the rows that get m = v = 0 exactly."""
    g64 = np.asarray(g64, f8)
    G = float(np.abs(g64).max())
    assert G > 0 and t >= 2
    m = (rng.standard_normal(g64.shape) * 0.3 * G).astype(f4)
    v = (rng.uniform(0.25, 4.0, g64.shape) * G * G).astype(f4)
    if fresh is not None:
        m[fresh] = 0
        v[fresh] = 0
    return m, v


def _k(steps_so_far):
    return int(steps_so_far) % PERIOD


def to_stored(m, v, steps_so_far, scaled):
    """The fp32 buffers the kernel is handed after `steps_so_far` Adam steps."""
    k = _k(steps_so_far) if scaled else 0
    return (np.asarray(m, f8) / B1 ** k).astype(f4), (np.asarray(v, f8) / B2 ** k).astype(f4)


def to_plain(ms, vs, steps_so_far, scaled):
    k = _k(steps_so_far) if scaled else 0
    return np.asarray(ms, f8) * B1 ** k, np.asarray(vs, f8) * B2 ** k


def step_fp64(p, g, m, v, t, lr=LR):
    """oracle.vfm_oracle.adam_step on copies: (p', m', v') in fp64."""
    p, m, v = (np.array(a, f8) for a in (p, m, v))
    O.adam_step(p, np.asarray(g, f8), m, v, int(t), lr, B1, B2, EPS)
    return p, m, v


def replay_fp64(p, m, v, t_from, t_to, lr_of_step=LR):
    """The zero-gradient steps t_from + 1 .. t_to applied to (p, m, v) = the state after step t_from.  t_from: an int, or
    one step per ROW (lagging rows; m, v are then each row's moments at ITS step).  lr_of_step: a float or a callable of
    the step.  Returns (p, m, v, sum of |updates|, steps replayed per row)."""
    p, m, v = (np.array(a, f8) for a in (p, m, v))
    tf = np.asarray(t_from, np.int64)
    tf_b = tf.reshape(tf.shape + (1,) * (p.ndim - tf.ndim)) if tf.ndim else tf
    moved = np.zeros_like(p)
    lr_of = lr_of_step if callable(lr_of_step) else (lambda s: lr_of_step)
    for s in range(int(tf.min()) + 1, int(t_to) + 1):
        act = np.broadcast_to(tf_b < s, p.shape)
        m = np.where(act, B1 * m, m)
        v = np.where(act, B2 * v, v)
        upd = (lr_of(s) / (1 - B1 ** s)) * m / (np.sqrt(v) / math.sqrt(1 - B2 ** s) + EPS)
        p = np.where(act, p - upd, p)
        moved += np.where(act, np.abs(upd), 0.0)
    return p, m, v, moved, np.maximum(int(t_to) - tf, 0)


def step_fp32_plain(p, g, m, v, t, lr=LR):
    """adam_update's plain branch (and k_adam), operation for operation in numpy fp32 (no fma contraction)."""
    p, g, m, v = (np.asarray(a, f4) for a in (p, g, m, v))
    step_size, bc2_sqrt = f4(lr / (1.0 - B1 ** t)), f4(math.sqrt(1.0 - B2 ** t))
    m2 = m + (g - m) * (f4(1) - f4(B1))
    v2 = v * f4(B2) + ((f4(1) - f4(B2)) * g) * g
    den = np.sqrt(v2) / bc2_sqrt + f4(EPS)
    return p + (-step_size * m2) / den, m2, v2


def scaled_consts(t, lr=LR):
    """scaled_moment_consts / scaled_step_consts of vfm_abi.hip in fp64, each rounded to fp32 where the host does."""
    k = (int(t) - 1) % PERIOD + 1
    s1, s2 = B1 ** k, B2 ** k
    step_size, bc2_sqrt = f4(lr / (1.0 - B1 ** t)), f4(math.sqrt(1.0 - B2 ** t))
    return dict(k=k, s1=f4(s1), s2=f4(s2), c1=f4((1.0 - B1) / s1), c2=f4((1.0 - B2) / s2), step_size=step_size,
                bc2_sqrt=bc2_sqrt, a1=f4(float(step_size) * s1), q2=f4(math.sqrt(s2) / float(bc2_sqrt)),
                store_true=int(k == PERIOD))


def _fma(a, b, c):
    return (np.asarray(a, f8) * np.asarray(b, f8) + np.asarray(c, f8)).astype(f4)


def step_fp32_scaled(p, g, ms, vs, t, lr=LR):
    """adam_update's scaled branch (adam_accum + adam_apply) on the STORED buffers; returns (p', ms', vs') as stored after
    the step (true moments when the step ends a period).  sqrt / rcp correctly rounded here, 1 ulp on the hardware."""
    p, g, ms, vs = (np.asarray(a, f4) for a in (p, g, ms, vs))
    c = scaled_consts(t, lr)
    ms2 = _fma(c["c1"], g, ms)
    vs2 = _fma(c["c2"] * g, g, vs)
    r = np.sqrt(vs2)
    den = _fma(r, c["q2"], f4(EPS))
    pn = _fma(-c["a1"] * ms2, f4(1) / den, p)
    if c["store_true"]:
        ms2, vs2 = ms2 * c["s1"], vs2 * c["s2"]
    return pn, ms2, vs2


def bounds(G, tol_g, p, m, v, t, lr=LR, k=0):
    """(|dm'|, |dv'|, |d(p' - p)|) allowed per entry.  G: max |g| of the tensor; tol_g: granted gradient error / G (a
    number, or one per entry); p: the parameters before the step; m, v: the fp64 reference's NEW moments; k: 0 for the
    plain form, else the scaled form (the position in the period: any k >= 1 pays the conversion roundings)."""
    p, m, v = (np.asarray(a, f8) for a in (p, m, v))
    scaled = bool(k)
    dg = np.asarray(tol_g, f8) * G
    dm = (1.0 - B1) * dg + C_M[scaled] * ulp32(np.abs(m) + G)
    dv = (1.0 - B2) * (2.0 * G * dg + dg * dg) + C_V[scaled] * ulp32(np.abs(v) + (1.0 - B2) * G * G)
    step, sb = lr / (1.0 - B1 ** t), math.sqrt(1.0 - B2 ** t)
    rt = np.sqrt(v)
    den = rt / sb + EPS
    upd = step * np.abs(m) / den
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        dden = np.where(rt > 0, dv / (2.0 * np.maximum(rt, 1e-300) * sb), np.inf)
        du = step / den * dm + np.where(upd > 0, upd / den * dden, 0.0) + C_U * U * upd + ulp32(np.abs(p) + upd)
    return dm, dv, np.nan_to_num(du, nan=np.inf)      # (v' = 0: no statement; `asserted` leaves those entries out)


def replay_bound(p, moved, n_steps):
    """|dp| allowed after n_steps replayed zero-gradient steps whose fp64 updates sum to `moved` in magnitude."""
    n = np.asarray(n_steps, f8)
    n = n.reshape(n.shape + (1,) * (np.ndim(p) - n.ndim)) if n.ndim else n
    return (C_U + 2.0) * U * moved + n * ulp32(np.abs(np.asarray(p, f8)) + moved)


def asserted(G, g64, v_new, fresh=None):
    """Entries on which the update bound is asserted: v' >= (0.1 G)^2, on fresh rows additionally |g| >= 1e-3 G."""
    ok = np.asarray(v_new, f8) >= (0.1 * G) ** 2
    if fresh is not None and np.any(fresh):
        fr = np.zeros(ok.shape, bool)
        fr[fresh] = True
        ok &= ~fr | (np.abs(np.asarray(g64, f8)) >= 1e-3 * G)
    return ok


def scalar_tolerances(r, P, y, eg, nb_train, B, S, output, link):
    """The granted error of the three scalar gradients, the summation bound of tests/fuzz_parity.py:
    5e-4 |want| + 1e-4 * (sum of the magnitudes of the summed terms).  r: the oracle's result; eg: eps of the global bias."""
    L = (lambda x: abs(x)) if link == "abs" else (lambda x: float(np.logaddexp(0.0, x)))
    a_, sg0 = L(float(P["alpha"][0])), L(float(P["global_bias_scale"][0]))
    scale = nb_train / (B * S)
    sum_abs_g = float(np.abs(r["g_row"]).sum())
    pr_ = np.asarray(r["pred"], f8).reshape(S, B)
    mags = [scale * float((0.5 * (np.asarray(y, f8)[None, :] - pr_) ** 2 + 0.5 / a_).sum()) if output == "reg" else 1.0,
            sum_abs_g + abs(float(P["global_bias_mean"][0])),
            float(np.abs(eg).max()) * sum_abs_g + sg0 + 1.0 / sg0]
    want = [r["g_alpha"][0], r["g_global_bias_mean"][0], r["g_global_bias_scale"][0]]
    return np.array([5e-4 * abs(w) + 1e-4 * mg for w, mg in zip(want, mags)])
